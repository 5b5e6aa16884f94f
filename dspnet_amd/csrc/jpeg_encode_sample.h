// What the device kernels of the JPEG encode ask of an untrusted descriptor before they index the coefficient pool with it
// (jpeg_encode.hip adds the pixel side; jpeg_entropy_encode.hip reads coefficients only).
#pragma once
#include "../../include/dspn_jpeg_encode.h"

namespace dspn_jpeg_enc {

// true when the sample is not skipped, its geometry is a supported one, its grids are the real grids of its size and sampling,
// and every block of them lies inside a pool of coef_count coefficients; hs, vs receive luma's sampling
__device__ inline bool coefs_ok(const dspn_jpeg_enc_sample &s, long long coef_count, int &hs, int &vs) {
  if (s.skip) return false;
  if (s.width < 1 || s.height < 1 || s.width > 65535 || s.height > 65535) return false;
  if (s.ncomp != 1 && s.ncomp != 3) return false;
  hs = 1; vs = 1;
  if (s.ncomp == 3) {
    hs = s.hsamp; vs = s.vsamp;
    if (!((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)))) return false;
  }
  for (int c = 0; c < s.ncomp; ++c) {
    const int cw = c ? (s.width + hs - 1) / hs : s.width, ch = c ? (s.height + vs - 1) / vs : s.height;
    const int bw = s.blocks_w[c], bh = s.blocks_h[c];
    if (bw != (cw + 7) / 8 || bh != (ch + 7) / 8) return false;      // 1 .. 8192 each
    const long long off = s.coef_offset[c];
    if (off < 0 || (off & 63) || off > coef_count - 64LL * bw * bh) return false;
  }
  return true;
}

}  // namespace dspn_jpeg_enc
