// JPEG encode for MI355X (gfx950); C ABI and the arithmetic contract in include/dspn_jpeg_encode.h.  The host half (tables,
// markers, Huffman) is jpeg_encode_host.h.  The device half is two launches on the caller's stream, each a fixed grid of
// workgroups that strides over the work of the whole batch, as in jpeg.hip:
//   jpeg_enc_planes_kernel : interleaved pixels -> uint8 component planes in the workspace (a plane is a raster over the real
//                            block grid and sits at the byte offset its coefficients have as an int16 index, so the workspace
//                            is coef_count bytes).  One thread per 4 samples of a plane row: it converts the 4 (full-size
//                            plane), 8 (2 x 1) or 16 (2 x 2) pixels behind them, edges replicated by clamping the source
//                            coordinates, and stores one dword.
//   jpeg_enc_fdct_kernel   : planes -> quantised coefficients.  Eight lanes per block: lane t loads row t (8 B), runs the row
//                            pass, the block turns through LDS, lane t runs column t, the block turns back, and lane t
//                            quantises and stores row t of the result as 16 B, so a wave writes 1 KiB of consecutive coefficients.
// Per image of h x w pixels with n samples per pixel (3, 2, 1.5; 1 for grey):
//   planes reads 3 (or 1) bytes/pixel, writes n bytes/pixel;  fdct reads n bytes/pixel, writes 2 n bytes/pixel.
// Neither kernel knows the batch on the host: each workgroup first sums the work of the B descriptors in LDS (validating
// every one: a descriptor that could index outside a buffer, or whose grids are not the real grids of its size, counts as no
// work), then finds the sample of a unit by a binary search over those sums.
#include <cstdint>

#include "dspn_common.h"
#include "jpeg_encode_host.h"
#include "jpeg_encode_sample.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxB = 1024;
constexpr int kGrid = 2048;                // 256 CUs x 8 workgroups of 256 threads
constexpr int kBlocksPerWg = kT / 8;
constexpr int kRowSamples = kT * 4;        // samples of a plane row one workgroup covers per unit

struct Pools { long long images_bytes, coef_count; };
struct ChannelMap { int r, g, b; };

// true when every index the kernels derive from `s` stays inside images and coefs / workspace (coef_count)
__device__ bool sample_ok(const dspn_jpeg_enc_sample &s, const Pools &pl) {
  int hs, vs;
  if (!dspn_jpeg_enc::coefs_ok(s, pl.coef_count, hs, vs)) return false;
  return s.img_offset >= 0 && s.img_offset <= pl.images_bytes - (long long)s.ncomp * s.width * s.height;
}

// first[b] = units of samples 0 .. b - 1 (first[B] = all); units(s) is called for valid samples only
template <typename F>
__device__ void prefix_units(const dspn_jpeg_enc_sample *samples, int B, const Pools &pl, long long *first, F units) {
  for (int b = threadIdx.x; b < B; b += kT) {
    const dspn_jpeg_enc_sample &s = samples[b];
    first[b + 1] = sample_ok(s, pl) ? units(s) : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long acc = 0;
    first[0] = 0;
    for (int b = 1; b <= B; ++b) { acc += first[b]; first[b] = acc; }
  }
  __syncthreads();
}

// largest b in [0, B) with first[b] <= u (u < first[B])
__device__ __forceinline__ int find_sample(const long long *first, int B, long long u) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int row_chunks(int bw) { return (bw * 8 + kRowSamples - 1) / kRowSamples; }

// component c (0: Y, 1: Cb, 2: Cr) of one pixel
__device__ __forceinline__ int ycc(const unsigned char *__restrict__ px, const ChannelMap &cm, int c) {
  const int r = px[cm.r], g = px[cm.g], b = px[cm.b];
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(kT) void jpeg_enc_planes_kernel(const unsigned char *__restrict__ images,
                                                             const dspn_jpeg_enc_sample *__restrict__ samples, int B, Pools pl,
                                                             ChannelMap cm, unsigned char *__restrict__ planes) {
  __shared__ long long first[kMaxB + 1];
  prefix_units(samples, B, pl, first, [](const dspn_jpeg_enc_sample &s) {
    long long n = 0;
    for (int c = 0; c < s.ncomp; ++c) n += (long long)s.blocks_h[c] * 8 * row_chunks(s.blocks_w[c]);
    return n;
  });
  const long long total = first[B];
  for (long long u = blockIdx.x; u < total; u += gridDim.x) {
    const int b = find_sample(first, B, u);
    const dspn_jpeg_enc_sample &s = samples[b];
    long long l = u - first[b];
    int c = 0;
    for (; c < s.ncomp - 1; ++c) {
      const long long n = (long long)s.blocks_h[c] * 8 * row_chunks(s.blocks_w[c]);
      if (l < n) break;
      l -= n;
    }
    const int pw = s.blocks_w[c] * 8, chunks = row_chunks(s.blocks_w[c]);
    const int py = (int)(l / chunks);
    const int px0 = (int)(l - (long long)py * chunks) * kRowSamples + threadIdx.x * 4;
    if (px0 >= pw) continue;
    const int W = s.width, H = s.height;
    const unsigned char *img = images + s.img_offset;
    int out[4];
    if (s.ncomp == 1) {
      const unsigned char *row = img + (long long)min(py, H - 1) * W;
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = row[min(px0 + j, W - 1)];
    } else if (c == 0 || s.hsamp == 1) {
      const unsigned char *row = img + (long long)min(py, H - 1) * W * 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = ycc(row + min(px0 + j, W - 1) * 3, cm, c);
    } else if (s.vsamp == 1) {
      const unsigned char *row = img + (long long)min(py, H - 1) * W * 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = px0 + j;
        out[j] = (ycc(row + min(2 * x, W - 1) * 3, cm, c) + ycc(row + min(2 * x + 1, W - 1) * 3, cm, c) + (x & 1)) >> 1;
      }
    } else {
      // rows are repeated to an even count before the average and the last averaged row after it
      const int oy = min(py, (H + 1) / 2 - 1);
      const unsigned char *r0 = img + (long long)(2 * oy) * W * 3, *r1 = img + (long long)min(2 * oy + 1, H - 1) * W * 3;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = px0 + j;
        const int x0 = min(2 * x, W - 1) * 3, x1 = min(2 * x + 1, W - 1) * 3;
        out[j] = (ycc(r0 + x0, cm, c) + ycc(r0 + x1, cm, c) + ycc(r1 + x0, cm, c) + ycc(r1 + x1, cm, c) + 1 + (x & 1)) >> 2;
      }
    }
    *reinterpret_cast<unsigned *>(planes + s.coef_offset[c] + (long long)py * pw + px0) =
        (unsigned)out[0] | (unsigned)out[1] << 8 | (unsigned)out[2] << 16 | (unsigned)out[3] << 24;
  }
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of the slow integer forward DCT (include/dspn_jpeg_encode.h), in place; the row pass scales up by 4
template <bool kRows>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int s = kRows ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (kRows) { d[0] = (t10 + t11) * 4; d[4] = (t10 - t11) * 4; }
  else { d[0] = descale(t10 + t11, 2); d[4] = descale(t10 - t11, 2); }
  int z1 = (t12 + t13) * 4433;
  d[2] = descale(z1 + t13 * 6270, s);
  d[6] = descale(z1 - t12 * 15137, s);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = descale(a4 + z1 + z3, s);
  d[5] = descale(a5 + z2 + z4, s);
  d[3] = descale(a6 + z2 + z3, s);
  d[1] = descale(a7 + z1 + z4, s);
}

__global__ __launch_bounds__(kT) void jpeg_enc_fdct_kernel(const unsigned char *__restrict__ planes,
                                                           const dspn_jpeg_enc_sample *__restrict__ samples, int B, Pools pl,
                                                           short *__restrict__ coefs) {
  __shared__ long long first[kMaxB + 1];
  __shared__ int tile[kBlocksPerWg][8][9];          // one block per 8 lanes, rows padded to 9 words
  prefix_units(samples, B, pl, first, [](const dspn_jpeg_enc_sample &s) {
    long long n = 0;
    for (int c = 0; c < s.ncomp; ++c) n += (long long)s.blocks_w[c] * s.blocks_h[c];
    return n;
  });
  const long long total = first[B];
  const int g = threadIdx.x >> 3, t = threadIdx.x & 7;
  for (long long base = (long long)blockIdx.x * kBlocksPerWg; base < total; base += (long long)gridDim.x * kBlocksPerWg) {
    const long long u = base + g;
    const bool live = u < total;
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned qw[2] = {0x01010101u, 0x01010101u};
    short *dst = nullptr;
    if (live) {
      const int b = find_sample(first, B, u);
      const dspn_jpeg_enc_sample &s = samples[b];
      long long l = u - first[b];
      int c = 0;
      for (; c < s.ncomp - 1; ++c) {
        const long long n = (long long)s.blocks_w[c] * s.blocks_h[c];
        if (l < n) break;
        l -= n;
      }
      const int bw = s.blocks_w[c];
      const int by = (int)(l / bw), bx = (int)(l - (long long)by * bw);
      const uint2 raw = *reinterpret_cast<const uint2 *>(planes + s.coef_offset[c] + ((long long)by * 8 + t) * ((long long)bw * 8) + bx * 8);
      const uint2 q = *reinterpret_cast<const uint2 *>(&s.quant[c][t * 8]);
      qw[0] = q.x; qw[1] = q.y;
      const unsigned rw[2] = {raw.x, raw.y};
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (int)((rw[j >> 2] >> (8 * (j & 3))) & 255u) - 128;
      dst = coefs + s.coef_offset[c] + l * 64 + t * 8;
    }
    fdct8<true>(v);                                                 // row t
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[g][t][j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[g][j][t];               // column t of the pass-1 result
    __syncthreads();
    fdct8<false>(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[g][j][t] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[g][t][j];               // row t of the result: natural indices 8 t .. 8 t + 7
    __syncthreads();
    if (live) {
      unsigned o[4];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned q8 = ((qw[j >> 2] >> (8 * (j & 3))) & 255u) << 3;
        q8 = q8 ? q8 : 8u;                                          // a zero in an untrusted table: no division by zero
        const unsigned a = (unsigned)(v[j] < 0 ? -v[j] : v[j]);
        const int m = (int)((a + (q8 >> 1)) / q8);                  // the exact quotient: no reciprocal
        const unsigned h = (unsigned)(v[j] < 0 ? -m : m) & 0xFFFFu;
        if (j & 1) o[j >> 1] |= h << 16; else o[j >> 1] = h;
      }
      *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

}  // namespace

extern "C" int dspn_jpeg_quant_tables(int quality, unsigned char lum[64], unsigned char chr[64]) {
  return dspn_jpeg_enc::quant_tables(quality, lum, chr, dspn::last_error_buf(), 512) ? DSPN_ERR_ARG_ : 0;
}

extern "C" int dspn_jpeg_encode_geometry(dspn_jpeg_enc_sample *s, long long coef_base, long long *coef_count) {
  return dspn_jpeg_enc::fill_geometry(s, coef_base, coef_count, dspn::last_error_buf(), 512) ? DSPN_ERR_ARG_ : 0;
}

extern "C" int dspn_jpeg_entropy_encode(const short *coefs, const dspn_jpeg_enc_sample *s, unsigned char *out, size_t capacity,
                                        size_t *length) {
  return dspn_jpeg_entropy_encode_restart(coefs, s, 0, out, capacity, length);
}

extern "C" int dspn_jpeg_entropy_encode_restart(const short *coefs, const dspn_jpeg_enc_sample *s, int restart_interval,
                                                unsigned char *out, size_t capacity, size_t *length) {
  const int rc = dspn_jpeg_enc::entropy_encode(coefs, s, restart_interval, out, capacity, length, dspn::last_error_buf(), 512);
  return rc == 0 ? 0 : (rc == dspn_jpeg_enc::kTooSmall ? DSPN_ERR_WORKSPACE_ : DSPN_ERR_ARG_);
}

extern "C" size_t dspn_jpeg_encode_workspace_bytes(long long coef_count) {
  return coef_count > 0 ? (size_t)coef_count : 0;
}

extern "C" int dspn_jpeg_encode_blocks_batch_u8(const unsigned char *images, long long images_bytes, const int channel_map[3],
                                                const dspn_jpeg_enc_sample *samples, int B, short *coefs_out, long long coef_count,
                                                void *workspace, size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(images && channel_map && samples && coefs_out && workspace, "jpeg_encode_blocks: null argument");
  DSPN_REQUIRE(B > 0 && B <= kMaxB, "jpeg_encode_blocks: bad batch (0 < B <= %d)", kMaxB);
  DSPN_REQUIRE(coef_count > 0 && coef_count % 64 == 0 && images_bytes > 0, "jpeg_encode_blocks: bad pool sizes");
  bool perm = true;
  for (int i = 0; i < 3; ++i) perm = perm && channel_map[i] >= 0 && channel_map[i] <= 2;
  DSPN_REQUIRE(perm && channel_map[0] != channel_map[1] && channel_map[0] != channel_map[2] && channel_map[1] != channel_map[2],
               "jpeg_encode_blocks: channel_map must be a permutation of 0, 1, 2");
  DSPN_REQUIRE((reinterpret_cast<uintptr_t>(coefs_out) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(samples) & 7) == 0,
               "jpeg_encode_blocks: coefs_out and workspace must be 16-byte aligned, samples 8-byte aligned");
  if (workspace_bytes < dspn_jpeg_encode_workspace_bytes(coef_count))
    return dspn::fail(DSPN_ERR_WORKSPACE_, "jpeg_encode_blocks: workspace of %zu bytes, %zu needed", workspace_bytes,
                      dspn_jpeg_encode_workspace_bytes(coef_count));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Pools pl = {images_bytes, coef_count};
  const ChannelMap cm = {channel_map[0], channel_map[1], channel_map[2]};
  unsigned char *planes = static_cast<unsigned char *>(workspace);
  hipLaunchKernelGGL(jpeg_enc_planes_kernel, dim3(kGrid), dim3(kT), 0, s, images, samples, B, pl, cm, planes);
  hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3(kGrid), dim3(kT), 0, s, planes, samples, B, pl, coefs_out);
  return dspn::check_launch("jpeg_encode_blocks");
}
