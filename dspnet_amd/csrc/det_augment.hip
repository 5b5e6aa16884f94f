// Batch image pipeline of the detection iterator for MI355X (gfx950); C ABI and the arithmetic contract in
// include/dspn_det_augment.h.  One kernel on the caller's stream covering the whole batch:
//   det_augment_kernel : window (crop, or zoom-out padding with a fill value) + separable fixed-point resize over the
//                        host's tap tables + mirror + mean subtraction, uint8 HWC source -> float32 planes.
// A workgroup per (strip of kT pixels of one output row, sample), one thread per output pixel: consecutive lanes write
// consecutive floats of each plane (coalesced 256-B stores), as augment_image_kernel does.  The row's ky taps (first
// index and coefficients) depend on (blockIdx.y, blockIdx.z) only, so they are uniform across the workgroup; a row tap
// whose coefficient is zero (the padding of short area rows) is skipped by all of it without divergence.  The
// strip's x coefficients are read ky times by every thread: with more than two taps they are staged once in LDS,
// transposed to [tap][pixel] so that the lanes of a wave read consecutive int16 (no bank conflicts; the row-major layout
// of the table would put all lanes of a 64-tap table on one bank).
// HBM/L2-bound byte work (neighbouring pixels share their source bytes through L1/L2); nothing here is shaped for the
// matrix cores.  The one case with real arithmetic, area rows at large shrink factors (up to 64 x 64 taps per pixel),
// runs through the same loop: there is one variant, so there is one set of integers.
#include "dspn_common.h"
#include "../../include/dspn_det_augment.h"

namespace {

constexpr int kT = 256;
constexpr int kMaxTaps = 64;                                   // what the LDS tile holds; more taps read the table itself

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(kT) void det_augment_kernel(const unsigned char *__restrict__ images,
                                                         const dspn_det_sample *__restrict__ samples,
                                                         const int *__restrict__ tables, int H, int W, double mean0,
                                                         double mean1, double mean2, float *__restrict__ out) {
  __shared__ short cx_lds[kMaxTaps * kT];                      // [tap][pixel of the strip]
  const int b = blockIdx.z, y = blockIdx.y;
  const int xs = blockIdx.x * kT;                              // the strip is output columns [xs, xe)
  const int xe = min(xs + kT, W);
  const int x = xs + threadIdx.x;
  const bool live = x < W;
  const dspn_det_sample s = samples[b];
  const int kx = s.kx, ky = s.ky;
  const int *fxs = tables + s.xtab;
  const short *cxs = reinterpret_cast<const short *>(fxs + W);
  const int *fys = tables + s.ytab;
  const short *cys = reinterpret_cast<const short *>(fys + H) + (long long)y * ky;
  // columns of the unmirrored resize this strip covers: [lo, lo + (xe - xs)), still contiguous under the mirror
  const int lo = s.mirror ? W - xe : xs;
  const int xd = s.mirror ? W - 1 - x : x;
  const int t = xd - lo;                                       // 0 .. kT - 1 for a live thread
  const bool staged = kx > 2 && kx <= kMaxTaps;
  if (staged) {
    const int count = (xe - xs) * kx;
    const short *from = cxs + (long long)lo * kx;
    for (int e = threadIdx.x; e < count; e += kT) {
      const int d = e / kx;
      cx_lds[(e - d * kx) * kT + d] = from[e];
    }
    __syncthreads();
  }
  if (!live) return;
  const int fx = fxs[xd], fy = fys[y];
  const short *cx = cxs + (long long)xd * kx;
  const unsigned char *src = images + s.img_offset;
  const int cw1 = s.canvas_w - 1, ch1 = s.canvas_h - 1;
  long long acc0 = 0, acc1 = 0, acc2 = 0;                      // 255 * sum|qx| * sum|qy| passes 2^31 for cubic and lanczos rows
  for (int j = 0; j < ky; ++j) {
    const int qy = cys[j];
    if (qy == 0) continue;                                     // uniform across the workgroup
    const int iy = s.y0 + clampi(fy + j, ch1);
    const bool row_in = (unsigned)iy < (unsigned)s.src_h;
    const unsigned char *row = src + (long long)iy * s.src_w * 3;
    int r0 = 0, r1 = 0, r2 = 0;                                // |sum| <= 255 * sum|qx| <= 255 * 32768 * 64 < 2^31 at kx <= 64
    for (int i = 0; i < kx; ++i) {
      const int qx = staged ? cx_lds[i * kT + t] : cx[i];
      const int ix = s.x0 + clampi(fx + i, cw1);
      int p0 = s.fill, p1 = s.fill, p2 = s.fill;
      if (row_in && (unsigned)ix < (unsigned)s.src_w) {
        const unsigned char *p = row + (long long)ix * 3;
        p0 = p[0]; p1 = p[1]; p2 = p[2];
      }
      r0 += qx * p0; r1 += qx * p1; r2 += qx * p2;
    }
    acc0 += (long long)qy * r0; acc1 += (long long)qy * r1; acc2 += (long long)qy * r2;
  }
  const long long plane = (long long)H * W;
  float *o = out + (long long)b * 3 * plane + (long long)y * W + x;
  const long long acc[3] = {acc0, acc1, acc2};
  const double mean[3] = {mean0, mean1, mean2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    long long v = (acc[c] + (1ll << 21)) >> 22;                // arithmetic shift
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    o[c * plane] = (float)((double)v - mean[c]);
  }
}

}  // namespace

extern "C" int dspn_det_augment_batch_u8(const unsigned char *images, const dspn_det_sample *samples, const int *tables,
                                         int B, int H, int W, const double mean[3], float *data_out, void *stream) {
  DSPN_REQUIRE(images && samples && tables && mean && data_out, "det_augment_batch: null argument");
  DSPN_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && W > 0 && W <= (1 << 24),
               "det_augment_batch: bad shape (0 < B, H <= 65535; 0 < W <= 2^24)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(det_augment_kernel, dim3(dspn::cdiv(W, kT), H, B), dim3(kT), 0, s, images, samples, tables, H, W,
                     mean[0], mean[1], mean[2], data_out);
  return dspn::check_launch("det_augment_batch");
}
