// Element-wise, layout, loss and optimizer kernels on float tensors only (loss inputs, parameters, optimizer state), so
// compiled once (dspn_store.h), not twinned like nn.hip.  C ABI in include/dspn_nn.h.
#include "dspn_common.h"
#include "nn_launch.h"
#include "../../include/dspn_nn.h"

#pragma clang fp contract(fast)   // as nn.hip: the loss and SGD arithmetic keeps its bits

namespace {

// ------------------------------------------------------------------ element-wise and layout
__global__ void fill_kernel(float *p, float v, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    p[i] = v;
}
__global__ void nhwc_to_nchw_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                    int C, long long HW, long long total, int Cp) {
  // thread per dst element, hw fastest
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long hw = i % HW, nc = i / HW;
    const long long n = nc / C; const int c = (int)(nc - n * C);
    dst[i] = src[(n * HW + hw) * Cp + c];
  }
}
// many block copies in ONE launch (the SSD head packing: six small maps per pass): rows sorted by `begin`, the first
// element of the row's range in the launch's flat index space, found by binary search (as slab_reduce_batch_kernel)
struct CopyDesc { const float *src; float *dst; long long rows_per_sample, sss, dss; int C, lds, soff, ldd, doff, accumulate; long long begin; };
static_assert(sizeof(CopyDesc) == 72, "copy_block_batch table row (dspnet_amd/functional.py copy_block_table)");
__global__ void copy_block_batch_kernel(const CopyDesc *__restrict__ d, int n, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (d[mid].begin <= i) lo = mid; else hi = mid - 1;
    }
    const CopyDesc e = d[lo];
    const long long j = i - e.begin;
    const int c = (int)(j % e.C);
    const long long r = j / e.C;
    const long long sm = r / e.rows_per_sample, rr = r - sm * e.rows_per_sample;
    const float v = e.src[sm * e.sss + rr * e.lds + e.soff + c];
    const long long di = sm * e.dss + rr * e.ldd + e.doff + c;
    e.dst[di] = e.accumulate ? e.dst[di] + v : v;
  }
}
__global__ void transpose_bnc_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                     int N, int C, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(i % N);
    const long long bc = i / N;
    const int c = (int)(bc % C);
    const long long b = bc / C;
    dst[i] = src[(b * N + n) * C + c];
  }
}

// ------------------------------------------------------------------ losses
__global__ void count_kernel(const float *__restrict__ a, long long n, int mode, float ref, float *out) {
  float c = 0.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    c += (mode == 0 ? (a[i] != ref) : (a[i] > ref)) ? 1.f : 0.f;
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  // integer-valued float adds below 2^24 are exact, hence order independent
  if ((threadIdx.x & 63) == 0 && c != 0.f) atomicAdd(out, c);
}
__device__ __forceinline__ float smooth_l1(float x) {
  const float ax = fabsf(x);
  return ax < 1.f ? 0.5f * x * x : ax - 0.5f;
}
__global__ void smooth_l1_fwd_kernel(const float *pred, const float *target, const float *mask,
                                     float *loss, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    loss[i] = smooth_l1(mask[i] * (pred[i] - target[i]));
}
__global__ void smooth_l1_bwd_kernel(const float *pred, const float *target, const float *mask,
                                     float *grad, long long n, float grad_scale, const float *valid_count) {
  const float sc = grad_scale / fmaxf(1.f, *valid_count);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float m = mask[i];
    const float x = m * (pred[i] - target[i]);
    const float d = fabsf(x) < 1.f ? x : (x > 0.f ? 1.f : -1.f);
    grad[i] = sc * m * d;
  }
}
// single-block deterministic reductions for the (tiny) metric readouts
__global__ __launch_bounds__(1024) void ce_sum_kernel(const float *prob, const float *label, long long rows,
                                                      int C, int ld, float ignore_label, float eps,
                                                      float *out2) {
  __shared__ double s_a[1024];
  __shared__ double s_b[1024];
  double a = 0, b = 0;
  for (long long r = threadIdx.x; r < rows; r += 1024) {
    const float lab = label[r];
    if (lab == ignore_label) continue;
    const int li = (int)lab;
    if (li < 0 || li >= C) continue;
    a += -log((double)(prob[r * ld + li] + eps));
    b += 1.0;
  }
  s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
  __syncthreads();
  for (int s = 512; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) { s_a[threadIdx.x] += s_a[threadIdx.x + s]; s_b[threadIdx.x] += s_b[threadIdx.x + s]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out2[0] = (float)s_a[0]; out2[1] = (float)s_b[0]; }
}
__global__ __launch_bounds__(1024) void sum_kernel(const float *a, long long n, float *out) {
  __shared__ double s_a[1024];
  double v = 0;
  for (long long i = threadIdx.x; i < n; i += 1024) v += a[i];
  s_a[threadIdx.x] = v;
  __syncthreads();
  for (int s = 512; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) s_a[threadIdx.x] += s_a[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)s_a[0];
}

__global__ void sgd_kernel(float4 *__restrict__ w, const float4 *__restrict__ g, float4 *__restrict__ m,
                           long long n4, float lr, float mu, float wd, float rescale) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
       i += (long long)gridDim.x * blockDim.x) {
    float4 wv = w[i]; const float4 gv = g[i]; float4 mv = m[i];
    mv.x = mu * mv.x - lr * (rescale * gv.x + wd * wv.x); wv.x += mv.x;
    mv.y = mu * mv.y - lr * (rescale * gv.y + wd * wv.y); wv.y += mv.y;
    mv.z = mu * mv.z - lr * (rescale * gv.z + wd * wv.z); wv.z += mv.z;
    mv.w = mu * mv.w - lr * (rescale * gv.w + wd * wv.w); wv.w += mv.w;
    w[i] = wv; m[i] = mv;
  }
}

// Segmented SGD (dspn_sgd_momentum_segments_f32): the rows of `seg` cover disjoint, sorted float4 ranges of the arena; the
// launch walks the CONCATENATION of those ranges (total4 float4 in all).  Every block first forms the inclusive prefix of the
// row lengths in LDS (one scan of nseg values), then each thread finds the row of its first float4 by binary search and
// follows the rows forward.  Elements outside every row are never touched.  Per element the arithmetic is sgd_kernel's with
// lr * lr_mult and wd * wd_mult formed in float32 (multipliers 1.0 give sgd_kernel's bits).
constexpr int kSgdPer = 8;                // float4 per thread: one block covers kT * kSgdPer consecutive float4 of the rows
__global__ void __launch_bounds__(kT) sgd_segments_kernel(float4 *__restrict__ w, const float4 *__restrict__ g,
                                                          float4 *__restrict__ m, const dspn_sgd_segment *__restrict__ seg,
                                                          int nseg, long long total4, float lr, float mu, float wd,
                                                          float rescale) {
  extern __shared__ long long s_end[];    // s_end[r] = float4 in rows 0 .. r (inclusive prefix)
  __shared__ long long s_part[kT];
  const int t = threadIdx.x;
  const int per = (nseg + kT - 1) / kT;   // rows per thread in the scan
  long long acc = 0;
  for (int r = t * per; r < nseg && r < (t + 1) * per; ++r) { acc += seg[r].length >> 2; s_end[r] = acc; }
  s_part[t] = acc;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {     // inclusive scan of the per-thread sums (Hillis-Steele)
    const long long v = t >= d ? s_part[t - d] : 0;
    __syncthreads();
    s_part[t] += v;
    __syncthreads();
  }
  const long long before = t > 0 ? s_part[t - 1] : 0;
  for (int r = t * per; r < nseg && r < (t + 1) * per; ++r) s_end[r] += before;
  __syncthreads();
  const long long base = (long long)blockIdx.x * (kT * kSgdPer);
  long long j = base + t;
  if (j >= total4) return;
  int lo = 0, hi = nseg - 1;              // the first row whose end lies beyond j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_end[mid] > j) hi = mid; else lo = mid + 1;
  }
  int r = lo;
  for (int it = 0; it < kSgdPer && j < total4; ++it, j += kT) {
    while (r < nseg && s_end[r] <= j) ++r;
    if (r == nseg) return;                // (total4 larger than the rows hold: the rest is not ours to touch)
    const dspn_sgd_segment sr = seg[r];
    const float lre = lr * sr.lr_mult, wde = wd * sr.wd_mult;
    const long long i = (sr.offset >> 2) + (j - (s_end[r] - (sr.length >> 2)));
    float4 wv = w[i]; const float4 gv = g[i]; float4 mv = m[i];
    mv.x = mu * mv.x - lre * (rescale * gv.x + wde * wv.x); wv.x += mv.x;
    mv.y = mu * mv.y - lre * (rescale * gv.y + wde * wv.y); wv.y += mv.y;
    mv.z = mu * mv.z - lre * (rescale * gv.z + wde * wv.z); wv.z += mv.z;
    mv.w = mu * mv.w - lre * (rescale * gv.w + wde * wv.w); wv.w += mv.w;
    w[i] = wv; m[i] = mv;
  }
}

}  // namespace

extern "C" {

int dspn_fill_f32(float *p, float v, long long n, void *stream) {
  DSPN_REQUIRE(p && n >= 0, "fill: bad argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(kT), 0, S_(stream), p, v, n);
  return dspn::check_launch("fill");
}

int dspn_nhwc_to_nchw_f32(const float *src, float *dst, int N, int C, int H, int W, int Cp, void *stream) {
  DSPN_REQUIRE(src && dst && N > 0 && C > 0 && H > 0 && W > 0 && Cp >= C, "nhwc_to_nchw: bad argument");
  const long long HW = (long long)H * W, total = HW * N * C;
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for(total)), dim3(kT), 0, S_(stream), src, dst, C, HW, total, Cp);
  return dspn::check_launch("nhwc_to_nchw");
}

int dspn_copy_block_batch_f32(const void *table, int n, long long total, void *stream) {
  DSPN_REQUIRE(table && n > 0 && total > 0, "copy_block_batch: bad argument");
  hipLaunchKernelGGL(copy_block_batch_kernel, dim3(grid_for(total)), dim3(kT), 0, S_(stream),
                     static_cast<const CopyDesc *>(table), n, total);
  return dspn::check_launch("copy_block_batch");
}

int dspn_transpose_bnc_f32(const float *src, float *dst, int B, int N, int C, void *stream) {
  DSPN_REQUIRE(src && dst && B > 0 && N > 0 && C > 0, "transpose_bnc: bad argument");
  const long long total = (long long)B * N * C;
  hipLaunchKernelGGL(transpose_bnc_kernel, dim3(grid_for(total)), dim3(kT), 0, S_(stream), src, dst, N, C, total);
  return dspn::check_launch("transpose_bnc");
}

int dspn_count_f32(const float *a, long long n, int mode, float ref, float *out, void *stream) {
  DSPN_REQUIRE(a && out && n > 0 && n < (1ll << 24), "count: n must be in (0, 2^24)");
  hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(64), 0, S_(stream), out, 0.f, 1ll);
  hipLaunchKernelGGL(count_kernel, dim3(grid_for(n, kT, 1024)), dim3(kT), 0, S_(stream), a, n, mode, ref, out);
  return dspn::check_launch("count");
}
int dspn_smooth_l1_forward_f32(const float *pred, const float *target, const float *mask, float *loss,
                               long long n, void *stream) {
  DSPN_REQUIRE(pred && target && mask && loss && n > 0, "smooth_l1_forward: bad argument");
  hipLaunchKernelGGL(smooth_l1_fwd_kernel, dim3(grid_for(n)), dim3(kT), 0, S_(stream), pred, target, mask, loss, n);
  return dspn::check_launch("smooth_l1_forward");
}
int dspn_smooth_l1_backward_f32(const float *pred, const float *target, const float *mask, float *grad,
                                long long n, float grad_scale, const float *valid_count, void *stream) {
  DSPN_REQUIRE(pred && target && mask && grad && valid_count && n > 0, "smooth_l1_backward: bad argument");
  hipLaunchKernelGGL(smooth_l1_bwd_kernel, dim3(grid_for(n)), dim3(kT), 0, S_(stream), pred, target, mask, grad,
                     n, grad_scale, valid_count);
  return dspn::check_launch("smooth_l1_backward");
}
int dspn_cross_entropy_sum_f32(const float *prob, const float *label, long long rows, int C, int ld,
                               float ignore_label, float eps, float *out2, void *stream) {
  DSPN_REQUIRE(prob && label && out2 && rows > 0 && C > 0 && ld >= C, "cross_entropy_sum: bad argument");
  hipLaunchKernelGGL(ce_sum_kernel, dim3(1), dim3(1024), 0, S_(stream), prob, label, rows, C, ld, ignore_label, eps, out2);
  return dspn::check_launch("cross_entropy_sum");
}
int dspn_sum_f32(const float *a, long long n, float *out, void *stream) {
  DSPN_REQUIRE(a && out && n > 0, "sum: bad argument");
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, S_(stream), a, n, out);
  return dspn::check_launch("sum");
}

int dspn_sgd_momentum_f32(float *w, const float *grad, float *mom, long long n, float lr, float momentum,
                          float wd, float rescale, void *stream) {
  DSPN_REQUIRE(w && grad && mom && n > 0 && n % 4 == 0, "sgd_momentum: n must be a positive multiple of 4");
  hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n / 4)), dim3(kT), 0, S_(stream), reinterpret_cast<float4 *>(w),
                     reinterpret_cast<const float4 *>(grad), reinterpret_cast<float4 *>(mom), n / 4, lr,
                     momentum, wd, rescale);
  return dspn::check_launch("sgd_momentum");
}

int dspn_sgd_momentum_segments_f32(float *w, const float *grad, float *mom, const dspn_sgd_segment *segments, int nseg,
                                   long long total4, float lr, float momentum, float wd, float rescale, void *stream) {
  DSPN_REQUIRE(w && grad && mom && segments && nseg > 0 && nseg <= DSPN_SGD_MAX_SEGMENTS && total4 > 0,
               "sgd_momentum_segments: need w, grad, mom, a segment table of 1 .. DSPN_SGD_MAX_SEGMENTS rows and total4 > 0");
  const long long blocks = (total4 + (long long)kT * kSgdPer - 1) / ((long long)kT * kSgdPer);
  DSPN_REQUIRE(blocks <= 0x7fffffffLL, "sgd_momentum_segments: total4 too large");
  hipLaunchKernelGGL(sgd_segments_kernel, dim3((unsigned)blocks), dim3(kT), sizeof(long long) * (size_t)nseg, S_(stream),
                     reinterpret_cast<float4 *>(w), reinterpret_cast<const float4 *>(grad), reinterpret_cast<float4 *>(mom),
                     segments, nseg, total4, lr, momentum, wd, rescale);
  return dspn::check_launch("sgd_momentum_segments");
}

}  // extern "C"
