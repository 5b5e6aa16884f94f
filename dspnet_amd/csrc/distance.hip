// Box-median selection on disparity maps for MI355X (gfx950); C ABI in include/dspn_distance.h.
//
// box_rank_select_kernel: one workgroup per box, one launch.  The element of rank n / 2 is found by a radix selection
// over an order-preserving unsigned key of the pixel (the value itself for uint16; sign-flipped bits for float32, with
// -0.0 folded onto +0.0 and every NaN onto the largest key), most significant byte first: each pass walks the region
// once, counts the byte of the keys that still match the bytes fixed so far, and a scan of the 256 counts fixes the
// next byte and the rank inside it.  Counts are integers in LDS: the adds commute, the result does not depend on the
// order the pixels arrive in.  The histogram is kept 32 times, bin b of copy c at word b * 32 + c, and a lane adds into
// copy (lane & 31): a lane always uses its own LDS bank, so a region of one repeated value -- the usual content of a box
// on a disparity map -- costs no bank conflict.  Rows are read as 16-byte vectors where the row pitch allows it (every
// row then starts on a 16-byte boundary); the vector's lanes outside [x0, x1) are inside the row and are masked.
//
// distance_boxes: two launches of one workgroup per image.  The first counts the rows an image contributes, the second
// sums the counts of the images before it and writes the rows in order (ballot + popcount within a wave, the wave
// totals through LDS), so the table has the order of the host loop.
#include "dspn_common.h"
#include "../../include/dspn_distance.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kBins = 256;
constexpr int kCopies = 32;

template <typename T> struct Pixel;
template <> struct Pixel<float> {
  static constexpr int kVec = 4, kPasses = 4;
  __device__ static __forceinline__ unsigned key_of_word(const uint4 &v, int e) {
    unsigned u = e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
    return key(u);
  }
  __device__ static __forceinline__ unsigned key_of(const float *p) { return key(__float_as_uint(*p)); }
  __device__ static __forceinline__ unsigned key(unsigned u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;     // NaN: after every number
    if (u == 0x80000000u) u = 0u;                                // -0.0 is +0.0
    return (u >> 31) ? ~u : (u | 0x80000000u);
  }
  __device__ static __forceinline__ float value(unsigned k) {
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
  }
};
template <> struct Pixel<unsigned short> {
  static constexpr int kVec = 8, kPasses = 2;
  __device__ static __forceinline__ unsigned key_of_word(const uint4 &v, int e) {
    const unsigned w = (e >> 1) == 0 ? v.x : (e >> 1) == 1 ? v.y : (e >> 1) == 2 ? v.z : v.w;
    return (e & 1) ? (w >> 16) : (w & 0xffffu);
  }
  __device__ static __forceinline__ unsigned key_of(const unsigned short *p) { return *p; }
  __device__ static __forceinline__ float value(unsigned k) { return (float)k; }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void box_rank_select_kernel(const T *__restrict__ image, int B, int hh, int ww,
                                                                   const int *__restrict__ boxes, int K,
                                                                   const int *__restrict__ count, int vec_rows,
                                                                   float *__restrict__ q, int *__restrict__ n_out) {
  using P = Pixel<T>;
  __shared__ __attribute__((aligned(16))) unsigned hist[kBins * kCopies];
  __shared__ __attribute__((aligned(16))) unsigned cnt[kBins];
  __shared__ unsigned sel[2];
  const int k = blockIdx.x, tid = threadIdx.x;
  if (k >= K || (count && k >= *count)) return;
  const int b = boxes[k * 5], x0 = boxes[k * 5 + 1], x1 = boxes[k * 5 + 2], y0 = boxes[k * 5 + 3], y1 = boxes[k * 5 + 4];
  const bool inside = b >= 0 && b < B && x0 >= 0 && x0 <= x1 && x1 <= ww && y0 >= 0 && y0 <= y1 && y1 <= hh;
  const int w = inside ? x1 - x0 : 0, rows = inside ? y1 - y0 : 0;
  const int n = w * rows;                                      // <= hh * ww < 2^31
  if (n == 0) {
    if (tid == 0) { q[k] = 0.f; n_out[k] = 0; }
    return;
  }
  const T *img = image + (size_t)b * hh * ww + (size_t)y0 * ww;
  const int copy = tid & (kCopies - 1);
  // the vector form: whole 16-byte groups [a0, a1) of every row, a1 <= ww because ww is a multiple of the group
  const int a0 = x0 & ~(P::kVec - 1), nvec = ((x1 + P::kVec - 1) & ~(P::kVec - 1)) / P::kVec - a0 / P::kVec;
  unsigned prefix = 0, mask = 0, rank = (unsigned)n >> 1;
  for (int pass = 0; pass < P::kPasses; ++pass) {
    const int shift = (P::kPasses - 1 - pass) * 8;
    for (int i = tid; i < kBins * kCopies; i += kThreads) hist[i] = 0;
    __syncthreads();
    if (vec_rows) {
      const int total = rows * nvec;
      for (int i = tid; i < total; i += kThreads) {
        const int r = i / nvec, xs = a0 + (i - r * nvec) * P::kVec;
        const uint4 v = *reinterpret_cast<const uint4 *>(img + (size_t)r * ww + xs);
#pragma unroll
        for (int e = 0; e < P::kVec; ++e) {
          const unsigned key = P::key_of_word(v, e);
          if (xs + e >= x0 && xs + e < x1 && (key & mask) == prefix)
            atomicAdd(&hist[((key >> shift) & 255u) * kCopies + copy], 1u);
        }
      }
    } else {
      for (int i = tid; i < n; i += kThreads) {
        const int r = i / w;
        const unsigned key = P::key_of(img + (size_t)r * ww + x0 + (i - r * w));
        if ((key & mask) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * kCopies + copy], 1u);
      }
    }
    __syncthreads();
    if (tid < kBins) {
      unsigned s = 0;
#pragma unroll 8
      for (int j = 0; j < kCopies; ++j) s += hist[tid * kCopies + ((j + tid) & (kCopies - 1))];   // rotated: one bank per lane
      cnt[tid] = s;
    }
    __syncthreads();
    if (tid < 64) {                                            // wave 0: 4 bins per lane, inclusive scan over the lanes
      const uint4 c = *reinterpret_cast<const uint4 *>(&cnt[tid * 4]);
      const unsigned tot = c.x + c.y + c.z + c.w;
      unsigned incl = tot;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (tid >= off) incl += t;
      }
      const unsigned excl = incl - tot;
      if (rank >= excl && rank < incl) {                       // exactly one lane: the counts add up to more than rank
        unsigned r = rank - excl, d = tid * 4;
        if (r >= c.x) { r -= c.x; ++d; if (r >= c.y) { r -= c.y; ++d; if (r >= c.z) { r -= c.z; ++d; } } }
        sel[0] = d; sel[1] = r;
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 255u << shift;
    rank = sel[1];
  }
  if (tid == 0) { q[k] = P::value(prefix); n_out[k] = n; }
}

// the numpy slice [start:stop] of an axis of `size` elements -> [lo, hi), hi == lo when it is empty
__device__ __forceinline__ void slice_bounds(long long start, long long stop, int size, int &lo, int &hi) {
  long long s = start < 0 ? start + size : start, e = stop < 0 ? stop + size : stop;
  s = s < 0 ? 0 : (s > size ? size : s);
  e = e < 0 ? 0 : (e > size ? size : e);
  lo = (int)s;
  hi = (int)(e < s ? s : e);
}

__device__ __forceinline__ bool row_selected(const float *row, float score_thresh) {
  return row[0] >= 0.f && row[1] > score_thresh;
}

// counts[b]: mode 0 -- the index of the first row with id < 0 (N when there is none); mode 1 -- the rows selected
__global__ __launch_bounds__(kThreads) void distance_count_kernel(const float *__restrict__ det, int N, float score_thresh,
                                                                  int mode, int *__restrict__ counts) {
  __shared__ int acc;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) acc = mode == 0 ? N : 0;
  __syncthreads();
  const float *d = det + (size_t)b * N * 7;
  int mine = mode == 0 ? N : 0;
  for (int r = tid; r < N; r += kThreads) {
    if (mode == 0) { if (d[(size_t)r * 7] < 0.f && r < mine) mine = r; }
    else if (row_selected(d + (size_t)r * 7, score_thresh)) ++mine;
  }
  if (mode == 0) { if (mine < N) atomicMin(&acc, mine); }
  else if (mine) atomicAdd(&acc, mine);
  __syncthreads();
  if (tid == 0) counts[b] = acc;
}

__global__ __launch_bounds__(kThreads) void distance_emit_kernel(const float *__restrict__ det, int B, int N, int hh, int ww,
                                                                 float score_thresh, int mode, int max_boxes,
                                                                 const int *__restrict__ counts, int *__restrict__ boxes,
                                                                 int *__restrict__ src, int *__restrict__ count) {
  __shared__ int wave_tot[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long before = 0;
  for (int i = 0; i < b; ++i) before += counts[i];
  if (b == B - 1 && tid == 0) {
    const long long all = before + counts[b];
    *count = all > 0x7fffffffLL ? 0x7fffffff : (int)all;
  }
  const int limit = mode == 0 ? counts[b] : N;                 // mode 0: every row before the first id < 0
  const float *d = det + (size_t)b * N * 7;
  const float fw = (float)ww, fh = (float)hh;
  long long pos0 = before;
  for (int base = 0; base < limit && pos0 < max_boxes; base += kThreads) {
    const int r = base + tid;
    const bool take = r < limit && (mode == 0 || row_selected(d + (size_t)r * 7, score_thresh));
    const unsigned long long bal = __ballot(take);
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int ahead = 0, all = 0;
    for (int i = 0; i < kThreads / 64; ++i) { const int t = wave_tot[i]; all += t; if (i < wave) ahead += t; }
    const long long pos = pos0 + ahead + __popcll(bal & ((1ull << lane) - 1ull));
    if (take && pos < max_boxes) {
      const float *row = d + (size_t)r * 7;
      long long x0 = __float2int_rz(row[2] * fw), x1 = __float2int_rz(row[4] * fw);
      long long y0 = __float2int_rz(row[3] * fh), y1 = __float2int_rz(row[5] * fh);
      x0 = x0 < 0 ? 0 : x0;
      y0 = y0 < 0 ? 0 : y0;
      if (x0 == x1) x1 = x0 + 1;
      int *o = boxes + pos * 5;
      o[0] = b;
      slice_bounds(x0, x1, ww, o[1], o[2]);
      slice_bounds(y0, y1, hh, o[3], o[4]);
      src[pos] = b * N + r;
    }
    pos0 += all;
    __syncthreads();
  }
}

template <typename T>
int box_rank_select(const T *image, int B, int hh, int ww, const int *boxes, int K, const int *count, float *q, int *n,
                    void *stream, const char *what) {
  DSPN_REQUIRE(K >= 0, "%s: K < 0", what);
  DSPN_REQUIRE(B > 0 && hh > 0 && ww > 0, "%s: B, hh and ww must be > 0", what);
  DSPN_REQUIRE((long long)hh * ww < (1LL << 31), "%s: hh * ww must stay below 2^31", what);
  if (K == 0) return 0;
  DSPN_REQUIRE(image && boxes && q && n, "%s: null pointer", what);
  const int vec_rows = ww % Pixel<T>::kVec == 0 && reinterpret_cast<size_t>(image) % 16 == 0;
  hipLaunchKernelGGL(box_rank_select_kernel<T>, dim3(K), dim3(kThreads), 0, (hipStream_t)stream, image, B, hh, ww, boxes,
                     K, count, vec_rows, q, n);
  return dspn::check_launch(what);
}

}  // namespace

extern "C" {

int dspn_box_rank_select_f32(const float *image_dev, int B, int hh, int ww, const int *boxes_dev, int K,
                             const int *count_dev, float *q_dev, int *n_dev, void *stream) {
  return box_rank_select(image_dev, B, hh, ww, boxes_dev, K, count_dev, q_dev, n_dev, stream, "box_rank_select_f32");
}

int dspn_box_rank_select_u16(const unsigned short *image_dev, int B, int hh, int ww, const int *boxes_dev, int K,
                             const int *count_dev, float *q_dev, int *n_dev, void *stream) {
  return box_rank_select(image_dev, B, hh, ww, boxes_dev, K, count_dev, q_dev, n_dev, stream, "box_rank_select_u16");
}

size_t dspn_distance_boxes_workspace_bytes(int B) { return B > 0 ? sizeof(int) * (size_t)B : 0; }

int dspn_distance_boxes_f32(const float *det_dev, int B, int N, int hh, int ww, float score_thresh, int mode,
                            int max_boxes, int *boxes_dev, int *src_dev, int *count_dev, void *workspace,
                            size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(B >= 0 && N >= 0 && max_boxes >= 0, "distance_boxes: negative count");
  DSPN_REQUIRE((long long)B * N < (1LL << 31), "distance_boxes: B * N must stay below 2^31");
  DSPN_REQUIRE(hh > 0 && ww > 0, "distance_boxes: hh and ww must be > 0");
  DSPN_REQUIRE(mode == 0 || mode == 1, "distance_boxes: mode is 0 (rows before the first id < 0) or 1 (id >= 0 and score > score_thresh)");
  DSPN_REQUIRE(count_dev, "distance_boxes: null count pointer");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0 || N == 0) {
    const hipError_t e = hipMemsetAsync(count_dev, 0, sizeof(int), s);
    if (e != hipSuccess) return dspn::fail(DSPN_ERR_LAUNCH_, "distance_boxes: %s", hipGetErrorString(e));
    return 0;
  }
  DSPN_REQUIRE(det_dev && (max_boxes == 0 || (boxes_dev && src_dev)), "distance_boxes: null pointer");
  if (!workspace || workspace_bytes < dspn_distance_boxes_workspace_bytes(B))
    return dspn::fail(DSPN_ERR_WORKSPACE_, "distance_boxes: workspace too small");
  int *counts = static_cast<int *>(workspace);
  hipLaunchKernelGGL(distance_count_kernel, dim3(B), dim3(kThreads), 0, s, det_dev, N, score_thresh, mode, counts);
  hipLaunchKernelGGL(distance_emit_kernel, dim3(B), dim3(kThreads), 0, s, det_dev, B, N, hh, ww, score_thresh, mode,
                     max_boxes, counts, boxes_dev, src_dev, count_dev);
  return dspn::check_launch("distance_boxes");
}

}  // extern "C"
