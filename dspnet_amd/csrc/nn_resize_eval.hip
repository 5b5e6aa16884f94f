// Plain resize (identity grid) and the evaluation read-outs: float tensors only, so compiled once (dspn_store.h), not
// twinned like nn.hip.  C ABI in include/dspn_nn.h.
#include "dspn_common.h"
#include "nn_launch.h"
#include "../../include/dspn_nn.h"

#pragma clang fp contract(fast)   // as nn.hip: sampler.hip reproduces this file's resize kernel bit for bit

namespace {

// ------------------------------------------------------------------ bilinear sampler
// GridGenerator(affine identity, target (Ho,Wo)) + BilinearSampler: normalised target coordinate
// g = -1 + o*2/(O-1); source coordinate s = (g+1)*(I-1)/2; corners outside [0,I-1] contribute 0.
__device__ __forceinline__ float src_coord(int o, int O, int I) {
  const float g = O > 1 ? -1.f + (float)o * (2.f / (float)(O - 1)) : 0.f;
  return (g + 1.f) * (float)(I - 1) / 2.f;
}
template <bool ACC>   // ACC: y += resize(x) (sum of several resized maps in a fixed order)
__global__ void bilinear_fwd_kernel(const float4 *__restrict__ x, float *__restrict__ y, int Hin,
                                    int Win, int C4, int Ho, int Wo, int ldo, int coff, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    long long t = i / C4;
    const int wo = (int)(t % Wo); t /= Wo;
    const int ho = (int)(t % Ho);
    const long long n = t / Ho;
    const float ys = src_coord(ho, Ho, Hin), xs = src_coord(wo, Wo, Win);
    const int y0 = (int)floorf(ys), x0 = (int)floorf(xs);
    const float wy0 = 1.f - (ys - (float)y0), wx0 = 1.f - (xs - (float)x0);
    float4 acc = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int dyy = 0; dyy < 2; ++dyy)
#pragma unroll
      for (int dxx = 0; dxx < 2; ++dxx) {
        const int yy = y0 + dyy, xx = x0 + dxx;
        if ((unsigned)yy >= (unsigned)Hin || (unsigned)xx >= (unsigned)Win) continue;
        const float wgt = (dyy ? 1.f - wy0 : wy0) * (dxx ? 1.f - wx0 : wx0);
        const float4 v = x[((n * Hin + yy) * Win + xx) * C4 + c4];
        acc.x += wgt * v.x; acc.y += wgt * v.y; acc.z += wgt * v.z; acc.w += wgt * v.w;
      }
    float4 *o = reinterpret_cast<float4 *>(y + ((n * Ho + ho) * Wo + wo) * (long long)ldo + coff + c4 * 4);
    if (ACC) { const float4 p = *o; acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w; }
    *o = acc;
  }
}
// gather form of the backward: every source pixel collects from the target pixels that touch it
__global__ void bilinear_bwd_kernel(const float *__restrict__ dy, float4 *__restrict__ dx, int Hin,
                                    int Win, int C4, int Ho, int Wo, int ldo, int coff, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    long long t = i / C4;
    const int w = (int)(t % Win); t /= Win;
    const int h = (int)(t % Hin);
    const long long n = t / Hin;
    // candidate target range: |s(o) - h| < 1  (s is monotone in o); widen by one and test exactly
    const float sy = Hin > 1 ? (float)(Ho - 1) / (float)(Hin - 1) : 0.f;
    const float sx = Win > 1 ? (float)(Wo - 1) / (float)(Win - 1) : 0.f;
    int ho_lo = Hin > 1 ? (int)floorf((float)(h - 1) * sy) - 1 : 0;
    int ho_hi = Hin > 1 ? (int)ceilf((float)(h + 1) * sy) + 1 : Ho - 1;
    int wo_lo = Win > 1 ? (int)floorf((float)(w - 1) * sx) - 1 : 0;
    int wo_hi = Win > 1 ? (int)ceilf((float)(w + 1) * sx) + 1 : Wo - 1;
    ho_lo = max(ho_lo, 0); wo_lo = max(wo_lo, 0); ho_hi = min(ho_hi, Ho - 1); wo_hi = min(wo_hi, Wo - 1);
    float4 acc = make_float4(0, 0, 0, 0);
    for (int ho = ho_lo; ho <= ho_hi; ++ho) {
      const float ys = src_coord(ho, Ho, Hin);
      const int y0 = (int)floorf(ys);
      float wy;
      if (y0 == h) wy = 1.f - (ys - (float)y0);
      else if (y0 + 1 == h) wy = ys - (float)y0;
      else continue;
      for (int wo = wo_lo; wo <= wo_hi; ++wo) {
        const float xs = src_coord(wo, Wo, Win);
        const int x0 = (int)floorf(xs);
        float wx;
        if (x0 == w) wx = 1.f - (xs - (float)x0);
        else if (x0 + 1 == w) wx = xs - (float)x0;
        else continue;
        const float wgt = wy * wx;
        const float4 v = *reinterpret_cast<const float4 *>(
            dy + ((n * Ho + ho) * Wo + wo) * (long long)ldo + coff + c4 * 4);
        acc.x += wgt * v.x; acc.y += wgt * v.y; acc.z += wgt * v.z; acc.w += wgt * v.w;
      }
    }
    dx[i] = acc;
  }
}

// Separable form of the same backward pass (the bilinear weights factor into wy * wx): first along W into a
// (N, Ho, Win, C) scratch tensor, then along H.  A source pixel of a map upsampled by s collects from ~2s targets per
// pass instead of ~(2s)^2 (the 4x4 pyramid level upsampled to 64x64: 84 loads instead of 1764), and the first pass
// has N*Ho*Win*C/4 threads however small the source map is.
__device__ __forceinline__ void bl_range(int i, int I, int O, int &lo, int &hi) {
  const float s = I > 1 ? (float)(O - 1) / (float)(I - 1) : 0.f;
  lo = I > 1 ? (int)floorf((float)(i - 1) * s) - 1 : 0;
  hi = I > 1 ? (int)ceilf((float)(i + 1) * s) + 1 : O - 1;
  lo = max(lo, 0); hi = min(hi, O - 1);
}
__device__ __forceinline__ bool bl_weight(int o, int O, int I, int i, float &wgt) {
  const float ss = src_coord(o, O, I);
  const int i0 = (int)floorf(ss);
  if (i0 == i) { wgt = 1.f - (ss - (float)i0); return true; }
  if (i0 + 1 == i) { wgt = ss - (float)i0; return true; }
  return false;
}
__global__ void bilinear_bwd_w_kernel(const float *__restrict__ dy, float4 *__restrict__ tmp, int Win, int C4,
                                      int Ho, int Wo, int ldo, int coff, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    long long t = i / C4;
    const int w = (int)(t % Win); t /= Win;          // t = n * Ho + ho
    int lo, hi;
    bl_range(w, Win, Wo, lo, hi);
    float4 acc = make_float4(0, 0, 0, 0);
    for (int wo = lo; wo <= hi; ++wo) {
      float wx;
      if (!bl_weight(wo, Wo, Win, w, wx)) continue;
      const float4 v = *reinterpret_cast<const float4 *>(dy + (t * Wo + wo) * (long long)ldo + coff + c4 * 4);
      acc.x += wx * v.x; acc.y += wx * v.y; acc.z += wx * v.z; acc.w += wx * v.w;
    }
    tmp[i] = acc;
  }
}
__global__ void bilinear_bwd_h_kernel(const float4 *__restrict__ tmp, float4 *__restrict__ dx, int Hin, int Win,
                                      int C4, int Ho, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    long long t = i / C4;
    const int w = (int)(t % Win); t /= Win;
    const int h = (int)(t % Hin);
    const long long n = t / Hin;
    int lo, hi;
    bl_range(h, Hin, Ho, lo, hi);
    float4 acc = make_float4(0, 0, 0, 0);
    for (int ho = lo; ho <= hi; ++ho) {
      float wy;
      if (!bl_weight(ho, Ho, Hin, h, wy)) continue;
      const float4 v = tmp[((n * Ho + ho) * Win + w) * C4 + c4];
      acc.x += wy * v.x; acc.y += wy * v.y; acc.z += wy * v.z; acc.w += wy * v.w;
    }
    dx[i] = acc;
  }
}

// ------------------------------------------------------------------ segmentation readouts
// Counts behind CustomAccuracyMetric (train/metric.py:100-133) and IoUMetric (evaluate/eval_metric.py:359-384):
// pred = argmax over the class axis (first maximum), counts[0*C + c] = #(label == c & pred == c),
// counts[1*C + c] = #(pred == c), counts[2*C + c] = #(label == c), counts[3*C] = #(pred == label) -- integer
// atomics (order independent).  scores: rows x ld floats, classes [0, C); label: rows floats (any value, e.g. 255).
constexpr int kMaxSegC = 64;
__global__ __launch_bounds__(kT) void seg_counts_kernel(const float *__restrict__ scores, const float *__restrict__ label,
                                                       long long rows, int C, int ld,
                                                       unsigned long long *__restrict__ counts) {
  __shared__ unsigned int h[3 * kMaxSegC + 1];
  for (int i = threadIdx.x; i < 3 * C + 1; i += kT) h[i] = 0;
  __syncthreads();
  for (long long r = blockIdx.x * (long long)kT + threadIdx.x; r < rows; r += (long long)gridDim.x * kT) {
    const float *p = scores + r * ld;
    int best = 0;
    float bv = p[0];
    for (int c = 1; c < C; ++c) {
      const float v = p[c];
      if (v > bv) { bv = v; best = c; }
    }
    const int lab = (int)label[r];
    atomicAdd(&h[C + best], 1u);
    if (lab >= 0 && lab < C) atomicAdd(&h[2 * C + lab], 1u);
    if (lab == best) { atomicAdd(&h[best], 1u); atomicAdd(&h[3 * C], 1u); }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * C + 1; i += kT)
    if (h[i]) atomicAdd(&counts[i < 3 * C ? i : 3 * C], (unsigned long long)h[i]);
}

// Segmentation read-out at full resolution (multi_eval.py:28-34, prob_upsampling): BilinearSampler of the class
// probabilities onto an identity-affine grid of Ho x Wo followed by argmax over classes -- fused, the (C, Ho, Wo)
// probability volume (19 x 1024 x 2048 floats per image) is never written.  Each thread produces 4 neighbouring
// output pixels (one 4-byte store); the <= 4 x 2 source pixels they touch are L1/L2 hits for the whole 8x8 patch.
// Arithmetic order per class follows the sampler: tl*wy*wx + tr*wy*(1-wx) + bl*(1-wy)*wx + br*(1-wy)*(1-wx),
// corners outside the map contribute 0; ties keep the lowest class (argmax).
// (separate, uncontracted multiplies and adds: the class map is compared bit for bit with the CPU restatement)
__device__ __forceinline__ float src_coord_exact(int o, int O, int I) {
#pragma clang fp contract(off)
  const float step = 2.f / (float)(O - 1);
  const float prod = (float)o * step;
  const float g = O > 1 ? -1.f + prod : 0.f;
  return (g + 1.f) * (float)(I - 1) / 2.f;
}
// The two source rows of output row ho and the weight of the upper one
struct SegRows {
  const float *r0, *r1;
  bool vy0, vy1;
  float wy;
};
__device__ __forceinline__ SegRows seg_rows(const float *__restrict__ prob, long long n, int ho, int Ho, int Hin, int Win, int ld) {
#pragma clang fp contract(off)
  SegRows r;
  const float ys = src_coord_exact(ho, Ho, Hin);
  const int y0 = (int)floorf(ys);
  r.wy = 1.f - (ys - (float)y0);
  r.vy0 = (unsigned)y0 < (unsigned)Hin; r.vy1 = (unsigned)(y0 + 1) < (unsigned)Hin;
  r.r0 = prob + ((n * Hin + (r.vy0 ? y0 : 0)) * Win) * (long long)ld;
  r.r1 = prob + ((n * Hin + (r.vy1 ? y0 + 1 : 0)) * Win) * (long long)ld;
  return r;
}
// argmax over the classes of output pixel (row r, column wo): the one definition both read-outs below share
template <bool VEC>   // VEC: ld % 4 == 0, the class vectors of the four corners are read as float4
__device__ __forceinline__ int seg_pixel_argmax(const SegRows &r, int wo, int Wo, int Win, int C, int ld) {
#pragma clang fp contract(off)
  const float wy = r.wy;
  const bool vy0 = r.vy0, vy1 = r.vy1;
  const float xs = src_coord_exact(wo, Wo, Win);
  const int x0 = (int)floorf(xs);
  const float wx = 1.f - (xs - (float)x0);
  const bool vx0 = (unsigned)x0 < (unsigned)Win, vx1 = (unsigned)(x0 + 1) < (unsigned)Win;
  const float *tl = r.r0 + (long long)(vx0 ? x0 : 0) * ld, *tr = r.r0 + (long long)(vx1 ? x0 + 1 : 0) * ld;
  const float *bl = r.r1 + (long long)(vx0 ? x0 : 0) * ld, *br = r.r1 + (long long)(vx1 ? x0 + 1 : 0) * ld;
  // a corner outside the map contributes 0: its weight product is applied to a zero value
  const float mtl = (vy0 && vx0) ? 1.f : 0.f, mtr = (vy0 && vx1) ? 1.f : 0.f;
  const float mbl = (vy1 && vx0) ? 1.f : 0.f, mbr = (vy1 && vx1) ? 1.f : 0.f;
  const float wx1 = 1.f - wx, wy1 = 1.f - wy;
  float bv = -INFINITY;
  int best = 0;
  auto consider = [&](const int c, float a, float b, float d, float f) __attribute__((always_inline)) {
    a = mtl != 0.f ? a : 0.f; b = mtr != 0.f ? b : 0.f; d = mbl != 0.f ? d : 0.f; f = mbr != 0.f ? f : 0.f;
    const float v = a * wy * wx + b * wy * wx1 + d * wy1 * wx + f * wy1 * wx1;
    if (c < C && (v > bv || c == 0)) { bv = v; best = c; }
  };
  if constexpr (VEC) {
    for (int c = 0; c < C; c += 4) {
      const float4 a = *reinterpret_cast<const float4 *>(tl + c), b = *reinterpret_cast<const float4 *>(tr + c);
      const float4 d = *reinterpret_cast<const float4 *>(bl + c), f = *reinterpret_cast<const float4 *>(br + c);
      consider(c, a.x, b.x, d.x, f.x);
      consider(c + 1, a.y, b.y, d.y, f.y);
      consider(c + 2, a.z, b.z, d.z, f.z);
      consider(c + 3, a.w, b.w, d.w, f.w);
    }
  } else {
    for (int c = 0; c < C; ++c) consider(c, tl[c], tr[c], bl[c], br[c]);
  }
  return best;
}
template <bool VEC>
__global__ __launch_bounds__(kT) void seg_upsample_argmax_kernel(const float *__restrict__ prob, unsigned char *__restrict__ out,
                                                                int Hin, int Win, int C, int ld, int Ho, int Wo,
                                                                long long total) {
  const int Wq = (Wo + 3) / 4;
  for (long long i = blockIdx.x * (long long)kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
    const int wq = (int)(i % Wq);
    long long t = i / Wq;
    const int ho = (int)(t % Ho);
    const long long n = t / Ho;
    const SegRows rows = seg_rows(prob, n, ho, Ho, Hin, Win, ld);
    unsigned char res[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int wo = wq * 4 + e;
      if (wo >= Wo) break;
      res[e] = (unsigned char)seg_pixel_argmax<VEC>(rows, wo, Wo, Win, C, ld);
    }
    unsigned char *o = out + (n * Ho + ho) * (long long)Wo + wq * 4;
    if (wq * 4 + 3 < Wo && (Wo & 3) == 0) {
      *reinterpret_cast<uchar4 *>(o) = make_uchar4(res[0], res[1], res[2], res[3]);
    } else {
      for (int e = 0; e < 4 && wq * 4 + e < Wo; ++e) o[e] = res[e];
    }
  }
}

// ------------------------------------------------------------------ Cityscapes pixel-level evaluation counts
// (data/cityscapes/Scripts/evaluation/evalPixelLevelSemanticLabeling.py evaluatePair, :583-635): one pass over the
// pixels gives the confusion matrix and, per ground-truth instance, its size and the pixels predicted as its label /
// as a label of its category.  Every output is an integer and is added with atomics: the order does not matter.
// Layout of the tables: include/dspn_nn.h.
constexpr int kCsLabels = DSPN_CITYSCAPES_LABELS;                         // labelIds 0..33
constexpr int kCsInstLabel0 = DSPN_CITYSCAPES_INST_LABEL0;                // labels 24..33 have instances
constexpr int kCsInstLabels = DSPN_CITYSCAPES_INST_LABELS;
constexpr int kCsInstPerLabel = DSPN_CITYSCAPES_INST_PER_LABEL;           // inst = labelId * 1000 + k
constexpr int kCsInstPerImage = kCsInstLabels * kCsInstPerLabel;
constexpr int kCsMaxImages = 0x7fffffff / kCsInstPerImage;                // instance keys are ints

struct CsShared {
  unsigned int conf[kCsLabels * kCsLabels];
  unsigned int errors;
  unsigned char category[256], label_of[256];
};
__device__ __forceinline__ void cs_shared_init(CsShared &s, const unsigned char *__restrict__ category,
                                               const unsigned char *__restrict__ label_of) {
  for (int i = threadIdx.x; i < kCsLabels * kCsLabels; i += kT) s.conf[i] = 0;
  if (threadIdx.x == 0) s.errors = 0;
  for (int i = threadIdx.x; i < 256; i += kT) { s.category[i] = category[i]; s.label_of[i] = label_of ? label_of[i] : 0; }
  __syncthreads();
}
__device__ __forceinline__ void cs_shared_flush(CsShared &s, unsigned long long *__restrict__ conf,
                                                unsigned long long *__restrict__ errors) {
  __syncthreads();
  for (int i = threadIdx.x; i < kCsLabels * kCsLabels; i += kT)
    if (s.conf[i]) atomicAdd(&conf[i], (unsigned long long)s.conf[i]);
  if (threadIdx.x == 0 && s.errors) atomicAdd(errors, (unsigned long long)s.errors);
}
// The four pixels of a thread (cnt of them inside the image; image n) -> the tables.  Called by WHOLE waves (lanes without
// pixels pass cnt = 0).  Most of a wave's 256 neighbouring pixels share one confusion cell and one or two instances, so equal
// keys are first added up across the wave (a ballot per pixel slot and distinct key) and ONE lane issues the atomic.
__device__ __forceinline__ void cs_accumulate(CsShared &s, unsigned int *__restrict__ inst, long long n, int cnt,
                                              const unsigned char (&pred)[4], const unsigned char (&gt)[4], const int (&id)[4]) {
  const int lane = threadIdx.x & 63;
  int ck[4], ik[4];                 // confusion cell / instance entry of each pixel, -1: none
  unsigned long long tp[4], ct[4];  // lanes whose pixel e is predicted as the instance's label / category
  int nerr = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool have = e < cnt;
    const int g = gt[e], p = pred[e];
    bool bad = g >= kCsLabels || p >= kCsLabels;
    ck[e] = have && !bad ? g * kCsLabels + p : -1;
    ik[e] = -1;
    bool is_tp = false, is_ct = false;
    if (have && id[e] > 1000) {     // a value < 1000 is a bare labelId (no instance), 1000 itself is none either (:601)
      const int lab = id[e] / 1000, k = id[e] - lab * 1000;
      if (lab >= kCsInstLabel0 && lab < kCsInstLabel0 + kCsInstLabels) {
        ik[e] = (int)n * kCsInstPerImage + (lab - kCsInstLabel0) * kCsInstPerLabel + k;
        const unsigned char c = s.category[lab];
        is_tp = p == lab;
        is_ct = c != 0 && s.category[p] == c;
      } else {
        bad = true;
      }
    }
    nerr += have && bad;
    tp[e] = __ballot(is_tp);
    ct[e] = __ballot(is_ct);
  }
  if (nerr) atomicAdd(&s.errors, (unsigned)nerr);
  auto pick = [](const int (&v)[4], int e) { return e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3]; };
  unsigned long long todo[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) todo[e] = __ballot(ck[e] >= 0);
  while (todo[0] | todo[1] | todo[2] | todo[3]) {
    const int le = todo[0] ? 0 : todo[1] ? 1 : todo[2] ? 2 : 3;
    const int leader = __ffsll((long long)(le == 0 ? todo[0] : le == 1 ? todo[1] : le == 2 ? todo[2] : todo[3])) - 1;
    const int key = __shfl(pick(ck, le), leader, 64);
    unsigned total = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned long long m = __ballot(ck[e] == key);
      total += (unsigned)__popcll(m);
      todo[e] &= ~m;
    }
    if (lane == leader) atomicAdd(&s.conf[key], total);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) todo[e] = __ballot(ik[e] >= 0);
  while (todo[0] | todo[1] | todo[2] | todo[3]) {
    const int le = todo[0] ? 0 : todo[1] ? 1 : todo[2] ? 2 : 3;
    const int leader = __ffsll((long long)(le == 0 ? todo[0] : le == 1 ? todo[1] : le == 2 ? todo[2] : todo[3])) - 1;
    const int key = __shfl(pick(ik, le), leader, 64);
    unsigned size = 0, ntp = 0, nct = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned long long m = __ballot(ik[e] == key);
      size += (unsigned)__popcll(m);
      ntp += (unsigned)__popcll(m & tp[e]);
      nct += (unsigned)__popcll(m & ct[e]);
      todo[e] &= ~m;
    }
    if (lane == leader) {
      unsigned int *o = inst + (size_t)key * 3;
      atomicAdd(o, size);
      if (ntp) atomicAdd(o + 1, ntp);
      if (nct) atomicAdd(o + 2, nct);
    }
  }
}
// ground truth of the four pixels of a thread: one uchar4 and one int4 where the rows allow it
__device__ __forceinline__ void cs_load_gt(const unsigned char *__restrict__ gt_label, const int *__restrict__ gt_inst,
                                           long long at, int cnt, bool vec, unsigned char (&gt)[4], int (&id)[4]) {
  if (vec) {
    const uchar4 g = *reinterpret_cast<const uchar4 *>(gt_label + at);
    const int4 v = *reinterpret_cast<const int4 *>(gt_inst + at);
    gt[0] = g.x; gt[1] = g.y; gt[2] = g.z; gt[3] = g.w;
    id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) { gt[e] = e < cnt ? gt_label[at + e] : 0; id[e] = e < cnt ? gt_inst[at + e] : 0; }
  }
}
// vec: W % 4 == 0 and the three maps are aligned for 4-pixel accesses.  The loop runs per WAVE (the ballots need every lane).
__global__ __launch_bounds__(kT) void cityscapes_counts_kernel(const unsigned char *__restrict__ pred_map,
                                                              const unsigned char *__restrict__ gt_label, const int *__restrict__ gt_inst,
                                                              int H, int W, long long total, bool vec,
                                                              const unsigned char *__restrict__ category,
                                                              unsigned long long *__restrict__ conf, unsigned int *__restrict__ inst,
                                                              unsigned long long *__restrict__ errors) {
  __shared__ CsShared s;
  cs_shared_init(s, category, nullptr);
  const int Wq = (W + 3) / 4, lane = threadIdx.x & 63;
  for (long long base = blockIdx.x * (long long)kT + (threadIdx.x - lane); base < total; base += (long long)gridDim.x * kT) {
    const long long i = base + lane;
    unsigned char pred[4] = {0, 0, 0, 0}, gt[4] = {0, 0, 0, 0};
    int id[4] = {0, 0, 0, 0}, cnt = 0;
    long long n = 0;
    if (i < total) {
      const int wq = (int)(i % Wq);
      long long t = i / Wq;
      const int h = (int)(t % H);
      n = t / H;
      cnt = min(4, W - wq * 4);
      const long long at = (n * H + h) * (long long)W + wq * 4;
      cs_load_gt(gt_label, gt_inst, at, cnt, vec, gt, id);
      if (vec) {
        const uchar4 p = *reinterpret_cast<const uchar4 *>(pred_map + at);
        pred[0] = p.x; pred[1] = p.y; pred[2] = p.z; pred[3] = p.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pred[e] = e < cnt ? pred_map[at + e] : 0;
      }
    }
    cs_accumulate(s, inst, n, cnt, pred, gt, id);
  }
  cs_shared_flush(s, conf, errors);
}
// The same counts straight from the class probabilities: the prediction of a pixel is seg_upsample_argmax_kernel's class
// (seg_pixel_argmax) sent through the trainId -> labelId table; the class map is never written.
template <bool VEC>
__global__ __launch_bounds__(kT) void cityscapes_counts_prob_kernel(const float *__restrict__ prob, int Hin, int Win, int C, int ld,
                                                                   const unsigned char *__restrict__ label_of,
                                                                   const unsigned char *__restrict__ gt_label, const int *__restrict__ gt_inst,
                                                                   int Ho, int Wo, long long total, bool vec,
                                                                   const unsigned char *__restrict__ category,
                                                                   unsigned long long *__restrict__ conf, unsigned int *__restrict__ inst,
                                                                   unsigned long long *__restrict__ errors) {
  __shared__ CsShared s;
  cs_shared_init(s, category, label_of);
  const int Wq = (Wo + 3) / 4, lane = threadIdx.x & 63;
  for (long long base = blockIdx.x * (long long)kT + (threadIdx.x - lane); base < total; base += (long long)gridDim.x * kT) {
    const long long i = base + lane;
    unsigned char pred[4] = {0, 0, 0, 0}, gt[4] = {0, 0, 0, 0};
    int id[4] = {0, 0, 0, 0}, cnt = 0;
    long long n = 0;
    if (i < total) {
      const int wq = (int)(i % Wq);
      long long t = i / Wq;
      const int ho = (int)(t % Ho);
      n = t / Ho;
      cnt = min(4, Wo - wq * 4);
      cs_load_gt(gt_label, gt_inst, (n * Ho + ho) * (long long)Wo + wq * 4, cnt, vec, gt, id);
      const SegRows rows = seg_rows(prob, n, ho, Ho, Hin, Win, ld);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) pred[e] = s.label_of[seg_pixel_argmax<VEC>(rows, wq * 4 + e, Wo, Win, C, ld)];
    }
    cs_accumulate(s, inst, n, cnt, pred, gt, id);
  }
  cs_shared_flush(s, conf, errors);
}

}  // namespace

extern "C" {

int dspn_bilinear_forward_f32(const float *x, float *y, int N, int Hin, int Win, int C, int Ho, int Wo,
                              int ldo, int coff, void *stream) {
  DSPN_REQUIRE(x && y && C % 4 == 0 && ldo % 4 == 0 && coff % 4 == 0 && coff + C <= ldo, "bilinear_forward: bad argument");
  const long long total = (long long)N * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(bilinear_fwd_kernel<false>, dim3(grid_for(total)), dim3(kT), 0, S_(stream),
                     reinterpret_cast<const float4 *>(x), y, Hin, Win, C / 4, Ho, Wo, ldo, coff, total);
  return dspn::check_launch("bilinear_forward");
}
int dspn_bilinear_forward_acc_f32(const float *x, float *y, int N, int Hin, int Win, int C, int Ho, int Wo,
                                  int ldo, int coff, void *stream) {
  DSPN_REQUIRE(x && y && C % 4 == 0 && ldo % 4 == 0 && coff % 4 == 0 && coff + C <= ldo, "bilinear_forward_acc: bad argument");
  const long long total = (long long)N * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(bilinear_fwd_kernel<true>, dim3(grid_for(total)), dim3(kT), 0, S_(stream),
                     reinterpret_cast<const float4 *>(x), y, Hin, Win, C / 4, Ho, Wo, ldo, coff, total);
  return dspn::check_launch("bilinear_forward_acc");
}
int dspn_bilinear_backward_f32(const float *dy, float *dx, int N, int Hin, int Win, int C, int Ho, int Wo,
                               int ldo, int coff, void *stream) {
  DSPN_REQUIRE(dy && dx && C % 4 == 0 && ldo % 4 == 0 && coff % 4 == 0 && coff + C <= ldo, "bilinear_backward: bad argument");
  const long long total = (long long)N * Hin * Win * (C / 4);
  hipLaunchKernelGGL(bilinear_bwd_kernel, dim3(grid_for(total)), dim3(kT), 0, S_(stream), dy,
                     reinterpret_cast<float4 *>(dx), Hin, Win, C / 4, Ho, Wo, ldo, coff, total);
  return dspn::check_launch("bilinear_backward");
}

size_t dspn_bilinear_backward_workspace_bytes(int N, int Win, int C, int Ho) {
  if (N <= 0 || Win <= 0 || C <= 0 || Ho <= 0) return 0;
  return sizeof(float) * (size_t)N * Ho * Win * C;
}
/* separable two-pass backward (needs dspn_bilinear_backward_workspace_bytes of scratch) */
int dspn_bilinear_backward_ws_f32(const float *dy, float *dx, int N, int Hin, int Win, int C, int Ho, int Wo,
                                  int ldo, int coff, void *workspace, size_t workspace_bytes, void *stream) {
  DSPN_REQUIRE(dy && dx && workspace && C % 4 == 0 && ldo % 4 == 0 && coff % 4 == 0 && coff + C <= ldo,
               "bilinear_backward: bad argument");
  if (workspace_bytes < dspn_bilinear_backward_workspace_bytes(N, Win, C, Ho))
    return dspn::fail(DSPN_ERR_WORKSPACE_, "bilinear_backward: workspace too small");
  const long long t1 = (long long)N * Ho * Win * (C / 4), t2 = (long long)N * Hin * Win * (C / 4);
  hipLaunchKernelGGL(bilinear_bwd_w_kernel, dim3(grid_for(t1, kT, 65535)), dim3(kT), 0, S_(stream), dy,
                     static_cast<float4 *>(workspace), Win, C / 4, Ho, Wo, ldo, coff, t1);
  hipLaunchKernelGGL(bilinear_bwd_h_kernel, dim3(grid_for(t2, kT, 65535)), dim3(kT), 0, S_(stream),
                     static_cast<const float4 *>(workspace), reinterpret_cast<float4 *>(dx), Hin, Win, C / 4, Ho, t2);
  return dspn::check_launch("bilinear_backward_ws");
}

int dspn_seg_counts_f32(const float *scores, const float *label, long long rows, int C, int ld,
                        unsigned long long *counts, void *stream) {
  DSPN_REQUIRE(scores && label && counts && rows > 0 && C > 0 && C <= kMaxSegC && ld >= C, "seg_counts: bad argument (C <= 64)");
  (void)hipMemsetAsync(counts, 0, sizeof(unsigned long long) * (3 * C + 1), S_(stream));
  hipLaunchKernelGGL(seg_counts_kernel, dim3(grid_for(rows, kT, 2048)), dim3(kT), 0, S_(stream), scores, label, rows, C, ld,
                     counts);
  return dspn::check_launch("seg_counts");
}

int dspn_seg_upsample_argmax_f32(const float *prob, unsigned char *out, int N, int Hin, int Win, int C, int ld,
                                 int Ho, int Wo, void *stream) {
  DSPN_REQUIRE(prob && out && N > 0 && Hin > 0 && Win > 0 && Ho > 0 && Wo > 0 && C > 0 && C <= 256 && ld >= C,
               "seg_upsample_argmax: bad argument (0 < C <= 256, ld >= C)");
  const long long total = (long long)N * Ho * ((Wo + 3) / 4);
  // float4 reads of the class vectors need 16-byte aligned rows that hold the rounded-up channel count
  const bool vec = ld % 4 == 0 && (C + 3) / 4 * 4 <= ld && reinterpret_cast<uintptr_t>(prob) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(seg_upsample_argmax_kernel<true>, dim3(grid_for(total, kT, 65535)), dim3(kT), 0, S_(stream), prob, out,
                       Hin, Win, C, ld, Ho, Wo, total);
  else
    hipLaunchKernelGGL(seg_upsample_argmax_kernel<false>, dim3(grid_for(total, kT, 65535)), dim3(kT), 0, S_(stream), prob, out,
                       Hin, Win, C, ld, Ho, Wo, total);
  return dspn::check_launch("seg_upsample_argmax");
}

// 4-pixel accesses of the ground-truth maps: whole groups of four per row, bases aligned for a uchar4 / an int4
static bool cs_vec_ok(int W, const void *bytes_a, const void *bytes_b, const int *gt_inst) {
  return W % 4 == 0 && reinterpret_cast<uintptr_t>(bytes_a) % 4 == 0 && reinterpret_cast<uintptr_t>(bytes_b) % 4 == 0 &&
         reinterpret_cast<uintptr_t>(gt_inst) % 16 == 0;
}
// Workgroups of the Cityscapes count kernels: every one of them ends with an atomic per non-empty cell of its confusion
// matrix, so the grid is a few workgroups per compute unit that walk the image, not one per 1024 pixels.
constexpr int kCsGridCap = 2048;

int dspn_cityscapes_counts_u8(const unsigned char *pred, const unsigned char *gt_label, const int *gt_inst, int N, int H,
                              int W, const unsigned char *category, unsigned long long *conf, unsigned int *inst,
                              unsigned long long *errors, void *stream) {
  DSPN_REQUIRE(pred && gt_label && gt_inst && category && conf && inst && errors, "cityscapes_counts: null pointer");
  DSPN_REQUIRE(N > 0 && N <= kCsMaxImages && H > 0 && W > 0 && (long long)H * W < (1ll << 32) && (long long)N * H * W <= (1ll << 40),
               "cityscapes_counts: bad argument (0 < N <= %d, 0 < H * W < 2^32, N * H * W <= 2^40)", kCsMaxImages);
  const long long total = (long long)N * H * ((W + 3) / 4);
  hipLaunchKernelGGL(cityscapes_counts_kernel, dim3(grid_for(total, kT, kCsGridCap)), dim3(kT), 0, S_(stream), pred, gt_label,
                     gt_inst, H, W, total, cs_vec_ok(W, pred, gt_label, gt_inst), category, conf, inst, errors);
  return dspn::check_launch("cityscapes_counts");
}

int dspn_cityscapes_counts_prob_f32(const float *prob, int N, int Hin, int Win, int C, int ld,
                                    const unsigned char *label_of_train_id, const unsigned char *gt_label,
                                    const int *gt_inst, int Ho, int Wo, const unsigned char *category,
                                    unsigned long long *conf, unsigned int *inst, unsigned long long *errors, void *stream) {
  DSPN_REQUIRE(prob && label_of_train_id && gt_label && gt_inst && category && conf && inst && errors,
               "cityscapes_counts_prob: null pointer");
  DSPN_REQUIRE(N > 0 && N <= kCsMaxImages && Hin > 0 && Win > 0 && Ho > 0 && Wo > 0 && (long long)Ho * Wo < (1ll << 32) &&
               (long long)N * Ho * Wo <= (1ll << 40) && C > 0 && C <= 256 && ld >= C,
               "cityscapes_counts_prob: bad argument (0 < N <= %d, 0 < Ho * Wo < 2^32, N * Ho * Wo <= 2^40, 0 < C <= 256, ld >= C)",
               kCsMaxImages);
  const long long total = (long long)N * Ho * ((Wo + 3) / 4);
  const bool vec = cs_vec_ok(Wo, gt_label, gt_label, gt_inst);
  // float4 reads of the class vectors: as in dspn_seg_upsample_argmax_f32
  const bool vec_prob = ld % 4 == 0 && (C + 3) / 4 * 4 <= ld && reinterpret_cast<uintptr_t>(prob) % 16 == 0;
  if (vec_prob)
    hipLaunchKernelGGL(cityscapes_counts_prob_kernel<true>, dim3(grid_for(total, kT, kCsGridCap)), dim3(kT), 0, S_(stream), prob,
                       Hin, Win, C, ld, label_of_train_id, gt_label, gt_inst, Ho, Wo, total, vec, category, conf, inst, errors);
  else
    hipLaunchKernelGGL(cityscapes_counts_prob_kernel<false>, dim3(grid_for(total, kT, kCsGridCap)), dim3(kT), 0, S_(stream), prob,
                       Hin, Win, C, ld, label_of_train_id, gt_label, gt_inst, Ho, Wo, total, vec, category, conf, inst, errors);
  return dspn::check_launch("cityscapes_counts_prob");
}

}  // extern "C"
