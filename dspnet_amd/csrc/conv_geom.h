// Geometry record and helpers shared by the convolution translation units (conv.hip: every math mode and storage type;
// conv_wide.hip: the wide tile family of the two-piece math).  PRIVATE to csrc/.
#pragma once
#include <hip/hip_runtime.h>

namespace dspn {
namespace conv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <typename st_t>
struct ConvGeomT {
  int N, Hin, Win, Cin;            // gathered tensor (Cin % kEPC == 0)
  int Hg, Wg;                      // grid of output points per image
  int ish, isw, ioh, iow, idh, idw;  // ih = i*ish + ioh + tr*idh
  int TR, TS;                      // taps enumerated
  int WTAPS, WS, wr0, wrs, ws0, wss;  // weight tap = (wr0+tr*wrs)*WS + ws0+ts*wss
  int Cout;
  long long obs;                   // output batch stride (floats)
  int OW, osh, osw, ooh, oow, ldc; // out pixel = ((i*osh+ooh)*OW + j*osw+oow)*ldc
  int flags;                       // 1 bias, 2 relu, 4 accumulate, 8 add residual (same layout as out), 16 float4 rows legal, 32 ReLU after the input affine
  int dense;                       // output address = m*ldc (no decomposition needed)
  int dbg;                         // timing-only ablation bits (DSPN_ABLATE builds), 0 in production
  int bf16;                        // host side only: the call's math mode (DSPN_MATH_*): 0 fp32 MFMA, 1 bf16 MFMA, 2 three-piece bf16
  unsigned in_bytes, w_bytes;      // sizes of the gathered tensor / weight tensor (buffer bounds)
  // optional per-input-channel affine (+ReLU when flags & 32) applied to the gathered tensor on its way into
  // LDS: the BatchNorm(+ReLU) in front of a convolution (symbol/resnet.py:30-45) without materialising its output
  const float *in_scale, *in_shift;
  // optional BatchNorm statistics of the OUTPUT, per row tile: stats[(mt*2 + 0)*Cout + c] = mean over the tile's
  // rows, stats[(mt*2 + 1)*Cout + c] = sum of squared deviations from that mean (merged by dspn_bn_stats_from_tiles_f32)
  float *stats;
  // optional (two-piece math, with stats): minmax[(mt*2 + 0)*Cout + c] = smallest, [(mt*2 + 1)*Cout + c] = largest stored value
  // of the tile's rows in column c.  A BatchNorm(+ReLU) of the output is monotone per channel, so the magnitude of what the
  // NEXT convolution's loader forms from this tensor is the largest |f_c(extreme)| over this small table
  // (dspn_absmax_f32 on it, with the affine) -- instead of a pass over the whole tensor
  float *minmax;
  // optional BatchNorm-backward sums of the OUTPUT (a data gradient dy of a BatchNorm(+ReLU) output whose input was
  // bn_x, same layout as out): per row tile t, bn_sums[((tile_base + t)*2 + 0)*Cout + c] = sum of dy' and
  // [... + 1 ...] = sum of dy' * xhat, with dy' = dy where (bn_x*bn_scale + bn_shift > 0 or no ReLU) else 0 and
  // xhat = (bn_x - bn_mean) * bn_rstd: the layout dspn_bn_backward_from_sums_f32 reads
  const st_t *bn_x;
  const float *bn_scale, *bn_shift, *bn_mean, *bn_rstd;
  float *bn_sums;
  int bn_relu, bn_tile_base;
  // optional, with bn_sums (round 4): 64 partial maxima of |dx| as stored -- the largest output gradient the following
  // BatchNorm backward meets, from which it bounds the dx IT stores before it writes it as fp16 piece planes (dspn_nn.h)
  unsigned *bn_dy_absmax;
  // DSPN_MATH_F32_F16X2: device scalars holding the largest magnitude of the A operand (the gathered tensor AFTER its input
  // affine) and of the B operand (the weights); the kernel derives the power-of-two scales that put them just below 2^15
  // (operand_scale) and undoes both in the epilogue.  NULL = scale 1 (the caller vouches for |operand| < 65504).
  const float *a_absmax, *b_absmax;
  int a_planes;                    // host side only: the gathered tensor is fp16 piece planes (conv_nt_kernel, EPIX & 4)
  // host side only: the weight operand as three bf16 piece planes [Cout][WTAPS][Cin / 32][3][32] (split mode, Cin % 32 == 0:
  // dspn_conv2d_weight_planes_f32); the kernel then receives this pointer in place of the float weights
  const void *w_planes;
  // optional, with bn_sums (a dense stride-1 data gradient that is the ONLY writer of its output): a compact tensor
  // (N, sadd_h, sadd_w, Cout) with sadd_h = ceil(Hg / 2), sadd_w = ceil(Wg / 2) -- the data gradient of a 1 x 1 / stride-2
  // convolution of the same input -- added at the even positions: out[n,h,w,:] = conv + (h, w both even ? sadd[n,h/2,w/2,:] : +0.0f),
  // where the accumulate addend would be added.  Only the plane-fed 128-row members on the tile-spanning loop take it
  // (plan_nt refuses every other route).
  const st_t *sadd;
  int sadd_h, sadd_w;
  unsigned sadd_bytes;             // its size (buffer bound)
  int layout_pad_;                 // read by nothing (always 0): keeps the kernel-argument layout; goes with the next change to the kernels
  // The data gradient of a BatchNorm(+ReLU) output that is never stored (dspn_nn.h dspn_conv2d_dgrad_bn_sums_f32 / _apply_f32),
  // on the routes of the strided addend: 1 = the sums pass (bn_sums as ever, out == NULL: no store, no addend, no magnitude
  // block), 2 = the apply pass -- out (+)= a g' + c1 bn_x + c0 with the finalize's coefficients bn_coef = [a | c1 | c0], 3 Cout
  // floats; bn_mean / bn_rstd / bn_sums unused, bn_dy_absmax receives the partial maxima of |out| as stored.
  int bn_recompute;
  const float *bn_coef;
};

__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  // blocks b, b+8, ... share an XCD (round-robin dispatch): give each XCD a
  // contiguous run of logical tiles so neighbouring tiles share its L2.
  const int q = nblk >> 3, r = nblk & 7, x = bid & 7;
  const int start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return start + (bid >> 3);
}


// The wide tile family (conv_wide.hip).  A member is a tile and the kernel that feeds it: P* take both operands as piece planes
// (conv_ntw_kernel; bfloat16 tensors: the tensors themselves), F* a float A operand that the loader cuts, with or without the
// folded BatchNorm affine (conv_ntv_kernel).  256 x 128 and 128 x 256 run on eight waves (one workgroup per CU), 128 x 128 and
// 256 x 64 (Cout <= 64, 64-row BatchNorm tables) on four (two per CU).
enum class WideTile { None, P256x128, P128x256, P128x128, P256x64, F128x256, F128x128, F256x64 };
// ... and the loop a call takes: Plain = the round-5 loop with the staged epilogue; Spanning = the next tile's first operands
// are requested before the epilogue of the current one (XT); Direct = the round-5 loop with the direct epilogue (F* only)
enum class WideLoop { Plain, Spanning, Direct };
struct WideRoute {
  WideTile tile = WideTile::None; WideLoop loop = WideLoop::Plain;
  explicit operator bool() const { return tile != WideTile::None; }
};
// the route of one call (M output points, nk k-steps) that is legal for the family -- vector epilogue, at least one tap, no split-K,
// A a pure copy or a float tensor: plan_nt checks; every run-time setting and environment knob of the family is evaluated here, once
WideRoute wide_route(const ConvGeomT<float> &g, long long M, int nk);
WideRoute wide_route(const ConvGeomT<__bf16> &g, long long M, int nk);
// one launch of the family; bfloat16 tensors (conv_wide_h.hip): whole 64-channel blocks, no input affine
int launch_wide(WideRoute r, const float *in, const float *w_planes, const float *bias, float *out, const ConvGeomT<float> &g,
                hipStream_t s, const float *residual);
int launch_wide(WideRoute r, const __bf16 *in, const __bf16 *w, const float *bias, __bf16 *out, const ConvGeomT<__bf16> &g,
                hipStream_t s, const __bf16 *residual);

// conv_wide.hip (conv_stem.h): the 7x7 / 2, pad 3, 4 -> 64 channel stem convolution in the two-piece math with BatchNorm
// statistics (64-row tiles) and extremes: 0 = launched, 1 = not this shape (the generic kernel runs), < 0 = launch error
int launch_stem(const float *x, const float *w, float *y, int N, int H, int W, int Cin, int Cout, int Ho, int Wo,
                const float *x_absmax, const float *w_absmax, float *stats, float *minmax, hipStream_t s);

}  // namespace conv
}  // namespace dspn
