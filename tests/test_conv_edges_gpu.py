"""The convolution kernels of dspnet_amd/csrc/conv.hip (conv_nt_kernel, its split-K reduce, conv_wgrad_kernel and its slab
reduce, the wide family and the stem kernel they dispatch to) at the shapes where the host dispatch changes its mind, element
by element against float64 references computed here with torch on the CPU (F.conv2d, autograd for both gradients; never
another kernel of this library; tests/ref_conv.py).  Every call passes `math=` explicitly.  Five arithmetic variants: the math
modes "fp32", "bf16", "bf16x3", "f16x2" on float tensors, and "bf16t", the bfloat16-tensor build.

BIT-EXACT CLAIMS.  Precondition, asserted on the reference before the device is touched ("inputs unfit" otherwise): both
operands are multiples of a power of two ("unit" = the product of the two) with few significant bits, and per output
sum|a||b| (the float64 convolution of the absolute values, bias / residual / prior output included) stays below 2^22 units.
Every partial product is then exact in every operand format of the library and every fp32 partial sum is exact in ANY order
-- across k-steps, split-K slabs, pixel splits and the slab reduce (2^24 would do for fp32 itself; two bits are kept as a
guard for the alignment inside the MFMA).  So the result must equal the float64 reference bit for bit, bfloat16 tensors
bf16_of(reference) bit for bit (one rounding of an exact fp32 value on store):
  A  both operands integers in [-6, 6]; bias, residual, prior output integers; the input affine's scale in {-2, -1, 1, 2}, its
     shift an integer (fmaf of integers is exact, ReLU is exact).  All five variants.
  B  one operand m 2^-6 with odd-rich |m| < 2^13 (needs piece p1 of the bf16 cut and h1 of the fp16 cut; p2 is zero), the other a
     sparse integer in [-2, 2]; both assignments of the roles (B1: the activation / output gradient carries m, B2: the
     weight -- piece 1 of the weight planes and of the transposed planes).  Float tensors, "fp32", "bf16x3", "f16x2".
  C  one operand an integer of up to 17 significant bits (needs p2; in "f16x2" both fp16 pieces to their last bit), the other
     sparse in {-1, 0, 1}.  Roles and modes as in B.  "f16x2" gives an element 2^17 below the tensor's maximum an absolute error
     only (include/dspn_nn.h): the class stays inside that -- the smallest magnitude is 1, the largest below 2^17, and after the
     scale that puts the maximum into [2^14, 2^15) a 1 is 2^-3 or more, far above the fp16 subnormals.
No class had to fall back to a bar.

GENERAL VALUES (randn operands, randn / sqrt(K) weights, float bias / residual / affine): per element, nothing excluded,
    bar = (n_acc U + e_mode) S + epilogue terms,        U = 2^-24,  S = sum|a||b| in float64
  n_acc   the accumulated terms of one output: the reduction length padded to whole 32-element k-steps, times the partial
          products per multiply (1 "fp32" / "bf16", 6 "bf16x3", 3 "f16x2"), plus 32 for the slabs of a split.  Each
          addition rounds once and every partial sum is at most S: n_acc U S.
  e_mode  "fp32", and "bf16" on operands that ARE bfloat16 values (what this module hands that mode and the bf16 tensors): 0.
          Behind an input affine those two feed the MFMA the bfloat16 value of fmaf(x, scale, shift): so does their reference.
          "bf16x3": |x - p0| <= 2^-9 |x|, |x - p0 - p1| <= 2^-18 |x|, |x - p0 - p1 - p2| <= 2^-27 |x|.  Kept pairs p + q <= 2;
          dropped: p1 q2, p2 q1 (2^-9 2^-18 each), p2 q2 (2^-36), and the cut's remainder of either operand (2^-27 each):
          e = 4 2^-27 + 2^-36.
          "f16x2": h0 = fp16(s x): |s x - h0| <= 2^-11 |s x|; the remainder is a multiple of the float's last bit, below
          2^-11 |s x|, so fp16 (11 bits) keeps it to 2^-23 |s x|.  Dropped: h1 g1 <= 2^-22 |x w|, the remainders 2^-23 each:
          e = 2^-21.  (include/dspn_nn.h says "within 2^-24" and "h1 g1 below 2^-24 |x w|", about 3 2^-24 together: that is
          the typical size; the figures here are the worst case of an 11-bit cut, |h1| <= 2^-11 |s x|, and are what the bar uses.)
          Plus the contract's absolute term for elements far below the maximum: 2^-39 (max|x| sum|w| + max|w| sum|x|).
  epilogue  one rounding for each of bias, residual and prior output, of a value of at most S + |bias| + |residual| + |prior|;
          the input affine's fmaf rounds the operand once: U sum (|x scale| + |shift|) |w|.
  bfloat16 tensors: rule 4 of tests/test_bn_edges_gpu.py (fp_bars.bf16_within).  Its third clause -- fewer than 1e-3 of the stored
          values differ from bf16(reference) -- holds for a float32 evaluation only while the accumulated error, about sqrt(K) U,
          stays well below 1e-3 of a bfloat16 step (2^-8) -- an estimate, not a bound.  So at K > 320 (the bf16 build's split-K
          route among them: K >= 1024) the pass applies the rule's first two clauses only: inside [bf16(ref - bar), bf16(ref + bar)],
          and at most one bfloat16 step from bf16(reference) wherever the bar is below half a step.
          None of the bars comes from a run.

STATISTICS (out_stats / out_minmax) are checked against float64 recomputed from the kernel's OWN stored y (the link rule of
test_bn_edges_gpu.py), in class A, where y and the per-thread shifted sums s1 = sum (v - v0), s2 = sum (v - v0)^2 are exact.
Extremes: bit for bit.  (mean, M2) per tile, from the epilogue's merge (conv.hip, EPI == 1; conv_wide.h has the same scheme),
V = max|v| of the tile's column, n its rows, RPP <= 32 row groups:
  a thread's mean v0 + s1 inv: the reciprocal, the product, the sum: 3 roundings of at most 2V, 2V, V: 5 U V.
  merge: d = mean_e - m_0 (1 rounding of 2V, inherits 10 U V): 12 U V; n_e d (1); the RPP additions of sum n_e d (each of at most
  2 n V); the division; mean = m_0 + dm (inherits 5 U V, rounds once):  mean bar = (20 + 2 RPP) U V = 84 U V.
  M2_e = s2 - s1 s1 inv: 4 roundings of at most 4 n_e V^2 (16 U n V^2 summed); d^2 (48 + 4), n_e d^2 (4), m2_e + n_e d^2 (8):
  64 U n V^2; RPP additions of at most 8 n V^2; n dm^2 from dm's (22 + 2 RPP) U V: (88 + 8 RPP) U n V^2; its three roundings: 12:
  M2 bar = (180 + 16 RPP) U n V^2 = 692 U n V^2.  A tile that counts one row too many or too few moves its mean by |v - mean| / n,
  four orders of magnitude above the bar at n <= 256.  The stem kernel (conv_stem.h) merges halves of 16 rows pairwise with exact
  powers of two for the counts: 5 roundings in the mean, fewer than 60 in M2 -- inside the same bars.

ROUTES.  ref_conv.py restates nt_config, dispatch_nt's split rule, dgrad_tiles, wgrad_plan and the wide family's automatic
choice (default environment, float build; the bfloat16 build's k-step holds 64 channels, so its splits differ: it runs the same
cases on whatever route they give it).  test_case_tables_cover_every_route asserts the coverage; test_restatement_agrees_with_
the_library compares it with every decision the library exports, so a retuned threshold fails there ("the restatement is
stale") instead of silently un-covering an edge.  The split-K rule and the wide family's choice are NOT exported: a retune of
either moves no assertion here, and nothing confirms which kernel a "wide" case ran -- those tables hold as long as
dispatch_nt and wide_tile_choice read as they do today."""
import ctypes

import pytest
import torch

from dspnet_amd import functional as fn
from bf16_twins import BF
from fp_bars import U, bf16_of, within, bf16_within
import ref_conv as R
from ref_conv import pair, out_hw, problem

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = 12352.0          # (a bfloat16 value too) what an output holds before the call: an element left unwritten shows
VARIANTS = ("fp32", "bf16", "bf16x3", "f16x2", "bf16t")
BF16T_GENERAL_K = 320          # see the docstring: rule 4's third clause is applied up to this sum length
SPLIT_VARIANTS = ("fp32", "bf16x3", "f16x2")          # classes B and C
NPROD = {"fp32": 1, "bf16": 1, "bf16x3": 6, "f16x2": 3, "bf16t": 1}
E_MODE = {"fp32": 0.0, "bf16": 0.0, "bf16x3": 4 * 2.0 ** -27 + 2.0 ** -36, "f16x2": 2.0 ** -21, "bf16t": 0.0}


def vinfo(variant):
    """(tensor dtype, math argument, elements per 16-byte chunk)"""
    return (BF, "bf16", 8) if variant == "bf16t" else (F32, variant, 4)


# ---------------------------------------------------------------------------------------------------------------------
# case tables: (N, H, W, Cin, Cout, k, stride, pad, dil).  FULL_FLAGS cases run every epilogue flag alone and all together,
# the others the plain call and all flags together
FWD_TILE = [
    (1, 127, 128, 32, 256, 1, 1, 0, 1),      # 127 x 2 tiles of 128 x 128 < 256: cfg 2 (64 x 64)
    (1, 127, 129, 32, 256, 1, 1, 0, 1),      # 128 x 2 tiles: cfg 0 on eight waves, last row tile 127 rows
    (1, 90, 90, 32, 512, 1, 1, 0, 1),        # cfg 0 at exactly 256 tiles
    (1, 127, 129, 32, 192, 1, 1, 0, 1),      # cfg 1 (128 x 64), full column tiles
    (1, 127, 129, 32, 132, 1, 1, 0, 1),      # cfg 1, ragged column tile, Cout % 64 != 0
    (1, 255, 256, 32, 32, 1, 1, 0, 1),       # Cout <= 32: 255 tiles of 256 x 32: cfg 2
    (1, 255, 257, 32, 32, 1, 1, 0, 1),       # 256 tiles (the last of 255 rows): cfg 3
    (1, 256, 256, 32, 32, 1, 1, 0, 1),       # cfg 3, full last row tile
    (1, 255, 257, 32, 20, 1, 1, 0, 1),       # cfg 3, ragged columns
    (1, 255, 257, 32, 19, 3, 1, 1, 1),       # cfg 3, Cout % 4 != 0: a pad channel
    (1, 64, 64, 32, 19, 1, 1, 0, 1),         # cfg 2 with a pad channel, full row tiles
    (1, 7, 9, 32, 36, 1, 1, 0, 1),           # Cout in 33 .. 64, M = 63
    (1, 8, 8, 32, 54, 1, 1, 0, 1),           # M = 64, Cout % 4 != 0
    (1, 5, 13, 32, 64, 1, 1, 0, 1),          # M = 65
    (1, 1, 1, 32, 1, 1, 1, 0, 1),            # M = 1, Cout = 1
    (1, 1, 2, 32, 3, 1, 1, 0, 1),            # M = 2, Cout = 3
    (1, 7, 9, 4, 4, 1, 1, 0, 1),             # M = 63, Cout = 4, one chunk of channels
    (1, 128, 256, 32, 256, 1, 1, 0, 1),      # cfg 0, full last row tile
    (1, 127, 129, 32, 200, 1, 1, 0, 1),      # cfg 0 with a ragged column tile (200 rounds to 256 either way: not cfg 1)
    (1, 128, 128, 32, 192, 1, 1, 0, 1),      # cfg 1, full last row tile
]
FWD_TAPS = [
    (2, 9, 11, 20, 24, 3, 1, 1, 1),          # 3x3 pad 1, non-uniform taps (a k-step straddles taps)
    (1, 17, 19, 36, 24, 3, 2, 1, 1),         # 3x3 s2 on odd sizes
    (1, 15, 16, 4, 24, 5, 1, 2, 1),          # 5x5 pad 2, 3 real channels would sit in 4
    (1, 21, 23, 4, 40, 7, 2, 3, 1),          # 7x7 s2 pad 3 (not the stem: Cout != 64)
    (1, 12, 25, 20, 24, (1, 7), 1, (0, 3), 1),
    (1, 25, 12, 20, 24, (7, 1), 1, (3, 0), 1),
    (1, 20, 20, 64, 96, 3, 1, 6, 6),         # dilation 6
    (2, 3, 3, 48, 24, 3, 1, 0, 1),           # one output per image
    (1, 2, 3, 20, 8, 5, 1, 2, 1),            # kernel larger than the map
    (1, 9, 11, 200, 24, 3, 1, 1, 1),         # Cin = 200: ragged last k-step, split-K
    (1, 16, 16, 96, 48, 3, 1, 1, 1),         # uniform taps, planes
    (1, 12, 12, 256, 40, 1, 1, 0, 1),
]
FWD_SPLIT = [
    (1, 8, 8, 480, 64, 1, 1, 0, 1),          # nk = 15: no split
    (1, 8, 8, 512, 64, 1, 1, 0, 1),          # nk = 16: two equal slices
    (1, 8, 8, 92, 64, 3, 1, 1, 1),           # nk = 26: three slices, the last short
    (1, 8, 8, 960, 24, 3, 1, 1, 1),          # nk = 270: capped at 32 slices, then 30 of 9 k-steps
    (1, 191, 64, 512, 64, 1, 1, 0, 1),       # nblk = 191: split
    (1, 192, 64, 512, 64, 1, 1, 0, 1),       # nblk = 192: not
    (1, 8, 8, 1024, 24, 3, 1, 1, 1),         # nk = 288: 32 slices of 9 (Cin = 960 above asks for 32 and ends at 30 of 9)
]
FULL_FLAGS = {FWD_TILE[1], FWD_TILE[0], FWD_TILE[6], FWD_SPLIT[2]}          # one cfg 0, one cfg 2, one cfg 3, one split-K
FWD_CASES = FWD_TILE + FWD_TAPS + FWD_SPLIT
# the wide family's automatic choice ("f16x2", Cin % 32 == 0): (case, with statistics)
WIDE_CASES = [
    ((1, 16, 16, 96, 64, 1, 1, 0, 1), False),      # Cout = 64, nk = 3: not routed
    ((1, 16, 16, 128, 64, 1, 1, 0, 1), False),     # nk = 4: 256 x 64, M % 256 == 0 (direct)
    ((1, 16, 17, 128, 64, 1, 1, 0, 1), True),      # ... staged, with statistics on 64-row tiles
    ((1, 128, 256, 32, 128, 1, 1, 0, 1), False),   # Cout = 128 at 256 row tiles (cfg 0), nk = 1: not routed
    ((1, 128, 256, 32, 128, 1, 1, 0, 1), True),
    ((1, 128, 256, 64, 128, 1, 1, 0, 1), False),   # nk = 2: only behind a fused epilogue
    ((1, 129, 255, 64, 128, 1, 1, 0, 1), True),    # ... 128 x 128, ragged last tile (staged)
    ((1, 128, 256, 96, 128, 1, 1, 0, 1), True),    # nk = 3, M % 128 == 0 (direct)
    ((1, 128, 256, 128, 128, 1, 1, 0, 1), False),  # nk = 4: 128 x 128 without statistics
    ((1, 129, 255, 128, 128, 1, 1, 0, 1), False),
    ((1, 128, 256, 224, 256, 1, 1, 0, 1), False),  # Cout = 256, nk = 7: 128 x 128
    ((1, 128, 256, 256, 256, 1, 1, 0, 1), False),  # nk = 8 at exactly 256 tiles of 128 x 256
    ((1, 127, 256, 256, 256, 1, 1, 0, 1), False),  # 254 tiles: 128 x 128
    ((1, 129, 255, 256, 256, 1, 1, 0, 1), True),   # 128 x 256, ragged last row tile
    ((1, 129, 255, 32, 128, 3, 1, 1, 1), True),    # multi-tap on the family
    ((1, 128, 256, 96, 128, 1, 1, 0, 1), False),   # nk = 3 without statistics: the lower side of the unfused gate, not routed
    ((1, 128, 256, 128, 128, 1, 1, 0, 1), True),   # nk = 4 with statistics
]
PLANES_B1 = (1, 2, 6, 8, 11, 13, 14)      # one per plane-fed member and epilogue: the rows of WIDE_CASES that also run class B1 planes
STEM_CASES = [(1, 1, 512), (1, 2, 511), (1, 13, 511), (2, 37, 512)]      # (N, H, W) of the 7x7 / 2, 4 -> 64 stem
# data gradient, stride 1: the forward edges transposed (Cin is the column count, Cout the reduction)
DGRAD_S1 = [
    (1, 127, 128, 256, 32, 1, 1, 0, 1), (1, 127, 129, 256, 32, 1, 1, 0, 1), (1, 127, 129, 132, 32, 1, 1, 0, 1),
    (1, 255, 257, 32, 32, 1, 1, 0, 1), (1, 255, 257, 20, 32, 3, 1, 1, 1), (1, 64, 65, 20, 32, 1, 1, 0, 1),
    (1, 5, 13, 36, 20, 3, 1, 1, 1), (1, 8, 8, 64, 512, 1, 1, 0, 1), (1, 8, 8, 64, 92, 3, 1, 1, 1),
    (1, 20, 20, 64, 96, 3, 1, 6, 6), (1, 12, 25, 24, 20, (1, 7), 1, (0, 3), 1), (1, 1, 2, 3, 32, 1, 1, 0, 1),
    (1, 128, 256, 256, 32, 1, 1, 0, 1), (1, 127, 129, 200, 32, 1, 1, 0, 1), (1, 128, 128, 192, 32, 1, 1, 0, 1),
    (1, 256, 256, 32, 32, 1, 1, 0, 1), (1, 192, 64, 64, 512, 1, 1, 0, 1),
]
DGRAD_S2_MAPS = [(1, 1), (1, 6), (2, 2), (5, 5), (6, 5), (17, 19)]
DGRAD_S2_K = [1, 2, 3, 4, 5, 7]
DGRAD_S2_EXTRA = [
    (2, 24, 20, 24, 16, 4, 2, 1, 1),           # the 4x4 / 2 deconvolution form: (2, 12, 10) -> (24, 20)
    (1, 361, 363, 32, 32, 3, 2, 1, 1),         # four classes of 181 x 182 .. 180 x 181 rows, all on 64 x 64 tiles
    (1, 511, 513, 32, 32, 3, 2, 1, 1),         # classes of 256x257 (cfg 3) .. 255x256 (cfg 2): different tile configs in one layer
    (1, 17, 19, 1, 4, (1, 7), 2, (0, 3), 1),   # 1x7: the odd rows have no tap (r0 = 1 >= R)
]
WGRAD_CASES = [
    (1, 1, 1, 4, 19, 1, 1, 0, 1),              # P = 1, J = 4, bm 32
    (1, 1, 31, 64, 32, 1, 1, 0, 1),            # P = 31, J = 64
    (1, 4, 8, 4, 33, 1, 1, 0, 1),              # P = 32, bm 64
    (1, 3, 11, 64, 64, 1, 1, 0, 1),            # P = 33
    (1, 1, 127, 64, 65, 1, 1, 0, 1),           # P = 127, bm 64 (Cout just past 64), J = 64
    (1, 8, 16, 64, 128, 1, 1, 0, 1),           # P = 128, bm 128, bn 64
    (1, 3, 43, 68, 132, 1, 1, 0, 1),           # P = 129, J = 68: bn 128, bm 64 (132)
    (1, 8, 16, 128, 192, 1, 1, 0, 1),          # bm 64 (192), J = 128
    (1, 8, 16, 132, 256, 1, 1, 0, 1),          # bm 128, bn 128, J = 132
    (1, 63, 65, 32, 256, 3, 1, 1, 1),          # P = 4095, J = 288
    (1, 17, 241, 200, 24, 3, 1, 1, 1),         # P = 4097, J = 1800
    (1, 127, 129, 4, 40, 1, 1, 0, 1),          # P = 16383, tiny J
    (1, 109, 151, 32, 64, 1, 1, 0, 1),         # P = 16384 + 64 + 11
    (1, 16449, 1, 32, 20, 1, 1, 0, 1),         # P = 16384 + 64 + 1
    (1, 33, 35, 36, 24, 3, 2, 1, 1),           # stride 2
    (1, 20, 20, 64, 96, 3, 1, 6, 6),           # dilation
]
WALK_CASES = [
    (2, 240, 281, 32, 64, 1, 1, 0, 1),         # 2108 tiles of 64 x 64 (the wide 256 x 64 member needs nk >= 4: conv_nt here)
    (2, 240, 281, 128, 64, 1, 1, 0, 1),        # ... and 527 tiles of the wide 256 x 64 member in f16x2
    (1, 363, 363, 32, 256, 1, 1, 0, 1),        # 1030 x 2 = 2060 tiles of 128 x 128, last of 57 rows
    (2, 240, 281, 64, 64, 1, 1, 0, 1),         # 2108 tiles of 64 x 64 in the data gradient too (its columns are Cin)
]
STEM_GENERAL = (1, 13, 511, 4, 64, 7, 2, 3, 1)      # the stem kernel's geometry: its plain f16x2 call runs conv_stem.h
WIDE_WALK = (1, 514, 511, 128, 128, 1, 1, 0, 1)     # 2052 tiles of the wide 128 x 128 member, the last of 126 rows
GENERAL_FWD = [FWD_TILE[1], FWD_TILE[0], FWD_TILE[4], FWD_TILE[9], FWD_TAPS[0], FWD_TAPS[3], FWD_TAPS[6], FWD_SPLIT[2], FWD_SPLIT[3],
               WIDE_CASES[1][0], WIDE_CASES[8][0], WIDE_CASES[11][0], STEM_GENERAL]
GENERAL_DGRAD = [DGRAD_S1[1], DGRAD_S1[4], DGRAD_S1[8], DGRAD_S2_EXTRA[0], (1, 17, 19, 36, 24, 3, 2, 1, 1)]
GENERAL_WGRAD = [WGRAD_CASES[5], WGRAD_CASES[9], WGRAD_CASES[10], WGRAD_CASES[13], WGRAD_CASES[14]]
# (the largest case is there for the wide 128 x 256 member: the variant that reaches it, and the bf16 tensors)
GENERAL_VARIANTS = {WIDE_CASES[11][0]: ("f16x2", "bf16t")}
BC_FWD = [FWD_TILE[1], FWD_TILE[6], FWD_TAPS[0], FWD_TAPS[10], FWD_SPLIT[2], WIDE_CASES[8][0], WIDE_CASES[14][0], STEM_GENERAL]
BC_DGRAD = [DGRAD_S1[6], DGRAD_S1[8], (1, 17, 19, 32, 32, 3, 2, 1, 1)]
BC_WGRAD = [WGRAD_CASES[3], WGRAD_CASES[5], WGRAD_CASES[9]]


def dgrad_s2_cases():
    out = []
    for k in DGRAD_S2_K:
        for pad in sorted({0, 1, k // 2}):
            for H, W in DGRAD_S2_MAPS:
                if H + 2 * pad >= k and W + 2 * pad >= k:
                    out.append((2 if H * W < 30 else 1, H, W, 8, 12, k, 2, pad, 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# section 1: the route table
def test_case_tables_cover_every_route():
    fwd = [R.fwd_route(c) for c in FWD_CASES]
    dg = [r for c in DGRAD_S1 for _, r in R.dgrad_routes(c)]
    for name, routes in (("forward", fwd), ("data gradient", dg)):
        for cfg in range(4):
            rs = [r for r in routes if r["cfg"] == cfg]
            assert any(r["row_rem"] == 0 for r in rs), f"{name}: no cfg {cfg} case with a full last row tile"
            assert any(r["row_rem"] != 0 for r in rs), f"{name}: no cfg {cfg} case with a ragged last row tile"
            assert any(r["col_rem"] != 0 for r in rs), f"{name}: no cfg {cfg} case with a ragged last column tile"
        assert any(r["splits"] == 1 and r["nk"] >= 16 for r in routes), f"{name}: no long-K case without a split"
        assert any(r["splits"] > 1 and r["last"] == r["per"] for r in routes), f"{name}: no split with equal slices"
        assert any(r["splits"] > 1 and r["last"] < r["per"] for r in routes), f"{name}: no split with a short last slice"
        # (piece planes = uniform taps in the "bf16x3" / "f16x2" variants of a float-tensor call: every case runs in all five
        # variants, so uniform taps on and off is planes on and off, and on with planes unused -- "fp32", "bf16", bf16 tensors)
        assert {r["uniform"] for r in routes} == {False, True}, f"{name}: UNIFORM_TAP is not both on and off"
    assert R.fwd_route(FWD_SPLIT[0])["nk"] == 15 and R.fwd_route(FWD_SPLIT[1])["nk"] == 16 and R.fwd_route(FWD_SPLIT[2])["nk"] == 26
    assert R.fwd_route(FWD_SPLIT[4])["nblk"] == 191 and R.fwd_route(FWD_SPLIT[4])["splits"] > 1
    assert R.fwd_route(FWD_SPLIT[5])["nblk"] == 192 and R.fwd_route(FWD_SPLIT[5])["splits"] == 1
    assert R.fwd_route(FWD_TILE[2])["nblk"] == 256 and R.fwd_route(FWD_TILE[2])["cfg"] == 0
    assert [R.fwd_route(c)["cfg"] for c in sorted(FULL_FLAGS, key=FWD_CASES.index)] == [2, 0, 3, 2]
    assert R.fwd_route(FWD_SPLIT[2])["splits"] > 1
    assert R.fwd_route(FWD_SPLIT[3])["splits"] == 30 and R.fwd_route(FWD_SPLIT[6])["splits"] == 32
    # a stride-2 layer whose classes land on different tile configs, classes without rows and without taps
    cfgs = {r["cfg"] for _, r in R.dgrad_routes(DGRAD_S2_EXTRA[2])}
    assert len(cfgs) > 1, "no stride-2 layer with classes on different tile configs"
    s2 = dgrad_s2_cases()
    assert any(hg * wg == 0 for c in s2 for _, hg, wg in R.dgrad_classes(c[0], c[1], c[2], 2)), "no class without rows"
    assert any(0 in R.dgrad_class_taps(c[5], c[7], 2, q) for c in s2 + DGRAD_S2_EXTRA for q in range(4)), "no class without taps"
    # weight gradient
    wg = [R.wgrad_route(c) for c in WGRAD_CASES]
    assert {(r["bm"], r["bn"]) for r in wg} == {(32, 128), (64, 128), (128, 64), (128, 128)}
    assert any(r["splits"] == 1 for r in wg) and any(r["splits"] > 1 for r in wg)
    assert any(r["splits"] > 1 and r["last"] < r["pps"] for r in wg), "no weight gradient with a short last split"
    assert any(r["P"] % 32 != 0 for r in wg) and any(r["P"] % 32 == 0 for r in wg)
    # the wide family: every member of the automatic choice, direct and staged epilogue, and the cases it must not take
    wide = {R.wide_route(c, fused=st) for c, st in WIDE_CASES}
    assert wide >= {None, (256, 64, True), (256, 64, False), (128, 128, True), (128, 128, False), (128, 256, True), (128, 256, False)}
    assert R.wide_route(WIDE_CASES[5][0], False) is None and R.wide_route(WIDE_CASES[6][0], True) is not None
    assert R.wide_route(WIDE_CASES[0][0], False) is None and R.wide_route(WIDE_CASES[3][0], True) is None
    # Cout = 128 on both sides of `nk < 4 && !(fused && nk >= 2)`: nk = 1 .. 4, with and without statistics
    c128 = {(c[3] // 32, st): R.wide_route(c, st) is not None for c, st in WIDE_CASES if c[4] == 128 and pair(c[5]) == (1, 1)}
    assert c128 == {(1, False): False, (1, True): False, (2, False): False, (2, True): True, (3, False): False, (3, True): True,
                    (4, False): True, (4, True): True}, c128
    # walks: more tiles than 8 workgroups x 256 CUs
    for c in WALK_CASES:
        r = R.fwd_route(c)
        assert r["nblk"] > 2048 and r["row_rem"] != 0, c
    assert any(r["nblk"] > 2048 and r["row_rem"] != 0 for c in WALK_CASES for _, r in R.dgrad_routes(c)), "no data-gradient walk"
    wr = R.wide_route(WIDE_WALK)
    Mw = WIDE_WALK[0] * WIDE_WALK[1] * WIDE_WALK[2]
    assert wr is not None and R.cdiv(Mw, wr[0]) * R.cdiv(WIDE_WALK[4], wr[1]) > 2048 and Mw % wr[0] != 0, "no walk on the wide family"


def test_restatement_agrees_with_the_library():
    """every decision the library exports, at the rows / columns of all case tables"""
    stale = "the restatement is stale"
    L = fn.L()
    for c in FWD_CASES + [w for w, _ in WIDE_CASES] + WALK_CASES + DGRAD_S1:
        for M, cols in ((c[0] * out_hw(c)[0] * out_hw(c)[1], c[4]), (c[0] * c[1] * c[2], c[3])):
            if cols % 4 == 0:
                tiles, rows = fn.conv_stats_layout(M, cols)
                assert (tiles, rows) == (R.cdiv(M, R.NT_BM[R.nt_config(M, cols)]), R.NT_BM[R.nt_config(M, cols)]), f"{stale}: nt_config({M}, {cols})"
    for c in DGRAD_S1 + dgrad_s2_cases() + DGRAD_S2_EXTRA:
        N, H, W, Cin, Cout, k, stride, pad, dil = c
        Cp = R.padc(Cin, 4)
        assert L.dspn_conv2d_dgrad_bn_tiles(N, H, W, Cp, stride) == R.dgrad_tiles(N, H, W, Cp, stride), f"{stale}: dgrad_tiles{c}"
    for c in WGRAD_CASES + FWD_CASES:
        N, H, W, Cin, Cout, k, stride, pad, dil = c
        (Ho, Wo), (kh, kw) = out_hw(c), pair(k)
        got = L.dspn_conv2d_wgrad_splits(N, Ho, Wo, R.padc(Cin, 4), Cout, kh, kw, stride)
        assert got == R.wgrad_route(c)["splits"], f"{stale}: wgrad_plan{c}: {got} != {R.wgrad_route(c)['splits']}"
    for M, C in ((1, 64), (12224, 64), (12288, 64), (100, 19)):
        assert L.dspn_conv2d_split_workspace_bytes(M, C) == 4 * R.split_workspace_floats(M, C), f"{stale}: split workspace"


# ---------------------------------------------------------------------------------------------------------------------
# device layouts
def act(t, dtype, ld=None):
    """float64 NCHW -> device NHWC with the channels zero-padded to a 16-byte chunk (or to ld)"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, ld or fn.padc(c, dtype), dtype=F64)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out.to(dtype).cuda()


def wgt(w, dtype):
    """float64 OIHW -> (float32 master (Cout, kh, kw, Cin padded), the forward operand in dtype)"""
    co, ci, kh, kw = w.shape
    m = torch.zeros(co, kh, kw, fn.padc(ci, dtype), dtype=F64)
    m[..., :ci] = w.permute(0, 2, 3, 1)
    m = m.float().cuda()
    return m, (m if dtype == F32 else m.to(BF))


def vec(t):
    return t.float().cuda()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def out_buffer(prior, C, ld, dtype):
    """an output of ld columns: the prior value (accumulate) or the sentinel in the first C, the sentinel in the rest"""
    n, h, w, _ = prior.shape
    o = torch.full((n, h, w, ld), SENTINEL, dtype=F64)
    o[..., :C] = prior
    return o.to(dtype).cuda()


class Failures:
    """collects the mismatches of one test so that every variant is reported before the test fails"""

    def __init__(self):
        self.msgs = []

    def exact(self, got, exp, C, what, bf16=False):
        """got (device, ..., ld) against the float64 reference (..., C): bit for bit; columns >= C keep the sentinel"""
        g = got.detach().cpu().double()
        e = bf16_of(exp) if bf16 else exp
        assert bf16 or torch.equal(e.float().double(), e), f"{what}: inputs unfit, the reference is not a float32 value"
        bad = g[..., :C] != e
        if bool(bad.any()):
            idx = tuple(int(v) for v in bad.nonzero()[0])
            self.msgs.append(f"{what}: {int(bad.sum())} of {e.numel()} elements differ from the float64 reference, first at {idx}: "
                             f"got {float(g[..., :C][idx])!r}, expected {float(e[idx])!r}; largest difference {float((g[..., :C] - e).abs().max()):.6g}")
        if g.shape[-1] > C and not bool((g[..., C:] == SENTINEL).all()):
            self.msgs.append(f"{what}: {int((g[..., C:] != SENTINEL).sum())} elements in columns >= {C} were written")

    def check(self, fun, *a, **kw):
        try:
            fun(*a, **kw)
        except AssertionError as err:
            self.msgs.append(str(err))

    def done(self):
        assert not self.msgs, "\n".join(self.msgs)


FLAGSETS = {"plain": (), "bias": ("bias",), "relu": ("relu",), "res": ("res",), "acc": ("acc",), "aff": ("aff",),
            "affrelu": ("affrelu",), "all": ("bias", "relu", "res", "acc", "affrelu")}


def fwd_expected(p, flags):
    """(float64 result in NHWC, S with the epilogue operands, the linear part) of the forward call with `flags`"""
    aff = 2 if "affrelu" in flags else 1 if "aff" in flags else 0
    lin, S = p.forward(aff)
    y, S = nhwc(lin).clone(), nhwc(S).clone()
    if "bias" in flags:
        y += p.bias; S += p.bias.abs()
    if "res" in flags:
        y += nhwc(p.res); S += nhwc(p.res).abs()
    if "acc" in flags:
        y += nhwc(p.prior); S += nhwc(p.prior).abs()
    return (y.clamp(min=0) if "relu" in flags else y), S


def fwd_call(p, variant, flags, ld=None, **kw):
    """the forward call of problem p -> the device output (N, Ho, Wo, ld)"""
    dtype, math, _ = vinfo(variant)
    N, H, W, Cin, Cout, k, stride, pad, dil = p.case
    master, w = wgt(p.w, dtype)
    ld = ld or fn.padc(Cout, dtype)
    prior = nhwc(p.prior) if "acc" in flags else torch.full_like(nhwc(p.prior), SENTINEL)
    out = out_buffer(prior, Cout, ld, dtype)
    aff = None
    if "aff" in flags or "affrelu" in flags:
        cp = fn.padc(Cin, dtype)
        sc, sh = torch.ones(cp, dtype=F64), torch.zeros(cp, dtype=F64)
        sc[:Cin], sh[:Cin] = p.scale, p.shift
        # (a pad channel holds 0 and shift 0: it stays 0)
        aff = (vec(sc), vec(sh), "affrelu" in flags)
    res = None
    if "res" in flags:
        res = out_buffer(nhwc(p.res), Cout, ld, dtype)
    return fn.conv2d_forward(act(p.x, dtype), w, vec(p.bias) if "bias" in flags else None, stride=stride, pad=pad, dil=dil,
                             relu="relu" in flags, out=out, accumulate="acc" in flags, residual=res, in_affine=aff, math=math, **kw)


def general_bar(variant, S, K, n_epilogue, extra=0.0):
    n_acc = NPROD[variant] * R.cdiv(K, 32) * 32 + 32
    return (n_acc * U + E_MODE[variant]) * S + n_epilogue * U * S + extra


def f16x2_abs_term(p, conv_abs_x_ones, conv_ones_abs_w, xmax, wmax):
    return 2.0 ** -39 * (xmax * conv_ones_abs_w + wmax * conv_abs_x_ones)


# ---------------------------------------------------------------------------------------------------------------------
# section 2: forward
@pytest.mark.parametrize("case", FWD_CASES, ids=str)
def test_forward_class_a_is_bit_exact(gpu_device, case):
    p, f = problem(case, "A"), Failures()
    Cout = case[4]
    names = list(FLAGSETS) if case in FULL_FLAGS else ["plain", "all"]
    for name in names:
        y, S = fwd_expected(p, FLAGSETS[name])
        R.assert_fit(S, 0.0, p.unit, f"forward {name}")
        for v in VARIANTS:
            f.exact(fwd_call(p, v, FLAGSETS[name]), y, Cout, f"forward[{v}, {name}]", bf16=(v == "bf16t"))
    f.done()


@pytest.mark.parametrize("cls", ["B1", "B2", "C1", "C2"])
@pytest.mark.parametrize("case", BC_FWD, ids=str)
def test_forward_second_and_third_piece_are_bit_exact(gpu_device, case, cls):
    p, f = problem(case, cls), Failures()
    for flags in ((), ("bias", "relu", "res", "acc")):
        y, S = fwd_expected(p, flags)
        R.assert_fit(S, 0.0, p.unit, f"forward class {cls}")
        for v in SPLIT_VARIANTS:
            f.exact(fwd_call(p, v, flags), y, case[4], f"forward[{v}, class {cls}, {'+'.join(flags) or 'plain'}]")
    f.done()


@pytest.mark.parametrize("case", GENERAL_FWD, ids=str)
def test_forward_general_values_within_the_bar(gpu_device, case):
    f = Failures()
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    K = pair(k)[0] * pair(k)[1] * R.padc(Cin, 4)
    for flags in ((), ("bias", "relu", "res", "acc", "affrelu")):
        for v in GENERAL_VARIANTS.get(case, VARIANTS):
            p = problem(case, "G", v in ("bf16", "bf16t"))
            y, S = fwd_expected(p, flags)
            extra = 0.0
            if flags:      # the affine's fmaf rounds the operand once
                extra = U * nhwc(p.conv((p.x * p.scale.view(1, -1, 1, 1)).abs() + p.shift.abs().view(1, -1, 1, 1), p.w.abs()))
            if v == "f16x2":
                xa = p.x if not flags else p.affine(p.x, True)
                extra = extra + 2.0 ** -39 * nhwc(float(xa.abs().max()) * p.conv(torch.ones_like(p.x), p.w.abs()) +
                                                  float(p.w.abs().max()) * p.conv(xa.abs(), torch.ones_like(p.w)))
            bar = general_bar(v, S, K, 3 if flags else 0, extra)
            got = fwd_call(p, v, flags)
            what = f"forward[{v}, general, {'all' if flags else 'plain'}]"
            if v == "bf16t":
                aff = p.affine(p.x, True) if flags else p.x
                e32 = nhwc(p.conv(aff.float(), p.w.float()))
                if flags:
                    e32 = (e32 + p.bias.float() + nhwc(p.res).float() + nhwc(p.prior).float()).clamp(min=0)
                f.check(bf16_within, got[..., :Cout], y, bar, e32, what, rare=K <= BF16T_GENERAL_K)
            else:
                f.check(within, got[..., :Cout].cpu().double(), y, bar, what)
    f.done()


def test_forward_into_wider_rows_keeps_the_other_columns(gpu_device):
    """out with ldc > pad4(Cout): Cout = 19 into 32 columns (cfg 2 and cfg 3), Cout = 64 into 96; plain and accumulate"""
    f = Failures()
    for case, ld in ((FWD_TILE[10], 32), (FWD_TILE[9], 32), ((1, 9, 11, 32, 64, 3, 1, 1, 1), 96), (FWD_SPLIT[2], 96)):
        p = problem(case, "A")
        for name in ("plain", "all"):
            y, S = fwd_expected(p, FLAGSETS[name])
            R.assert_fit(S, 0.0, p.unit, "wider rows")
            for v in VARIANTS:
                f.exact(fwd_call(p, v, FLAGSETS[name], ld=ld), y, case[4], f"forward[{v}, {name}, ldc {ld}] {case}", bf16=(v == "bf16t"))
    f.done()


def strided_forward(p, variant, y, chan0, ldc, batch_stride):
    """a test-local caller of dspn_conv2d_forward_bn_*: the result goes to y + chan0 with row stride ldc and the given batch stride"""
    dtype, math, _ = vinfo(variant)
    N, H, W, Cin, Cout, k, stride, pad, dil = p.case
    (kh, kw), (ph, pw), (Ho, Wo) = pair(k), pair(pad), out_hw(p.case)
    x = act(p.x, dtype)
    master, w = wgt(p.w, dtype)
    mcode = fn._math_code(math)
    xam = wam = planes = None
    if mcode == 3 and dtype == F32:
        xam, wam = fn.absmax(x), fn.absmax(w)
    if fn.needs_planes(dtype, x.shape[3], mcode):
        planes = fn.weight_planes(w, math=mcode, w_absmax=wam)
    ws = fn.workspace(fn.L().dspn_conv2d_split_workspace_bytes(N * Ho * Wo, Cout), x.device, "split")
    b = vec(p.bias)
    fn.check(fn._f("dspn_conv2d_forward_bn", x)(fn.ptr(x), 0, 0, 0, fn.ptr(w), fn.ptr(planes), fn.ptr(b), 0,
                                               y.data_ptr() + chan0 * y.element_size(), N, H, W, x.shape[3], Cout, kh, kw, stride, ph,
                                               pw, dil, Ho, Wo, batch_stride, ldc, 0, 0, 0, 0, 0, mcode, fn.ptr(xam), fn.ptr(wam),
                                               fn.ptr(ws), ws.numel(), fn.stream()), "conv2d_forward (strided)")


@pytest.mark.parametrize("chan0", [8, 3])
def test_forward_into_a_channel_slice(gpu_device, chan0):
    """Cout = 24 written into channels chan0 .. of a 40-channel tensor whose batch stride is larger than an image (chan0 = 3 turns
    the 16-byte epilogue off); everything outside the slice keeps its sentinel.  Class A exact, one general-value run to the bar."""
    f = Failures()
    case = (2, 9, 11, 20, 24, 3, 1, 1, 1)
    Ho, Wo = out_hw(case)
    rows = Ho * Wo + 5                               # 5 rows of slack between the images
    for cls in ("A", "G"):
        for v in VARIANTS:
            dtype = vinfo(v)[0]
            p = problem(case, cls, cls == "G" and v in ("bf16", "bf16t"))
            y, S = fwd_expected(p, ("bias",))
            buf = torch.full((2, rows, 40), SENTINEL, dtype=dtype, device="cuda")
            strided_forward(p, v, buf, chan0, 40, rows * 40)
            g = buf.cpu().double()
            inside = g[:, :Ho * Wo, chan0:chan0 + 24].reshape(2, Ho, Wo, 24).clone()
            g[:, :Ho * Wo, chan0:chan0 + 24] = SENTINEL
            if not bool((g == SENTINEL).all()):
                f.msgs.append(f"[{v}, class {cls}] {int((g != SENTINEL).sum())} elements outside the slice were written")
            what = f"forward[{v}, class {cls}, channels {chan0}..]"
            if cls == "A":
                R.assert_fit(S, 0.0, p.unit, what)
                f.exact(inside, y, 24, what, bf16=(v == "bf16t"))
            elif v == "bf16t":
                e32 = nhwc(p.conv(p.x.float(), p.w.float())) + p.bias.float()
                f.check(bf16_within, inside.to(BF), y, general_bar(v, S, 9 * 20, 1), e32, what)
            else:
                extra = 0.0
                if v == "f16x2":
                    extra = 2.0 ** -39 * nhwc(float(p.x.abs().max()) * p.conv(torch.ones_like(p.x), p.w.abs()) +
                                              float(p.w.abs().max()) * p.conv(p.x.abs(), torch.ones_like(p.w)))
                f.check(within, inside, y, general_bar(v, S, 9 * 20, 1, extra), what)
    f.done()


# ---------------------------------------------------------------------------------------------------------------------
# section 6 (used by the wide and stem tests too): per-tile statistics against float64 from the stored y
def check_tile_stats(f, y, st, mm, tile_rows, what):
    """y (M, C) as stored (class A: integers), st / mm (tiles, 2, C) from the same call"""
    yd = y.detach().cpu().double()
    M, C = yd.shape
    tiles = R.cdiv(M, tile_rows)
    assert st.shape[0] == tiles
    std, mmd = st.cpu().double(), (mm.cpu().double() if mm is not None else None)
    # every tile at once: rows past M are masked out of the sums and hold the tile's first row for the extremes
    pad = tiles * tile_rows - M
    blk = torch.cat([yd, torch.zeros(pad, C, dtype=F64)]).view(tiles, tile_rows, C)
    n = torch.full((tiles, 1), float(tile_rows), dtype=F64)
    n[-1, 0] = tile_rows - pad
    live = (torch.arange(tile_rows).view(1, -1, 1) < n.view(-1, 1, 1))
    V = (blk.abs() * live).max(1).values
    mean = (blk * live).sum(1) / n
    m2 = (((blk - mean.unsqueeze(1)) ** 2) * live).sum(1)
    f.check(within, std[:, 0], mean, 84 * U * V, f"{what}: mean of all {tiles} tiles (the last of {int(n[-1, 0])} rows)")
    f.check(within, std[:, 1], m2, 692 * U * n * V * V, f"{what}: M2 of all {tiles} tiles (the last of {int(n[-1, 0])} rows)")
    if mmd is not None:
        first = blk[:, :1].expand_as(blk)
        lo, hi = torch.where(live, blk, first).min(1).values, torch.where(live, blk, first).max(1).values
        bad = (mmd[:, 0] != lo) | (mmd[:, 1] != hi)
        if bool(bad.any()):
            f.msgs.append(f"{what}: extremes of {int(bad.sum())} (tile, column) pairs differ from those of the stored rows, first at {tuple(int(v) for v in bad.nonzero()[0])}")


STATS_CASES = [      # M % tile_rows in {0, 1, tile_rows - 1} for 64-, 128- and 256-row tiles
    (1, 16, 16, 32, 64, 1, 1, 0, 1), (1, 5, 13, 32, 64, 1, 1, 0, 1), (1, 7, 9, 32, 36, 1, 1, 0, 1),                 # 64 rows: 0, 1, 63
    (1, 128, 256, 32, 128, 1, 1, 0, 1), (1, 127, 129, 32, 256, 1, 1, 0, 1), (5, 29, 113, 32, 256, 1, 1, 0, 1),      # 128 rows: 0, 127, 1
    (1, 256, 256, 32, 32, 1, 1, 0, 1), (1, 255, 257, 32, 32, 1, 1, 0, 1), (1, 257, 255, 32, 20, 1, 1, 0, 1),        # 256 rows: 0, 255, 255
    (1, 1, 65537, 32, 32, 1, 1, 0, 1),                                                                            # 256 rows: 1
]


def test_stats_cases_sit_on_the_ragged_tiles():
    want = {64: set(), 128: set(), 256: set()}
    for c in STATS_CASES:
        r = R.fwd_route(c, fused=True)
        want[r["bm"]].add(r["row_rem"])
    assert want[64] >= {0, 1, 63} and want[128] >= {0, 1, 127} and want[256] >= {0, 1, 255}, want


@pytest.mark.parametrize("case", STATS_CASES, ids=str)
def test_tile_statistics_at_ragged_tiles(gpu_device, case):
    """out_stats (and out_minmax in "f16x2") of a class A call, with bias and residual, against float64 from the stored y"""
    p, f = problem(case, "A"), Failures()
    Cout = case[4]
    M = case[0] * out_hw(case)[0] * out_hw(case)[1]
    y_ref, S = fwd_expected(p, ("bias", "res"))
    R.assert_fit(S, 0.0, p.unit, "statistics")
    for v in VARIANTS:
        dtype = vinfo(v)[0]
        if fn.padc(Cout, dtype) != Cout:
            continue                                 # (statistics need a dense output: Cout = 20 and 36 are float-tensor cases)
        tiles, tile_rows = fn.conv_stats_layout(M, Cout)
        assert tile_rows == R.fwd_route(case, fused=True)["bm"] and tiles == R.cdiv(M, tile_rows), "the restatement is stale"
        st = torch.full((tiles, 2, Cout), float("nan"), device="cuda")
        mm = torch.full((tiles, 2, Cout), float("nan"), device="cuda") if v == "f16x2" else None
        y = fwd_call(p, v, ("bias", "res"), out_stats=st, out_minmax=mm)
        f.exact(y, y_ref, Cout, f"forward with statistics[{v}]", bf16=(v == "bf16t"))
        check_tile_stats(f, y.view(M, Cout), st, mm, tile_rows, f"[{v}]")
    f.done()


# ---------------------------------------------------------------------------------------------------------------------
# the wide family and the stem ("f16x2")
@pytest.mark.parametrize("case,stats", WIDE_CASES, ids=str)
def test_wide_family_automatic_choice_class_a(gpu_device, case, stats):
    """float operand and the same operand as piece planes from bn_apply_planes (integer scale and shift), with and without
    the statistics epilogue; plain, and bias + residual + ReLU (+ accumulate without statistics)"""
    p, f = problem(case, "A"), Failures()
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    M = N * out_hw(case)[0] * out_hw(case)[1]
    for flags in ((), ("bias", "relu", "res") + (() if stats else ("acc",))):
        y_ref, S = fwd_expected(p, flags)
        R.assert_fit(S, 0.0, p.unit, "wide")
        kw, st, mm = {}, None, None
        if stats:
            tiles, tile_rows = fn.conv_stats_layout(M, Cout)
            st, mm = (torch.full((tiles, 2, Cout), float("nan"), device="cuda") for _ in range(2))
            kw = dict(out_stats=st, out_minmax=mm)
        y = fwd_call(p, "f16x2", flags, **kw)
        f.exact(y, y_ref, Cout, f"wide[float operand, {'+'.join(flags) or 'plain'}]")
        if stats:
            check_tile_stats(f, y.view(M, Cout), st, mm, tile_rows, "wide[float operand]")
    # the A operand as piece planes: relu(x0 * scale + shift) written by bn_apply_planes; the reference is the affine forward
    y_ref, S = fwd_expected(p, ("affrelu",))
    R.assert_fit(S, 0.0, p.unit, "wide, planes")
    sc, sh, x0 = vec(p.scale), vec(p.shift), act(p.x, F32)
    am = fn.absmax(x0, (sc, sh, True))
    pl = fn.bn_apply_planes(x0, sc, sh, am, relu=True)
    master, w = wgt(p.w, F32)
    out = out_buffer(torch.full_like(nhwc(p.prior), SENTINEL), Cout, Cout, F32)
    kw, st, mm = {}, None, None
    if stats:
        tiles, tile_rows = fn.conv_stats_layout(M, Cout)
        st, mm = (torch.full((tiles, 2, Cout), float("nan"), device="cuda") for _ in range(2))
        kw = dict(out_stats=st, out_minmax=mm)
    y = fn.conv2d_forward(pl, w, None, stride=stride, pad=pad, dil=dil, out=out, math="f16x2", x_absmax=am, x_planes=True, **kw)
    f.exact(y, y_ref, Cout, "wide[piece planes]")
    if stats:
        check_tile_stats(f, y.view(M, Cout), st, mm, tile_rows, "wide[piece planes]")
    if (case, stats) in [WIDE_CASES[i] for i in PLANES_B1]:
        # piece 1 of the plane operand: class B1 (x = m 2^-6) through scale 1, shift 0 and the ReLU, all exact
        pb = problem(case, "B1")
        xr = pb.x.clamp(min=0)
        y_ref = nhwc(pb.conv(xr, pb.w))
        R.assert_fit(nhwc(pb.conv(xr, pb.w.abs())), 0.0, pb.unit, "wide, planes, class B1")
        x0 = act(pb.x, F32)
        sc, sh = torch.ones(x0.shape[3], device="cuda"), torch.zeros(x0.shape[3], device="cuda")
        am = fn.absmax(x0, (sc, sh, True))
        pl = fn.bn_apply_planes(x0, sc, sh, am, relu=True)
        out = out_buffer(torch.full_like(nhwc(pb.prior), SENTINEL), Cout, Cout, F32)
        y = fn.conv2d_forward(pl, wgt(pb.w, F32)[1], None, stride=stride, pad=pad, dil=dil, out=out, math="f16x2", x_absmax=am, x_planes=True)
        f.exact(y, y_ref, Cout, "wide[piece planes, class B1]")
    f.done()


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("nhw", STEM_CASES, ids=str)
def test_stem_kernel_class_a(gpu_device, nhw, stats):
    """7x7 / 2 pad 3 on 4 physical channels -> 64 in "f16x2": one output row, two, thirteen, and two images; the fourth channel
    carries values too (the kernel contracts over all four)"""
    N, H, W = nhw
    case = (N, H, W, 4, 64, 7, 2, 3, 1)
    p, f = problem(case, "A"), Failures()
    Ho, Wo = out_hw(case)
    M = N * Ho * Wo
    y_ref, S = fwd_expected(p, ())
    R.assert_fit(S, 0.0, p.unit, "stem")
    kw, st, mm = {}, None, None
    if stats:
        tiles, tile_rows = fn.conv_stats_layout(M, 64)
        st, mm = (torch.full((tiles, 2, 64), float("nan"), device="cuda") for _ in range(2))
        kw = dict(out_stats=st, out_minmax=mm)
    y = fwd_call(p, "f16x2", (), **kw)
    f.exact(y, y_ref, 64, f"stem {nhw}")
    if stats:
        check_tile_stats(f, y.view(M, 64), st, mm, tile_rows, f"stem {nhw}")
    f.done()


@pytest.mark.parametrize("case", [WIDE_CASES[8][0], FWD_TAPS[0]], ids=["wide", "generic"])
def test_out_absmax_is_the_stored_maximum(gpu_device, case):
    p = problem(case, "G")
    block = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    y = fwd_call(p, "f16x2", ("bias", "relu"), out_absmax=block)
    assert float(block.max()) == float(y[..., :case[4]].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# section 3: data gradient
def dgrad_call(p, variant, accumulate, ld=None):
    dtype, math, _ = vinfo(variant)
    N, H, W, Cin, Cout, k, stride, pad, dil = p.case
    master, _ = wgt(p.w, dtype)
    wt = fn.weight_transpose(master, dtype=dtype)
    cp = fn.padc(Cin, dtype)
    ld = ld or cp
    prior = nhwc(p.prior_dx) if accumulate else torch.full_like(nhwc(p.prior_dx), SENTINEL)
    out = out_buffer(prior, Cin, ld, dtype)
    if cp > Cin:
        out[..., Cin:cp] = 0          # the weight's pad rows are zero: a pad channel of dx receives + 0
    return fn.conv2d_dgrad(act(p.dy, dtype), wt, (N, H, W, ld), stride=stride, pad=pad, dil=dil, out=out, accumulate=accumulate,
                           math=math), cp


def dgrad_check(f, p, variants, label, ld=None):
    dx, S = p.dgrad()
    Cin = p.case[3]
    for acc in (False, True):
        exp = nhwc(dx) + (nhwc(p.prior_dx) if acc else 0.0)
        R.assert_fit(nhwc(S) + (nhwc(p.prior_dx).abs() if acc else 0.0), 0.0, p.unit, f"data gradient {label}")
        for v in variants:
            got, cp = dgrad_call(p, v, acc, ld)
            what = f"dgrad[{v}, {label}, {'accumulate' if acc else 'plain'}]"
            f.exact(got[..., :Cin], exp, Cin, what, bf16=(v == "bf16t"))
            g = got.cpu().double()
            if cp > Cin and not bool((g[..., Cin:cp] == 0).all()):
                f.msgs.append(f"{what}: pad channels of dx are not zero")
            if g.shape[-1] > cp and not bool((g[..., cp:] == SENTINEL).all()):
                f.msgs.append(f"{what}: columns >= {cp} were written")


@pytest.mark.parametrize("case", DGRAD_S1, ids=str)
def test_dgrad_stride1_class_a_is_bit_exact(gpu_device, case):
    p, f = problem(case, "A"), Failures()
    dgrad_check(f, p, VARIANTS, "class A")
    f.done()


def test_dgrad_into_wider_rows(gpu_device):
    f = Failures()
    for case, ld in (((1, 5, 13, 36, 20, 3, 1, 1, 1), 48), ((1, 64, 65, 20, 32, 1, 1, 0, 1), 32), ((1, 8, 8, 64, 92, 3, 1, 1, 1), 96)):
        dgrad_check(f, problem(case, "A"), VARIANTS, f"class A, ldc {ld}", ld)
    f.done()


@pytest.mark.parametrize("k", DGRAD_S2_K)
def test_dgrad_stride2_parity_classes_class_a(gpu_device, k):
    """k x k / 2 with pad in {0, 1, k // 2} on maps from 1 x 1 to 17 x 19: classes of different sizes, classes without rows,
    and (k = 1) classes without taps: zero-filled without accumulate, left alone with it"""
    f = Failures()
    for case in [c for c in dgrad_s2_cases() if c[5] == k]:
        dgrad_check(f, problem(case, "A"), VARIANTS, f"class A {case}")
    f.done()


@pytest.mark.parametrize("case", DGRAD_S2_EXTRA, ids=str)
def test_dgrad_stride2_layers_class_a(gpu_device, case):
    p, f = problem(case, "A"), Failures()
    dgrad_check(f, p, VARIANTS, "class A")
    f.done()


@pytest.mark.parametrize("cls", ["B1", "B2", "C1", "C2"])
@pytest.mark.parametrize("case", BC_DGRAD, ids=str)
def test_dgrad_second_and_third_piece_are_bit_exact(gpu_device, case, cls):
    p, f = problem(case, cls), Failures()
    dgrad_check(f, p, SPLIT_VARIANTS, f"class {cls}")
    f.done()


@pytest.mark.parametrize("case", GENERAL_DGRAD, ids=str)
def test_dgrad_general_values_within_the_bar(gpu_device, case):
    f = Failures()
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    K = pair(k)[0] * pair(k)[1] * R.padc(Cout, 4)
    for v in VARIANTS:
        p = problem(case, "G", v in ("bf16", "bf16t"))
        dx, S = p.dgrad()
        for acc in (False, True):
            exp = nhwc(dx) + (nhwc(p.prior_dx) if acc else 0.0)
            Sa = nhwc(S) + (nhwc(p.prior_dx).abs() if acc else 0.0)
            extra = 0.0
            if v == "f16x2":
                ones_w, ones_y = torch.ones_like(p.w), torch.ones_like(p.dy)
                x0 = torch.zeros_like(p.x, requires_grad=True)
                t1 = torch.autograd.grad(p.conv(x0, p.w.abs()), x0, ones_y)[0]
                t2 = torch.autograd.grad(p.conv(x0, ones_w), x0, p.dy.abs())[0]
                extra = 2.0 ** -39 * nhwc(float(p.dy.abs().max()) * t1 + float(p.w.abs().max()) * t2)
            bar = general_bar(v, Sa, K, 1 if acc else 0, extra)
            got, _ = dgrad_call(p, v, acc)
            what = f"dgrad[{v}, general, {'accumulate' if acc else 'plain'}]"
            if v == "bf16t":
                x0 = torch.zeros_like(p.x, dtype=F32, requires_grad=True)
                e32 = nhwc(torch.autograd.grad(p.conv(x0, p.w.float()), x0, p.dy.float())[0]) + (nhwc(p.prior_dx).float() if acc else 0.0)
                f.check(bf16_within, got[..., :Cin], exp, bar, e32, what, rare=K <= BF16T_GENERAL_K)
            else:
                f.check(within, got[..., :Cin].cpu().double(), exp, bar, what)
    f.done()


# ---------------------------------------------------------------------------------------------------------------------
# section 4: weight gradient
def ohwi(t):
    return t.permute(0, 2, 3, 1).contiguous()


def wgrad_operands(p, variant, affine, ldy=None):
    dtype, math, _ = vinfo(variant)
    Cin = p.case[3]
    aff = None
    if affine:
        cp = fn.padc(Cin, dtype)
        sc, sh = torch.ones(cp, dtype=F64), torch.zeros(cp, dtype=F64)
        sc[:Cin], sh[:Cin] = p.scale, p.shift
        aff = (vec(sc), vec(sh), True)
    return act(p.xg, dtype), act(p.dyg, dtype, ldy), aff, math, dtype


def wgrad_check(f, p, variants, label, affine=False, ldy=None, slabs=False, colsum=False):
    N, H, W, Cin, Cout, k, stride, pad, dil = p.case
    kh, kw = pair(k)
    dw, S = p.wgrad(2 if affine else 0)
    for acc in (False, True):
        exp = ohwi(dw) + (ohwi(p.prior_dw) if acc else 0.0)
        R.assert_fit(ohwi(S) + (ohwi(p.prior_dw).abs() if acc else 0.0), 0.0, p.unit, f"weight gradient {label}")
        for v in variants:
            x, dy, aff, math, dtype = wgrad_operands(p, v, affine, ldy)
            cp = x.shape[3]
            shape = (Cout, kh, kw, cp)
            out = torch.full(shape, SENTINEL, device="cuda")
            if acc:
                out.zero_()
                out[..., :Cin] = ohwi(p.prior_dw).float().cuda()
            got = fn.conv2d_wgrad(x, dy, shape, stride=stride, pad=pad, dil=dil, out=out, accumulate=acc, in_affine=aff, math=math)
            what = f"wgrad[{v}, {label}, {'accumulate' if acc else 'plain'}]"
            f.exact(got[..., :Cin], exp, Cin, what)
            if cp > Cin and not affine and not bool((got[..., Cin:] == 0).all()):
                f.msgs.append(f"{what}: the gradient of a pad channel (x == 0 there) is not zero")
            if slabs and not acc and dtype == F32:
                # the GEMM alone + the batched reduce: same bits as the one-call form; the slabs themselves sum to the reference
                n = fn.conv2d_wgrad_splits(tuple(x.shape), tuple(dy.shape), shape, stride)
                assert n == R.wgrad_route(p.case)["splits"], "the restatement is stale"
                sl = torch.full((n,) + shape, SENTINEL, device="cuda")
                fn.conv2d_wgrad_slabs(x, dy, shape, sl, stride=stride, pad=pad, dil=dil, in_affine=aff, math=math)
                f.exact(sl.double().sum(0)[..., :Cin], exp, Cin, f"{what}: sum of the {n} slabs")
                dw2 = torch.full(shape, SENTINEL, device="cuda")
                fn.slab_reduce_batch(*fn.slab_reduce_table([(sl, dw2, False)], x.device))
                if not torch.equal(dw2, got):
                    f.msgs.append(f"{what}: slabs + slab_reduce_batch differ from the one-call form")
            if colsum and not acc:
                cs = fn.colsum(dy, Cout).cpu().double()
                e = p.dyg.sum(dim=(0, 2, 3))
                if not torch.equal(cs, e):
                    f.msgs.append(f"colsum(dy)[{v}, {label}]: {int((cs != e).sum())} of {Cout} columns differ, worst {float((cs - e).abs().max()):.6g}")


@pytest.mark.parametrize("case", WGRAD_CASES, ids=str)
def test_wgrad_class_a_is_bit_exact(gpu_device, case):
    p, f = problem(case, "A"), Failures()
    dyabs = p.dyg.abs().sum(dim=(0, 2, 3))
    assert float(dyabs.max()) < R.FIT, "colsum: inputs unfit"
    wgrad_check(f, p, VARIANTS, "class A", slabs=True, colsum=True)
    f.done()


@pytest.mark.parametrize("case", [WGRAD_CASES[3], WGRAD_CASES[9], WGRAD_CASES[14]], ids=str)
def test_wgrad_input_affine_and_wider_dy_rows(gpu_device, case):
    p, f = problem(case, "A"), Failures()
    wgrad_check(f, p, VARIANTS, "class A, affine + ReLU", affine=True, slabs=True)
    wgrad_check(f, p, VARIANTS, "class A, ldy > Cout", ldy=fn.padc(case[4], BF) + 8, colsum=True)
    f.done()


@pytest.mark.parametrize("cls", ["B1", "B2", "C1", "C2"])
@pytest.mark.parametrize("case", BC_WGRAD, ids=str)
def test_wgrad_second_and_third_piece_are_bit_exact(gpu_device, case, cls):
    p, f = problem(case, cls), Failures()
    wgrad_check(f, p, SPLIT_VARIANTS, f"class {cls}", slabs=True)
    f.done()


@pytest.mark.parametrize("case", GENERAL_WGRAD, ids=str)
def test_wgrad_general_values_within_the_bar(gpu_device, case):
    f = Failures()
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    kh, kw = pair(k)
    P = N * out_hw(case)[0] * out_hw(case)[1]
    for v in VARIANTS:
        p = problem(case, "G", v in ("bf16", "bf16t"))
        dw, S = p.wgrad(0)
        x, dy, aff, math, dtype = wgrad_operands(p, v, False)
        shape = (Cout, kh, kw, x.shape[3])
        got = fn.conv2d_wgrad(x, dy, shape, stride=stride, pad=pad, dil=dil, math=math)
        extra = 0.0
        if v == "f16x2":
            w0 = torch.zeros_like(p.w, requires_grad=True)
            t1 = torch.autograd.grad(p.conv(torch.ones_like(p.xg), w0), w0, p.dyg.abs())[0]
            t2 = torch.autograd.grad(p.conv(p.xg.abs(), w0), w0, torch.ones_like(p.dyg))[0]
            extra = 2.0 ** -39 * ohwi(float(p.xg.abs().max()) * t1 + float(p.dyg.abs().max()) * t2)
        # (the slabs of the pixel split are added by the reduce: up to 1024 further additions)
        bar = general_bar(v, ohwi(S), P, R.wgrad_route(case)["splits"], extra)
        f.check(within, got[..., :Cin].cpu().double(), ohwi(dw), bar, f"wgrad[{v}, general]")
    f.done()


def test_wgrad_refuses_empty_weights_and_leaves_nothing_behind(gpu_device):
    """A weight gradient with Cout, R or S of 0 is refused on the host as bad geometry, before any launch (the slab count used to be
    workspace_bytes / (4 Cout R S Cin): a division by zero) -- real tensors, both float entries.  The ordinary call of the same
    shape that follows is bit-exact as ever (class A), in the one-call form and as slabs + reduce: the refused calls wrote
    nothing, parked nothing and left no error behind."""
    case = (1, 8, 8, 64, 64, 3, 1, 1, 1)
    p, f = problem(case, "A"), Failures()
    x, dy, _, _, _ = wgrad_operands(p, "fp32", False)
    assert x.shape == (1, 8, 8, 64) and dy.shape == (1, 8, 8, 64)
    lib = fn.L()
    out = torch.full((64, 3, 3, 64), SENTINEL, device="cuda")
    ws = fn.workspace(lib.dspn_conv2d_wgrad_workspace_bytes(1, 8, 8, 64, 64, 3, 3), x.device, "wgrad")
    for Cout, kh, kw in ((0, 3, 3), (64, 0, 3), (64, 3, 0)):
        geom = (1, 8, 8, 64, Cout, 64, kh, kw, 1, 1, 1, 1, 8, 8)
        rc = lib.dspn_conv2d_wgrad_bn_f32(fn.ptr(x), None, None, 0, fn.ptr(dy), fn.ptr(out), *geom, 0, 0, None, None,
                                          fn.ptr(ws), ws.numel(), fn.stream())
        assert rc == -1 and b"bad geometry" in lib.dspn_last_error(), (geom, rc, lib.dspn_last_error())
        rc = lib.dspn_conv2d_wgrad_slabs_f32(fn.ptr(x), None, None, 0, fn.ptr(dy), fn.ptr(out), out.numel() * 4, *geom, 0, None, None,
                                             fn.stream())
        assert rc == -1 and b"bad geometry" in lib.dspn_last_error(), (geom, rc, lib.dspn_last_error())
    assert bool((out == SENTINEL).all()), "a refused call wrote"
    wgrad_check(f, p, ("fp32",), "class A, after refused calls", slabs=True)
    f.done()


# ---------------------------------------------------------------------------------------------------------------------
# section 5: launch settings that must not change results
@pytest.fixture
def reserved_cus():
    def set_(n):
        fn.check(fn.L().dspn_conv_set_reserved_cus(int(n)), "conv_set_reserved_cus")
    yield set_
    set_(0)


@pytest.mark.parametrize("case", WALK_CASES, ids=str)
def test_persistent_grid_walk_and_reserved_cus(gpu_device, reserved_cus, case):
    """more tiles than any grid holds (> 8 workgroups x 256 CUs), a ragged last tile: forward and stride-1 data gradient, class A
    exact with 0 and with 128 reserved CUs; a general-value run bit-identical between the two settings"""
    f = Failures()
    pa, pg = problem(case, "A"), problem(case, "G")
    y, S = fwd_expected(pa, ("bias", "relu"))
    R.assert_fit(S, 0.0, pa.unit, "walk")
    general = {}
    for cus in (0, 128):
        reserved_cus(cus)
        for v in VARIANTS:
            f.exact(fwd_call(pa, v, ("bias", "relu")), y, case[4], f"forward[{v}, class A, {cus} reserved CUs]", bf16=(v == "bf16t"))
        if any(r["nblk"] > 2048 for _, r in R.dgrad_routes(case)):      # (the data gradient walks where ITS tiles outnumber the grid)
            dgrad_check(f, pa, ("f16x2", "bf16t"), f"class A, {cus} reserved CUs")
        for v in ("f16x2", "bf16x3"):
            g = fwd_call(pg, v, ("bias",))
            if cus == 0:
                general[v] = g
            elif not torch.equal(general[v], g):
                f.msgs.append(f"forward[{v}, general]: {int((general[v] != g).sum())} elements depend on the reserved CUs")
    f.done()


def test_wide_family_walk_and_reserved_cus(gpu_device, reserved_cus):
    """2052 tiles of the wide 128 x 128 member ("f16x2", 1x1, Cin = Cout = 128), the last of 126 rows: class A exact with 0 and
    with 128 reserved CUs, a general-value run bit-identical between the two settings.  (Its own operands, not a Problem: at
    this size only what the test uses is made.)"""
    N, H, W, Cin, Cout = WIDE_WALK[:5]
    g = torch.Generator().manual_seed(514511)
    xa = torch.randint(-6, 7, (N, H, W, Cin), generator=g).double()
    wa = torch.randint(-6, 7, (Cout, 1, 1, Cin), generator=g).double()
    bias = torch.randint(-5, 6, (Cout,), generator=g).double()
    S = xa.abs().view(-1, Cin) @ wa.abs().view(Cout, Cin).t() + bias.abs()
    R.assert_fit(S, 0.0, 1.0, "wide walk")
    y = (xa.view(-1, Cin) @ wa.view(Cout, Cin).t() + bias).clamp(min=0).view(N, H, W, Cout)
    xg, wg = torch.randn(N, H, W, Cin, generator=g), torch.randn(Cout, 1, 1, Cin, generator=g) / Cin ** 0.5
    f, first = Failures(), None
    xa, wa, bias, xg, wg = xa.float().cuda(), wa.float().cuda(), bias.float().cuda(), xg.cuda(), wg.cuda()
    for cus in (0, 128):
        reserved_cus(cus)
        out = torch.full((N, H, W, Cout), SENTINEL, device="cuda")
        f.exact(fn.conv2d_forward(xa, wa, bias, relu=True, out=out, math="f16x2"), y, Cout, f"forward[f16x2, class A, {cus} reserved CUs]")
        gq = fn.conv2d_forward(xg, wg, bias, math="f16x2")
        if first is None:
            first = gq
        elif not torch.equal(first, gq):
            f.msgs.append(f"forward[f16x2, general]: {int((first != gq).sum())} elements depend on the reserved CUs")
    f.done()
