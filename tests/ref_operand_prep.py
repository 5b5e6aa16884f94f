"""Plain numpy restatements of the stand-alone kernels that prepare the operands of the two-piece ("f16x2") convolution math:
the magnitude passes (absmax, its batch form, the affine bound), the range guard's bookkeeping (smallest row magnitude of a
weight, per-tile extremes), the split-K slab sum and the fp16 / bf16 piece planes of a weight.  Host only; nothing here
calls the library.  tests/test_operand_prep_host.py checks the restatements themselves, tests/test_operand_prep_edges_gpu.py
holds the kernels to them bit for bit.

The input builders of the affine magnitude cases live here too, so that the host test can assert on the very inputs the GPU
test uses that float64 arithmetic reproduces the kernel's fmaf exactly."""
import numpy as np

F32, F64 = np.float32, np.float64
SLOTS = 64                      # include/dspn_nn.h DSPN_ABSMAX_SLOTS
NONFINITE = F32(3.0e38)         # csrc/dspn_pieces.h operand_scale: a slot that is not below this says "the tensor holds an inf"


# ---------------------------------------------------------------------------------------------------------------------
# magnitudes
def affine_f64(x, scale, shift, relu):
    """(relu)(x * scale[c] + shift[c]) in float64, x (..., C).  Equal to the kernel's fmaf wherever the float64 value is a
    float32 (affine_is_exact): a product of two float32 is exact in float64, and on a dyadic grid so is the sum.
    fmaxf(u, 0) of the ReLU turns a NaN into 0."""
    with np.errstate(invalid="ignore"):
        u = x.astype(F64) * scale.astype(F64) + shift.astype(F64)
    return np.fmax(u, 0.0) if relu else u


def affine_is_exact(x, scale, shift):
    """does every x * scale + shift of the case round-trip through float32 (NaNs aside)?"""
    u = affine_f64(x, scale, shift, False)
    with np.errstate(invalid="ignore"):
        back = u.astype(F32).astype(F64)
    return bool(np.all((back == u) | np.isnan(u)))


def absmax_ref(x, scale=None, shift=None, relu=False):
    """float32 value of max |u|, u = x or (relu)(x * scale[c] + shift[c]); NaNs skipped (fmaxf), infinities kept; 0 for a
    tensor without a non-zero number"""
    u = x.astype(F64) if scale is None else affine_f64(x, scale, shift, relu)
    m = np.fmax.reduce(np.abs(u).reshape(-1), initial=0.0)
    return F32(0.0) if np.isnan(m) else F32(m)


def affine_bound_f64(scale, shift, m):
    """max_c |scale[c]| * m + |shift[c]| in float64 (NaN if a coefficient is)"""
    with np.errstate(invalid="ignore"):
        return float(np.max(np.abs(scale.astype(F64)) * float(m) + np.abs(shift.astype(F64))))


def absmin_rows_ref(w):
    """min over the rows of w (rows, row_len) of max |w[row]|, NaNs skipped inside a row, over the rows with
    0 < max < inf only; +inf when no row qualifies"""
    w = np.asarray(w, F32).reshape(w.shape[0], -1)
    m = np.fmax.reduce(np.abs(w), axis=1, initial=F32(0.0))
    ok = (m > 0) & (m < np.inf)
    return F32(m[ok].min()) if ok.any() else F32(np.inf)


def tile_minmax_ref(x, tile_rows):
    """x (rows, C) -> (tiles, 2, C): fmin / fmax (NaN skipped) of each channel over each tile of tile_rows rows; a channel
    that is all NaN in a tile keeps the initial values +inf / -inf"""
    rows, C = x.shape
    tiles = -(-rows // tile_rows)
    out = np.empty((tiles, 2, C), F32)
    for t in range(tiles):
        blk = x[t * tile_rows:(t + 1) * tile_rows]
        out[t, 0] = np.fmin.reduce(blk, axis=0, initial=F32(np.inf))
        out[t, 1] = np.fmax.reduce(blk, axis=0, initial=F32(-np.inf))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# split-K slab sum
def slab_sum_ref(slabs, dw=None, accumulate=False):
    """slabs (splits, n) float32 -> float32 sum in the kernels' order, one rounding per add: slab[0] + slab[1] + ... +
    slab[splits - 1], then the prior dw last when accumulating"""
    slabs = np.asarray(slabs, F32)
    s = slabs[0].copy()
    for k in range(1, slabs.shape[0]):
        s = s + slabs[k]            # float32 + float32: one IEEE add
    if accumulate:
        s = s + np.asarray(dw, F32)
    assert s.dtype == F32
    return s


# ---------------------------------------------------------------------------------------------------------------------
# piece planes
def operand_scale_ref(block):
    """the power of two csrc/dspn_pieces.h operand_scale() derives from a 64-slot magnitude block: from the slots below 3e38
    only (an inf slot only says "an inf is in there"; a NaN compares false and drops out too), 2^(15 - e) with
    max = f 2^e, 0.5 <= f < 1, the exponent clamped to [-100, 100]; 1 when no slot is a positive finite number"""
    b = np.asarray(block, F32).reshape(-1)
    assert b.size == SLOTS
    with np.errstate(invalid="ignore"):
        b = np.where(b < NONFINITE, b, F32(0.0))
    m = np.fmax.reduce(b, initial=F32(0.0))
    if not m > 0:
        return F32(1.0)
    e = 15 - int(np.frexp(F32(m))[1])
    return F32(np.ldexp(F32(1.0), max(-100, min(100, e))))


def _planes_layout(pieces):
    """[piece][row][tap][col] -> [row][tap][col / 32][piece][32]"""
    n, rows, taps, cols = pieces.shape
    return np.ascontiguousarray(pieces.reshape(n, rows, taps, cols // 32, 32).transpose(1, 2, 3, 0, 4))


def planes2_ref(m, block):
    """m (rows, taps, cols % 32 == 0) float32 -> the float16 planes [row][tap][col / 32][2][32] of the two-piece cut:
    u = m * operand_scale(block) in float32, h0 = fp16(u), h1 = fp16(u - h0), and repair_inf: where h0 is infinite (an infinite
    element, or one the block does not bound) the pieces are h0 = +-65504, h1 = +-inf"""
    s = operand_scale_ref(block)
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.asarray(m, F32) * s
        h0 = u.astype(np.float16)
        h1 = (u - h0.astype(F32)).astype(np.float16)
    inf = np.isinf(h0)
    h1 = np.where(inf, h0, h1)
    h0 = np.where(inf, np.copysign(np.float16(65504.0), h0), h0)
    return _planes_layout(np.stack([h0, h1]))


def bf16_bits(x):
    """float32 -> the 16 bits of its bfloat16 (round to nearest even), as uint16; finite values and infinities"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(F32)


def planes3_ref(m):
    """m (rows, taps, cols % 32 == 0) float32 -> the bits (uint16) of the bfloat16 planes [row][tap][col / 32][3][32]:
    p0 = bf16(m), p1 = bf16(m - p0), p2 = bf16(m - p0 - p1)"""
    m = np.asarray(m, F32)
    p0 = bf16_bits(m)
    r1 = m - bf16_value(p0)
    p1 = bf16_bits(r1)
    p2 = bf16_bits(r1 - bf16_value(p1))
    return _planes_layout(np.stack([p0, p1, p2]))


def transposed_operand(w, cols):
    """w (Cout, R, S, Cin) -> (Cin, R * S, cols) zero padded: the matrix whose planes the data gradient reads"""
    Cout, R, S, Cin = w.shape
    wt = np.zeros((Cin, R * S, cols), F32)
    wt[:, :, :Cout] = np.asarray(w, F32).reshape(Cout, R * S, Cin).transpose(2, 1, 0)
    return wt


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def wide_values(shape, rng):
    """randn * exp(4 randn): a wide exponent spread, so that a changed order of additions changes bits"""
    return (rng.standard_normal(shape) * np.exp(4.0 * rng.standard_normal(shape))).astype(F32)


AFFINE_KINDS = ("tiny_scale", "shift_only", "negative_extreme", "nan_scale")
AFFINE_SHAPES = ((5, 64), (32769, 64), (7, 12), (174763, 12))     # (rows, C): see test_operand_prep_edges_gpu.py


def affine_case(kind, rows, C, seed=0):
    """-> x (rows, C), scale (C), shift (C) float32 on a coarse dyadic grid (small integers times powers of two: x * scale +
    shift is exact in float32, so float64 arithmetic gives the fmaf's number).  The planted element sits in the LAST row, which
    the two-trip shapes reach only on the second grid trip.
      tiny_scale        the largest |x| (2^12) sits in a channel whose scale is 2^-20
      shift_only        x = 0; the extreme is one shift, negative
      negative_extreme  the largest |u| is negative (a ReLU removes it: the largest positive value is the answer then)
      nan_scale         as negative_extreme, and one channel's scale is NaN"""
    rng = np.random.default_rng(seed + 1000 * AFFINE_KINDS.index(kind) + rows + C)
    x = rng.integers(-6, 7, (rows, C)).astype(F32) * F32(0.125)
    scale = rng.choice(np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], F32), C)
    shift = rng.integers(-4, 5, C).astype(F32) * F32(0.25)
    c = C // 2 + 1
    if kind == "tiny_scale":
        scale[c], shift[c] = F32(2.0 ** -20), F32(0.0)
        x[:, c] = 0.0
        x[rows - 1, c] = F32(4096.0)
    elif kind == "shift_only":
        x[:] = 0.0
        shift[c] = F32(-7.25)
    else:
        scale[c], shift[c] = F32(2.0), F32(0.5)
        x[rows - 1, c] = F32(-40.0)                 # u = -79.5
        scale[c - 1], shift[c - 1] = F32(-1.0), F32(0.25)
        x[rows - 1, c - 1] = F32(-9.0)              # u = +9.25: the largest positive value
        if kind == "nan_scale":
            scale[0] = F32(np.nan)
    return x, scale, shift
