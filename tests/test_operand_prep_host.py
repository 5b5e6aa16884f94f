"""The numpy restatements of tests/ref_operand_prep.py on their own (no GPU): each against hand-worked values or an
independent evaluation, and the exactness precondition of the affine magnitude cases on the very inputs the GPU test uses."""
import math

import numpy as np
import pytest
import torch

import ref_operand_prep as P

F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("rows,C", P.AFFINE_SHAPES)
@pytest.mark.parametrize("kind", P.AFFINE_KINDS)
def test_affine_cases_are_exact_in_float32(kind, rows, C):
    """x * scale + shift of every element round-trips through float32: float64 arithmetic gives the fmaf's number"""
    x, scale, shift = P.affine_case(kind, rows, C)
    assert x.dtype == scale.dtype == shift.dtype == F32
    assert P.affine_is_exact(x, scale, shift)
    off, on = P.absmax_ref(x, scale, shift, False), P.absmax_ref(x, scale, shift, True)
    assert float(abs(x).max()) == {"tiny_scale": 4096.0, "shift_only": 0.0}.get(kind, 40.0)
    if kind == "tiny_scale":
        assert float(off) <= 2.5                                         # the large x does not show
    else:
        assert float(off) == (7.25 if kind == "shift_only" else 79.5)
    if kind in ("negative_extreme", "nan_scale"):
        assert float(on) == 9.25                                          # the ReLU removed the -79.5
    if kind == "shift_only":
        assert float(on) == max(float(shift.max()), 0.0)


def test_absmax_ref_skips_nans_and_keeps_infinities():
    x = np.array([[1.0, -3.0, NAN, 2.0]], F32)
    assert float(P.absmax_ref(x)) == 3.0
    assert float(P.absmax_ref(np.array([[NAN, NAN, -0.0, 0.0]], F32))) == 0.0
    assert float(P.absmax_ref(np.array([[1.0, -INF, NAN, 2.0]], F32))) == INF
    sc, sh = np.array([2.0, NAN, -1.0, 1.0], F32), np.array([0.5, 0.0, 0.0, -8.0], F32)
    assert float(P.absmax_ref(x, sc, sh, False)) == 6.0            # 2.5, NaN (skipped), NaN, -6
    assert float(P.absmax_ref(x, sc, sh, True)) == 2.5             # the ReLU removes the -6 and turns the NaNs into 0
    assert not P.affine_is_exact(np.array([[1.0]], F32), np.array([1.0], F32), np.array([2.0 ** -30], F32))


@pytest.mark.parametrize("splits", [1, 2, 15, 16, 17, 18, 32, 33, 49])
def test_slab_sum_ref_is_a_float32_sum_close_to_float64(splits):
    rng = np.random.default_rng(splits)
    slabs, dw = P.wide_values((splits, 1200), rng), P.wide_values((1200,), rng)
    for acc in (False, True):
        got = P.slab_sum_ref(slabs, dw, acc)
        terms = np.concatenate([slabs, dw[None]]) if acc else slabs
        partial = np.abs(np.cumsum(terms.astype(F64), axis=0)).max(axis=0)
        exact = terms.astype(F64).sum(axis=0)
        ulp = np.spacing(partial.astype(F32)).astype(F64)
        assert got.dtype == F32 and np.all(np.abs(got.astype(F64) - exact) <= splits * ulp)
    a = np.array([[2.0 ** 24], [1.0], [1.0]], F32)                # order shows: (2^24 + 1) + 1 = 2^24, 1 + 1 + 2^24 = 2^24 + 2
    assert float(P.slab_sum_ref(a)[0]) == 2.0 ** 24 and float(P.slab_sum_ref(a[::-1])[0]) == 2.0 ** 24 + 2
    assert float(P.slab_sum_ref(a[1:], a[0], True)[0]) == 2.0 ** 24 + 2      # the prior value is added LAST


def test_absmin_rows_ref_counts_only_rows_with_a_finite_non_zero_maximum():
    tiny = 3 * 2.0 ** -149
    w = np.array([[0.0, -0.0, 0.0], [1.0, INF, 2.0], [NAN, NAN, NAN], [0.0, -tiny, 0.0], [0.5, NAN, -4.0], [3.0, 1.0, 0.25]], F32)
    assert float(P.absmin_rows_ref(w)) == tiny
    assert float(P.absmin_rows_ref(w[[0, 1, 2, 4, 5]])) == 3.0
    assert float(P.absmin_rows_ref(w[:3])) == INF


def test_tile_minmax_ref_skips_nans_and_keeps_the_initial_values():
    x = np.array([[1.0, NAN, -INF, 4.0], [-2.0, NAN, 5.0, NAN], [3.0, 7.0, NAN, NAN]], F32)
    out = P.tile_minmax_ref(x, 2)
    assert out.shape == (2, 2, 4)
    assert out[0, 0].tolist() == [-2.0, INF, -INF, 4.0] and out[0, 1].tolist() == [1.0, -INF, 5.0, 4.0]
    assert out[1, 0].tolist() == [3.0, 7.0, INF, INF] and out[1, 1].tolist() == [3.0, 7.0, -INF, -INF]


def test_operand_scale_ref_reads_the_finite_slots_and_clamps():
    def block(**slots):
        b = np.zeros(P.SLOTS, F32)
        for k, v in slots.items():
            b[int(k[1:])] = v
        return b
    assert float(P.operand_scale_ref(block())) == 1.0
    assert float(P.operand_scale_ref(block(s5=1.0))) == 2.0 ** 14            # 1 = 0.5 2^1 -> 2^14: the maximum lands on 2^14
    assert float(P.operand_scale_ref(block(s5=1.0, s63=1.999))) == 2.0 ** 14
    assert float(P.operand_scale_ref(block(s0=2.0))) == 2.0 ** 13
    assert float(P.operand_scale_ref(block(s0=INF, s9=3.0))) == 2.0 ** 13      # the scale comes from the finite slots
    assert float(P.operand_scale_ref(block(s0=INF))) == 1.0
    assert float(P.operand_scale_ref(block(s0=3.0e38))) == 1.0                 # float32(3e38) is not below the threshold
    assert float(P.operand_scale_ref(block(s0=np.nextafter(F32(3.0e38), F32(0))))) == 2.0 ** -100     # 15 - 128, clamped
    assert float(P.operand_scale_ref(block(s1=2.0 ** -140))) == 2.0 ** 100     # 15 + 139, clamped
    for m in (0.75, 1.0, 1000.0, 2.0 ** -30 * 1.5):
        assert 2.0 ** 14 <= m * float(P.operand_scale_ref(block(s7=m))) < 2.0 ** 15


def test_planes_refs_agree_with_torch_and_reconstruct_the_value():
    rng = np.random.default_rng(5)
    m = P.wide_values((5, 2, 64), rng)
    blk = np.zeros(P.SLOTS, F32)
    blk[11] = np.abs(m).max()
    e = 15 - math.frexp(float(blk[11]))[1]
    t = torch.from_numpy(m)
    u = t * 2.0 ** e
    h0 = u.half()
    h1 = (u - h0.float()).half()
    exp = torch.stack([h0, h1]).view(2, 5, 2, 2, 32).permute(1, 2, 3, 0, 4).contiguous().numpy()
    got = P.planes2_ref(m, blk)
    assert got.dtype == np.float16 and got.shape == (5, 2, 2, 2, 32) and np.array_equal(got.view(np.uint16), exp.view(np.uint16))
    assert np.all(np.isfinite(got)) and float(np.abs(got[:, :, :, 0]).max()) < 2.0 ** 15
    back = got.astype(F64).sum(axis=3).reshape(5, 2, 64) * 2.0 ** -e
    big = np.abs(m) >= np.abs(m).max() * 2.0 ** -10                  # (far below the maximum the error is absolute)
    assert np.all(np.abs(back - m)[big] <= 2.0 ** -22 * np.abs(m)[big])
    # three bf16 pieces: torch's round-to-nearest-even conversions
    p0 = t.bfloat16(); r1 = t - p0.float(); p1 = r1.bfloat16(); p2 = (r1 - p1.float()).bfloat16()
    exp3 = torch.stack([p0, p1, p2]).view(3, 5, 2, 2, 32).permute(1, 2, 3, 0, 4).contiguous().view(torch.int16).numpy()
    assert np.array_equal(P.planes3_ref(m).view(np.int16), exp3)
    # an infinite element, and one the block does not bound: h0 = +-65504, h1 = +-inf
    m2 = np.zeros((1, 1, 32), F32)
    m2[0, 0, :4] = [INF, -INF, 8.0, -1.0]
    blk2 = np.zeros(P.SLOTS, F32)
    blk2[0], blk2[1] = INF, 1.0
    g2 = P.planes2_ref(m2, blk2)[0, 0, 0]
    assert g2[0, :4].tolist() == [65504.0, -65504.0, 65504.0, -(2.0 ** 14)] and g2[1, :4].tolist() == [INF, -INF, INF, 0.0]


def test_transposed_operand_is_the_zero_padded_permutation():
    w = np.arange(2 * 3 * 1 * 4, dtype=F32).reshape(2, 3, 1, 4)
    wt = P.transposed_operand(w, 32)
    assert wt.shape == (4, 3, 32) and float(np.abs(wt[:, :, 2:]).max()) == 0.0
    assert all(wt[c, t, k] == w[k, t, 0, c] for c in range(4) for t in range(3) for k in range(2))
