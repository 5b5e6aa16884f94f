"""Element-wise comparison helpers of the float64-parity modules (test_bn_edges_gpu.py, test_conv_edges_gpu.py): the spacing
of float32, round-to-nearest-even bfloat16 of a float64, a derived per-element bar with nothing excluded, and the rule for a
bfloat16 result (rule 4 of test_bn_edges_gpu.py's docstring)."""
import torch

from bf16_twins import BF

U = 2.0 ** -24                       # unit roundoff of float32
F64 = torch.float64


def ulp32(v):
    """spacing of float32 at |v| (float64 tensor; 0 at 0)"""
    v = v.abs().float().double()
    _, e = torch.frexp(v)
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 24))


def bf16_of(v):
    """round-to-nearest-even bfloat16 of a float64 tensor, straight from the float64 bits (8 of the 53 significant bits stay)"""
    b = v.contiguous().view(torch.int64)
    return ((b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)).view(F64)


def within(got, exp, bound, what):
    """element-wise derived bound on float64 tensors of one shape; nothing is excluded"""
    err = (got - exp).abs()
    print(f"    {what}: worst err {float(err.max()):.3e}, largest bar {float(torch.as_tensor(bound).max()):.3e}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    over = err - bound
    assert not bool((over > 0).any()), f"{what}: {int((over > 0).sum())} over the bar, worst by {float(over.max()):.3e}"


def bf16_within(got, exp, bound, emul32, what, rare=True):
    """rule 4 of test_bn_edges_gpu.py's docstring for a bfloat16 result; emul32: a float32 CPU evaluation of the same quantity.
    rare=False: without the third clause (fewer than 1e-3 of the results differ from bf16(reference)) and its pre-check"""
    assert got.dtype == BF
    r, n = bf16_of(exp), exp.numel()
    pre = int((emul32.to(BF).double() != r).sum())
    assert not rare or pre < 1e-3 * n or pre <= 1, f"{what}: the inputs are unfit, float32 and float64 references differ in {pre} of {n} bf16 results"
    g = got.cpu().double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite result"
    lo, hi = bf16_of(exp - bound), bf16_of(exp + bound)
    out = int(((g < lo) | (g > hi)).sum())
    step = ulp32(r) * 65536.0
    # (where the float bar itself exceeds half a bf16 step -- a dx that cancels to almost nothing -- [lo, hi] above is the bar)
    far = int((((g - r).abs() > step) & (bound <= 0.5 * step)).sum())
    diff = int((g != r).sum())
    print(f"    {what}: {diff} of {n} differ from bf16(reference) (CPU float32 evaluation: {pre}), {out} outside the bar, "
          f"{far} further than one bf16 step; worst err {float((g - exp).abs().max()):.3e}")
    assert out == 0 and far == 0 and (not rare or diff < 1e-3 * n or diff <= 1), what
