"""The BatchNorm kernels of dspnet_amd/csrc/nn.hip at their dispatch edges, against plain float64 references written here
(torch CPU / numpy; never another kernel of this library).  A BatchNorm is a chain
    x -> (mean, rstd) -> (scale, shift) -> y        and        x, dy -> (dbeta, dgamma, coefficients) -> dx
and every link is checked against float64 evaluated from the kernel's OWN float outputs of the link before, so a bar holds the
roundings of one link only; the first link is also checked end to end against float64 on x alone.  No element and no channel
is left out of any comparison.  U = 2^-24 is the unit roundoff of float32, "ulp" the spacing of float32 at the reference.

Bars (each is exact, or a count of roundings times U times the magnitudes they apply to; none comes from a run):
 1. statistics, exact-sum inputs: integer x with |x - x[row 0]| <= 6 on a per-channel integer offset of at most 1000.  A
    slab partial of bn_stats_partial_kernel adds at most 512 terms of at most 6 resp. 36: far below 2^24, every float sum is
    exact, the finalize is double.  mean: 1 ulp, rstd: 2 ulp of 1 / sqrt(var + float32(eps)) -- one dropped or doubled row shows.
 2. statistics, general inputs (K = row 0, the kernel's shift): a slab sum is a chain of at most slab_rows float operations
    (the subtraction and slab_rows - 1 additions), the slabs are added in double:
      mean:  slab_rows U mean|x - K|  +  U |mean|               (the last term: the result's own rounding to float)
      var:   slab_rows U (mean (x - K)^2 + 2 |mean(x - K)| mean|x - K|)   (the second term: the error of the shifted mean
             m through var = SS / n - m^2), carried to rstd = (var + eps)^-1/2 by evaluating it at var -+ bar, plus 1 ulp.
    A constant channel has x - K == 0: both bars collapse to the result's rounding, var is 0 and rstd = 1 / sqrt(eps) to 1 ulp.
 3. scale == float32(gamma) * rstd bit for bit (one rounding); shift within 1 ulp of |beta| + |mean scale| (`fp contract(fast)`
    leaves the compiler free to fuse beta - mean * scale or not: two half-ulp roundings at most).
 4. y within 1 ulp of float32(x scale + shift) evaluated in float64, then ReLU (the kernel's fmaf rounds once; the float64
    evaluation rounds twice).  bf16 tensors: got == round-to-nearest-even bf16 of SOME value within the float bar of the
    reference, at most one bf16 step from bf16(reference) wherever the float bar is below half such a step (everywhere for y),
    and fewer than 1e-3 of the elements differ from bf16(reference) at all (checked first on the CPU: a float32 evaluation
    rounded to bf16 differs from the float64 one less often than that).  The rule itself admits the float ambiguity, so ONE
    such element passes also where the tensor has fewer than 1000 (the 7-row tensors of the one-tile sum tables).
    out_absmax: `.max()` of the block == max|y| of the kernel's y, bit for bit.
 5. The ReLU mask.  The backward recomputes it as fmaf(x, scale, shift) > 0.  The reference is double(x) double(scale) +
    double(shift) > 0 on the kernel's float scale / shift: the product of two floats is exact in double and a double sum
    keeps the sign of a non-zero exact value, as the single rounding of fmaf does -- the two masks are IDENTICAL for every
    element, none is excluded.  Elements with x scale + shift == 0 exactly are constructed: mask 0, y == +0, dx masked.
 6. dbeta = sum dy', dgamma = sum dy' (x - mean) rstd from the kernel's mean / rstd and the reference mask.  dy is integer
    valued, so dbeta is exact up to its final rounding: 1 ulp.  dgamma: (slab_rows + 3) U sum|dy' xhat| (three roundings per
    term, slab_rows - 1 additions, the result's rounding).
 7. dx = a dy' + c1 x + c0, a = gamma rstd, c1 = -a rstd SS / n, c0 = -a S / n - c1 mean in float64 (bn_final_channel's formula)
    from the kernel's float mean / rstd / gamma and the float64 sums S, SS.  Per element
      4 U (|a dy'| + |c1 x| + |c0|)  +  |x| dc1 + dc0,   dc1 = |a rstd| / n dSS,   dc0 = |a| / n dS + |mean| dc1
    (a coefficient's rounding to float, the product, two additions; dS = 0 for integer dy, dSS = the bar of 6).
    accumulate: + the prior dx, + one rounding of the result.  dx_absmax: block max == max|dx| as stored.  bf16: as in 4.
 Tile tables.  (mean, M2) tables ungrouped (< 1024 tiles): one double sweep, mean 1 ulp, rstd 2 ulp of the float64 merge of
 the float table.  Grouped: the group table is float, mean_g and M2_g carry one rounding each:
      mean:  U sum (n_g / n) |m_g|;     var:  sum (n_g / n) 2 U |m_g| |m_g - m|  +  U sum M2_g / n      (first order; the
 derivative of sum n_g (m_g - m)^2 by m vanishes at the mean), from the reference's own group means.  The same formula one
 level down (tiles for groups) bounds the distance of the table's statistics from those of x itself.  Plain-sum tables: the
 double sum of float entries is exact to 2^-50 sum|entries| ungrouped; grouped sums are rounded to float: U sum|entries|.
 Piece planes of dx: the dx bar plus the two-piece cut's 2^-21 of the block scale; the block must bound max|dx|."""
import ctypes

import numpy as np
import pytest
import torch

from dspnet_amd import functional as fn
from bf16_twins import BF
from fp_bars import ulp32, bf16_of, within, bf16_within

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 2e-5
EPS32 = float(np.float32(EPS))       # the entry points take eps as a float
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def slab_rows_for(rows):
    """rows per slab of the two-stage reductions (nn.hip slab_rows_for); checked against dspn_bn_workspace_bytes below"""
    return min(512, max(32, ((rows + 1023) // 1024 + 7) // 8 * 8))


def slabs_of(rows, C):
    """the slab count the library uses, read back from its workspace size: 4 * (slabs * 2 * C + 4 * C) bytes"""
    return (fn.L().dspn_bn_workspace_bytes(rows, C) // 4 - 4 * C) // (2 * C)


def h64(t):
    return t.detach().cpu().double()


def dev(t, dtype=torch.float32):
    return t.to(dtype).contiguous().cuda()


def nanvec(C):
    return torch.full((C,), float("nan"), device="cuda")


def block_max(block):
    return float(block.max())


SENTINEL = 12352.0      # (a bfloat16 value too) what an output holds before the call: an element left unwritten shows


class BwdRef:
    """float64 backward of one BatchNorm from the float mean / rstd / scale / shift it is GIVEN (float64 copies of floats)"""

    def __init__(self, x, dy, mean, rstd, scale, shift, relu):
        self.x, self.n, self.mean, self.rstd = x, x.shape[0], mean, rstd
        self.mask = (x * scale + shift) > 0 if relu else torch.ones_like(x, dtype=torch.bool)     # bar 5: identical to fmaf > 0
        self.dyp = torch.where(self.mask, dy, torch.zeros_like(dy))
        t = self.dyp * ((x - mean) * rstd)
        self.S, self.SS, self.absT = self.dyp.sum(0), t.sum(0), t.abs().sum(0)

    def dx(self, gamma, S=None, SS=None, dS=0.0, dSS=0.0):
        """-> (dx, per-element bar, float32 CPU evaluation); gamma None: fix_gamma, the coefficients use 1"""
        S, SS = self.S if S is None else S, self.SS if SS is None else SS
        a = self.rstd if gamma is None else gamma * self.rstd
        c1 = -a * self.rstd * (SS / self.n)
        c0 = -a * (S / self.n) - c1 * self.mean
        dc1 = (a * self.rstd).abs() / self.n * dSS          # the propagation of the two sums' bars:
        dc0 = a.abs() / self.n * dS + self.mean.abs() * dc1  # c1 is linear in SS, c0 in S and c1
        t1, t2 = a * self.dyp, c1 * self.x
        bar = 4 * U * (t1.abs() + t2.abs() + c0.abs()) + self.x.abs() * dc1 + dc0
        emul = a.float() * self.dyp.float() + c1.float() * self.x.float() + c0.float()
        return t1 + t2 + c0, bar, emul


def gamma_beta(C, g):
    gamma = (torch.rand(C, generator=g) + 0.5).double()
    gamma[1::5] *= -1.0                                    # negative scales among them
    return gamma.float().double(), torch.randn(C, generator=g).float().double()


def int_dy(shape, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


# ---------------------------------------------------------------------------------------------------------------------
# links 1, 2, 3, 4, 6, 7 at the slab and channel-group boundaries
def exact_sum_input(rows, C, g):
    """bar 1: offset + {0..3}, and offset + 6 (a spike) in every other channel of the first row, the last row, the first and
    the last row of the last slab and one row in the middle"""
    off = torch.randint(-1000, 1001, (C,), generator=g).double()
    off[0] = 0.0
    x = off + torch.randint(0, 4, (rows, C), generator=g).double()
    sr = slab_rows_for(rows)
    for k, r in enumerate(sorted({0, rows - 1, (rows - 1) // sr * sr, rows // 2})):
        x[r, (k % 2)::2] = off[(k % 2)::2] + 6.0
    assert float((x - x[0]).abs().max()) <= 6.0
    return x


def general_input(rows, C, g):
    """bar 2: per-channel std 1e-3 .. 1e3, |mean| / std 1 .. 1e4 (independently ordered), one constant channel"""
    std = 10.0 ** (torch.linspace(-3, 3, C).double()[torch.randperm(C, generator=g)])
    ratio = 10.0 ** (torch.linspace(0, 4, C).double()[torch.randperm(C, generator=g)])
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    x = sign * ratio * std + std * torch.randn(rows, C, generator=g).double()
    x[:, C // 2] = 7.25
    return x.float().double()                              # what the device is given, exactly


# (rows, C): the branch each is there for
STAT_SHAPES = [(1, 4), (1, 20),          # rows = 1: var = 0, dx finite.  C = 4: 256 row lanes, most without a row; C = 20: CL = 5, one idle thread
               (2, 4), (2, 20),          # rows < 32: one short slab
               (31, 4), (31, 20),
               (32, 4), (32, 20),        # exactly one slab
               (33, 4), (33, 20),        # rows = 32 k + 1: a last slab of one row
               (1025, 4), (1025, 20),    # 33 slabs (not a multiple of the finalize's 16 slab lanes), last slab of one row
               (257, 260),               # C4 = 65: the second blockIdx.y has one active channel group; the finalize's fifth block has four channels
               (70, 2048),               # non-fixed apply (C4 = 512), 32 finalize blocks
               (600_011, 4),             # 512-row slabs, 1172 slabs, partial last
               (40_000, 48)]             # slab_rows 40, non-fixed apply (C4 = 12)


def test_slab_geometry_is_what_the_bars_assume(gpu_device):
    for rows, C in STAT_SHAPES:
        sr = slab_rows_for(rows)
        assert slabs_of(rows, C) == -(-rows // sr), (rows, C)
    assert slab_rows_for(600_011) == 512 and slab_rows_for(40_000) == 40 and -(-600_011 // 512) == 1172


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("rows,C", STAT_SHAPES)
def test_chain_at_slab_and_channel_boundaries(gpu_device, rows, C, relu):
    g = torch.Generator().manual_seed(1000 * C + rows + int(relu))
    sr = slab_rows_for(rows)
    gamma, beta = gamma_beta(C, g)
    dy = int_dy((rows, C), g)
    for kind in ("exact", "general"):
        print(f"  [{kind}]")
        x = exact_sum_input(rows, C, g) if kind == "exact" else general_input(rows, C, g)
        xd, dyd, gd, bd = dev(x).view(1, 1, rows, C), dev(dy).view(1, 1, rows, C), dev(gamma), dev(beta)
        mean, rstd, scale, shift = fn.bn_stats(xd, EPS, gd, bd, mean=nanvec(C), rstd=nanvec(C), scale=nanvec(C), shift=nanvec(C))
        mk, rk, sk, hk = h64(mean), h64(rstd), h64(scale), h64(shift)
        # links 1 / 2: against float64 on x alone
        m_ref = x.mean(0)
        var_ref = ((x - m_ref) ** 2).mean(0)
        r_ref = 1.0 / torch.sqrt(var_ref + EPS32)
        if kind == "exact":
            m_bar, r_bar = ulp32(m_ref), 2 * ulp32(r_ref)
        else:
            d = x - x[0]
            m_bar = sr * U * d.abs().mean(0) + U * m_ref.abs()
            v_bar = sr * U * ((d * d).mean(0) + 2 * d.mean(0).abs() * d.abs().mean(0))
            r_bar = torch.maximum(1.0 / torch.sqrt((var_ref - v_bar).clamp(min=0) + EPS32) - r_ref,
                                  r_ref - 1.0 / torch.sqrt(var_ref + v_bar + EPS32)) + ulp32(r_ref)
            assert float(var_ref[C // 2]) == 0.0 and float(r_bar[C // 2]) == float(ulp32(r_ref)[C // 2])   # the constant channel
        within(mk, m_ref, m_bar, "mean")
        within(rk, r_ref, r_bar, "rstd")
        if rows == 1:
            assert torch.equal(mk, x[0]) and torch.equal(rk, torch.full_like(rk, 1.0 / np.sqrt(EPS32)).float().double())
        # link 3, from the kernel's own mean / rstd
        assert torch.equal(scale.cpu(), gamma.float() * rstd.cpu()), "scale != float32(gamma) * rstd"
        within(hk, beta - mk * sk, ulp32(beta.abs() + (mk * sk).abs()), "shift")
        _, _, s1, h1 = fn.bn_stats(xd, EPS, None, bd)                       # gamma = None: scale is rstd itself
        assert torch.equal(s1, rstd)
        within(h64(h1), beta - mk * rk, ulp32(beta.abs() + (mk * rk).abs()), "shift (fix_gamma)")
        # link 4, from the kernel's own scale / shift
        block = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
        y = fn.bn_apply(xd, scale, shift, relu=relu, out=torch.full_like(xd, SENTINEL), out_absmax=block)
        y_ref = (x * sk + hk).float().double()
        y_ref = y_ref.clamp(min=0) if relu else y_ref
        within(h64(y).view(rows, C), y_ref, ulp32(y_ref), "y")
        assert block_max(block) == float(y.abs().max())
        # links 6 / 7, from the kernel's mean / rstd / scale / shift
        ref = BwdRef(x, dy, mk, rk, sk, hk, relu)
        dSS = (sr + 3) * U * ref.absT
        for gm, gmd, name in ((None, None, "fix_gamma"), (gamma, gd, "gamma")):
            am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
            dx, dgam, dbet = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gmd, relu=relu, dx=torch.full_like(xd, SENTINEL),
                                            dgamma=nanvec(C), dbeta=nanvec(C), dx_absmax=am)
            within(h64(dbet), ref.S, ulp32(ref.S), f"dbeta ({name})")
            within(h64(dgam), ref.SS, dSS, f"dgamma ({name})")
            dx_ref, dx_bar, _ = ref.dx(gm, dSS=dSS)
            within(h64(dx).view(rows, C), dx_ref, dx_bar, f"dx ({name})")
            assert block_max(am) == float(dx.abs().max()), "dx_absmax"
        # (gamma given from here on) accumulate, and the outputs that may be left out
        prior = torch.randn(rows, C, generator=g).double()
        acc, _, _ = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, dx=dev(prior).view(1, 1, rows, C), accumulate=True)
        exp = dx_ref + prior
        within(h64(acc).view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), "dx accumulate")
        none, dg2, db2 = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, dx=fn.NO_OUTPUT)
        assert none is None and torch.equal(dg2, dgam) and torch.equal(db2, dbet), "dx = NO_OUTPUT changed dgamma / dbeta"
        dx3, n1, n2 = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, dgamma=fn.NO_OUTPUT, dbeta=fn.NO_OUTPUT)
        assert n1 is None and n2 is None and torch.equal(dx3, dx), "dgamma / dbeta = NO_OUTPUT changed dx"


# ---------------------------------------------------------------------------------------------------------------------
# link 5: elements that sit at y == 0 exactly
@pytest.mark.parametrize("rows,C", [(33, 20), (1025, 4), (300, 64)])
def test_relu_mask_at_exact_zero(gpu_device, rows, C):
    """x integer, scale a small dyadic number, shift = -scale * k: x == k gives x * scale + shift == 0 exactly.  There the mask
    is 0 (strictly greater), the forward y is +0 and dx takes the masked branch; dy is LARGE there, so the unmasked branch
    would be an O(1000) error in dx, dbeta and dgamma"""
    g = torch.Generator().manual_seed(rows + C)
    scale = torch.tensor([0.5, -0.25, 1.5, 2.0 ** -10])[torch.arange(C) % 4].double()
    k = torch.randint(-3, 4, (C,), generator=g).double()
    shift = -(scale * k)
    x = torch.randint(-8, 9, (rows, C), generator=g).double()
    x[0] = k                                                # at least one zero per channel
    zero = x == k
    assert bool(((x * scale + shift) == 0).eq(zero).all()) and int(zero.sum()) >= C
    dy = int_dy((rows, C), g)
    dy[zero] = 1000.0
    mean, rstd = x.mean(0).float().double(), (1.0 / torch.sqrt(x.var(0, unbiased=False) + EPS32)).float().double()
    gamma, _ = gamma_beta(C, g)
    xd, dyd = dev(x).view(1, 1, rows, C), dev(dy).view(1, 1, rows, C)
    sd, hd, md, rd, gd = dev(scale), dev(shift), dev(mean), dev(rstd), dev(gamma)
    y = fn.bn_apply(xd, sd, hd, relu=True, out=torch.full_like(xd, SENTINEL)).cpu().view(rows, C)
    assert torch.equal(y.double(), (x * scale + shift).clamp(min=0)), "every value here is exact"
    assert not bool(y[zero].any()) and not bool(torch.signbit(y[zero]).any()), "y must be +0 where x * scale + shift == 0"
    ref = BwdRef(x, dy, mean, rstd, scale, shift, True)
    assert not bool(ref.mask[zero].any())
    sr = slab_rows_for(rows)
    dSS = (sr + 3) * U * ref.absT
    dx, dgam, dbet = fn.bn_backward(xd, sd, hd, dyd, md, rd, gd, relu=True, dx=torch.full_like(xd, SENTINEL))
    within(h64(dbet), ref.S, ulp32(ref.S), "dbeta")
    within(h64(dgam), ref.SS, dSS, "dgamma")
    dx_ref, dx_bar, _ = ref.dx(gamma, dSS=dSS)
    within(h64(dx).view(rows, C), dx_ref, dx_bar, "dx")
    assert float((1000.0 * (gamma * rstd).abs()).min()) > 100 * float(dx_bar.max()), "the unmasked branch would not show"


# ---------------------------------------------------------------------------------------------------------------------
# links 4, 5, 7 at the dispatch sizes of the apply passes
U1_CAP4 = 4096 * 256             # float4 (16-byte) elements one launch of the chunked apply kernels covers at U = 1 ...
U4_CAP4 = 4096 * 4 * 256         # ... and at U = 4, before their grid-stride loop
APPLY_CAP4 = 8192 * 256          # bn_apply_kernel / bn_apply8_kernel: grid_for's cap

# (rows, C, also bf16)
APPLY_SHAPES = [(8192 + 3, 256, False),      # n4 = 524 480: U = 1, fixed, partial last chunk
                (16_384 + 5, 256, False),    # n4 just past 1 048 576: U = 1 past the 4096-workgroup cap, the stride loop runs
                (32_768 + 5, 256, True),     # n4 = 2 097 472: U = 4 with a partial last chunk; past bn_apply_kernel's grid_for cap
                (65_536 + 37, 256, True),    # n4 = 4 196 672: U = 4 past the cap, stride loop and tail together
                (87_400, 96, False)]         # n4 = 2 097 600: U = 4, non-fixed (C4 = 24)


def test_apply_shapes_meet_their_branches():
    n4 = [r * c // 4 for r, c, _ in APPLY_SHAPES]
    assert n4[0] < U1_CAP4 and n4[0] % 256 and U1_CAP4 < n4[1] < 2_097_152 <= n4[2] < U4_CAP4 < n4[3]
    assert n4[2] % 1024 and n4[3] % 1024 and n4[2] > APPLY_CAP4 and n4[4] >= 2_097_152 and 256 % (96 // 4)
    assert n4[3] // 2 >= 2_097_152 and n4[3] // 2 > APPLY_CAP4          # bf16, 16-byte elements: U = 4, past grid_for's cap


@pytest.mark.parametrize("rows,C,half", APPLY_SHAPES)
def test_apply_passes_at_their_dispatch_sizes(gpu_device, rows, C, half):
    g = torch.Generator().manual_seed(rows + C)
    n = rows * C
    # bf16-representable x, prior and (integer) dy: the float and the bf16 tensors hold the same values
    x = (torch.randn(n, generator=g) * 1.5 + 0.5).to(BF).float()
    dy = torch.randint(-8, 9, (n,), generator=g).float()
    prior = torch.randn(n, generator=g).to(BF).float()
    # distinctive values in the last 1024 float4 and in the first chunk of every second stride the tensor reaches: a skipped
    # or twice-written element there is an O(1) error
    for c4 in (U1_CAP4, U4_CAP4, APPLY_CAP4, n // 4 - 1024):
        if 0 <= c4 < n // 4:
            sl = slice(4 * c4, min(n, 4 * (c4 + 1024)))
            x[sl] = 6.0
            dy[sl] = torch.where(torch.arange(sl.stop - sl.start) % 2 == 0, 64.0, -64.0)
    gamma, beta = gamma_beta(C, g)
    xd, dyd, gd, bd = x.view(1, 1, rows, C).cuda(), dy.view(1, 1, rows, C).cuda(), dev(gamma), dev(beta)
    mean, rstd, scale, shift = fn.bn_stats(xd, EPS, gd, bd)
    mk, rk, sk, hk = h64(mean), h64(rstd), h64(scale), h64(shift)
    x64 = x.double().view(rows, C)
    # link 4
    y_ref = (x64 * sk + hk).clamp(min=0)
    y32 = y_ref.float().double()
    block = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    y = fn.bn_apply(xd, scale, shift, relu=True, out=torch.full_like(xd, SENTINEL), out_absmax=block)
    within(h64(y).view(rows, C), y32, ulp32(y32), "y")
    assert block_max(block) == float(y.abs().max())
    del y
    # links 5 - 7
    ref = BwdRef(x64, dy.double().view(rows, C), mk, rk, sk, hk, True)
    dSS = (slab_rows_for(rows) + 3) * U * ref.absT
    dx_ref, dx_bar, emul = ref.dx(gamma, dSS=dSS)
    am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    dx, dgam, dbet = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=True, dx=torch.full_like(xd, SENTINEL), dx_absmax=am)
    within(h64(dbet), ref.S, ulp32(ref.S), "dbeta")
    within(h64(dgam), ref.SS, dSS, "dgamma")
    within(h64(dx).view(rows, C), dx_ref, dx_bar, "dx")
    assert block_max(am) == float(dx.abs().max()), "dx_absmax"
    del dx
    p64 = prior.double().view(rows, C)
    exp = dx_ref + p64
    acc_bar = dx_bar + U * (exp.abs() + dx_bar)
    acc, _, _ = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=True, dx=prior.view(1, 1, rows, C).cuda(), accumulate=True)
    within(h64(acc).view(rows, C), exp, acc_bar, "dx accumulate")
    del acc
    if half:
        xh, dyh = xd.to(BF), dyd.to(BF)
        assert torch.equal(xh.float(), xd) and torch.equal(dyh.float(), dyd)
        yh = fn.bn_apply(xh, scale, shift, relu=True, out=torch.full_like(xh, SENTINEL))
        bf16_within(yh.view(rows, C), y_ref, ulp32(y_ref), y_ref.float(), "y (bf16)")
        dxh, dgh, dbh = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=True, dx=torch.full_like(xh, SENTINEL))
        within(h64(dbh), ref.S, ulp32(ref.S), "dbeta (bf16)")
        within(h64(dgh), ref.SS, dSS, "dgamma (bf16)")
        bf16_within(dxh.view(rows, C), dx_ref, dx_bar, emul, "dx (bf16)")
        acch, _, _ = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=True, dx=prior.view(1, 1, rows, C).to(BF).cuda(),
                                    accumulate=True)
        bf16_within(acch.view(rows, C), exp, acc_bar, emul + prior.view(rows, C), "dx accumulate (bf16)")


# ---------------------------------------------------------------------------------------------------------------------
# which bf16 kernel a call takes
def _small_case(C, seed, rows=77):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.5).to(BF).float()
    dy = torch.randint(-8, 9, (rows, C), generator=g).float()
    prior = torch.randn(rows, C, generator=g).to(BF).float()
    gamma, beta = gamma_beta(C, g)
    return x, dy, prior, gamma, beta


@pytest.mark.parametrize("C", [24, 40,       # the 16-byte path; C / 8 does not divide 256: its non-fixed branch
                               20,           # C % 8 != 0: the 4-wide kernels
                               64])          # the 16-byte path, fixed
def test_bf16_path_selection(gpu_device, C):
    rows = 77
    x, dy, prior, gamma, beta = _small_case(C, 500 + C)
    xh, dyh, gd, bd = dev(x, BF).view(1, 1, rows, C), dev(dy, BF).view(1, 1, rows, C), dev(gamma), dev(beta)
    mean, rstd, scale, shift = fn.bn_stats(xh, EPS, gd, bd)
    mk, rk, sk, hk = h64(mean), h64(rstd), h64(scale), h64(shift)
    x64 = x.double()
    sr = slab_rows_for(rows)
    d = x64 - x64[0]
    m_ref = x64.mean(0)
    within(mk, m_ref, sr * U * d.abs().mean(0) + U * m_ref.abs(), "mean (bf16 x)")
    for relu in (False, True):
        y_ref = x64 * sk + hk
        y_ref = y_ref.clamp(min=0) if relu else y_ref
        yh = fn.bn_apply(xh, scale, shift, relu=relu, out=torch.full_like(xh, SENTINEL))
        bf16_within(yh.view(rows, C), y_ref, ulp32(y_ref), y_ref.float(), f"y relu={relu}")
        ref = BwdRef(x64, dy.double(), mk, rk, sk, hk, relu)
        dSS = (sr + 3) * U * ref.absT
        dx_ref, dx_bar, emul = ref.dx(gamma, dSS=dSS)
        dxh, dgh, dbh = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=relu, dx=torch.full_like(xh, SENTINEL))
        within(h64(dbh), ref.S, ulp32(ref.S), "dbeta")
        within(h64(dgh), ref.SS, dSS, "dgamma")
        bf16_within(dxh.view(rows, C), dx_ref, dx_bar, emul, f"dx relu={relu}")
        exp = dx_ref + prior.double()
        acch, _, _ = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=relu, dx=dev(prior, BF).view(1, 1, rows, C), accumulate=True)
        bf16_within(acch.view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), emul + prior, f"dx accumulate relu={relu}")


def test_bf16_operands_off_16_byte_alignment(gpu_device):
    """x, dy, dx, y as views that start 8 bytes into a larger buffer: the 4-wide kernels run instead of the 16-byte ones, with
    bit for bit the result of the aligned call on the same values (which test_bf16_path_selection holds to float64), and the
    bytes in front of and behind each view stay as they were"""
    rows, C = 77, 64
    x, dy, prior, gamma, beta = _small_case(C, 564)
    n = rows * C

    def off8(t, fill=-7.0):
        buf = torch.full((n + 16,), fill, dtype=BF, device="cuda")
        buf[4:4 + n] = t.reshape(-1).to(BF).cuda()
        v = buf[4:4 + n].view(1, 1, rows, C)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return buf, v

    def untouched(buf, fill=-7.0):
        return bool((buf[:4] == fill).all()) and bool((buf[4 + n:] == fill).all())

    xa, dya, gd, bd = dev(x, BF).view(1, 1, rows, C), dev(dy, BF).view(1, 1, rows, C), dev(gamma), dev(beta)
    assert xa.data_ptr() % 16 == 0 and dya.data_ptr() % 16 == 0
    (xb, xv), (dyb, dyv) = off8(x), off8(dy)
    mean, rstd, scale, shift = fn.bn_stats(xa, EPS, gd, bd)
    for got, exp in zip(fn.bn_stats(xv, EPS, gd, bd), (mean, rstd, scale, shift)):
        assert torch.equal(got, exp)
    ya = fn.bn_apply(xa, scale, shift, relu=True)
    yb, yv = off8(torch.zeros(n))
    fn.bn_apply(xv, scale, shift, relu=True, out=yv)
    assert torch.equal(yv, ya) and untouched(yb)
    for acc in (False, True):
        dxa, dga, dba = fn.bn_backward(xa, scale, shift, dya, mean, rstd, gd, relu=True, dx=dev(prior, BF).view(1, 1, rows, C), accumulate=acc)
        dxb, dxv = off8(prior)
        _, dgb, dbb = fn.bn_backward(xv, scale, shift, dyv, mean, rstd, gd, relu=True, dx=dxv, accumulate=acc)
        assert torch.equal(dxv, dxa) and torch.equal(dgb, dga) and torch.equal(dbb, dba), f"accumulate={acc}"
        assert untouched(dxb)
    assert untouched(xb) and untouched(dyb)
    assert torch.equal(xv, xa) and torch.equal(dyv, dya)


# ---------------------------------------------------------------------------------------------------------------------
# (mean, M2) tile tables, built by hand
TILE_ROWS = 8
GROUP = 32            # nn.hip kTileGroup
GROUP_MIN = 1024      # nn.hip tile_group_min()


def tile_table(x, tiles, tile_rows):
    """float64 x (rows, C) -> float32 table [tiles][2][C] of per-tile (mean, M2), per-tile row counts"""
    rows, C = x.shape
    tab = torch.zeros(tiles, 2, C, dtype=F64)
    cnt = torch.zeros(tiles, dtype=F64)
    full = (rows // tile_rows) * tile_rows
    if full:
        xt = x[:full].view(-1, tile_rows, C)
        m = xt.mean(1)
        tab[:full // tile_rows, 0], tab[:full // tile_rows, 1] = m, ((xt - m[:, None]) ** 2).sum(1)
        cnt[:full // tile_rows] = tile_rows
    if full < rows:
        m = x[full:].mean(0)
        tab[-1, 0], tab[-1, 1], cnt[-1] = m, ((x[full:] - m) ** 2).sum(0), rows - full
    return tab.float(), cnt


def merge(cnt, m_t, q_t):
    """Chan's merge of (count, mean, M2) entries in float64 -> (mean, M2)"""
    n = cnt.sum()
    m = (cnt[:, None] * m_t).sum(0) / n
    return m, (q_t + cnt[:, None] * (m_t - m) ** 2).sum(0)


def rounding_bars(cnt, m_t, q_t, m):
    """what one float rounding of every entry's mean and M2 does to the merged (mean, var), first order (module docstring)"""
    w = cnt[:, None] / cnt.sum()
    return U * (w * m_t.abs()).sum(0), (w * 2 * U * m_t.abs() * (m_t - m).abs()).sum(0) + U * q_t.sum(0) / cnt.sum()


def rstd_bar(var, v_bar, ulps):
    r = 1.0 / torch.sqrt(var + EPS32)
    return torch.maximum(1.0 / torch.sqrt((var - v_bar).clamp(min=0) + EPS32) - r, r - 1.0 / torch.sqrt(var + v_bar + EPS32)) + ulps * ulp32(r)


def tiles_input(rows, C, regime, g):
    if regime == "drift":         # tile means that drift strongly along the rows: m_g - m is several standard deviations
        x = torch.randn(rows, C, generator=g).double() + torch.linspace(-20, 20, rows).double()[:, None] * torch.linspace(0.2, 1, C).double()
    else:                         # the large common offset: |mean| = 30 .. 90 x std
        x = torch.randn(rows, C, generator=g).double() + torch.linspace(30, 90, C).double() * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    return x.float().double()


def run_tiles(tab, mm, tiles, rows, C, gamma, beta, relu, workspace_bytes=None):
    """dspn_bn_stats_from_tiles_f32 through fn, or directly with a workspace of the given size"""
    o = {k: nanvec(C) for k in ("mean", "rstd", "scale", "shift")}
    block, amin, cmm = None, None, None
    if mm is not None:
        block, amin = torch.zeros(fn.ABSMAX_SLOTS, device="cuda"), torch.full((1,), float("inf"), device="cuda")
        cmm = torch.full((2, C), float("nan"), device="cuda")
    if workspace_bytes is None:
        fn.bn_stats_from_tiles(tab, tiles, TILE_ROWS, rows, C, EPS, gamma, beta, o["mean"], o["rstd"], o["scale"], o["shift"],
                               tile_minmax=mm, relu=relu, out_absmax=block, out_absmin=amin, out_chan_minmax=cmm)
    else:
        ws = torch.zeros(max(workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        rc = fn.L().dspn_bn_stats_from_tiles_f32(fn.ptr(tab), tiles, TILE_ROWS, rows, C, EPS, fn.ptr(gamma), fn.ptr(beta), fn.ptr(o["mean"]),
                                                 fn.ptr(o["rstd"]), fn.ptr(o["scale"]), fn.ptr(o["shift"]), fn.ptr(mm), int(relu),
                                                 fn.ptr(block), fn.ptr(amin), fn.ptr(cmm), fn.ptr(ws), workspace_bytes, fn.stream())
        assert rc == 0, fn.L().dspn_last_error()
    return o, block, amin, cmm


def check_tiles(x, tiles, C, regime_name, g, workspace_bytes=None):
    rows = x.shape[0]
    tab, cnt = tile_table(x, tiles, TILE_ROWS)
    m_t, q_t = tab[:, 0].double(), tab[:, 1].double()
    m_ref, M2 = merge(cnt, m_t, q_t)                     # the float64 merge of the ROUNDED table
    var_ref = M2 / rows
    grouped = tiles >= GROUP_MIN and workspace_bytes is None
    if grouped:                                           # the reference's own groups of 32 tiles
        gm, gq, gc = [], [], []
        for t0 in range(0, tiles, GROUP):
            a, b = merge(cnt[t0:t0 + GROUP], m_t[t0:t0 + GROUP], q_t[t0:t0 + GROUP])
            gm.append(a); gq.append(b); gc.append(cnt[t0:t0 + GROUP].sum())
        mb, vb = rounding_bars(torch.stack(gc), torch.stack(gm), torch.stack(gq), m_ref)
        m_bar, r_bar = mb + ulp32(m_ref), rstd_bar(var_ref, vb, 2)
    else:
        m_bar, r_bar = ulp32(m_ref), rstd_bar(var_ref, torch.zeros_like(var_ref), 2)
    gamma, beta = gamma_beta(C, g)                        # (gamma_beta: channels 1, 6, ... have a negative scale)
    beta[0] = -1000.0                                     # a channel whose value is 0 everywhere after ReLU
    lo_t = torch.stack([x[t * TILE_ROWS:(t + 1) * TILE_ROWS].min(0).values for t in range(tiles)])
    hi_t = torch.stack([x[t * TILE_ROWS:(t + 1) * TILE_ROWS].max(0).values for t in range(tiles)])
    mm = torch.stack([lo_t, hi_t], 1).float().cuda()
    tabd, gd, bd = tab.cuda(), dev(gamma), dev(beta)
    what = f"{regime_name} rows={rows}" + (" grouped" if grouped else "")
    first = None
    for relu in (False, True):
        o, block, amin, cmm = run_tiles(tabd, mm, tiles, rows, C, gd, bd, relu, workspace_bytes)
        mk, rk, sk, hk = (h64(o[k]) for k in ("mean", "rstd", "scale", "shift"))
        if first is None:
            within(mk, m_ref, m_bar, f"mean [{what}]")
            within(rk, 1.0 / torch.sqrt(var_ref + EPS32), r_bar, f"rstd [{what}]")
            # ... and the statistics of x itself, up to the table's own rounding
            xm = x.mean(0)
            xv = ((x - xm) ** 2).mean(0)
            tb_m, tb_v = rounding_bars(cnt, m_t, q_t, xm)
            within(mk, xm, m_bar + tb_m, f"mean vs x [{what}]")
            within(rk, 1.0 / torch.sqrt(xv + EPS32), rstd_bar(xv, tb_v, 0) + r_bar, f"rstd vs x [{what}]")
            assert torch.equal(o["scale"].cpu(), gamma.float() * o["rstd"].cpu())
            within(hk, beta - mk * sk, ulp32(beta.abs() + (mk * sk).abs()), f"shift [{what}]")
            none = run_tiles(tabd, None, tiles, rows, C, gd, bd, relu, workspace_bytes)[0]       # without the extremes: same bits
            assert all(torch.equal(none[k], o[k]) for k in o)
            first = o
        else:
            assert all(torch.equal(first[k], o[k]) for k in o)
        lo, hi = x.min(0).values, x.max(0).values
        assert torch.equal(h64(cmm[0]), lo) and torch.equal(h64(cmm[1]), hi), "per-channel extremes"
        a, b = (lo * sk + hk).float(), (hi * sk + hk).float()
        if relu:
            a, b = a.clamp(min=0), b.clamp(min=0)
        v = torch.maximum(a.abs(), b.abs())
        assert block_max(block) == float(v.max()), "out_absmax"
        assert float(amin) == float(v[v > 0].min()), "out_absmin"
        if relu:
            assert float(v[0]) == 0.0 and float(v.min()) == 0.0          # the all-zero channel is not the smallest NON-ZERO one
    return first


TABLE_TILES = [1, 2, 63, 64, 65,             # around the finalize's 64 tile lanes
               1023, 1024, 1025,             # around tile_group_min(): ungrouped, 32 whole groups, a last group of one tile
               1055]                         # a last group of 31 tiles


@pytest.mark.parametrize("C", [4, 20, 260])
@pytest.mark.parametrize("tiles", TABLE_TILES)
def test_statistics_from_mean_m2_tables(gpu_device, tiles, C):
    g = torch.Generator().manual_seed(10 * tiles + C)
    for rows in (tiles * TILE_ROWS - 7, tiles * TILE_ROWS):      # a last tile of one row; a whole last tile
        for regime in ("drift", "offset"):
            check_tiles(tiles_input(rows, C, regime, g), tiles, C, regime, g)


@pytest.mark.parametrize("C", [4, 260])
def test_table_stays_ungrouped_in_a_small_workspace(gpu_device, C):
    """1025 tiles and a workspace one byte short of dspn_bn_tiles_workspace_bytes: the one-sweep merge, held to the UNGROUPED
    bars (1 ulp / 2 ulp of the float64 merge -- tighter than any grouped result is promised to be)"""
    tiles = 1025
    need = fn.L().dspn_bn_tiles_workspace_bytes(tiles, C)
    assert need == 4 * 4 * ((tiles + GROUP - 1) // GROUP) * C
    g = torch.Generator().manual_seed(C)
    for rows in (tiles * TILE_ROWS - 7, tiles * TILE_ROWS):
        for regime in ("drift", "offset"):
            x = tiles_input(rows, C, regime, g)
            for nbytes in (need - 1, 0):
                check_tiles(x, tiles, C, regime, g, workspace_bytes=nbytes)


# ---------------------------------------------------------------------------------------------------------------------
# plain-sum tables
def _decode_planes(planes, shape, block):
    """fp16 piece planes [rows][C / 32][2][32] in a float32 buffer of `shape` -> float64 (h0 + h1) / s, and the block scale
    2^15 / s, s the power of two csrc/dspn_pieces.h operand_scale derives from the magnitude block"""
    C = shape[-1]
    h = planes.view(torch.float16).view(-1, C // 32, 2, 32).double()
    m = float(block[torch.isfinite(block)].max())
    e = max(-100, min(100, 15 - (int(np.floor(np.log2(m))) + 1)))
    return ((h[:, :, 0] + h[:, :, 1]) / 2.0 ** e).reshape(shape).cpu(), 2.0 ** 15 / 2.0 ** e


def split_sums(S, SS, tiles, g):
    """a float32 table [tiles][2][C] whose columns add up to (S, SS), split unevenly: integer parts for the integer S"""
    C = S.numel()
    tab = torch.zeros(tiles, 2, C, dtype=F64)
    if tiles > 1:
        tab[:-1, 0] = torch.randint(-50, 51, (tiles - 1, C), generator=g).double() * (torch.rand(tiles - 1, 1, generator=g) < 0.7)
        w = torch.randn(tiles - 1, C, generator=g).double() * torch.rand(tiles - 1, 1, generator=g).double() ** 4
        tab[:-1, 1] = (w / tiles * SS.abs()).float().double()     # (a channel the ReLU masks entirely: sums 0, a column of zeros)
    tab[-1, 0] = S - tab[:-1, 0].sum(0)
    tab[-1, 1] = SS - tab[:-1, 1].sum(0)
    return tab.float()


@pytest.mark.parametrize("C", [4, 20, 64, 260])
@pytest.mark.parametrize("tiles", [1, 15, 16, 17,            # around the finalize's 16 table lanes
                                   1023, 1024, 1025, 1055])  # around the grouping threshold; last groups of 1 and 31 rows
def test_backward_from_sum_tables(gpu_device, tiles, C):
    rows = 4 * tiles + 3
    x, dy, prior, gamma, beta = _small_case(C, 7 * tiles + C, rows)
    g = torch.Generator().manual_seed(tiles + C)
    x64, dy64 = x.double(), dy.double()
    mean = x64.mean(0).float().double()
    rstd = (1.0 / torch.sqrt(x64.var(0, unbiased=False) + EPS32)).float().double()
    scale = (gamma.float() * rstd.float()).double()
    shift = (beta - mean * scale).float().double()
    grouped = tiles >= GROUP_MIN
    for relu in (False, True):
        ref = BwdRef(x64, dy64, mean, rstd, scale, shift, relu)
        tab = split_sums(ref.S, (ref.SS).float().double(), tiles, g)
        S, SS = tab[:, 0].double().sum(0), tab[:, 1].double().sum(0)      # what the table holds IS the pair of sums
        assert bool((tab[:, 0] == tab[:, 0].round()).all()) and float(tab[:, 0].abs().sum(0).max()) < 2 ** 24
        assert torch.equal(S, ref.S)
        dSS = (U if grouped else 2.0 ** -50) * tab[:, 1].double().abs().sum(0)
        dx_ref, dx_bar, emul = ref.dx(gamma, S=S, SS=SS, dSS=dSS)
        for dt in (torch.float32, BF):
            xd, dyd = dev(x, dt).view(1, 1, rows, C), dev(dy, dt).view(1, 1, rows, C)
            md, rd, sd, hd, gd, td = dev(mean), dev(rstd), dev(scale), dev(shift), dev(gamma), tab.cuda()
            name = f"relu={relu} {'bf16' if dt == BF else 'float'}"

            def call(**kw):
                return fn.bn_backward_from_sums(xd, sd, hd, dyd, md, rd, gd, td, tiles, relu=relu, **kw)
            dx, dgam, dbet = call(dx=torch.full_like(xd, SENTINEL), dgamma=nanvec(C), dbeta=nanvec(C))
            within(h64(dbet), S, ulp32(S), f"dbeta {name}")
            within(h64(dgam), SS, dSS + ulp32(SS), f"dgamma {name}")
            if dt == BF:
                bf16_within(dx.view(rows, C), dx_ref, dx_bar, emul, f"dx {name}")
            else:
                within(h64(dx).view(rows, C), dx_ref, dx_bar, f"dx {name}")
            # the same bits from the two halves and from the parameters-only form
            ws = fn.bn_from_sums_workspace(tiles, C, xd.device)
            dx2 = torch.full_like(xd, SENTINEL)
            _, dg2, db2 = call(dx=dx2, dgamma=nanvec(C), dbeta=nanvec(C), phase=1, workspace=ws)
            assert bool((dx2 == SENTINEL).all()), "the finalize half wrote dx"
            call(dx=dx2, phase=2, workspace=ws)
            assert torch.equal(dx2, dx) and torch.equal(dg2, dgam) and torch.equal(db2, dbet), f"phase 1 + 2 {name}"
            none, dg3, db3 = call(dx=fn.NO_OUTPUT)
            assert none is None and torch.equal(dg3, dgam) and torch.equal(db3, dbet), f"dx = NO_OUTPUT {name}"
            exp = dx_ref + prior.double()
            acc, _, _ = call(dx=dev(prior, dt).view(1, 1, rows, C), accumulate=True)
            if dt == BF:
                bf16_within(acc.view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), emul + prior, f"dx accumulate {name}")
            else:
                within(h64(acc).view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), f"dx accumulate {name}")
            if dt == torch.float32 and C % 32 == 0 and fn.get_conv_math() == "f16x2":
                dy_am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda"); dy_am[3] = float(dy.abs().max())
                x_mm = torch.stack([x.min(0).values, x.max(0).values]).cuda()
                bound, bmin = torch.zeros(fn.ABSMAX_SLOTS, device="cuda"), torch.full((1,), float("inf"), device="cuda")
                pl, dg4, db4 = call(dx=torch.full_like(xd, SENTINEL), dx_absmax=bound, dy_absmax=dy_am, x_chan_minmax=x_mm,
                                    dx_planes=True, dx_absmin=bmin)
                assert torch.equal(dg4, dgam) and torch.equal(db4, dbet)
                dec, block_scale = _decode_planes(pl, (rows, C), bound)
                within(dec, dx_ref, dx_bar + 2.0 ** -21 * block_scale, f"dx planes {name}")
                assert block_max(bound) >= float(dx_ref.abs().max()), "the block does not bound dx"
                assert 0.0 < float(bmin) <= block_max(bound)


# ---------------------------------------------------------------------------------------------------------------------
# the pooled-gradient form
def test_backward_with_the_pooled_gradient(gpu_device):
    """bn_backward_maxpool: dy is the max-pooling gradient of dy_pool routed through the argmax record on the fly; the record
    is written by hand, 255 (no maximum: no gradient) among its entries"""
    N, H, W, C, k, s, p = 2, 9, 11, 20, 3, 2, 1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(91)
    rows = N * H * W
    x = general_input(rows, C, g)
    gamma, beta = gamma_beta(C, g)
    rec = torch.randint(0, k * k, (N, Ho, Wo, C), generator=g).to(torch.uint8)
    rec[torch.rand(N, Ho, Wo, C, generator=g) < 0.15] = 255
    dyp = int_dy((N, Ho, Wo, C), g)
    # float64 routing: dx[pixel] = sum of dy_pool over the windows whose record names the pixel; padding takes nothing
    Hp, Wp = H + 2 * p + k, W + 2 * p + k
    routed = torch.zeros(N, Hp, Wp, C, dtype=F64)
    for r in range(k):
        for q in range(k):
            routed[:, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s] += torch.where(rec == r * k + q, dyp, torch.zeros_like(dyp))
    dy = routed[:, p:p + H, p:p + W].reshape(rows, C)
    assert int((rec == 255).sum()) > 50 and float(dy.abs().max()) > 8
    xd, gd, bd = dev(x).view(N, H, W, C), dev(gamma), dev(beta)
    mean, rstd, scale, shift = fn.bn_stats(xd, EPS, gd, bd)
    mk, rk, sk, hk = h64(mean), h64(rstd), h64(scale), h64(shift)
    ref = BwdRef(x, dy, mk, rk, sk, hk, True)
    dSS = (slab_rows_for(rows) + 3) * U * ref.absT
    am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    dx, dgam, dbet = fn.bn_backward_maxpool(xd, scale, shift, dev(dyp), rec.cuda(), k, s, p, mean, rstd, gd, relu=True,
                                            dx=torch.full_like(xd, SENTINEL), dgamma=nanvec(C), dbeta=nanvec(C), dx_absmax=am)
    within(h64(dbet), ref.S, ulp32(ref.S), "dbeta")
    within(h64(dgam), ref.SS, dSS, "dgamma")
    dx_ref, dx_bar, _ = ref.dx(gamma, dSS=dSS)
    within(h64(dx).view(rows, C), dx_ref, dx_bar, "dx")
    assert block_max(am) == float(dx.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# what the C ABI refuses
def test_c_abi_refusals(gpu_device):
    L = fn.L()
    C, rows = 64, 8
    f = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    x, dy, dx, y = f(rows, C), f(rows, C), f(rows, C), f(rows, C)
    v = [f(C) for _ in range(8)]
    mean, rstd, scale, shift, gamma, beta, dgam, dbet = v
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    P, st = fn.ptr, fn.stream()

    def refused(rc, text):
        assert rc != 0 and text in L.dspn_last_error(), (rc, L.dspn_last_error())

    for r, c in ((rows, 6), (rows, 0), (0, C)):
        refused(L.dspn_bn_stats_f32(P(x), r, c, EPS, P(gamma), P(beta), P(mean), P(rstd), P(scale), P(shift), P(ws), ws.numel(), st),
                b"positive multiple of 4")
        refused(L.dspn_bn_apply_f32(P(x), P(scale), P(shift), P(y), r, c, 1, 0, st), b"positive multiple of 4")
        refused(L.dspn_bn_backward_f32(P(x), P(scale), P(shift), P(dy), P(mean), P(rstd), P(gamma), P(dx), P(dgam), P(dbet), r, c, 1, 0,
                                       0, P(ws), ws.numel(), st), b"positive multiple of 4")
    tiles, tr = 4, 8
    tab, mm, block = f(tiles, 2, C), f(tiles, 2, C), f(fn.ABSMAX_SLOTS)

    def from_tiles(r, mm_, block_):
        return L.dspn_bn_stats_from_tiles_f32(P(tab), tiles, tr, r, C, EPS, P(gamma), P(beta), P(mean), P(rstd), P(scale), P(shift),
                                              P(mm_), 0, P(block_), 0, 0, P(ws), ws.numel(), st)
    for r in ((tiles - 1) * tr, tiles * tr + 1, 0):      # rows outside ((tiles - 1) * tile_rows, tiles * tile_rows]
        refused(from_tiles(r, None, None), b"bad argument")
    assert from_tiles((tiles - 1) * tr + 1, None, None) == 0 and from_tiles(tiles * tr, None, None) == 0
    refused(from_tiles(tiles * tr, mm, None), b"go together")
    refused(from_tiles(tiles * tr, None, block), b"go together")

    def from_sums(flags=0, accumulate=0, dx_=dx, c=C, r=rows, nbytes=ws.numel(), planes_ops=True):
        o = (P(block), 0, P(block), P(mm)) if planes_ops else (0, 0, 0, 0)
        return L.dspn_bn_backward_from_sums_f32(P(x), P(scale), P(shift), P(dy), P(mean), P(rstd), P(gamma), P(tab), tiles, P(dx_),
                                                P(dgam), P(dbet), r, c, 1, accumulate, *o, flags, P(ws), nbytes, st)
    assert from_sums() == 0
    refused(from_sums(flags=2 | 4), b"flag word")
    refused(from_sums(flags=8), b"flag word")                       # parked without finalize-only
    refused(from_sums(flags=8 | 4), b"flag word")
    refused(from_sums(flags=1, accumulate=1), b"piece planes")
    refused(from_sums(flags=1, dx_=x), b"piece planes")              # dx aliasing x
    refused(from_sums(flags=1, dx_=dy), b"piece planes")
    refused(from_sums(flags=1, planes_ops=False), b"piece planes")
    refused(from_sums(nbytes=3 * C * 4 - 1), b"workspace too small")
    assert from_sums(nbytes=3 * C * 4) == 0
    refused(from_sums(c=6), b"positive multiple of 4")
    refused(from_sums(r=0), b"positive multiple of 4")
    assert fn.bn_discard_parked(ctypes.c_void_p(st)) == 0            # nothing was parked by a refused call
    torch.cuda.synchronize()
