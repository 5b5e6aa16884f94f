"""The fixed-statistics mode of the BatchNorm backward (include/dspn_nn.h DSPN_BN_SUMS_FIXED_STATS, the `_ex` entry points) on
every route that ends in the finalize arithmetic of csrc/bn_final_job.h: the plain call, the call from sum tables (whole, in
two phases, parameters only, accumulating, as piece planes), the parked finalize (taken by a weight gradient / run by the apply
half), the pooled-gradient form and the recomputed data gradient.

mean / rstd / scale / shift are NOT the batch's: per channel, moving_mean = batch mean + 0.5 z std (z ~ N(0, 1)) and
moving_var = f var (f uniform in [0.5, 2]), z and f drawn independently of x, and the four vectors come out of the library's
own DSPN_BN_GLOBAL finalize (fn.bn_stats(moving=BN_GLOBAL)) from those arrays.  (Centred on the batch so that the ReLU mask is
mixed in every channel and xhat is O(1); the offsets are O(1) standard deviations, so a batch-mode dx is far outside every bar
here -- asserted in the plain route.)

The float64 machinery and every bar are those of tests/test_bn_edges_gpu.py (imported): with fixed statistics the closed form
dx = a dy' + c1 x + c0 has c1 = c0 = 0, which is BwdRef.dx evaluated with S = SS = 0 -- its bar collapses to 4 U |a dy'|.
Conditions (none measured):
 1. dgamma / dbeta are the bits of the batch-mode call of the same entry point on the same arguments.
 2. ... and within that file's bars 6 of the float64 sums.
 3. float tensors, no planes, no accumulation: dx == fl32(a) dy' exactly, a = fl32(fl64(gamma) fl64(rstd)) (1 rstd for
    fix_gamma): bn_apply_element with c1 = c0 = +-0 is one rounded product.
 4. after a finalize-only call the coefficient block is (fl32(a), 0, 0).
 5. bf16 tensors and accumulation: that file's bars 7 / 4 around float64 a dy' (+ prior).
 6. piece planes: its planes bar; the block bounds max|dx|, is at most (1 + 2e-6) max_c |a_c| D, and 0 < bmin <= block.
 7. an independent reading: torch.autograd of relu(F.batch_norm(..., training=False)) in float64 on the CPU, same bars."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from test_bn_edges_gpu import (BF, EPS, F64, GROUP_MIN, SENTINEL, U, BwdRef, _decode_planes, _small_case, bf16_within,
                               block_max, dev, gamma_beta, general_input, h64, int_dy, nanvec, slab_rows_for, split_sums, ulp32,
                               within)
from test_bn1_recompute_gpu import CASES, Unit, check_route
from test_strided_addend_gpu import same_bits, tiles  # noqa: F401  (tiles: fixture)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def draw_moving(x, g):
    """(moving_mean, moving_var), float64 copies of floats: not the batch's (module docstring)"""
    C = x.shape[1]
    bm, bs = x.mean(0), x.std(0, unbiased=False)
    mm = bm + 0.5 * torch.randn(C, generator=g).double() * bs
    mv = bs * bs * (0.5 + 1.5 * torch.rand(C, generator=g).double())
    return mm.float().double(), mv.float().double()


def global_stats(xd, gd, bd, mm, mv):
    """-> device (mean, rstd, scale, shift) of the DSPN_BN_GLOBAL finalize over the given moving arrays"""
    C = mm.numel()
    mmd, mvd = dev(mm), dev(mv)
    out = fn.bn_stats(xd, EPS, gd, bd, mean=nanvec(C), rstd=nanvec(C), scale=nanvec(C), shift=nanvec(C),
                      moving=fn.bn_moving(mmd, mvd, 0.9, fn.BN_GLOBAL))
    assert torch.equal(out[0], mmd) and torch.equal(mmd.cpu().double(), mm) and torch.equal(mvd.cpu().double(), mv)
    return out


def a32_of(gamma, rk):
    """fl32(fl64(gamma) fl64(rstd)), 1 for fix_gamma: the coefficient the finalize stores"""
    return (rk if gamma is None else gamma * rk).float()


def fixed_dx(ref, gamma):
    """BwdRef's closed form with S = SS = 0: (float64 a dy', its bar 4 U |a dy'|, float32 evaluation)"""
    zero = torch.zeros_like(ref.S)
    return ref.dx(gamma, S=zero, SS=zero)


def exact_dx(ref, gamma):
    """condition 3: the float32 product fl32(a) dy', one rounding (float32 tensor)"""
    return a32_of(gamma, ref.rstd) * ref.dyp.float()


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a, b)


def autograd_reading(x, dy, mm, mv, gamma, beta, relu):
    """condition 7: float64 autograd of (relu)(batch_norm(training=False)) -> (dx, dgamma, dbeta)"""
    xa = x.clone().requires_grad_(True)
    ga = (torch.ones_like(mm) if gamma is None else gamma.clone()).requires_grad_(True)
    ba = beta.clone().requires_grad_(True)
    y = F.batch_norm(xa, mm, mv, ga, ba, training=False, eps=2e-5)
    (F.relu(y) if relu else y).backward(dy)
    return xa.grad, ga.grad, ba.grad


def clear_of_zero(x, mm, mv, gamma, beta):
    """move the elements of x whose output lies within 64 U (|x s| + |h|) of zero one moving standard deviation away (the
    output moves by gamma, at least 0.5): the float scale / shift of the library and the float64 affine of the autograd
    reading then agree on every ReLU decision"""
    rs = 1.0 / torch.sqrt(mv + 2e-5)
    s, h = gamma * rs, beta - mm * gamma * rs

    def near(v):
        return (v * s + h).abs() <= 64 * U * ((v * s).abs() + h.abs())
    x = torch.where(near(x), x + torch.sqrt(mv + 2e-5), x).float().double()
    assert not bool(near(x).any())
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the plain route
B32 = 32 * 1024            # slab_rows_for: 32-row slabs up to here, 40-row slabs from B32 + 1 on
PLAIN_SHAPES = [(33, 20), (1025, 4), (300, 64), (B32 - 1, 260), (B32 + 1, 260)]


def test_slab_boundary_is_where_the_shapes_assume():
    assert slab_rows_for(B32 - 1) == slab_rows_for(B32) == 32 and slab_rows_for(B32 + 1) == 40


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("rows,C", PLAIN_SHAPES)
def test_plain_route(gpu_device, rows, C, relu):
    g = torch.Generator().manual_seed(77 * C + rows + int(relu))
    sr = slab_rows_for(rows)
    gamma, beta = gamma_beta(C, g)
    dy = int_dy((rows, C), g)
    x = general_input(rows, C, g)
    mm, mv = draw_moving(x, g)
    shape = (1, 1, rows, C)
    xd, dyd, gd, bd = dev(x).view(shape), dev(dy).view(shape), dev(gamma), dev(beta)
    mean, rstd, scale, shift = global_stats(xd, gd, bd, mm, mv)
    mk, rk, sk, hk = h64(mean), h64(rstd), h64(scale), h64(shift)
    ref = BwdRef(x, dy, mk, rk, sk, hk, relu)
    dSS = (sr + 3) * U * ref.absT
    for gm, gmd, name in ((None, None, "fix_gamma"), (gamma, gd, "gamma")):
        if gm is None:      # (the mask of a fix_gamma node comes from ITS scale / shift)
            m1, r1, s1, h1 = global_stats(xd, None, bd, mm, mv)
            assert torch.equal(m1, mean) and torch.equal(r1, rstd) and torch.equal(s1, rstd)
            rf, sc, sh = BwdRef(x, dy, mk, rk, rk, h64(h1), relu), s1, h1
            dS = (sr + 3) * U * rf.absT
        else:
            rf, sc, sh, dS = ref, scale, shift, dSS
        bdx, bdg, bdb = fn.bn_backward(xd, sc, sh, dyd, mean, rstd, gmd, relu=relu, dgamma=nanvec(C), dbeta=nanvec(C))
        am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
        dx, dgam, dbet = fn.bn_backward(xd, sc, sh, dyd, mean, rstd, gmd, relu=relu, dx=torch.full_like(xd, SENTINEL),
                                        dgamma=nanvec(C), dbeta=nanvec(C), dx_absmax=am, fixed_stats=True)
        assert same(dgam, bdg) and same(dbet, bdb), f"1: the sums know the mode ({name})"
        within(h64(dbet), rf.S, ulp32(rf.S), f"2: dbeta ({name})")
        within(h64(dgam), rf.SS, dS, f"2: dgamma ({name})")
        exp = exact_dx(rf, gm)
        got = dx.cpu().view(rows, C)
        assert bool(torch.isfinite(got).all()) and bool((got == exp).all()), \
            f"3: dx != fl32(a) dy' in {int((got != exp).sum())} elements ({name})"
        assert block_max(am) == float(dx.abs().max()), "dx_absmax"
        # (the test has power: the batch-mode dx of these arguments is far from it)
        dx_ref, dx_bar, _ = fixed_dx(rf, gm)
        assert float(((h64(bdx).view(rows, C) - dx_ref).abs() - 100 * dx_bar).max()) > 0
    # (gamma given from here on) accumulate, the outputs that may be left out
    prior = torch.randn(rows, C, generator=g).double()
    acc, _, _ = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, dx=dev(prior).view(shape), accumulate=True,
                               fixed_stats=True)
    exp = dx_ref + prior.float().double()
    within(h64(acc).view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), "5: dx accumulate")
    none, dg2, db2 = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, dx=fn.NO_OUTPUT, fixed_stats=True)
    assert none is None and same(dg2, dgam) and same(db2, dbet), "dx = NO_OUTPUT changed dgamma / dbeta"
    dx3, n1, n2 = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, dgamma=fn.NO_OUTPUT, dbeta=fn.NO_OUTPUT,
                                 fixed_stats=True)
    assert n1 is None and n2 is None and same(dx3, dx), "dgamma / dbeta = NO_OUTPUT changed dx"
    del bdx, dx, dx3, acc, got, exp
    # bf16 tensors hold bf16(x); dy is integer: the same values on both sides
    xb = x.to(BF).double()
    xh, dyh = dev(xb, BF).view(shape), dev(dy, BF).view(shape)
    mmb, mvb = draw_moving(xb, g)
    mean, rstd, scale, shift = global_stats(xh, gd, bd, mmb, mvb)
    refb = BwdRef(xb, dy, h64(mean), h64(rstd), h64(scale), h64(shift), relu)
    dSS = (sr + 3) * U * refb.absT
    dx_ref, dx_bar, emul = fixed_dx(refb, gamma)
    _, bdg, bdb = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=relu, dx=fn.NO_OUTPUT)
    dxh, dgh, dbh = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=relu, dx=torch.full_like(xh, SENTINEL),
                                   fixed_stats=True)
    assert same(dgh, bdg) and same(dbh, bdb), "1: the sums know the mode (bf16)"
    within(h64(dbh), refb.S, ulp32(refb.S), "2: dbeta (bf16)")
    within(h64(dgh), refb.SS, dSS, "2: dgamma (bf16)")
    bf16_within(dxh.view(rows, C), dx_ref, dx_bar, emul, "5: dx (bf16)")
    pb = prior.to(BF)
    acch, _, _ = fn.bn_backward(xh, scale, shift, dyh, mean, rstd, gd, relu=relu, dx=pb.view(shape).cuda(), accumulate=True,
                                fixed_stats=True)
    exp = dx_ref + pb.double()
    bf16_within(acch.view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), emul + pb.float(), "5: dx accumulate (bf16)")


# ---------------------------------------------------------------------------------------------------------------------
# the route from sum tables
@pytest.mark.parametrize("C", [4, 64, 260])
@pytest.mark.parametrize("tiles_n", [1, 16, 17,          # the finalize's 16 table lanes
                                     1024, 1025])        # the grouping threshold
def test_from_sums_route(gpu_device, tiles_n, C):
    rows = 4 * tiles_n + 3
    x, dy, prior, gamma, beta = _small_case(C, 11 * tiles_n + C, rows)
    g = torch.Generator().manual_seed(3 * tiles_n + C)
    x64, dy64 = x.double(), dy.double()
    mm, mv = draw_moving(x64, g)
    shape = (1, 1, rows, C)
    gd, bd = dev(gamma), dev(beta)
    md, rd, sd, hd = global_stats(dev(x).view(shape), gd, bd, mm, mv)
    mk, rk, sk, hk = h64(md), h64(rd), h64(sd), h64(hd)
    grouped = tiles_n >= GROUP_MIN
    a32 = a32_of(gamma, rk)
    for relu in (False, True):
        ref = BwdRef(x64, dy64, mk, rk, sk, hk, relu)
        tab = split_sums(ref.S, ref.SS.float().double(), tiles_n, g)
        S, SS = tab[:, 0].double().sum(0), tab[:, 1].double().sum(0)
        assert torch.equal(S, ref.S)
        dSS = (U if grouped else 2.0 ** -50) * tab[:, 1].double().abs().sum(0)
        dx_ref, dx_bar, emul = fixed_dx(ref, gamma)
        td = tab.cuda()
        for dt in (torch.float32, BF):
            xd, dyd = dev(x, dt).view(shape), dev(dy, dt).view(shape)
            name = f"relu={relu} {'bf16' if dt == BF else 'float'}"

            def call(fixed_stats=True, **kw):
                return fn.bn_backward_from_sums(xd, sd, hd, dyd, md, rd, gd, td, tiles_n, relu=relu, fixed_stats=fixed_stats, **kw)
            _, bdg, bdb = call(fixed_stats=False, dgamma=nanvec(C), dbeta=nanvec(C))
            dx, dgam, dbet = call(dx=torch.full_like(xd, SENTINEL), dgamma=nanvec(C), dbeta=nanvec(C))
            assert same(dgam, bdg) and same(dbet, bdb), f"1: the sums know the mode {name}"
            within(h64(dbet), S, ulp32(S), f"2: dbeta {name}")
            within(h64(dgam), SS, dSS + ulp32(SS), f"2: dgamma {name}")
            if dt == BF:
                bf16_within(dx.view(rows, C), dx_ref, dx_bar, emul, f"5: dx {name}")
            else:
                got, exp = dx.cpu().view(rows, C), exact_dx(ref, gamma)
                assert bool(torch.isfinite(got).all()) and bool((got == exp).all()), f"3: dx != fl32(a) dy' {name}"
            # the two halves with a workspace of their own: the coefficient block in between, then the whole call's bits
            ws = fn.bn_from_sums_workspace(tiles_n, C, xd.device)
            ws.fill_(0xFF)
            dx2 = torch.full_like(xd, SENTINEL)
            _, dg2, db2 = call(dx=dx2, dgamma=nanvec(C), dbeta=nanvec(C), phase=1, workspace=ws)
            assert bool((dx2 == SENTINEL).all()), "the finalize half wrote dx"
            coef = ws[:12 * C].view(torch.float32).cpu()
            assert bool((coef[:C] == a32).all()) and bool((coef[C:] == 0).all()), f"4: the coefficient block {name}"
            call(dx=dx2, phase=2, workspace=ws)
            assert same(dx2, dx) and same(dg2, dgam) and same(db2, dbet), f"phase 1 + 2 {name}"
            none, dg3, db3 = call(dx=fn.NO_OUTPUT)
            assert none is None and same(dg3, dgam) and same(db3, dbet), f"dx = NO_OUTPUT {name}"
            exp = dx_ref + prior.double()
            acc, _, _ = call(dx=dev(prior, dt).view(shape), accumulate=True)
            if dt == BF:
                bf16_within(acc.view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), emul + prior, f"5: dx accumulate {name}")
            else:
                within(h64(acc).view(rows, C), exp, dx_bar + U * (exp.abs() + dx_bar), f"5: dx accumulate {name}")
            if dt == torch.float32 and C % 32 == 0 and fn.get_conv_math() == "f16x2":
                D = float(dy.abs().max())
                dy_am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda"); dy_am[3] = D
                x_mm = torch.stack([x.min(0).values, x.max(0).values]).cuda()
                bound, bmin = torch.zeros(fn.ABSMAX_SLOTS, device="cuda"), torch.full((1,), float("inf"), device="cuda")
                pl, dg4, db4 = call(dx=torch.full_like(xd, SENTINEL), dx_absmax=bound, dy_absmax=dy_am, x_chan_minmax=x_mm,
                                    dx_planes=True, dx_absmin=bmin)
                assert same(dg4, dgam) and same(db4, dbet)
                dec, block_scale = _decode_planes(pl, (rows, C), bound)
                within(dec, dx_ref, dx_bar + 2.0 ** -21 * block_scale, f"6: dx planes {name}")
                assert block_max(bound) >= float(dx_ref.abs().max()), "6: the block does not bound dx"
                assert block_max(bound) <= (1 + 2e-6) * float((gamma * rk).abs().max()) * D, "6: the bound is not |a| D"
                assert 0.0 < float(bmin) <= block_max(bound)


# ---------------------------------------------------------------------------------------------------------------------
# the parked finalize and the recomputed data gradient, on the operands of tests/test_bn1_recompute_gpu.py
class FixedUnit(Unit):
    """a dim-match unit's bn1 backward (Unit) whose bn1 normalises with moving statistics that are not the batch's"""

    def __init__(self, N, H, W, K, C, seed):
        super().__init__(N, H, W, K, C, seed)
        g = torch.Generator().manual_seed(seed + 1000)
        mm, mv = draw_moving(self.x.cpu().double().view(-1, C), g)
        self.beta = torch.randn(C, generator=g).cuda()
        self.mean, self.rstd, self.scale, self.shift = global_stats(self.x, self.gamma, self.beta, mm, mv)

    def gradient(self, relu):
        """conv1's data gradient, stored, with bn1's backward sums: (g, tab)"""
        tab = torch.zeros(self.tiles, 2, self.C, device="cuda")
        g = fn.conv2d_dgrad(self.dyp, None, self.shape, out=torch.full(self.shape, float("nan"), device="cuda"),
                            bn_bwd=self.bn(relu, tab), **self.kw)
        return g, tab

    def from_sums(self, g, tab, relu, accumulate, dx, dgam, dbet, am, **kw):
        return fn.bn_backward_from_sums(self.x, self.scale, self.shift, g, self.mean, self.rstd, self.gamma, tab, self.tiles,
                                        relu=relu, dx=dx, dgamma=dgam, dbeta=dbet, accumulate=accumulate, dx_absmax=am,
                                        fixed_stats=True, **kw)


@pytest.mark.parametrize("accumulate", [False, True], ids=["first writer", "accumulate"])
def test_parked_finalize_and_recomputed_data_gradient(tiles, accumulate):
    name = "four waves, two k-steps, one tile per workgroup"
    N, H, W, K, C, mode = CASES[name]
    check_route(tiles, N, H, W, K, C, mode)
    relu = True
    u = FixedUnit(N, H, W, K, C, seed=21)
    g, tab = u.gradient(relu)
    st = fn.stream()
    # the unparked whole call: the yardstick of the three sequences below
    dx, _, dgam, dbet, am = u.outputs(accumulate)
    u.from_sums(g, tab, relu, accumulate, dx, dgam, dbet, am)
    if not accumulate:      # condition 3 on a gradient that is no integer: one rounded product per element
        a32 = a32_of(u.gamma.cpu().double(), u.rstd.cpu().double())
        mask = (u.x.cpu().double() * u.scale.cpu().double() + u.shift.cpu().double()) > 0
        exp = a32 * torch.where(mask, g.cpu(), torch.zeros(()))
        assert bool((dx.cpu() == exp).all()), "3: dx != fl32(a) g'"
    assert bool(torch.isfinite(dx).all()) and float(am.max()) == float(dx.abs().max()) > 0
    dw_alone = fn.conv2d_wgrad(u.x, u.dy, (K, 1, 1, C))
    # parked, a weight gradient on the stream takes it, the apply half follows
    dx1, _, dg1, db1, am1 = u.outputs(accumulate)
    ws = fn.bn_from_sums_workspace(u.tiles, C, "cuda")
    u.from_sums(g, tab, relu, accumulate, dx1, dg1, db1, am1, phase=1, park=True, workspace=ws)
    dw = fn.conv2d_wgrad(u.x, u.dy, (K, 1, 1, C))
    assert _lib.lib().dspn_bn_discard_parked(st) == 0, "the weight gradient did not take the parked job"
    u.from_sums(g, tab, relu, accumulate, dx1, dg1, db1, am1, phase=2, workspace=ws)
    for a, b, what in ((dx, dx1, "dx"), (dgam, dg1, "dgamma"), (dbet, db1, "dbeta"), (am, am1, "dx_absmax"), (dw_alone, dw, "dw")):
        same_bits(a, b, f"parked, taken by a weight gradient: {what}")
    coef = ws[:12 * C].view(torch.float32).cpu()
    assert bool((coef[:C] == a32_of(u.gamma.cpu().double(), u.rstd.cpu().double())).all()) and bool((coef[C:] == 0).all()), "4"
    # parked, no weight gradient comes by: the apply half runs the job itself
    dx2, _, dg2, db2, am2 = u.outputs(accumulate)
    ws2 = fn.bn_from_sums_workspace(u.tiles, C, "cuda")
    u.from_sums(g, tab, relu, accumulate, dx2, dg2, db2, am2, phase=1, park=True, workspace=ws2)
    u.from_sums(g, tab, relu, accumulate, dx2, dg2, db2, am2, phase=2, workspace=ws2)
    assert _lib.lib().dspn_bn_discard_parked(st) == 0, "the job was left parked"
    for a, b, what in ((dx, dx2, "dx"), (dgam, dg2, "dgamma"), (dbet, db2, "dbeta"), (am, am2, "dx_absmax")):
        same_bits(a, b, f"parked, run by the apply half: {what}")
    # the gradient never stored: sums-only data gradient, the finalize (parked: the apply entry runs it), the data gradient again
    for park in (False, True):
        dx3, tab3, dg3, db3, am3 = u.outputs(accumulate)
        assert fn.conv2d_dgrad(u.dyp, None, u.shape, bn_bwd=u.bn(relu, tab3), sums_only=True, **u.kw) is None
        ws3 = fn.bn_from_sums_workspace(u.tiles, C, "cuda")
        u.from_sums(None, tab3, relu, accumulate, dx3, dg3, db3, am3, phase=1, park=park, workspace=ws3)
        fn.conv2d_dgrad_bn_apply(u.dyp, None, u.x, u.scale, u.shift, relu, ws3, dx3, accumulate=accumulate, dx_absmax=am3, **u.kw)
        assert _lib.lib().dspn_bn_discard_parked(st) == 0
        for a, b, what in ((dx, dx3, "dx"), (tab, tab3, "sum tables"), (dgam, dg3, "dgamma"), (dbet, db3, "dbeta")):
            same_bits(a, b, f"recomputed data gradient (park={park}): {what}")
        same_bits(am.max(), am3.max(), "largest entry of the dx_absmax block")


# ---------------------------------------------------------------------------------------------------------------------
# the pooled-gradient form
def pooled_case(g):
    """the geometry of test_bn_edges_gpu.test_backward_with_the_pooled_gradient: x, the record, the pooled gradient and its
    float64 routing through the record"""
    N, H, W, C, k, s, p = 2, 9, 11, 20, 3, 2, 1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    rows = N * H * W
    x = general_input(rows, C, g)
    rec = torch.randint(0, k * k, (N, Ho, Wo, C), generator=g).to(torch.uint8)
    rec[torch.rand(N, Ho, Wo, C, generator=g) < 0.15] = 255
    dyp = int_dy((N, Ho, Wo, C), g)
    routed = torch.zeros(N, H + 2 * p + k, W + 2 * p + k, C, dtype=F64)
    for r in range(k):
        for q in range(k):
            routed[:, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s] += torch.where(rec == r * k + q, dyp, torch.zeros_like(dyp))
    dy = routed[:, p:p + H, p:p + W].reshape(rows, C)
    assert int((rec == 255).sum()) > 50 and float(dy.abs().max()) > 8
    return (N, H, W, C, k, s, p), x, rec, dyp, dy


def test_pooled_route(gpu_device):
    g = torch.Generator().manual_seed(191)
    (N, H, W, C, k, s, p), x, rec, dyp, dy = pooled_case(g)
    rows = N * H * W
    gamma, beta = gamma_beta(C, g)
    mm, mv = draw_moving(x, g)
    x = clear_of_zero(x, mm, mv, gamma, beta)
    xd, gd, bd = dev(x).view(N, H, W, C), dev(gamma), dev(beta)
    mean, rstd, scale, shift = global_stats(xd, gd, bd, mm, mv)
    ref = BwdRef(x, dy, h64(mean), h64(rstd), h64(scale), h64(shift), True)
    dSS = (slab_rows_for(rows) + 3) * U * ref.absT
    args = (xd, scale, shift, dev(dyp), rec.cuda(), k, s, p, mean, rstd, gd)
    _, bdg, bdb = fn.bn_backward_maxpool(*args, relu=True, dgamma=nanvec(C), dbeta=nanvec(C))
    am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    dx, dgam, dbet = fn.bn_backward_maxpool(*args, relu=True, dx=torch.full_like(xd, SENTINEL), dgamma=nanvec(C), dbeta=nanvec(C),
                                            dx_absmax=am, fixed_stats=True)
    assert same(dgam, bdg) and same(dbet, bdb), "1: the sums know the mode"
    within(h64(dbet), ref.S, ulp32(ref.S), "2: dbeta")
    within(h64(dgam), ref.SS, dSS, "2: dgamma")
    got = dx.cpu().view(rows, C)
    assert bool(torch.isfinite(got).all()) and bool((got == exact_dx(ref, gamma)).all()), "3: dx != fl32(a) dy'"
    assert block_max(am) == float(dx.abs().max())
    none, dg2, db2 = fn.bn_backward_maxpool(*args, relu=True, dx=fn.NO_OUTPUT, fixed_stats=True)
    assert none is None and same(dg2, dgam) and same(db2, dbet)
    # 7: the independent reading
    ax, ag, ab = autograd_reading(x, dy, mm, mv, gamma, beta, True)
    within(h64(dbet), ab, ulp32(ab), "7: dbeta")
    within(h64(dgam), ag, dSS, "7: dgamma")
    within(got.double(), ax, fixed_dx(ref, gamma)[1], "7: dx")


# ---------------------------------------------------------------------------------------------------------------------
# condition 7 on the plain route and the route from sum tables
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_autograd_reading_of_the_plain_and_the_sums_route(gpu_device, relu):
    rows, C, tiles_n = 300, 64, 17
    g = torch.Generator().manual_seed(4242 + int(relu))
    gamma, beta = gamma_beta(C, g)
    dy = int_dy((rows, C), g)
    x = general_input(rows, C, g)
    mm, mv = draw_moving(x, g)
    if relu:
        x = clear_of_zero(x, mm, mv, gamma, beta)
    shape = (1, 1, rows, C)
    xd, dyd, gd, bd = dev(x).view(shape), dev(dy).view(shape), dev(gamma), dev(beta)
    mean, rstd, scale, shift = global_stats(xd, gd, bd, mm, mv)
    ref = BwdRef(x, dy, h64(mean), h64(rstd), h64(scale), h64(shift), relu)
    ax, ag, ab = autograd_reading(x, dy, mm, mv, gamma, beta, relu)
    dx_bar = fixed_dx(ref, gamma)[1]
    # plain
    dSS = (slab_rows_for(rows) + 3) * U * ref.absT
    dx, dgam, dbet = fn.bn_backward(xd, scale, shift, dyd, mean, rstd, gd, relu=relu, fixed_stats=True)
    within(h64(dbet), ab, ulp32(ab), "7: dbeta (plain)")
    within(h64(dgam), ag, dSS, "7: dgamma (plain)")
    within(h64(dx).view(rows, C), ax, dx_bar, "7: dx (plain)")
    # from a table of the sums -- the reading's own: the finalize is held to them by the table route's bars
    tab = split_sums(ab, ag.float().double(), tiles_n, g)
    S, SS = tab[:, 0].double().sum(0), tab[:, 1].double().sum(0)
    assert torch.equal(S, ab)
    dx, dgam, dbet = fn.bn_backward_from_sums(xd, scale, shift, dyd, mean, rstd, gd, tab.cuda(), tiles_n, relu=relu,
                                              fixed_stats=True)
    within(h64(dbet), S, ulp32(S), "7: dbeta (from sums)")
    within(h64(dgam), SS, 2.0 ** -50 * tab[:, 1].double().abs().sum(0) + ulp32(SS), "7: dgamma (from sums)")
    within(h64(dx).view(rows, C), ax, dx_bar, "7: dx (from sums)")
    # the fix_gamma node (its own ReLU decisions: its own input)
    one = torch.ones_like(gamma)
    x1 = clear_of_zero(x, mm, mv, one, beta) if relu else x
    x1d = dev(x1).view(shape)
    m1, r1, s1, h1 = global_stats(x1d, None, bd, mm, mv)
    ref1 = BwdRef(x1, dy, h64(m1), h64(r1), h64(s1), h64(h1), relu)
    ax, ag, ab = autograd_reading(x1, dy, mm, mv, None, beta, relu)
    dx, dgam, dbet = fn.bn_backward(x1d, s1, h1, dyd, m1, r1, None, relu=relu, dgamma=nanvec(C), fixed_stats=True)
    within(h64(dbet), ab, ulp32(ab), "7: dbeta (fix_gamma)")
    within(h64(dgam), ag, (slab_rows_for(rows) + 3) * U * ref1.absT, "7: dgamma (fix_gamma)")
    within(h64(dx).view(rows, C), ax, fixed_dx(ref1, None)[1], "7: dx (fix_gamma)")


# ---------------------------------------------------------------------------------------------------------------------
# what the C ABI refuses, and that batch mode is what it was
def test_refusals_and_batch_mode_unchanged(gpu_device):
    L = fn.L()
    C, rows = 64, 40
    g = torch.Generator().manual_seed(5)
    P, st = fn.ptr, fn.stream()
    x, dy, _, gamma, beta = _small_case(C, 9, rows)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    tiles_n = 4
    gd, bd = dev(gamma), dev(beta)

    def refused(rc, text):
        assert rc != 0 and text in L.dspn_last_error(), (rc, L.dspn_last_error())

    for dt, sfx in ((torch.float32, "f32"), (BF, "bf16")):
        shape = (1, 1, rows, C)
        xd, dyd = dev(x, dt).view(shape), dev(dy, dt).view(shape)
        mean, rstd, scale, shift = fn.bn_stats(xd, EPS, gd, bd)
        plain, ex, sums = (getattr(L, f"dspn_bn_backward{n}_{sfx}") for n in ("", "_ex", "_from_sums"))

        def outs():
            return torch.full_like(xd, SENTINEL), nanvec(C), nanvec(C)

        def bwd(fn_, o, *tail, c=C):
            return fn_(P(xd), P(scale), P(shift), P(dyd), P(mean), P(rstd), P(gd), P(o[0]), P(o[1]), P(o[2]), rows, c, 1, 0, 0,
                       P(ws), ws.numel(), st, *tail)
        a, b, c_ = outs(), outs(), outs()
        assert bwd(plain, a) == 0 and bwd(ex, b, 0) == 0 and bwd(ex, c_, 1) == 0
        assert all(same(p, q) for p, q in zip(a, b)), f"_ex(..., 0) is not the plain entry point ({sfx})"
        assert same(a[1], c_[1]) and same(a[2], c_[2]) and not same(a[0], c_[0])
        for bad in (2, -1, 16):
            refused(bwd(ex, outs(), bad), b"fixed_stats")
        refused(bwd(ex, outs(), 1, c=6), b"positive multiple of 4")
        ref = BwdRef(x.double(), dy.double(), h64(mean), h64(rstd), h64(scale), h64(shift), True)
        tab = split_sums(ref.S, ref.SS.float().double(), tiles_n, g).cuda()

        def from_sums(flags, o, c=C):
            return sums(P(xd), P(scale), P(shift), P(dyd), P(mean), P(rstd), P(gd), P(tab), tiles_n, P(o[0]), P(o[1]), P(o[2]),
                        rows, c, 1, 0, 0, 0, 0, 0, flags, P(ws), ws.numel(), st)
        a, b = outs(), outs()
        assert from_sums(0, a) == 0
        got = fn.bn_backward_from_sums(xd, scale, shift, dyd, mean, rstd, gd, tab, tiles_n, relu=True, dx=b[0], dgamma=b[1],
                                       dbeta=b[2])
        assert all(same(p, q) for p, q in zip(a, got)), f"flag word 0 ({sfx})"
        refused(from_sums(16 | 2 | 4, outs()), b"flag word")
        refused(from_sums(16 | 8, outs()), b"flag word")                  # parked without finalize-only
        refused(from_sums(16 | 8 | 4, outs()), b"flag word")
        refused(from_sums(32, outs()), b"flag word")
        refused(from_sums(16, outs(), c=6), b"positive multiple of 4")
        # the apply half reads coefficients: the bit has no effect on it
        assert from_sums(16 | 2, a) == 0
        c1, c2 = outs(), outs()
        assert from_sums(4, c1) == 0 and from_sums(16 | 4, c2) == 0 and same(c1[0], c2[0])
        assert from_sums(16, b) == 0 and same(b[0], c1[0]), "whole call == finalize + apply"
    # the pooled form
    gq = torch.Generator().manual_seed(6)
    (N, H, W, Cp, k, s, p), xp, rec, dyp, _ = pooled_case(gq)
    gp, bp = gamma_beta(Cp, gq)
    xd, gpd = dev(xp).view(N, H, W, Cp), dev(gp)
    mean, rstd, scale, shift = fn.bn_stats(xd, EPS, gpd, dev(bp))
    dypd, recd = dev(dyp), rec.cuda()
    Ho, Wo = dyp.shape[1], dyp.shape[2]

    def pool(fn_, o, *tail, c=Cp):
        return fn_(P(xd), P(scale), P(shift), P(dypd), P(recd), N, H, W, c, k, s, p, Ho, Wo, P(mean), P(rstd), P(gpd), P(o[0]),
                   P(o[1]), P(o[2]), 1, 0, P(ws), ws.numel(), st, *tail)

    def pouts():
        return torch.full_like(xd, SENTINEL), nanvec(Cp), nanvec(Cp)
    a, b = pouts(), pouts()
    assert pool(L.dspn_bn_backward_maxpool_f32, a) == 0 and pool(L.dspn_bn_backward_maxpool_ex_f32, b, 0) == 0
    assert all(same(p_, q) for p_, q in zip(a, b)), "maxpool_ex(..., 0) is not the plain entry point"
    for bad in (2, -1):
        refused(pool(L.dspn_bn_backward_maxpool_ex_f32, pouts(), bad), b"fixed_stats")
    refused(pool(L.dspn_bn_backward_maxpool_ex_f32, pouts(), 1, c=6), b"C %")
    assert fn.bn_discard_parked(ctypes.c_void_p(st)) == 0            # nothing was parked by a refused call
    torch.cuda.synchronize()
