"""The gradient of a BatchNorm(+ReLU) output that is never stored (include/dspn_nn.h dspn_conv2d_dgrad_bn_sums_f32 /
dspn_conv2d_dgrad_bn_apply_f32).

bn1 of a dim-match residual unit reads the residual stream R; conv1 (1 x 1, C -> K = C / 4) alone reads its output.  PRESENT
pair: conv1's data gradient writes g, the gradient of that output, and gathers bn1's backward sums; the finalize; the apply
kernel reads R, g and dR and writes dR.  NEW sequence: the data gradient for the sums alone (no store), the same finalize, the
data gradient again with dR (+)= a g' + c1 R + c0 in its epilogue.  Same g per element, same sums, same element arithmetic:
the sum tables, dgamma / dbeta and dx must be the SAME BITS (the shared element function reproduces the apply kernel's
instruction sequence: no per-element rounding allowance is needed or given).

The magnitude block.  dx_absmax is 64 partial maxima; which slot holds which partial follows each kernel's launch grid
(blockIdx & 63 of a chunked element-wise grid there, of a persistent tile grid here), so slot by slot the two blocks cannot
agree and nothing reads them slot by slot: every consumer takes the maximum of the block.  Compared: that maximum, bit for bit,
and that it is max|dx| as stored.

Shapes (N, H, W, K, C, forced tile mode): the smallest that reach the wide family, tile configuration 0, ceil(M / 128)
ceil(C / 128) >= 256 (tests/ref_conv.py nt_config); K = 64 / 96 are two / three k-steps, the least either member takes.  1024
tiles are more than the persistent grid's workgroups: a workgroup walks several tiles, which is where the counted wait at the
head of a tile (no stores behind the sums pass's epilogue) matters.  The whole module runs in a few seconds."""
import numpy as np
import pytest
import torch

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from fp_bars import within
import ref_conv as R
import test_conv_edges_gpu as CE          # the data gradient's float64 bar (general_bar, its docstring derives it)
from test_strided_addend_gpu import planes_of, same_bits, tiles  # noqa: F401  (tiles: fixture)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

CASES = {
    "four waves, two k-steps, one tile per workgroup": (128, 16, 16, 64, 128, 0),
    "1024 tiles: a workgroup walks several, two column tiles": (256, 16, 16, 64, 256, 0),
    "a tile spans two images": (512, 8, 8, 64, 128, 0),
    "eight-wave 128 x 256 member, three k-steps": (64, 16, 16, 96, 256, 3),
    "eight-wave member, tiles span images": (256, 8, 8, 96, 256, 3),
}


class Unit:
    """operands of one dim-match unit's bn1 backward: R = x (N,H,W,C), conv1 C -> K with its dy as fp16 piece planes (as bn2's
    backward leaves it), dR0 = what the unit's other branch has already put into the residual stream's gradient"""

    def __init__(self, N, H, W, K, C, seed):
        g = torch.Generator().manual_seed(seed)
        self.shape, self.K, self.C = (N, H, W, C), K, C
        self.x = torch.randn(N, H, W, C, generator=g).cuda()
        self.dy = torch.randn(N, H, W, K, generator=g).cuda()
        self.w = (torch.randn(K, 1, 1, C, generator=g) / np.sqrt(K)).cuda()
        self.dR0 = torch.randn(N, H, W, C, generator=g).cuda()
        self.gamma, beta = torch.rand(C, generator=g).cuda() + 0.5, torch.randn(C, generator=g).cuda()
        self.mean, self.rstd, self.scale, self.shift = fn.bn_stats(self.x, 2e-5, self.gamma, beta)
        self.dyp, self.dya = planes_of(self.dy)
        self.wa = fn.absmax(self.w)
        self.wtp = fn.weight_planes(self.w, transposed=True, cols=K, math="f16x2", w_absmax=self.wa)
        self.tiles = fn.conv_dgrad_bn_tiles(self.shape, 1)
        self.kw = dict(wt_planes=self.wtp, math="f16x2", dy_absmax=self.dya, w_absmax=self.wa, dy_planes=True,
                       wt_shape=(C, 1, 1, K))

    def outputs(self, accumulate):
        C = self.C
        dx = self.dR0.clone() if accumulate else torch.full(self.shape, float("nan"), device="cuda")
        return dx, torch.zeros(self.tiles, 2, C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), \
            torch.zeros(fn.ABSMAX_SLOTS, device="cuda")

    def bn(self, relu, tab):
        return (self.x, self.scale, self.shift, self.mean, self.rstd, relu, tab)

    def present(self, relu, accumulate):
        dx, tab, dgam, dbet, am = self.outputs(accumulate)
        g = fn.conv2d_dgrad(self.dyp, None, self.shape, out=torch.full(self.shape, float("nan"), device="cuda"),
                            bn_bwd=self.bn(relu, tab), **self.kw)
        fn.bn_backward_from_sums(self.x, self.scale, self.shift, g, self.mean, self.rstd, self.gamma, tab, self.tiles, relu=relu,
                                 dx=dx, dgamma=dgam, dbeta=dbet, accumulate=accumulate, dx_absmax=am)
        return dx, tab, dgam, dbet, am

    def recomputed(self, relu, accumulate, park=False):
        dx, tab, dgam, dbet, am = self.outputs(accumulate)
        assert fn.conv2d_dgrad(self.dyp, None, self.shape, bn_bwd=self.bn(relu, tab), sums_only=True, **self.kw) is None
        self.ws = fn.bn_from_sums_workspace(self.tiles, self.C, "cuda")
        fn.bn_backward_from_sums(self.x, self.scale, self.shift, None, self.mean, self.rstd, self.gamma, tab, self.tiles, relu=relu,
                                 dx=dx, dgamma=dgam, dbeta=dbet, accumulate=accumulate, dx_absmax=am, phase=1, park=park,
                                 workspace=self.ws)
        fn.conv2d_dgrad_bn_apply(self.dyp, None, self.x, self.scale, self.shift, relu, self.ws, dx, accumulate=accumulate,
                                 dx_absmax=am, **self.kw)
        return dx, tab, dgam, dbet, am


def check_route(tiles, N, H, W, K, C, mode):
    tiles(mode)
    assert (N * H * W) % 128 == 0 and R.nt_config(N * H * W, C) == 0, "the case does not reach the wide family"
    assert fn.conv2d_dgrad_recompute_route((N, H, W, C), K, True), _lib.lib().dspn_last_error()


@pytest.mark.parametrize("relu", [False, True], ids=["no relu", "relu"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["first writer", "accumulate"])
@pytest.mark.parametrize("name", list(CASES))
def test_recomputed_sequence_gives_the_bits_of_the_present_pair(tiles, name, accumulate, relu):
    N, H, W, K, C, mode = CASES[name]
    check_route(tiles, N, H, W, K, C, mode)
    u = Unit(N, H, W, K, C, seed=N + W + C)
    old, new = u.present(relu, accumulate), u.recomputed(relu, accumulate)
    for a, b, what in zip(old[:4], new[:4], ("dx", "sum tables", "dgamma", "dbeta")):
        same_bits(a, b, f"{name}: {what}")
    dx, am = new[0], new[4]
    assert bool(torch.isfinite(dx).all())
    same_bits(old[4].max(), am.max(), f"{name}: largest entry of the dx_absmax block")
    assert float(am.max()) == float(dx.abs().max()) > 0


def test_a_parked_finalize_is_run_by_the_apply_pass(tiles):
    """the finalize parked for a weight gradient that never comes: the apply entry runs it first, as the apply half does"""
    N, H, W, K, C, mode = CASES["four waves, two k-steps, one tile per workgroup"]
    check_route(tiles, N, H, W, K, C, mode)
    u = Unit(N, H, W, K, C, seed=4)
    old, new = u.present(True, True), u.recomputed(True, True, park=True)
    for a, b, what in zip(old[:4], new[:4], ("dx", "sum tables", "dgamma", "dbeta")):
        same_bits(a, b, f"parked: {what}")
    assert _lib.lib().dspn_bn_discard_parked(fn.stream()) == 0, "the job was left parked"


@pytest.mark.parametrize("member", ["128 x 128 on four waves", "128 x 256 on eight waves"])
def test_float64_parity(tiles, member):
    """dR = a g' + c1 R + c0 + dR0 against float64 (torch CPU), per element.  g = dy w in float64; the mask from float64
    R scale + shift > 0 on the kernel's float scale / shift (tests/test_bn_edges_gpu.py item 5: identical to the kernel's fmaf
    mask for every element, none is excluded); the closed form with the coefficients a, c1, c0 the finalize left in the
    workspace -- the finalize is the present one, run on tables that are the present call's bits, and has its own float64 test
    there; what is new is the element.  Bar, derived: the data gradient's error reaches dR through a: |a| general_bar(f16x2)
    (+ its absolute term, as tests/test_strided_addend_gpu.py); then four roundings -- the product a g', the fused c1 R onto
    it, + c0, + dR0 -- each at most U times the magnitude of what it rounds, which the sum of the magnitudes of the terms
    added so far bounds: U (4 |a g'| + 3 |c1 R| + 2 |c0| + |dR0|) to first order."""
    N, H, W, K, C, mode = (128, 16, 16, 64, 128, 0) if member.startswith("128 x 128") else (64, 16, 16, 96, 256, 3)
    check_route(tiles, N, H, W, K, C, mode)
    u = Unit(N, H, W, K, C, seed=3)
    dx = u.recomputed(True, True)[0].cpu().double()
    coef = u.ws[:12 * C].view(torch.float32).cpu().double()
    a, c1, c0 = coef[:C], coef[C:2 * C], coef[2 * C:]
    dy, w, x, dR0 = (t.cpu().double() for t in (u.dy, u.w.view(K, C), u.x, u.dR0))
    g, S = dy @ w, dy.abs() @ w.abs()
    extra = 2.0 ** -39 * (float(dy.abs().max()) * w.abs().sum(0).expand_as(g) + float(w.abs().max()) * dy.abs().sum(-1, keepdim=True))
    mask = (x * u.scale.cpu().double() + u.shift.cpu().double()) > 0
    gm = torch.where(mask, g, torch.zeros_like(g))
    exp = a * gm + c1 * x + c0 + dR0
    bar = a.abs() * torch.where(mask, CE.general_bar("f16x2", S, K, 1, extra), torch.zeros_like(S))
    bar = bar + U * (4 * (a * gm).abs() + 3 * (c1 * x).abs() + 2 * c0.abs() + dR0.abs())
    within(dx, exp, bar, f"dx of the recomputed sequence [{member}]")


def test_refusals_name_the_entry_point_and_the_query_says_no(tiles):
    """M % 128 != 0, a float dy, fp32 and three-piece math, split-K, a strided dx, bfloat16 tensors: non-zero, dspn_last_error
    names the entry, nothing is launched; the query the engine asks first answers 0 for the shapes no kernel takes"""
    L = _lib.lib()
    tiles(0)
    N, H, W, K, C = 128, 16, 16, 64, 128
    u = Unit(N, H, W, K, C, seed=9)
    wt = fn.weight_transpose(u.w)
    tab = torch.zeros(u.tiles, 2, C, device="cuda")
    ws = fn.bn_from_sums_workspace(u.tiles, C, "cuda")
    dx = torch.zeros(u.shape, device="cuda")
    SUMS, APPLY = "dspn_conv2d_dgrad_bn_sums_f32", "dspn_conv2d_dgrad_bn_apply_f32"

    def refused(what, dy, wt_, x=u.x, shape=u.shape, tab=tab, ws=ws, dx=dx, sums=SUMS, apply=APPLY, **kw):
        with pytest.raises(_lib.DspnError, match=sums) as e:
            fn.conv2d_dgrad(dy, wt_, shape, bn_bwd=(x, u.scale, u.shift, u.mean, u.rstd, True, tab), sums_only=True, **kw)
        assert sums.encode() in L.dspn_last_error()
        print(f"    {what}: {e.value}")
        with pytest.raises(_lib.DspnError, match=apply) as e:
            fn.conv2d_dgrad_bn_apply(dy, wt_, x, u.scale, u.shift, True, ws, dx, accumulate=True, **kw)
        assert apply.encode() in L.dspn_last_error()
        print(f"    {what}: {e.value}")
    planes = dict(wt_planes=u.wtp, dy_absmax=u.dya, w_absmax=u.wa, wt_shape=(C, 1, 1, K))
    refused("fp32 math", u.dy, wt, math="fp32")
    refused("three-piece math", u.dy, None, math="bf16x3", wt_shape=(C, 1, 1, K),
            wt_planes=fn.weight_planes(u.w, transposed=True, cols=K, math="bf16x3"))
    refused("float dy", u.dy, None, math="f16x2", **planes)
    # M % 128 != 0: 129 images of 15 x 17 -- tile configuration 0, but no whole 128-row tiles: not the tile-spanning loop
    n3, h3, w3 = 129, 15, 17
    assert R.nt_config(n3 * h3 * w3, C) == 0 and (n3 * h3 * w3) % 128 != 0
    assert not fn.conv2d_dgrad_recompute_route((n3, h3, w3, C), K, True)
    o = Unit(n3, h3, w3, K, C, seed=5)
    refused("M % 128 != 0", o.dyp, None, x=o.x, shape=o.shape, tab=torch.zeros(o.tiles, 2, C, device="cuda"),
            dx=torch.zeros(o.shape, device="cuda"), **o.kw)
    # a strided dx (rows of 2 C floats): the raw entries
    wide = torch.zeros(N, H, W, 2 * C, device="cuda")
    with pytest.raises(_lib.DspnError, match=APPLY):
        _lib.check(L.dspn_conv2d_dgrad_bn_apply_f32(fn.ptr(u.dyp), None, fn.ptr(u.wtp), fn.ptr(wide), N, H, W, C, K, 1, 1, 1, 0, 0, 1, H, W,
                                                     2 * C, 0, fn.ptr(u.x), fn.ptr(u.scale), fn.ptr(u.shift), 1, None,
                                                     3 | fn.MATH_DY_PLANES, fn.ptr(u.dya), fn.ptr(u.wa), fn.ptr(ws), ws.numel(), fn.stream()))
    with pytest.raises(_lib.DspnError, match=SUMS):
        _lib.check(L.dspn_conv2d_dgrad_bn_sums_f32(fn.ptr(u.dyp), None, fn.ptr(u.wtp), None, N, H, W, C, K, 1, 1, 1, 0, 0, 1, H, W,
                                                    2 * C, 0, fn.ptr(u.x), fn.ptr(u.scale), fn.ptr(u.shift), fn.ptr(u.mean), fn.ptr(u.rstd),
                                                    1, fn.ptr(tab), tab.numel() * 4, None, 3 | fn.MATH_DY_PLANES, fn.ptr(u.dya),
                                                    fn.ptr(u.wa), None, 0, fn.stream()))
    # split-K: few row tiles, a long contraction -- a shape whose plain data gradient is split over K
    n2, k2 = 2, 1024
    assert R.nt_route(n2 * 64, C, k2, 1)["splits"] > 1 and not fn.conv2d_dgrad_recompute_route((n2, 8, 8, C), k2, True)
    s = Unit(n2, 8, 8, k2, C, seed=2)
    with pytest.raises(_lib.DspnError, match=APPLY):
        fn.conv2d_dgrad_bn_apply(s.dyp, None, s.x, s.scale, s.shift, True, fn.bn_from_sums_workspace(s.tiles, C, "cuda"),
                                 torch.zeros(s.shape, device="cuda"), **s.kw)
    assert b"split-K" in L.dspn_last_error()
    with pytest.raises(_lib.DspnError, match=SUMS):
        fn.conv2d_dgrad(s.dyp, None, s.shape, bn_bwd=(s.x, s.scale, s.shift, s.mean, s.rstd, True, torch.zeros(s.tiles, 2, C, device="cuda")),
                        sums_only=True, **s.kw)
    assert b"split-K" in L.dspn_last_error()
    # bfloat16 tensors
    BF = torch.bfloat16
    xb = u.x[:2].to(BF)
    wtb = fn.weight_transpose(u.w, dtype=BF)
    with pytest.raises(_lib.DspnError, match="dspn_conv2d_dgrad_bn_sums_bf16"):
        fn.conv2d_dgrad(u.dy[:2].to(BF), wtb, xb.shape, math="bf16", sums_only=True,
                        bn_bwd=(xb, u.scale, u.shift, u.mean, u.rstd, True, torch.zeros(fn.conv_dgrad_bn_tiles(xb.shape, 1), 2, C, device="cuda")))
    with pytest.raises(_lib.DspnError, match="dspn_conv2d_dgrad_bn_apply_bf16"):
        fn.conv2d_dgrad_bn_apply(u.dy[:2].to(BF), wtb, xb, u.scale, u.shift, True, ws, torch.zeros_like(xb), math="bf16")
    # nothing above launched or parked anything, and the routed shape still answers yes
    assert fn.conv2d_dgrad_recompute_route(u.shape, K, True) and not fn.conv2d_dgrad_recompute_route(u.shape, K, False)


# ---------------------------------------------------------------------------------------------------------------------
# the graph: conv0 (128 channels) -> a stride-1 projection unit (256 channels; its bn1 feeds conv1 AND the shortcut: no pair)
# -> a dim-match unit (the pair: bn1 reads the residual stream, conv1 256 -> 64 alone reads bn1).  B = 2 at 128 x 128: 256 row
# tiles x 2 column tiles, two k-steps -- the route runs.  (With 128 channels in the residual stream conv1's product has ONE
# k-step, K = 32, which the wide family does not take: the query says no and nothing would be tested.)
def toy_step(knob, monkeypatch, frozen=(), guard_on_conv1=False, wgrad_side=None, steps=2):
    from dspnet_amd import engine as E
    from dspnet_amd.symbol import resnet
    dev = torch.device("cuda", 0)
    B, size = 2, 128
    gen = torch.Generator().manual_seed(17)
    x0 = torch.randn(B, size, size, 32, generator=gen).to(dev)
    monkeypatch.setattr(E, "BN1_RECOMPUTE", 2 if knob else 0)
    if wgrad_side is not None:      # every weight gradient beside the chain, or none (tests/test_graph_gpu.py)
        monkeypatch.setattr(E, "WGRAD_SIDE", wgrad_side)
        monkeypatch.setattr(E, "WGRAD_SIDE_MIN_US", 0.0)
        monkeypatch.setattr(E.Graph, "batchnorm_chain", lambda self: True)
    prev = fn.get_conv_math()
    fn.set_conv_math("f16x2")
    try:
        g = E.Graph(dev)
        if frozen:
            g.set_freeze(list(frozen))
        x = g.tensor(x0.shape, "data", data=x0.clone())
        c0 = g.add(E.Conv(g, x, "conv0", 128, 3, pad=1)).out
        u1 = resnet.residual_unit(g, c0, 256, 1, False, "stage1_unit1", "_plus0")
        u2 = resnet.residual_unit(g, u1, 256, 1, True, "stage1_unit2", "_plus1")
        g.finalize(seed=5)
        conv1 = g.tensors["stage1_unit2_conv1_out"].producer
        assert conv1.bn1_recompute and conv1.bn_bwd_node is g.tensors["stage1_unit2_bn1_relu"].bn_node, "graph_plan did not mark the pair"
        assert not g.tensors["stage1_unit1_conv1_out"].producer.bn1_recompute, "conv1 of a projection unit shares bn1 with the shortcut"
        g.guard["enabled"] = False
        dy = torch.randn(u2.shape, generator=gen).to(dev)
        outs = []
        for _ in range(steps):          # (the second pass reads the first one's state: magnitudes, piece planes of the gradients)
            g.forward()
            conv1.guard_fb = guard_on_conv1
            g.begin_backward()
            u2.give_grad(dy.clone())
            for idx in range(len(g.nodes) - 1, -1, -1):
                g.backward_node(idx)
            g.join_side_backward()
            g.flush_slabs()
            torch.cuda.synchronize()
            outs.append((g.grad_arena.clone(), x.grad.clone(), u2.data.clone()))
        return outs, g.bn1_recompute_calls
    finally:
        fn.set_conv_math(prev)


VARIANTS = {
    "plain": dict(),
    "guard fallback on conv1": dict(guard_on_conv1=True),
    "bn1 gamma and beta frozen": dict(frozen=("stage1_unit2_bn1_gamma", "stage1_unit2_bn1_beta")),
    "every weight gradient beside the chain": dict(wgrad_side=1),
    "one stream, the finalize parked for the weight gradient": dict(wgrad_side=0),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_graph_step_is_bit_identical_with_the_knob_on_and_off(gpu_device, monkeypatch, variant):
    """Two steps with the knob on and off: every gradient of the arena, the input gradient and the output are the same bits.
    The route RUNS with the knob on (one apply pass per step, counted), also with bn1's gamma / beta frozen (dgamma / dbeta are
    then not computed; dx still is) and under either weight-gradient schedule -- beside the chain the finalize is a launch of
    its own, on one stream it is parked and rides in conv1's weight gradient -- and does NOT run with conv1 on the range guard's
    fallback (that call multiplies a float gradient in another math).  The schedules give each other's bits too."""
    kw = VARIANTS[variant]
    with monkeypatch.context() as m:
        off, n_off = toy_step(False, m, **kw)
    with monkeypatch.context() as m:
        on, n_on = toy_step(True, m, **kw)
    assert n_off == 0
    assert n_on == (0 if kw.get("guard_on_conv1") else 2), "the route did not run where it should (or ran where it should not)"
    for step, (a, b) in enumerate(zip(off, on)):
        for t, v, name in zip(a, b, ("gradient arena", "input gradient", "output")):
            assert bool(torch.isfinite(t).all()), name
            same_bits(t, v, f"step {step}: {name}")
    assert float(on[1][0].abs().max()) > 0
    if "wgrad_side" in kw:      # ... and the bits of the serial schedule
        with monkeypatch.context() as m:
            serial, _ = toy_step(True, m, wgrad_side=0)
        for t, v, name in zip(serial[1], on[1], ("gradient arena", "input gradient", "output")):
            same_bits(t, v, f"against the serial schedule: {name}")


def test_route_inside_a_captured_step(gpu_device, monkeypatch):
    """MultiTaskSolver.capture records the step as a graph: the route's two launches and the finalize between them are plain
    stream work, so the recorded step gives the knob-off bits.  resnet-50 at 128 x 128, batch 32: stage 1 (M = 32768, C = 256,
    K = 64) reaches the route; forced everywhere it exists (setting 2)."""
    from dspnet_amd import engine as E
    from dspnet_amd import synthetic
    from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
    from dspnet_amd.train.solver import MultiTaskSolver
    dev = torch.device("cuda", 0)
    prev = fn.get_conv_math()
    fn.set_conv_math("f16x2")

    def run(knob):
        monkeypatch.setattr(E, "BN1_RECOMPUTE", knob)
        net = get_multi_symbol_train("resnet-50", (3, 128, 128), num_classes=8, batch_size=32, device=dev, seed=0)
        gen = synthetic.rng(233)
        solver = MultiTaskSolver(net)
        solver.set_batch(torch.from_numpy(synthetic.images(32, 128, 128, gen)).to(dev),
                         torch.from_numpy(synthetic.det_labels(32, gen=gen, height=128, width=128)).to(dev),
                         torch.from_numpy(synthetic.seg_labels(32, 128, 128, gen=gen)).to(dev))
        solver.step()
        captured = solver.capture()
        calls = net.g.bn1_recompute_calls
        for _ in range(2):
            solver.step()          # (replays: no call goes through the engine)
        torch.cuda.synchronize()
        assert net.g.bn1_recompute_calls == calls or not captured
        return net.g.arena.detach().clone(), calls, captured
    try:
        a, n_a, _ = run(0)
        b, n_b, captured = run(2)
    finally:
        fn.set_conv_math(prev)
    assert n_a == 0 and n_b > 0 and captured, (n_a, n_b, captured)
    assert bool(torch.isfinite(a).all())
    same_bits(a, b, "parameter arena after the eager, the recorded and two replayed steps")
