"""The projection units' shortcut gradient kept compact (include/dspn_nn.h dspn_conv2d_dgrad_bn_sadd_f32).

act1 = relu(bn1(x)) feeds conv1 (1 x 1, stride 1) and the projection shortcut (1 x 1, stride 2, pad 0).  PRESENT pair of calls:
the shortcut's four-class stride-2 data gradient writes act1's gradient first (three quarters of it zeros), conv1's data
gradient accumulates and gathers the BatchNorm-backward sums.  NEW pair: the shortcut's gradient as the stride-1 data gradient
on the subsampled grid, a compact (N, ceil(H/2), ceil(W/2), C) tensor, which conv1's data gradient -- the only writer -- adds at
the even positions where the accumulate addend was added.  Same order of additions: dx, the sum tables and the bn_dy_absmax
block must be the SAME BITS.

Shapes.  The operand exists in the plane-fed 128-row tiles on the tile-spanning loop, which dispatch_nt reaches only on tile
configuration 0: ceil(M / 128) ceil(C / 128) >= 256 (tests/ref_conv.py nt_config).  The cases are the smallest that keep that
and still have the property they are there for (8 x 8 images of 64 rows: a tile spans two images; W = 16: eight image rows;
W = 24: no power of two -- the operand asks for W % 4 == 0 and W >= 8, which every stage of the ResNets has; 15 x 17: odd sizes and M % 128 != 0, which the tile-spanning loop does not take: the refusal, and the
route query by which the engine keeps the present pair).  K = 64 / 96 are two / three k-steps: the least either member takes.
The whole module runs in a few seconds."""
import numpy as np
import pytest
import torch

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from fp_bars import within
import ref_conv as R
import test_conv_edges_gpu as CE          # the data gradient's float64 bar (general_bar, its docstring derives it)

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture()
def tiles(gpu_device):
    L = _lib.lib()
    yield lambda mode: _lib.check(L.dspn_conv_set_wide_tiles(mode), "set_wide_tiles")
    L.dspn_conv_set_wide_tiles(0)


def planes_of(t):
    am = fn.absmax(t)
    one, zero = torch.ones(t.shape[-1], device="cuda"), torch.zeros(t.shape[-1], device="cuda")
    return fn.bn_apply_planes(t, one, zero, am), am


class Pair:
    """operands of one projection unit's two data gradients: conv1 C -> K (its dy as fp16 piece planes, as bn2's backward
    leaves it), shortcut C -> 2K at stride 2 (its dy a float tensor: conv3's output gradient)"""

    def __init__(self, N, H, W, K, C, seed, dy1=None):
        g = torch.Generator().manual_seed(seed)
        self.shape = (N, H, W, C)
        self.Ho, self.Wo = (H + 1) // 2, (W + 1) // 2
        self.x = torch.randn(N, H, W, C, generator=g).cuda()
        self.dy1 = (torch.randn(N, H, W, K, generator=g) if dy1 is None else dy1(g)).cuda()
        self.dys = torch.randn(N, self.Ho, self.Wo, 2 * K, generator=g).cuda()
        self.w1 = (torch.randn(K, 1, 1, C, generator=g) / np.sqrt(K)).cuda()
        self.ws = (torch.randn(2 * K, 1, 1, C, generator=g) / np.sqrt(2 * K)).cuda()
        gamma, beta = torch.rand(C, generator=g).cuda() + 0.5, torch.randn(C, generator=g).cuda()
        self.mean, self.rstd, self.scale, self.shift = fn.bn_stats(self.x, 2e-5, gamma, beta)
        self.dy1p, self.dy1a = planes_of(self.dy1)
        self.w1a, self.wsa, self.dysa = fn.absmax(self.w1), fn.absmax(self.ws), fn.absmax(self.dys)
        self.wt1p = fn.weight_planes(self.w1, transposed=True, cols=K, math="f16x2", w_absmax=self.w1a)
        self.wtsp = fn.weight_planes(self.ws, transposed=True, cols=2 * K, math="f16x2", w_absmax=self.wsa)
        self.K, self.C = K, C
        self.tiles = fn.conv_dgrad_bn_tiles(self.shape, 1)

    def shortcut(self, x_shape, stride, out):
        return fn.conv2d_dgrad(self.dys, None, x_shape, stride, 0, 1, out=out, wt_planes=self.wtsp, math="f16x2",
                               dy_absmax=self.dysa, w_absmax=self.wsa, wt_shape=(self.C, 1, 1, 2 * self.K))

    def conv1(self, out, sums=True, **kw):
        N, H, W, C = self.shape
        tab = torch.zeros(self.tiles, 2, C, device="cuda") if sums else None
        bam = torch.zeros(fn.ABSMAX_SLOTS, device="cuda") if sums else None
        fn.conv2d_dgrad(self.dy1p, None, self.shape, 1, 0, 1, out=out, wt_planes=self.wt1p, math="f16x2", dy_absmax=self.dy1a,
                        w_absmax=self.w1a, dy_planes=True, wt_shape=(C, 1, 1, self.K), bn_dy_absmax=bam,
                        bn_bwd=(self.x, self.scale, self.shift, self.mean, self.rstd, True, tab) if sums else None, **kw)
        return out, tab, bam

    def present(self):
        dx = torch.full(self.shape, float("nan"), device="cuda")
        self.shortcut(self.shape, 2, dx)
        return self.conv1(dx, accumulate=True)

    def compact(self):
        N, H, W, C = self.shape
        dxc = self.shortcut((N, self.Ho, self.Wo, C), 1, torch.full((N, self.Ho, self.Wo, C), float("nan"), device="cuda"))
        return self.conv1(torch.full(self.shape, float("nan"), device="cuda"), strided_addend=dxc)


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    diff = a.view(torch.int32) != b.view(torch.int32)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {a.numel()} words differ"


def compare(p, what):
    old, new = p.present(), p.compact()
    for a, b, name in zip(old, new, ("dx", "sum tables", "bn_dy_absmax")):
        same_bits(a, b, f"{what}: {name}")
    assert bool(torch.isfinite(new[0]).all()) and float(new[2].max()) == float(new[0].abs().max()) > 0
    return new


# (N, H, W, K, C, forced tile mode): M = N H W; rows per image H W
CASES = {
    "plain: a tile spans 8 image rows": (128, 16, 16, 64, 128, 0),
    "a tile spans two images": (512, 8, 8, 64, 128, 0),
    "W not a power of two": (86, 16, 24, 64, 128, 0),
    "eight-wave 128 x 256 member": (64, 16, 16, 96, 256, 3),
    "eight-wave member, tiles span images": (256, 8, 8, 96, 256, 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_compact_pair_gives_the_bits_of_the_accumulating_pair(tiles, name):
    N, H, W, K, C, mode = CASES[name]
    tiles(mode)
    assert (N * H * W) % 128 == 0 and R.nt_config(N * H * W, C) == 0, "the case does not reach the wide family"
    assert fn.conv2d_dgrad_addend_route((N, H, W, C), K, True), _lib.lib().dspn_last_error()
    compare(Pair(N, H, W, K, C, seed=N + W + C), name)


# the shapes as the issue's table lists them (N = 1, 4, 1, 2): one to four row tiles -- tile configuration 2, 64-row BatchNorm
# tables, conv_nt_kernel -- which no setting of dspn_conv_set_wide_tiles moves into the wide family (dispatch_nt asks for
# configuration 0 first).  Kept as cases of the legality rule: the query says no, the call is refused by name, and the
# accumulating pair is what runs there.  CASES above are the same H x W, K, C with N raised until configuration 0 is reached.
@pytest.mark.parametrize("shape", [(1, 16, 16, 64, 128, 0), (4, 8, 8, 64, 128, 0), (1, 16, 24, 64, 128, 0), (2, 15, 17, 64, 128, 0),
                                   (1, 16, 16, 96, 256, 3)], ids=str)
def test_issue_table_shapes_stay_on_the_accumulating_pair(tiles, shape):
    N, H, W, K, C, mode = shape
    tiles(mode)
    assert R.nt_config(N * H * W, C) != 0
    assert not fn.conv2d_dgrad_addend_route((N, H, W, C), K, True)
    p = Pair(N, H, W, K, C, seed=N + H)
    with pytest.raises(_lib.DspnError, match="dspn_conv2d_dgrad_bn_sadd_f32"):
        p.compact()
    dx, tab, bam = p.present()
    assert bool(torch.isfinite(dx).all()) and float(bam.max()) == float(dx.abs().max())


def test_signed_zero_becomes_plus_zero_as_on_the_accumulating_path(tiles):
    """Rows of dy whose only non-zero element is the smallest float32 subnormal, in a dy of magnitude 2^-110: the two-piece
    operand keeps it (2^-24 after the scale), its product with a weight below 1/2 underflows in the epilogue's rescaling to a
    signed zero (no call of the library stores one: every epilogue adds its addend or +0.0f; the precondition is taken from
    float64).  Where there is no addend the accumulating path adds the +0.0f the shortcut stored and the new path adds
    +0.0f itself: -0.0f becomes +0.0f on both, bit for bit."""
    N, H, W, K, C = 128, 16, 16, 64, 128

    def dy1(g):
        t = torch.randn(N, H, W, K, generator=g) * 2.0 ** -112
        t[:, 1::4, :, :] = 0.0                       # (odd rows: no addend there)
        t[:, 1::4, :, 0] = -(2.0 ** -149)
        t[:, 2::4, 1::2, :] = 0.0                    # (even rows, odd columns)
        t[:, 2::4, 1::2, 0] = 2.0 ** -149
        return t
    tiles(0)
    p = Pair(N, H, W, K, C, seed=11, dy1=dy1)
    assert float(p.dy1[0, 1, 0, 0]) == -(2.0 ** -149), "the subnormal did not survive the copy to the device"
    # float64: at these positions the gradient is negative and below half the smallest subnormal -- its float32 value is -0.0f
    exact = p.dy1.cpu().double() @ p.w1.view(K, C).cpu().double()
    odd = torch.zeros(p.shape, dtype=torch.bool)
    odd[:, 1::2] = True
    odd[:, :, 1::2] = True
    minus_zero = (exact < 0) & (exact > -(2.0 ** -150)) & odd
    assert int(minus_zero.sum()) > 1000, "the inputs are unfit: no result that rounds to -0.0f where there is no addend"
    dx = compare(p, "signed zero")[0].cpu()
    assert bool((dx[minus_zero].view(torch.int32) == 0).all()), "a -0.0f result was stored as it is: the +0.0f addend is missing"
    assert not bool(((dx.view(torch.int32) == -2 ** 31) & odd).any())


def test_odd_sizes_are_refused_and_the_route_query_says_so(tiles):
    """15 x 17 images, M % 128 != 0: the tile-spanning loop (whole 128-row tiles) does not take the call, so nothing takes
    the operand: the call is refused by name, the query the engine asks first answers 0, and the accumulating pair -- what
    the engine then runs -- is unaffected (covered by the existing suite; run here once to pin that it still gives finite,
    complete results at this shape)."""
    N, H, W, K, C = 129, 15, 17, 64, 128
    tiles(0)
    assert R.nt_config(N * H * W, C) == 0 and (N * H * W) % 128 != 0
    assert not fn.conv2d_dgrad_addend_route((N, H, W, C), K, True)
    # ... and a W that is no multiple of four (the epilogue places the addend per group of four rows inside one image row),
    # at a size that is otherwise routed: 128 images of 16 x 18, 288 tiles of 128 rows
    assert R.nt_config(128 * 16 * 18, C) == 0 and not fn.conv2d_dgrad_addend_route((128, 16, 18, C), K, True)
    assert b"W % 4 == 0" in _lib.lib().dspn_last_error() and fn.conv2d_dgrad_addend_route((128, 16, 20, C), K, True)
    p = Pair(N, H, W, K, C, seed=5)
    with pytest.raises(_lib.DspnError, match="dspn_conv2d_dgrad_bn_sadd_f32"):
        p.compact()
    dx, tab, bam = p.present()
    assert bool(torch.isfinite(dx).all()) and float(bam.max()) == float(dx.abs().max())


@pytest.mark.parametrize("member", ["128 x 128 on four waves", "128 x 256 on eight waves"])
def test_float64_parity(tiles, member):
    """dx = conv1's data gradient + the shortcut's at the even positions, against float64 (torch CPU), per element, at the
    data gradient's bar of tests/test_conv_edges_gpu.py (general_bar: (n_acc U + 2^-21) S per convolution, the two-piece
    math's absolute term 2^-39 (max|dy| sum|w| + max|w| sum|dy|) each, one rounding for the addition of the addend)."""
    N, H, W, K, C, mode = (128, 16, 16, 64, 128, 0) if member.startswith("128 x 128") else (64, 16, 16, 96, 256, 3)
    tiles(mode)
    p = Pair(N, H, W, K, C, seed=3)
    dx = p.compact()[0].cpu().double()
    dy1, dys, w1, ws = (t.cpu().double() for t in (p.dy1, p.dys, p.w1.view(K, C), p.ws.view(2 * K, C)))
    exp, S = dy1 @ w1, dy1.abs() @ w1.abs()
    extra = 2.0 ** -39 * (float(dy1.abs().max()) * w1.abs().sum(0).expand_as(exp) + float(w1.abs().max()) * dy1.abs().sum(-1, keepdim=True))
    bar = CE.general_bar("f16x2", S, K, 1, extra)
    es, Ss = dys @ ws, dys.abs() @ ws.abs()
    extra_s = 2.0 ** -39 * (float(dys.abs().max()) * ws.abs().sum(0).expand_as(es) + float(ws.abs().max()) * dys.abs().sum(-1, keepdim=True))
    exp[:, ::2, ::2] += es
    bar[:, ::2, ::2] += CE.general_bar("f16x2", Ss, 2 * K, 0, extra_s) + CE.U * Ss
    within(dx, exp, bar, f"dx with the strided addend [{member}]")


def test_refusals_name_the_entry_point(tiles):
    """the operand with fp32 math, bf16 tensors, split-K or a strided dx: non-zero, and dspn_last_error names the entry"""
    L = _lib.lib()
    tiles(0)
    N, H, W, K, C = 128, 16, 16, 64, 128
    p = Pair(N, H, W, K, C, seed=9)
    dxc = p.shortcut((N, p.Ho, p.Wo, C), 1, torch.empty(N, p.Ho, p.Wo, C, device="cuda"))
    wt1 = fn.weight_transpose(p.w1)
    dx = torch.zeros(p.shape, device="cuda")
    tab = torch.zeros(p.tiles, 2, C, device="cuda")
    bn = (p.x, p.scale, p.shift, p.mean, p.rstd, True, tab)

    def refused(what, entry="dspn_conv2d_dgrad_bn_sadd_f32", **kw):
        with pytest.raises(_lib.DspnError, match=entry) as e:
            fn.conv2d_dgrad(**kw)
        print(f"    {what}: {e.value}")
        assert entry.encode() in L.dspn_last_error()
    refused("fp32 math", dy=p.dy1, wt=wt1, x_shape=p.shape, out=dx, bn_bwd=bn, math="fp32", strided_addend=dxc)
    refused("three-piece math", dy=p.dy1, wt=None, x_shape=p.shape, out=dx, bn_bwd=bn, math="bf16x3", wt_shape=(C, 1, 1, K),
            wt_planes=fn.weight_planes(p.w1, transposed=True, cols=K, math="bf16x3"), strided_addend=dxc)
    # dy as a float tensor: the float-operand members have no such epilogue
    refused("float dy", dy=p.dy1, wt=None, x_shape=p.shape, out=dx, bn_bwd=bn, math="f16x2", wt_shape=(C, 1, 1, K),
            wt_planes=p.wt1p, dy_absmax=p.dy1a, w_absmax=p.w1a, strided_addend=dxc)
    # a strided dx (rows of 2 C floats)
    wide = torch.zeros(N, H, W, 2 * C, device="cuda")
    with pytest.raises(_lib.DspnError, match="dspn_conv2d_dgrad_bn_sadd_f32"):
        _lib.check(L.dspn_conv2d_dgrad_bn_sadd_f32(fn.ptr(p.dy1p), None, fn.ptr(p.wt1p), fn.ptr(wide), N, H, W, C, K, 1, 1, 1, 0, 0, 1, H, W,
                                                    2 * C, 0, None, None, None, None, None, 0, None, 0, None, 3 | fn.MATH_DY_PLANES,
                                                    fn.ptr(p.dy1a), fn.ptr(p.w1a), None, 0, fn.ptr(dxc), p.Ho, p.Wo, fn.stream()))
    # accumulate beside the operand
    refused("accumulate", dy=p.dy1p, wt=None, x_shape=p.shape, out=dx, bn_bwd=bn, math="f16x2", wt_shape=(C, 1, 1, K), accumulate=True,
            wt_planes=p.wt1p, dy_absmax=p.dy1a, w_absmax=p.w1a, dy_planes=True, strided_addend=dxc)
    # split-K: few row tiles, a long contraction, no BatchNorm sums
    n2, k2 = 2, 1024
    g = torch.Generator().manual_seed(2)
    dy2 = torch.randn(n2, 8, 8, k2, generator=g).cuda()
    w2 = (torch.randn(k2, 1, 1, C, generator=g) / 32).cuda()
    assert R.nt_route(n2 * 64, C, k2, 1)["splits"] > 1
    dy2p, dy2a = planes_of(dy2)
    w2a = fn.absmax(w2)
    refused("split-K", dy=dy2p, wt=None, x_shape=(n2, 8, 8, C), out=torch.zeros(n2, 8, 8, C, device="cuda"), math="f16x2",
            wt_shape=(C, 1, 1, k2), wt_planes=fn.weight_planes(w2, transposed=True, cols=k2, math="f16x2", w_absmax=w2a),
            dy_absmax=dy2a, w_absmax=w2a, dy_planes=True, strided_addend=torch.zeros(n2, 4, 4, C, device="cuda"))
    assert b"split-K" in L.dspn_last_error()
    # bfloat16 tensors
    BF = torch.bfloat16
    xb = p.x[:2].to(BF)
    with pytest.raises(_lib.DspnError, match="dspn_conv2d_dgrad_bn_sadd_bf16"):
        fn.conv2d_dgrad(p.dy1[:2].to(BF), fn.weight_transpose(p.w1, dtype=BF), xb.shape, out=torch.zeros_like(xb), math="bf16",
                        strided_addend=torch.zeros(2, p.Ho, p.Wo, C, device="cuda", dtype=BF))


# ---------------------------------------------------------------------------------------------------------------------
# the graph: conv0 -> a stride-1 projection unit (no pair) -> a stride-2 projection unit (the pair)
def toy_step(size, C, knob, monkeypatch, frozen=False, guard_on_conv1=False):
    from dspnet_amd import engine as E
    from dspnet_amd.symbol import resnet
    dev = torch.device("cuda", 0)
    B = 2
    gen = torch.Generator().manual_seed(17)
    x0 = torch.randn(B, size, size, 32, generator=gen).to(dev)
    monkeypatch.setattr(E, "SC_COMPACT", knob)
    used = []
    orig = fn.conv2d_dgrad

    def counting(*a, **kw):
        used.append(kw.get("strided_addend") is not None)
        return orig(*a, **kw)
    monkeypatch.setattr(fn, "conv2d_dgrad", counting)
    prev = fn.get_conv_math()
    fn.set_conv_math("f16x2")
    try:
        g = E.Graph(dev)
        if frozen:
            g.set_freeze(["stage2_unit1_sc_weight"])
        x = g.tensor(x0.shape, "data", data=x0.clone())
        c0 = g.add(E.Conv(g, x, "conv0", C // 2, 3, pad=1)).out
        u1 = resnet.residual_unit(g, c0, C, 1, False, "stage1_unit1", "_plus0")
        u2 = resnet.residual_unit(g, u1, 2 * C, 2, False, "stage2_unit1", "_plus1")
        g.finalize(seed=5)
        conv1, sc = g.tensors["stage2_unit1_conv1_out"].producer, g.tensors["stage2_unit1_sc_out"].producer
        assert conv1.sc_pair is sc and sc.sc_pair is conv1, "graph_plan did not mark the pair"
        assert g.tensors["stage1_unit1_sc_out"].producer.sc_pair is None, "a stride-1 shortcut is no pair"
        assert sc.w.fixed == frozen
        g.guard["enabled"] = False
        dy = torch.randn(u2.shape, generator=gen).to(dev)
        outs = []
        for _ in range(2):          # (the second pass reads the first one's state: magnitudes, piece planes of the gradients)
            g.forward()
            conv1.guard_fb = guard_on_conv1
            g.begin_backward()
            u2.give_grad(dy.clone())
            for idx in range(len(g.nodes) - 1, -1, -1):
                g.backward_node(idx)
            g.join_side_backward()
            g.flush_slabs()
            torch.cuda.synchronize()
            outs.append((g.grad_arena.clone(), x.grad.clone(), u2.data.clone(), g.tensors["stage2_unit1_bn1_relu"].grad.clone()))
        return outs, sum(used)
    finally:
        fn.set_conv_math(prev)


@pytest.mark.parametrize("variant", ["plain", "shortcut frozen", "guard fallback on conv1"])
@pytest.mark.parametrize("size,C", [(32, 64), (128, 128)], ids=["32x32", "128x128"])
def test_graph_step_is_bit_identical_with_the_knob_on_and_off(gpu_device, monkeypatch, size, C, variant):
    """B = 2.  32 x 32: the issue's toy -- its gradients are too small for the wide family, the route query keeps the present
    pair, the knob changes nothing.  128 x 128, 128 channels into the pair: the compact path RUNS (asserted) unless conv1 is on
    the range guard's fallback.  Every gradient of the arena, the input gradient, the output and act1's gradient: same bits."""
    kw = dict(frozen=variant == "shortcut frozen", guard_on_conv1=variant.startswith("guard"))
    with monkeypatch.context() as m:
        off, n_off = toy_step(size, C, False, m, **kw)
    with monkeypatch.context() as m:
        on, n_on = toy_step(size, C, True, m, **kw)
    assert n_off == 0
    assert n_on == (2 if (size == 128 and not kw["guard_on_conv1"]) else 0), "the compact path did not run where it should (or ran where it should not)"
    for step, (a, b) in enumerate(zip(off, on)):
        for t, u, name in zip(a, b, ("gradient arena", "input gradient", "output", "act1 gradient")):
            assert bool(torch.isfinite(t).all()), name
            same_bits(t, u, f"step {step}: {name}")
    assert float(on[1][0].abs().max()) > 0
