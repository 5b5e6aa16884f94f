"""Frozen parameters and the Module optimizer rule on the GPU: the segmented SGD kernel against a float64 rule and against
dspn_sgd_momentum_f32's bits, and whole training steps of frozen graphs against the same graph without freezing."""
import numpy as np
import pytest
import torch

from dspnet_amd import functional as fn
from dspnet_amd import synthetic
from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
from dspnet_amd.train.solver import MultiTaskSolver, rule_multipliers

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the kernel
def _arena(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3)]


@pytest.mark.parametrize("nseg", [3, 700])
def test_segmented_sgd_matches_float64_and_leaves_gaps(gpu_device, nseg):
    dev = gpu_device
    rng = np.random.default_rng(nseg)
    rows, off = [], 0
    for i in range(nseg):
        off += 4 * int(rng.integers(0, 40))                  # a gap (possibly none) in front of every row
        length = 4 * int(rng.integers(1, 3000 if nseg < 10 else 60))
        rows.append((off, length, float(rng.choice([1.0, 2.0, 0.5])), float(rng.choice([1.0, 0.0]))))
        off += length
    n = off + 4 * 17
    w, grad, mom = _arena(n, nseg, dev)
    lr, mu, wd, rs = 0.01, 0.9, 0.0005, 1 / 8
    wd_, gd, md = w.float().to(dev), grad.float().to(dev), mom.float().to(dev)
    w0, m0 = wd_.clone(), md.clone()
    fn.sgd_momentum_segments(wd_, gd, md, fn.sgd_segment_table(rows, n, dev), lr, mu, wd, rs)
    torch.cuda.synchronize()
    wref, mref = w.clone(), mom.clone()
    inside = torch.zeros(n, dtype=torch.bool)
    for o, length, lm, wm in rows:
        s = slice(o, o + length)
        lre = float(np.float32(lr) * np.float32(lm))
        wde = float(np.float32(wd) * np.float32(wm))
        mref[s] = mu * mom[s] - lre * (rs * grad[s] + wde * w[s])
        wref[s] = w[s] + mref[s]
        inside[s] = True
    got_w, got_m = wd_.cpu(), md.cpu()
    assert torch.equal(got_w[~inside], w0.cpu()[~inside]) and torch.equal(got_m[~inside], m0.cpu()[~inside])
    np.testing.assert_allclose(got_m[inside].double().numpy(), mref[inside].numpy(), rtol=0,
                               atol=2e-6 * float(mref.abs().max()))
    np.testing.assert_allclose(got_w[inside].double().numpy(), wref[inside].numpy(), rtol=0,
                               atol=2e-6 * float(wref.abs().max()))


def test_segmented_sgd_multiplier_one_is_bit_identical(gpu_device):
    dev = gpu_device
    n = 1 << 20
    w, grad, mom = (t.float().to(dev) for t in _arena(n, 5, dev))
    rows = [(0, 4096, 1.0, 1.0), (4096 + 64, 300000, 1.0, 1.0), (600000, n - 600000, 1.0, 1.0)]
    a = [w.clone(), grad, mom.clone()]
    b = [w.clone(), grad, mom.clone()]
    fn.sgd_momentum(a[0], a[1], a[2], 0.0005, 0.9, 0.0005, 1 / 32)
    fn.sgd_momentum_segments(b[0], b[1], b[2], fn.sgd_segment_table(rows, n, dev), 0.0005, 0.9, 0.0005, 1 / 32)
    torch.cuda.synchronize()
    for o, length, _, _ in rows:
        assert torch.equal(a[0][o:o + length], b[0][o:o + length])
        assert torch.equal(a[2][o:o + length], b[2][o:o + length])
    for lo, hi in ((4096, 4096 + 64), (304160, 600000)):
        assert torch.equal(b[0][lo:hi], w[lo:hi]) and torch.equal(b[2][lo:hi], mom[lo:hi])


# ---------------------------------------------------------------- graph steps
def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _net(dev, network="resnet-50", size=128, batch=2, seed=233, solver_kw=None, **build_kw):
    net = get_multi_symbol_train(network, (3, size, size), num_classes=8, batch_size=batch, device=dev, seed=1, **build_kw)
    gen = synthetic.rng(seed)
    data = _dev(synthetic.images(batch, size, size, gen), dev)
    lab = _dev(synthetic.det_labels(batch, gen=gen, height=size, width=size, first_empty=False), dev)
    seg = _dev(synthetic.seg_labels(batch, size, size, gen=gen), dev)
    solver = MultiTaskSolver(net, **(solver_kw or {}))
    solver.set_batch(data, lab, seg)
    return net, solver


def _forward_backward(solver):
    def body():
        solver._calibrate_guard()
        solver._train_forward()
        solver.backward()
    solver._on_step_stream(body)
    torch.cuda.synchronize()


def _update(solver):
    solver._on_step_stream(solver.update)
    torch.cuda.synchronize()


CONFIGS = [("resnet-50", 128, r"^(bn_data|conv0|bn0|stage1_)"),      # frozen prefix: backward stops at stage 2
           ("resnet-50", 128, r"^stage3_"),                          # frozen middle: data gradient without weight gradient
           ("vgg16_reduced", 300, r"^(conv1_|conv2_).*")]           # the reference's default --freeze


@pytest.mark.parametrize("network,size,pattern", CONFIGS)
def test_frozen_step_matches_the_unfrozen_graph(gpu_device, network, size, pattern):
    dev = gpu_device
    base, sb = _net(dev, network, size)
    frz, sf = _net(dev, network, size, freeze_pattern=pattern)
    fixed = set(frz.fixed_param_names)
    assert fixed and torch.equal(base.g.arena, frz.g.arena)
    _forward_backward(sb)
    _forward_backward(sf)
    for x, y in zip(base.outputs(), frz.outputs()):      # the forward pass (losses, detections, segmentation) is untouched
        assert torch.equal(x, y)
    for p in frz.g.param_order:
        if not p.fixed:                                   # every trainable gradient, bit for bit
            assert torch.equal(p.grad, base.g.params[p.name].grad), p.name
    w0, m0 = frz.g.arena.clone(), frz.g.mom_arena.clone()
    _update(sb)
    _update(sf)
    for p in frz.g.param_order:
        s = slice(p.offset, p.offset + p.size)
        if p.fixed:
            assert torch.equal(frz.g.arena[s], w0[s]) and torch.equal(frz.g.mom_arena[s], m0[s]), p.name
        else:
            assert torch.equal(frz.g.arena[s], base.g.arena[s]), p.name
            assert torch.equal(frz.g.mom_arena[s], base.g.mom_arena[s]), p.name
    assert any(not torch.equal(base.g.arena[p.offset:p.offset + p.size], w0[p.offset:p.offset + p.size])
               for p in frz.g.param_order if p.fixed)     # (without freezing those parameters do move)


def test_captured_frozen_step_equals_the_eager_step(gpu_device):
    dev = gpu_device
    pattern = r"^(bn_data|conv0|bn0|stage1_)"
    eager, se = _net(dev, freeze_pattern=pattern)
    for _ in range(3):
        se.step()
    cap, sc = _net(dev, freeze_pattern=pattern)
    assert sc.capture(warmup=1)
    for _ in range(2):
        sc.step()
    torch.cuda.synchronize()
    assert torch.equal(eager.g.arena, cap.g.arena) and torch.equal(eager.g.mom_arena, cap.g.mom_arena)
    fresh, _ = _net(dev, freeze_pattern=pattern)
    for p in cap.g.param_order:
        if p.fixed:
            assert torch.equal(p.data, fresh.g.params[p.name].data), p.name


def test_module_rules_step_matches_a_float64_update(gpu_device):
    dev = gpu_device
    lr, mu, wd = 0.01, 0.9, 0.0005
    net, solver = _net(dev, freeze_pattern="^conv0", solver_kw=dict(optimizer_rules="module", learning_rate=lr,
                                                                   momentum=mu, wd=wd))
    g = net.g
    g.mom_arena.copy_(torch.randn(g.mom_arena.shape, generator=torch.Generator().manual_seed(3)).to(dev) * 1e-3)
    _forward_backward(solver)
    w0, m0, gr = (t.double().cpu() for t in (g.arena, g.mom_arena, g.grad_arena))
    _update(solver)
    w1, m1 = g.arena.double().cpu(), g.mom_arena.double().cpu()
    rs = 1.0 / solver.world_size
    assert solver.rescale() == rs
    heads = 0
    for p in g.param_order:
        s = slice(p.offset, p.offset + p.size)
        if p.fixed:
            assert torch.equal(w1[s], w0[s]) and torch.equal(m1[s], m0[s]), p.name
            continue
        lm, wm = rule_multipliers(p.name, "module", p.lr_mult, p.wd_mult)
        heads += lm == 2.0
        lre, wde = float(np.float32(lr) * np.float32(lm)), float(np.float32(wd) * np.float32(wm))
        m = mu * m0[s] - lre * (rs * gr[s] + wde * w0[s])
        scale = max(float(m.abs().max()), 1e-12)
        assert float((m1[s] - m).abs().max()) <= 2e-6 * scale, p.name
        assert float((w1[s] - (w0[s] + m)).abs().max()) <= 2e-6 * max(float(w0[s].abs().max()), scale), p.name
    assert heads == 12


# ---------------------------------------------------------------- parameter-only BatchNorm backward
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_backward_parameters_only_is_bit_identical(gpu_device, dtype, relu):
    dev = gpu_device
    g = torch.Generator().manual_seed(21)
    rows, C = 3000, 96
    x = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(dev).to(dtype)
    dy = torch.randn(rows, C, generator=g).to(dev).to(dtype)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = torch.randn(C, generator=g).to(dev)
    mean, rstd, scale, shift = fn.bn_stats(x, 2e-5, gamma, beta)
    _, dg_full, db_full = fn.bn_backward(x, scale, shift, dy, mean, rstd, gamma, relu=relu)
    dx, dg, db = fn.bn_backward(x, scale, shift, dy, mean, rstd, gamma, relu=relu, dx=fn.NO_OUTPUT)
    _, dg2, db2 = fn.bn_backward(x, scale, shift, dy, mean, rstd, gamma, relu=relu, dx=fn.NO_OUTPUT, dbeta=fn.NO_OUTPUT)
    torch.cuda.synchronize()
    assert dx is None and db2 is None
    assert torch.equal(dg, dg_full) and torch.equal(db, db_full) and torch.equal(dg2, dg_full)


def test_bn_backward_maxpool_parameters_only_is_bit_identical(gpu_device):
    dev = gpu_device
    g = torch.Generator().manual_seed(22)
    N, H, W, C, k, s, p = 2, 16, 16, 64, 3, 2, 1
    x = (torch.randn(N, H, W, C, generator=g) + 0.3).to(dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = torch.randn(C, generator=g).to(dev)
    mean, rstd, scale, shift = fn.bn_stats(x, 2e-5, gamma, beta)
    Ho = Wo = (H + 2 * p - k) // s + 1
    pooled = torch.zeros(N, Ho, Wo, C, device=dev)
    argmax = torch.zeros(N, Ho, Wo, C, dtype=torch.uint8, device=dev)
    fn.maxpool_forward(x, k, s, p, out=pooled, argmax=argmax, in_affine=(scale, shift, True))
    dyp = torch.randn(N, Ho, Wo, C, generator=g).to(dev)
    _, dg_full, db_full = fn.bn_backward_maxpool(x, scale, shift, dyp, argmax, k, s, p, mean, rstd, gamma, relu=True)
    dx, dg, db = fn.bn_backward_maxpool(x, scale, shift, dyp, argmax, k, s, p, mean, rstd, gamma, relu=True, dx=fn.NO_OUTPUT)
    torch.cuda.synchronize()
    assert dx is None and torch.equal(dg, dg_full) and torch.equal(db, db_full)


def test_bn_backward_from_sums_parameters_only_is_bit_identical(gpu_device):
    """the graph's own from-sums BatchNorms: a frozen-prefix step's trainable gradients already equal the unfrozen graph's
    (test_frozen_step_matches_the_unfrozen_graph); here the call itself, with the sums a data gradient gathered"""
    dev = gpu_device
    net, solver = _net(dev, freeze_pattern=r"^(bn_data|conv0|bn0|stage1_)")
    bn = net.g.bn_nodes["stage2_unit1_bn1"]
    assert not bn.x.requires_grad and bn.out.requires_grad
    calls = []
    orig = fn.bn_backward_from_sums

    def spy(*a, **k):
        if a[0] is bn.x.data:
            calls.append(k.get("dx"))
        return orig(*a, **k)
    fn.bn_backward_from_sums = spy
    try:
        _forward_backward(solver)
    finally:
        fn.bn_backward_from_sums = orig
    if bn.bwd_sums is not None:      # (one call per backward pass: the range guard's calibration pass and the step's)
        assert calls and all(c is fn.NO_OUTPUT for c in calls)


def test_frozen_operands_follow_set_params(gpu_device):
    """derived operands of frozen weights are formed once; set_params on a frozen weight forms them again"""
    dev = gpu_device
    pattern = r"^(stage3_|conv0)"
    base, sb = _net(dev)
    frz, sf = _net(dev, freeze_pattern=pattern)
    for s in (sb, sf):
        s.step()
    torch.cuda.synchronize()
    rng = np.random.default_rng(4)
    new = {k: (v * rng.uniform(0.5, 1.5, v.shape)).astype(np.float32) for k, v in frz.g.get_params().items()
           if frz.g.params[k].fixed}
    base.g.arena.copy_(frz.g.arena)
    base.g.set_params(new, allow_missing=True)
    frz.g.set_params(new, allow_missing=True)
    assert frz.g.frozen_stale
    _forward_backward(sb)
    _forward_backward(sf)
    for x, y in zip(base.outputs(), frz.outputs()):
        assert torch.equal(x, y)
    for p in frz.g.param_order:
        if not p.fixed:
            assert torch.equal(p.grad, base.g.params[p.name].grad), p.name
