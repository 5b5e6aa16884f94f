"""BatchNorm moving statistics and global-statistics inference on the GPU: the `_ex` finalize kernels, the solver's
tracking, captured steps, global-mode test graphs, batch independence and the checkpoint round trip."""
import numpy as np
import pytest
import torch

from dspnet_amd import functional as fn
from dspnet_amd import synthetic
from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol, get_multi_symbol_train
from dspnet_amd.train.solver import MultiTaskSolver, do_checkpoint

pytestmark = pytest.mark.gpu
EPS = 2e-5


def _dev(t, dev):
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def _ema(m0, v0, steps, mom):
    """float64 EMA of the batch statistics [(mean, biased var, n)] (cuDNN's unbiased running variance)"""
    m, v = m0.astype(np.float64), v0.astype(np.float64)
    for mean, var, n in steps:
        uv = var * n / (n - 1) if n > 1 else var
        m = mom * m + (1 - mom) * mean
        v = mom * v + (1 - mom) * uv
    return m, v


def _moving(dev, C, gen):
    mm = (gen.standard_normal(C) * 0.5).astype(np.float32)
    mv = (gen.uniform(0.5, 2.0, C)).astype(np.float32)
    return _dev(mm, dev), _dev(mv, dev), mm, mv


# ---------------------------------------------------------------- 1 / 2: the finalize kernels
@pytest.mark.parametrize("C,logical,rows", [(4, 3, 1), (4, 3, 777), (48, 48, 1), (64, 64, 5000), (2048, 2048, 300)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_finalize_track_and_global(gpu_device, C, logical, rows, dtype):
    dev = gpu_device
    gen = np.random.default_rng(C * 7 + rows)
    xh = (gen.standard_normal((rows, C)) * gen.uniform(0.5, 3.0, C) + gen.uniform(-2, 2, C)).astype(np.float32)
    xh[:, logical:] = 0
    x = _dev(xh, dev).to(dtype)
    gamma = _dev(gen.uniform(0.5, 1.5, C).astype(np.float32), dev)
    beta = _dev(gen.standard_normal(C).astype(np.float32), dev)
    ref = fn.bn_stats(x, EPS, gamma, beta)
    mmd, mvd, mm, mv = _moving(dev, C, gen)
    got = fn.bn_stats(x, EPS, gamma, beta, moving=fn.bn_moving(mmd, mvd, 0.9, fn.BN_TRACK, logical))
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)                     # the batch outputs, bit for bit
    x64 = x.float().cpu().numpy().astype(np.float64)
    em, ev = _ema(mm[:logical], mv[:logical], [(x64[:, :logical].mean(0), x64[:, :logical].var(0), rows)], np.float64(np.float32(0.9)))
    np.testing.assert_allclose(mmd.cpu().numpy()[:logical], em, rtol=1e-6, atol=1e-6 * np.abs(em).max())
    np.testing.assert_allclose(mvd.cpu().numpy()[:logical], ev, rtol=1e-6, atol=1e-7)
    assert torch.equal(mmd[logical:].cpu(), torch.from_numpy(mm[logical:]))    # pad lanes untouched
    assert torch.equal(mvd[logical:].cpu(), torch.from_numpy(mv[logical:]))
    # global mode: the coefficients from the moving statistics
    mean, rstd, scale, shift = fn.bn_stats(x, EPS, gamma, beta, moving=fn.bn_moving(mmd, mvd, 0.9, fn.BN_GLOBAL, logical))
    m64, v64 = mmd.cpu().numpy().astype(np.float64), mvd.cpu().numpy().astype(np.float64)
    rs = (1.0 / np.sqrt(v64 + np.float32(EPS))).astype(np.float32)
    assert np.array_equal(mean.cpu().numpy(), mmd.cpu().numpy())
    np.testing.assert_allclose(rstd.cpu().numpy(), rs, rtol=2.5e-7, atol=0)
    sc = gamma.cpu().numpy().astype(np.float64) * rs
    np.testing.assert_allclose(scale.cpu().numpy(), sc, rtol=2.5e-7, atol=0)
    b64, s64 = beta.cpu().numpy().astype(np.float64), scale.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(shift.cpu().numpy(), b64 - m64 * s64, rtol=0, atol=2.5e-7 * (np.abs(b64) + np.abs(m64 * s64)).max())


def _tile_tables(gen, tiles, tile_rows, rows, C):
    ns = np.full(tiles, tile_rows, np.float64)
    ns[-1] = rows - (tiles - 1) * tile_rows
    off = gen.uniform(-1, 1, C)
    mt = (off + gen.standard_normal((tiles, C)) * 0.3).astype(np.float32)
    q = (ns[:, None] * gen.uniform(0.2, 2.0, (tiles, C))).astype(np.float32)
    ts = np.stack([mt, q], 1)                                   # [tiles][2][C]: (mean, M2)
    lo = (mt - gen.uniform(1, 3, (tiles, C))).astype(np.float32)
    hi = (mt + gen.uniform(1, 3, (tiles, C))).astype(np.float32)
    mmx = np.stack([lo, hi], 1)
    A = (ns[:, None] * mt.astype(np.float64)).sum(0)
    B = (q.astype(np.float64) + ns[:, None] * mt.astype(np.float64) ** 2).sum(0)
    mean = A / rows
    var = np.maximum(B / rows - mean * mean, 0)
    return ts, mmx, mean, var


@pytest.mark.parametrize("C,logical,tiles,tile_rows", [(3, 3, 1, 1), (48, 48, 5, 128), (64, 60, 1500, 64), (2048, 2048, 40, 256),
                                                       (64, 64, 1100, 1)])
@pytest.mark.parametrize("relu", [False, True])
def test_tiles_finalize_track_and_global(gpu_device, C, logical, tiles, tile_rows, relu):
    dev = gpu_device
    gen = np.random.default_rng(C + tiles)
    rows = (tiles - 1) * tile_rows + max(1, tile_rows // 2)
    ts, mmx, mean64, var64 = _tile_tables(gen, tiles, tile_rows, rows, C)
    ts_d, mm_d = _dev(ts, dev), _dev(mmx, dev)
    gamma = _dev(gen.uniform(0.5, 1.5, C).astype(np.float32), dev)
    beta = _dev(gen.standard_normal(C).astype(np.float32), dev)

    def run(moving):
        outs = [torch.zeros(C, device=dev) for _ in range(4)]
        am = torch.zeros(fn.ABSMAX_SLOTS, device=dev)
        amin = torch.full((1,), float("inf"), device=dev)
        ext = torch.zeros(2 * C, device=dev)
        fn.bn_stats_from_tiles(ts_d, tiles, tile_rows, rows, C, EPS, gamma, beta, *outs, tile_minmax=mm_d, relu=relu,
                               out_absmax=am, out_absmin=amin, out_chan_minmax=ext, moving=moving)
        return outs + [am, amin, ext]

    ref = run(None)
    mmd, mvd, mm, mv = _moving(dev, C, gen)
    got = run(fn.bn_moving(mmd, mvd, 0.9, fn.BN_TRACK, logical))
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    em, ev = _ema(mm[:logical], mv[:logical], [(mean64[:logical], var64[:logical], rows)], np.float64(np.float32(0.9)))
    np.testing.assert_allclose(mmd.cpu().numpy()[:logical], em, rtol=1e-6, atol=1e-6 * np.abs(em).max())
    np.testing.assert_allclose(mvd.cpu().numpy()[:logical], ev, rtol=1e-6, atol=1e-7)
    assert np.array_equal(mmd.cpu().numpy()[logical:], mm[logical:]) and np.array_equal(mvd.cpu().numpy()[logical:], mv[logical:])
    # global mode: coefficients from the moving statistics, magnitudes under the global affine from the (min, max) table
    mean, rstd, scale, shift, am, amin, ext = [t.cpu().numpy() for t in run(fn.bn_moving(mmd, mvd, 0.9, fn.BN_GLOBAL, logical))]
    m64, v64 = mmd.cpu().numpy().astype(np.float64), mvd.cpu().numpy().astype(np.float64)
    rs = (1.0 / np.sqrt(v64 + np.float32(EPS))).astype(np.float32)
    assert np.array_equal(mean, mmd.cpu().numpy())
    np.testing.assert_allclose(rstd, rs, rtol=2.5e-7, atol=0)
    np.testing.assert_allclose(scale, gamma.cpu().numpy().astype(np.float64) * rs, rtol=2.5e-7, atol=0)
    b64 = beta.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(shift, b64 - m64 * scale, rtol=0, atol=2.5e-7 * (np.abs(b64) + np.abs(m64 * scale)).max())
    lo, hi = mmx[:, 0].min(0), mmx[:, 1].max(0)
    assert np.array_equal(ext, np.concatenate([lo, hi]))
    a = lo.astype(np.float64) * scale + shift                  # (the kernel's fmaf: one rounding of the exact value)
    b = hi.astype(np.float64) * scale + shift
    if relu:
        a, b = np.maximum(a, 0), np.maximum(b, 0)
    v = np.maximum(np.abs(a), np.abs(b)).astype(np.float32)
    want = np.zeros(fn.ABSMAX_SLOTS, np.float32)
    for c in range(C):
        want[c & 63] = max(want[c & 63], v[c])
    np.testing.assert_allclose(am, want, rtol=1.2e-7, atol=0)
    np.testing.assert_allclose(amin[0], v[v > 0].min(), rtol=1.2e-7)


# ---------------------------------------------------------------- 3 - 5: training
def _train_net(dev, network="resnet-50", batch=2, size=128, seed=233, **solver_kw):
    net = get_multi_symbol_train(network, (3, size, size), num_classes=8, batch_size=batch, device=dev, seed=1)
    gen = synthetic.rng(seed)
    data = _dev(synthetic.images(batch, size, size, gen), dev)
    lab = _dev(synthetic.det_labels(batch, gen=gen, height=size, width=size, first_empty=False), dev)
    seg = _dev(synthetic.seg_labels(batch, size, size, gen=gen), dev)
    solver = MultiTaskSolver(net, **solver_kw)
    solver.set_batch(data, lab, seg)
    return net, solver


def _watch_bn_inputs(net, names):
    """record, in every TRACKED forward, the float64 (mean, biased var, n) of each named BatchNorm's input"""
    g, seen = net.g, {k: [] for k in names}
    for name in names:
        node = g.bn_nodes[name]

        def fwd(node=node, orig=node.forward, name=name):
            if g.bn_track:
                x = node.x.data.float().reshape(-1, node.x.shape[-1])[:, :node.channels].double()
                seen[name].append((x.mean(0).cpu().numpy(), x.var(0, unbiased=False).cpu().numpy(), x.shape[0]))
            orig()
        node.forward = fwd
    return seen


def test_tracking_leaves_training_bit_identical_and_tracks_the_ema(gpu_device):
    dev = gpu_device
    names = ["bn_data", "bn0", "stage1_unit1_bn2", "res3_reduced_bn"]
    runs = {}
    for track in (True, False):
        net, solver = _train_net(dev, track_bn_stats=track)
        for n in names:
            assert n in net.g.bn_nodes, n
        assert not net.g.bn_nodes["res3_reduced_bn"].gamma         # a fix_gamma decoder BatchNorm
        seen = _watch_bn_inputs(net, names) if track else None
        for _ in range(3):
            solver.step()
        torch.cuda.synchronize()
        runs[track] = (net, seen)
    (a, seen), (b, _) = runs[True], runs[False]
    assert torch.equal(a.g.arena, b.g.arena) and torch.equal(a.g.mom_arena, b.g.mom_arena)
    for x, y in zip(a.outputs(), b.outputs()):
        assert torch.equal(x, y)
    aux_a, aux_b = a.g.get_aux(), b.g.get_aux()
    for name, channels, _ in b.g.bn_names:                     # untracked: 0 / 1 as built
        assert not aux_b[name + "_moving_mean"].any() and (aux_b[name + "_moving_var"] == 1).all()
    for name in names:
        assert len(seen[name]) == 3, (name, len(seen[name]))   # one advance per update (the guard's pass is not one)
        em, ev = _ema(np.zeros(a.g.bn_nodes[name].channels), np.ones(a.g.bn_nodes[name].channels), seen[name], 0.9)
        np.testing.assert_allclose(aux_a[name + "_moving_mean"], em, rtol=1e-5, atol=1e-5 * max(np.abs(em).max(), 1e-3))
        np.testing.assert_allclose(aux_a[name + "_moving_var"], ev, rtol=1e-5, atol=1e-5 * max(np.abs(ev).max(), 1e-3))


def test_inceptionv3_batchnorm_tracks_the_ema(gpu_device):
    net, solver = _train_net(gpu_device, network="inceptionv3", batch=1, size=512)
    name = net.g.bn_names[10][0]
    seen = _watch_bn_inputs(net, [name])
    for _ in range(3):
        solver.step()
    aux = net.g.get_aux()
    ch = net.g.bn_nodes[name].channels
    assert len(seen[name]) == 3
    em, ev = _ema(np.zeros(ch), np.ones(ch), seen[name], 0.9)
    np.testing.assert_allclose(aux[name + "_moving_mean"], em, rtol=1e-5, atol=1e-5 * max(np.abs(em).max(), 1e-3))
    np.testing.assert_allclose(aux[name + "_moving_var"], ev, rtol=1e-5, atol=1e-5 * max(np.abs(ev).max(), 1e-3))


def test_captured_steps_track_like_eager_steps(gpu_device):
    dev = gpu_device
    eager, se = _train_net(dev)
    for _ in range(3):
        se.step()
    cap, sc = _train_net(dev)
    assert sc.capture(warmup=1)                    # one eager update, then the recording (which runs nothing)
    for _ in range(2):
        sc.step()                                  # two replays
    torch.cuda.synchronize()
    assert torch.equal(eager.g.arena, cap.g.arena)
    ae, ac = eager.g.get_aux(), cap.g.get_aux()
    for k in ae:
        assert np.array_equal(ae[k], ac[k]), k
    # a bare forward and the solver's own forward leave the statistics alone
    cap.g.forward()
    sc.forward()
    torch.cuda.synchronize()
    for k, v in cap.g.get_aux().items():
        assert np.array_equal(v, ac[k]), k


# ---------------------------------------------------------------- 6 / 7: global-statistics inference
def _test_outputs(net):
    net.det.join()
    return [net.seg_out.prob.data.clone(), net.cls_out.cls_prob.data.clone(), net.loc_preds.data.clone()]


def _close(a, b, tol=1e-5):
    scale = max(float(b.abs().max()), 1e-6)
    return float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max()) / scale


def _batch_stats_aux(net):
    """each BatchNorm's moving statistics := the statistics of the batch in net.data (one tracked forward, momentum 0,
    the stored unbiased variance rescaled by (n - 1) / n)"""
    g = net.g
    for n in g.bn_nodes.values():
        n.momentum = 0.0
    g.bn_track = True
    g.forward()
    g.bn_track = False
    outs = _test_outputs(net)
    aux = g.get_aux()
    for name, _, _ in g.bn_names:
        rows = int(np.prod(g.bn_nodes[name].x.shape[:-1]))
        if rows > 1:
            aux[name + "_moving_var"] = (aux[name + "_moving_var"].astype(np.float64) * (rows - 1) / rows).astype(np.float32)
    return outs, aux


@pytest.mark.parametrize("network,batch,size,tol", [("resnet-50", 2, 128, 1e-3), ("vgg16_reduced", 1, 512, 1e-3),
                                                    ("inceptionv3", 1, 512, 2e-2)])
def test_global_inference_on_its_own_statistics_equals_batch_inference(gpu_device, network, batch, size, tol):
    """Every BatchNorm's folded affine in global mode equals the batch's to float rounding (1e-6).  The end-to-end outputs
    are compared more loosely: these untrained nets amplify the last-bit differences of rstd (the stored variance is
    rounded twice) through every later layer -- measured 7e-5 (resnet-50) and 4e-3 (inceptionv3, 94 BatchNorms) of the
    output scale."""
    dev = gpu_device
    prev = fn.get_conv_math()
    fn.set_conv_math("fp32")
    try:
        gen = synthetic.rng(5)
        data = _dev(synthetic.images(batch, size, size, gen), dev)
        bnet = get_multi_symbol(network, size, num_classes=8, batch_size=batch, device=dev, seed=1)
        bnet.data.data.copy_(data)
        ref, aux = _batch_stats_aux(bnet)
        gnet = get_multi_symbol(network, size, num_classes=8, batch_size=batch, device=dev, seed=1, use_global_stats=True)
        gnet.g.set_params(bnet.g.get_params())
        gnet.g.set_aux(aux)
        gnet.data.data.copy_(data)
        gnet.g.forward()
        outs = _test_outputs(gnet)
        for name, ch, _ in bnet.g.bn_names:          # (pad lanes: 0 / 1 against the batch's 0 / 0, on zero inputs)
            a, b = gnet.g.bn_nodes[name], bnet.g.bn_nodes[name]
            for got, want in ((a.scale[:ch], b.scale[:ch]), (a.shift[:ch], b.shift[:ch])):
                ok, err = _close(got, want, 1e-6)
                assert ok, (name, err)
        for got, want in zip(outs, ref):
            ok, err = _close(got, want, tol)
            assert ok, err
    finally:
        fn.set_conv_math(prev)


def test_global_inference_is_independent_of_the_batch(gpu_device):
    dev = gpu_device
    prev = fn.get_conv_math()
    fn.set_conv_math("fp32")
    try:
        size, B = 128, 4
        gen = synthetic.rng(11)
        data = _dev(synthetic.images(B, size, size, gen), dev)
        stats_net = get_multi_symbol("resnet-50", size, num_classes=8, batch_size=B, device=dev, seed=1)
        stats_net.data.data.copy_(_dev(synthetic.images(B, size, size, synthetic.rng(12)), dev))   # another batch's statistics
        _, aux = _batch_stats_aux(stats_net)
        params = stats_net.g.get_params()
        res = {}
        for glob in (True, False):
            four = get_multi_symbol("resnet-50", size, num_classes=8, batch_size=B, device=dev, seed=1, use_global_stats=glob)
            one = get_multi_symbol("resnet-50", size, num_classes=8, batch_size=1, device=dev, seed=1, use_global_stats=glob)
            for net in (four, one):
                net.g.set_params(params)
                net.g.set_aux(aux)
            four.data.data.copy_(data)
            four.g.forward()
            together = _test_outputs(four)
            alone = []
            for b in range(B):
                one.data.data.copy_(data[b:b + 1])
                one.g.forward()
                alone.append(_test_outputs(one))
            res[glob] = [_close(torch.cat([a[k] for a in alone]), together[k]) for k in range(3)]
        for ok, err in res[True]:
            assert ok, err
        # batch statistics: the same comparison shows a clear difference (the test can tell)
        assert max(err for _, err in res[False]) > 100 * 1e-5, res[False]
    finally:
        fn.set_conv_math(prev)


# ---------------------------------------------------------------- 8: checkpoint round trip
def test_checkpoint_round_trip_into_a_global_stats_detector(gpu_device, tmp_path):
    from dspnet_amd.detect.multitask_detector import Detector
    dev = gpu_device
    net, solver = _train_net(dev)
    for _ in range(2):
        solver.step()
    torch.cuda.synchronize()
    aux = net.g.get_aux()
    assert any(v.any() for k, v in aux.items() if k.endswith("_moving_mean"))
    prefix = str(tmp_path / "dspnet")
    do_checkpoint(prefix)(0, net)
    det = Detector("resnet-50", data_shape=128, num_classes=8, batch_size=2, device=dev, seed=7, model_prefix=prefix, epoch=1,
                   use_global_stats=True)
    got = det.net.g.get_aux()
    for k in aux:
        assert np.array_equal(got[k], aux[k]), k
    mem = get_multi_symbol("resnet-50", 128, num_classes=8, batch_size=2, device=dev, seed=7, use_global_stats=True)
    mem.g.set_params(net.g.get_params())
    mem.g.set_aux(aux)
    data = _dev(synthetic.images(2, 128, 128, synthetic.rng(3)), dev)
    det_out, seg = det.forward(data)
    mem.data.data.copy_(data)
    if mem.g.scalars is not None and mem.g.guard["enabled"]:   # (what Detector.forward does on a fresh net)
        mem.g.forward()
        mem.g.guard["decide_now"] = True
    mem.g.forward()
    mem.det.join()
    assert torch.equal(det_out, mem.det.out.data) and torch.equal(seg, mem.seg_out.prob.data)
