"""Training with fixed BatchNorm statistics at the graph level (the training builders' global_stats_pattern, engine.BatchNorm.backward's fixed_stats on every route, the solver): gradients against the float64
restatement with a fixed-statistics `bn`, forward consistency with the global-statistics test graph, the aux states through a
step, a captured step, recalibrate_bn_stats, bf16 tensors.

The restatement is oracle/dspnet_torch.py as it is: its `bn` is replaced under monkeypatch by one that normalises the nodes
in fixed mode with the moving statistics the device graph was given (Graph.set_aux) and ends in the oracle's own `_relu`.  A
call of `bn` carries no node name where there is no ReLU, so the node is identified by the `beta` tensor it is handed:
Params.__getitem__ is wrapped to record id(tensor) -> key, and "<bn>_beta" names the node -- for every call, the unnamed ones
(bn_data, the decoder's conv_bn, res5_reduced_bn, score3_conv_bn) included."""
import numpy as np
import pytest
import torch

from dspnet_amd import functional as fn
from dspnet_amd import synthetic
from dspnet_amd.symbol.multitask_symbol_builder import DECODER_GLOBAL_STATS_PATTERN, EVERY_BATCHNORM_PATTERN
from dspnet_amd.symbol.multitask_symbol_factory import get_config, get_multi_symbol, get_multi_symbol_train
from dspnet_amd.train.metric import MultiBoxMetric
from dspnet_amd.train.solver import MultiTaskSolver, recalibrate_bn_stats
from oracle import dspnet_torch as ot
from test_bn_moving_stats_gpu import _close, _dev, _watch_bn_inputs
from test_graph_gpu import assert_within_yardstick          # the yardstick and its constants: the float32 oracle's own deviation

pytestmark = pytest.mark.gpu

BATCH, SIZE = 2, 256          # where tests/test_graph_gpu.py runs its oracle-gradient tests of the resnet-50 graph


def drawn_aux(g, seed):
    """'<bn>_moving_mean' / '<bn>_moving_var' for every BatchNorm of graph g: per channel, mean ~ 0.5 N(0, 1), variance
    uniform in [0.5, 2]"""
    gen = np.random.default_rng(seed)
    aux = {}
    for name, channels, _ in g.bn_names:
        aux[name + "_moving_mean"] = (0.5 * gen.standard_normal(channels)).astype(np.float32)
        aux[name + "_moving_var"] = gen.uniform(0.5, 2.0, channels).astype(np.float32)
    return aux


def patch_oracle_bn(monkeypatch, aux, fixed_nodes):
    """oracle `bn` with fixed statistics for the nodes in fixed_nodes (module docstring) -> the list of nodes it normalised
    that way, in call order, over every forward_loss call made while the patch is on"""
    keys, orig_bn, orig_get, used = {}, ot.bn, ot.Params.__getitem__, []

    def getitem(self, k):
        t = orig_get(self, k)
        keys[id(t)] = k
        return t

    def bn(x, gamma, beta, relu=False, name=None):
        key = keys[id(beta)]
        assert key.endswith("_beta"), key
        node = key[:-len("_beta")]
        assert name is None or name == node, (name, node)
        if node not in fixed_nodes:
            return orig_bn(x, gamma, beta, relu=relu, name=name)
        used.append(node)
        mean = torch.tensor(aux[node + "_moving_mean"], dtype=x.dtype).view(1, -1, 1, 1)
        var = torch.tensor(aux[node + "_moving_var"], dtype=x.dtype).view(1, -1, 1, 1)
        y = (x - mean) / torch.sqrt(var + ot.EPS)
        if gamma is not None:
            y = y * gamma.view(1, -1, 1, 1)
        y = y + beta.view(1, -1, 1, 1)
        return ot._relu(y, name) if relu else y
    monkeypatch.setattr(ot.Params, "__getitem__", getitem)
    monkeypatch.setattr(ot, "bn", bn)
    return used


def batch_of(dev, batch, size, seed=233):
    gen = synthetic.rng(seed)
    data = synthetic.images(batch, size, size, gen)
    lab = synthetic.det_labels(batch, gen=gen, height=size, width=size)
    seg = synthetic.seg_labels(batch, size, size, gen=gen)
    return data, lab, seg


def fixed_net(dev, batch, size, aux_seed=7, solver_kw=None, data_seed=233, **builder_kw):
    net = get_multi_symbol_train("resnet-50", (3, size, size), num_classes=8, batch_size=batch, device=dev, seed=1, **builder_kw)
    aux = drawn_aux(net.g, aux_seed)
    net.g.set_aux(aux)
    data, lab, seg = batch_of(dev, batch, size, data_seed)
    solver = MultiTaskSolver(net, **(solver_kw or {}))
    solver.set_batch(_dev(data, dev), _dev(lab, dev), _dev(seg, dev))
    return net, solver, aux, (data, lab, seg)


def parity_report(net, data, lab, seg, cfg):
    """tests/test_graph_gpu.py bf16_parity_report without the operand rounding: the device against the (patched) oracle in
    float64, and the same oracle in float32 against its float64 self -> (dev, ref32), relative errors"""
    dev_targets = [net.target.loc_target.cpu().numpy(), net.target.loc_mask.cpu().numpy(), net.target.cls_target.cpu().numpy()]
    values = ot.export_params(net.g)
    kw = dict(num_classes=8, targets=dev_targets, config=cfg)
    r64 = ot.forward_loss(values, data, lab, seg, dtype=torch.float64, **kw)
    r32 = ot.forward_loss(values, data, lab, seg, dtype=torch.float32, **kw)
    r64["objective"].backward()
    r32["objective"].backward()

    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))

    outs = [o.cpu().numpy() for o in net.outputs()]
    m = MultiBoxMetric(); m.update(net)
    dev, c32 = {}, {}
    for key, dv in (("loc_preds", net.loc_preds.data.cpu().numpy()), ("cls_prob", outs[0]), ("seg_out", outs[4])):
        dev[key], c32[key] = rel(dv, r64[key].numpy()), rel(r32[key].numpy(), r64[key].numpy())
    for n, v in zip(*m.get()):
        if n in r64:
            dev["loss:" + n], c32["loss:" + n] = abs(v - r64[n]) / abs(r64[n]), abs(r32[n] - r64[n]) / abs(r64[n])
    nd = dd = n3 = hd = h3 = hh = 0.0
    bd = b3 = bb = 0.0
    for p in net.g.param_order:
        if p.name == "affine_matrix":          # identity grid: on the interpolation kinks (tests/test_graph_gpu.py)
            continue
        g64 = ot.import_grad(p.name, r64["params"][p.name].grad).astype(np.float64)
        g32 = ot.import_grad(p.name, r32["params"][p.name].grad).astype(np.float64)
        gdev = p.grad.cpu().numpy().astype(np.float64)
        gdev = gdev[:g64.shape[0], :, :, :g64.shape[3]] if gdev.ndim == 4 else gdev[:g64.shape[0]]
        assert np.isfinite(gdev).all(), p.name
        e_d, e_3, sq = float(((gdev - g64) ** 2).sum()), float(((g32 - g64) ** 2).sum()), float((g64 ** 2).sum())
        nd += e_d; n3 += e_3; dd += sq
        if p.name.endswith("pred_conv_weight"):
            hd += e_d; h3 += e_3; hh += sq
        if p.name.endswith(("_gamma", "_beta")):      # the BatchNorm parameters: dgamma / dbeta of the mode itself
            bd += e_d; b3 += e_3; bb += sq
    dev["grad_L2:all"], c32["grad_L2:all"] = (nd / dd) ** 0.5, (n3 / dd) ** 0.5
    dev["grad_L2:heads"], c32["grad_L2:heads"] = (hd / hh) ** 0.5, (h3 / hh) ** 0.5
    dev["grad_L2:batchnorm"], c32["grad_L2:batchnorm"] = (bd / bb) ** 0.5, (b3 / bb) ** 0.5
    return dev, c32


# ---------------------------------------------------------------- (a) gradients against the float64 restatement
@pytest.mark.parametrize("mode", ["every BatchNorm", "the decoder's BatchNorms"])
def test_gradients_match_the_fixed_statistics_restatement(gpu_device, monkeypatch, mode):
    kw = dict(global_stats_pattern=EVERY_BATCHNORM_PATTERN) if mode == "every BatchNorm" else dict(global_stats_pattern=DECODER_GLOBAL_STATS_PATTERN)
    net, solver, aux, (data, lab, seg) = fixed_net(gpu_device, BATCH, SIZE, **kw)
    fixed_nodes = {n for n, node in net.g.bn_nodes.items() if node.use_global_stats}
    assert len(fixed_nodes) == (len(net.g.bn_nodes) if mode == "every BatchNorm" else 9)
    # every BatchNorm backward call of the pass, by entry point and form, with the mode it was given
    calls = []
    for entry in ("bn_backward", "bn_backward_maxpool", "bn_backward_from_sums"):
        def spy(*a, _orig=getattr(fn, entry), _entry=entry, **k):
            form = _entry + (" planes" if k.get("dx_planes") else "") + (" parked" if k.get("park") else "")
            calls.append((form + " phase %d" % k.get("phase", 0), bool(k.get("fixed_stats", False))))
            return _orig(*a, **k)
        monkeypatch.setattr(fn, entry, spy)
    solver.forward()
    solver.backward()
    torch.cuda.synchronize()
    forms = {f: (sum(m for g, m in calls if g == f), sum(1 for g, _ in calls if g == f)) for f in sorted({f for f, _ in calls})}
    print("BatchNorm backward calls, form: (fixed, all)", forms)
    if mode == "every BatchNorm":      # no call site drops the mode, and the pass reaches all four of BatchNorm.backward
        assert calls and all(m for _, m in calls), forms
        sites = {f.split(" phase")[0].replace(" parked", "") for f in forms}
        want = {"bn_backward", "bn_backward_maxpool", "bn_backward_from_sums"}
        assert sites >= want | ({"bn_backward_from_sums planes"} if fn.get_conv_math() == "f16x2" else set()), forms
    else:
        assert any(m for _, m in calls) and not all(m for _, m in calls), forms
    used = patch_oracle_bn(monkeypatch, aux, fixed_nodes)
    dev, c32 = parity_report(net, data, lab, seg, get_config("resnet-50", SIZE))
    assert set(used) == fixed_nodes and len(used) == 2 * len(fixed_nodes), "the restatement did not fix the nodes the graph fixes"
    print(mode, "device vs float64:", dev, "| float32 restatement vs float64:", c32)
    assert_within_yardstick(dev, c32)


# ---------------------------------------------------------------- (b) forward consistency with the test graph
def test_forward_equals_the_global_statistics_test_graph(gpu_device):
    dev = gpu_device
    net, solver, aux, (data, _, _) = fixed_net(dev, 2, 128, global_stats_pattern=EVERY_BATCHNORM_PATTERN)
    solver.forward()
    net.det.join()
    test = get_multi_symbol("resnet-50", 128, num_classes=8, batch_size=2, device=dev, seed=1, use_global_stats=True)
    test.g.set_params(net.g.get_params())
    test.g.set_aux(aux)
    test.data.data.copy_(_dev(data, dev))
    test.g.forward()
    test.det.join()
    for got, want, what in ((net.outputs()[3], test.det.out.data, "det"), (net.outputs()[4], test.outputs()[1], "seg")):
        ok, err = _close(got, want)
        assert ok, (what, err)
    assert float(net.outputs()[4].abs().max()) > 0


# ---------------------------------------------------------------- (c) the aux states through a step
def test_a_step_leaves_fixed_nodes_alone_and_advances_the_others(gpu_device):
    net, solver, aux, _ = fixed_net(gpu_device, 2, 128, solver_kw=dict(track_bn_stats=True),
                                    global_stats_pattern=DECODER_GLOBAL_STATS_PATTERN)
    g = net.g
    fixed_nodes = {n for n, node in g.bn_nodes.items() if node.use_global_stats}
    free = ["bn_data", "bn0", "stage1_unit1_bn2", "stage4_unit3_bn3"]
    assert len(fixed_nodes) == 9 and not fixed_nodes & set(free)
    seen = _watch_bn_inputs(net, free)
    before = g.get_aux()
    for k, v in aux.items():
        assert np.array_equal(before[k], v), k
    w0 = g.arena.clone()
    solver.step()
    solver.step()
    torch.cuda.synchronize()
    after = g.get_aux()
    assert not torch.equal(g.arena, w0) and bool(torch.isfinite(g.arena).all())
    for name in g.bn_nodes:
        for sfx in ("_moving_mean", "_moving_var"):
            same = np.array_equal(before[name + sfx], after[name + sfx])
            assert same == (name in fixed_nodes), (name, sfx)
    for name in free:          # ... by the EMA of the batch statistics, as ever (test_bn_moving_stats_gpu.py's bars)
        assert len(seen[name]) == 2
        m, v = before[name + "_moving_mean"].astype(np.float64), before[name + "_moving_var"].astype(np.float64)
        for mean, var, n in seen[name]:
            m, v = 0.9 * m + (1 - 0.9) * mean, 0.9 * v + (1 - 0.9) * var * n / (n - 1)
        np.testing.assert_allclose(after[name + "_moving_mean"], m, rtol=1e-5, atol=1e-5 * max(np.abs(m).max(), 1e-3))
        np.testing.assert_allclose(after[name + "_moving_var"], v, rtol=1e-5, atol=1e-5 * max(np.abs(v).max(), 1e-3))


# ---------------------------------------------------------------- (d) a captured step
def test_captured_step_equals_the_eager_step_and_reads_the_statistics_at_replay(gpu_device):
    dev = gpu_device
    kw = dict(global_stats_pattern=DECODER_GLOBAL_STATS_PATTERN)
    eager, se, aux, _ = fixed_net(dev, 2, 128, **kw)
    for _ in range(3):
        se.step()
    cap, sc, _, _ = fixed_net(dev, 2, 128, **kw)
    assert sc.capture(warmup=1)
    for _ in range(2):
        sc.step()
    torch.cuda.synchronize()
    assert torch.equal(eager.g.arena, cap.g.arena) and torch.equal(eager.g.mom_arena, cap.g.mom_arena)
    for k, v in eager.g.get_aux().items():
        assert np.array_equal(v, cap.g.get_aux()[k]), k
    # other statistics: the next replay is the eager step from the same state -- the recording holds pointers, not values
    other = drawn_aux(cap.g, 99)
    other = {k: v for k, v in other.items() if cap.g.bn_nodes[k.rsplit("_moving_", 1)[0]].use_global_stats}
    for net in (eager, cap):
        net.g.set_aux(other, allow_missing=True)
    se.step()
    sc.step()
    torch.cuda.synchronize()
    assert sc._graph is not None, "the recording was dropped"
    assert torch.equal(eager.g.arena, cap.g.arena) and torch.equal(eager.g.mom_arena, cap.g.mom_arena)
    # ... and the statistics matter: with the earlier ones the same step ends elsewhere
    ctl, sx, _, _ = fixed_net(dev, 2, 128, **kw)
    for _ in range(4):
        sx.step()
    torch.cuda.synchronize()
    assert not torch.equal(ctl.g.arena, cap.g.arena)


# ---------------------------------------------------------------- (e) recalibrate_bn_stats
def test_recalibrate_bn_stats_averages_the_batch_statistics(gpu_device):
    dev = gpu_device
    net, solver, aux, _ = fixed_net(dev, 2, 128, global_stats_pattern=EVERY_BATCHNORM_PATTERN)
    g = net.g
    names = ["bn_data", "bn0", "stage1_unit1_bn2", "res3_reduced_bn", "score3_conv_bn"]
    seen = _watch_bn_inputs(net, names)
    w0, mom0, bn_mom0 = g.arena.clone(), g.mom_arena.clone(), g.bn_momentum
    node_state = {n: (node.momentum, node.use_global_stats) for n, node in g.bn_nodes.items()}
    batches = [tuple(_dev(t, dev) for t in batch_of(dev, 2, 128, seed)) for seed in (1, 2, 3)]
    assert recalibrate_bn_stats(net, batches) == 3
    torch.cuda.synchronize()
    assert torch.equal(g.arena, w0) and torch.equal(g.mom_arena, mom0) and g.bn_momentum == bn_mom0 and not g.bn_track
    assert {n: (node.momentum, node.use_global_stats) for n, node in g.bn_nodes.items()} == node_state
    got = g.get_aux()
    for name in names:
        assert len(seen[name]) == 3, (name, len(seen[name]))
        m = np.mean([mean for mean, _, _ in seen[name]], axis=0)
        v = np.mean([var * n / (n - 1) for _, var, n in seen[name]], axis=0)
        np.testing.assert_allclose(got[name + "_moving_mean"], m, rtol=1e-5, atol=1e-5 * max(np.abs(m).max(), 1e-3))
        np.testing.assert_allclose(got[name + "_moving_var"], v, rtol=1e-5, atol=1e-5 * max(np.abs(v).max(), 1e-3))
    # a list of bare data tensors does too, and the statistics are worth training with: one step, finite
    assert recalibrate_bn_stats(net, [b[0] for b in batches[:1]]) == 1
    solver.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g.arena).all()) and not torch.equal(g.arena, w0)
    with pytest.raises(ValueError):
        recalibrate_bn_stats(net, [])


# ---------------------------------------------------------------- (f) bf16 tensors
def test_bf16_tensor_step_with_fixed_statistics(gpu_device):
    """One fixed-statistics step of the bf16-storage graph at the size its batch-mode training test runs
    (tests/test_graph_gpu.py test_bf16_tensor_training_tracks_the_float_run: bf16 MFMA math, 2 x 256 x 256) is finite, and its
    loss readouts lie within that test's bounds of the float-storage run of the same graph and math: 8 % / 15 % / 3 % for
    CrossEntropy / SmoothL1 / SegCrossEntropy.  The statistics are the recalibrated ones of the batch itself."""
    def run(store):
        fn.set_conv_math("bf16")
        fn.set_activation_dtype(store)
        try:
            net, solver, _, (data, lab, seg) = fixed_net(gpu_device, 2, 256, global_stats_pattern=EVERY_BATCHNORM_PATTERN)
        finally:
            fn.set_activation_dtype("fp32")
        recalibrate_bn_stats(net, [_dev(data, gpu_device)])
        solver.step()
        m = MultiBoxMetric(); m.update(net)
        torch.cuda.synchronize()
        return net, dict(zip(*m.get()))
    try:
        net_h, loss_h = run("bf16")
        net_f, loss_f = run("fp32")
    finally:
        fn.set_conv_math(fn.DEFAULT_CONV_MATH)
    assert net_h.g.tensors["_plus15"].data.dtype == torch.bfloat16 and net_f.g.tensors["_plus15"].data.dtype == torch.float32
    assert all(n.use_global_stats for n in net_h.g.bn_nodes.values())
    assert bool(torch.isfinite(net_h.g.arena).all()) and bool(torch.isfinite(net_h.g.grad_arena).all())
    assert all(np.isfinite(v) for v in loss_h.values())
    dev = {k: abs(loss_h[k] / loss_f[k] - 1) for k in loss_f}
    print("bf16 tensors vs float tensors, fixed statistics:", dev, loss_h, loss_f)
    assert dev["CrossEntropy"] < 8e-2 and dev["SegCrossEntropy"] < 3e-2 and dev["SmoothL1"] < 0.15, (dev, loss_h, loss_f)
