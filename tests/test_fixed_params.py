"""Frozen parameters (fixed_param_names / freeze_pattern) and the Module optimizer rule, without a GPU: name selection and
validation on graphs built on the CPU, the gradient-flow rule, per-name multipliers, the segment table of the segmented SGD,
frozen-aware bucket plans on the real resnet-50 layout, a world-2 gloo reduction that leaves frozen ranges alone, and the
argument checks of dspn_sgd_momentum_segments_f32."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from dspnet_amd import operator as op
from dspnet_amd.symbol import multitask_symbol_factory as F
from dspnet_amd.train.solver import (GradBucketReducer, plan_buckets, rule_multipliers, sgd_segments, side_buckets)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bucket_layout_resnet50_512.json")
REFERENCE_FREEZE = r"^(conv1_|conv2_).*"       # multi_train.py's --freeze default


@pytest.fixture()
def stub_prior(monkeypatch):
    def fake_prior(data, sizes, ratios, **kw):
        H, W = data if isinstance(data, tuple) else data.shape[-2:]
        return torch.zeros(1, H * W * (len(sizes) + len(ratios) - 1), 4)
    monkeypatch.setattr(op, "MultiBoxPrior", fake_prior)


def build(network, size=None, builder=F.get_multi_symbol_train, **kw):
    size = size or (300 if network == "vgg16_reduced" else 128)      # (vgg16_reduced's extra layers need 300 x 300)
    return builder(network, size, num_classes=8, batch_size=1, device=torch.device("cpu"), **kw)


def golden():
    doc = json.load(open(GOLDEN))
    params = [(n, o, s) for n, o, s, _ in doc["params"]]
    owner = {n: i for n, _, _, i in doc["params"]}
    return params, owner, doc["arena"], doc


# ---------------------------------------------------------------- name selection
def test_reference_default_freezes_the_vgg16_reduced_stem(stub_prior):
    net = build("vgg16_reduced", freeze_pattern=REFERENCE_FREEZE)
    want = sorted("conv%d_%d_%s" % (a, b, k) for a in (1, 2) for b in (1, 2) for k in ("weight", "bias"))
    assert net.fixed_param_names == want
    g = net.g
    assert all(g.params[n].fixed for n in want)
    assert sum(p.fixed for p in g.param_order) == 8


def test_finetune_prefix_on_resnet50_is_conv0(stub_prior):
    net = build("resnet-50", freeze_pattern="^conv")       # train_multitask.py --finetune freezes names starting with conv
    assert net.fixed_param_names == ["conv0_weight"]


def test_names_and_pattern_are_unioned(stub_prior):
    net = build("resnet-50", freeze_pattern="^bn0_", fixed_param_names=["conv0_weight", "affine_matrix"])
    assert net.fixed_param_names == ["affine_matrix", "bn0_beta", "bn0_gamma", "conv0_weight"]


@pytest.mark.parametrize("builder", [F.get_multi_symbol_train, F.get_det_symbol_train, F.get_seg_symbol_train])
def test_unknown_names_raise(stub_prior, builder):
    with pytest.raises(ValueError, match="no_such_weight"):
        build("resnet-50", builder=builder, fixed_param_names=["conv0_weight", "no_such_weight"])


def test_fix_gamma_and_input_names_are_known_without_effect(stub_prior):
    # bn_data and the decoder BatchNorms are fix_gamma: MXNet lists their _gamma, this build has no such parameter
    net = build("resnet-50", fixed_param_names=["bn_data_gamma", "res3_reduced_bn_gamma", "data", "label_det",
                                                 "seg_out_label"])
    assert net.fixed_param_names == []
    assert "bn_data_gamma" not in net.g.params
    det = build("resnet-50", builder=F.get_det_symbol_train, fixed_param_names=["data", "label_det"])
    assert det.fixed_param_names == []
    with pytest.raises(ValueError, match="seg_out_label"):          # a detection-only graph has no segmentation label
        build("resnet-50", builder=F.get_det_symbol_train, fixed_param_names=["seg_out_label"])


def test_default_build_freezes_nothing(stub_prior):
    net = build("resnet-50")
    assert net.fixed_param_names == [] and not net.g.freezing
    assert not any(p.fixed for p in net.g.param_order)


# ---------------------------------------------------------------- gradient flow
def _grad_map(net):
    return {n.out.name: n.out.requires_grad for n in net.g.nodes if getattr(n, "out", None) is not None}


def test_frozen_prefix_leaves_backward(stub_prior):
    rg = _grad_map(build("resnet-50", freeze_pattern=r"^(bn_data|conv0|bn0|stage1_)"))
    base = _grad_map(build("resnet-50"))
    for name in ("conv0_out", "bn0_relu", "pooling0", "stage1_unit1_conv1_out", "_plus0", "_plus2"):
        assert base[name] and not rg[name], name
    # stage2's first BatchNorm owns trainable parameters: its output needs a gradient, its input does not
    assert rg["stage2_unit1_bn1_relu"] and rg["stage2_unit1_conv1_out"] and rg["_plus3"]
    # nothing behind the prefix changes
    for name, v in base.items():
        if not name.startswith(("conv0", "bn0", "bn_data", "pooling0", "stage1_", "_plus0", "_plus1", "_plus2")):
            assert rg[name] == v, name


def test_frozen_middle_keeps_the_data_gradient(stub_prior):
    net = build("resnet-50", freeze_pattern=r"^stage3_")
    assert _grad_map(net) == _grad_map(build("resnet-50"))        # stage 2 still needs its gradient through stage 3
    g = net.g
    frozen_convs = [n for n in g.nodes if getattr(n, "w", None) is not None and n.w.fixed]
    assert frozen_convs and all(n.slabs is None for n in frozen_convs)   # (CPU graphs allocate no slabs either way)


def test_vgg_reference_freeze_flow(stub_prior):
    rg = _grad_map(build("vgg16_reduced", freeze_pattern=REFERENCE_FREEZE))
    assert not rg["conv1_1_out"] and not rg["conv2_2_out"] and not rg["pool2"]
    assert rg["conv3_1_out"] and rg["pool3"]
    net = build("vgg16_reduced", freeze_pattern=REFERENCE_FREEZE)
    conv3_1 = [n for n in net.g.nodes if getattr(n, "w", None) is not None and n.w.name == "conv3_1_weight"][0]
    assert not conv3_1.x.requires_grad                  # conv3_1 computes its weight gradient only


# ---------------------------------------------------------------- multipliers
def test_module_rule_multipliers():
    assert rule_multipliers("conv0_weight", "module") == (1.0, 1.0)
    assert rule_multipliers("bn0_gamma", "module") == (1.0, 1.0)
    assert rule_multipliers("bn0_beta", "module") == (1.0, 0.0)
    assert rule_multipliers("conv1_1_bias", "module") == (1.0, 0.0)
    assert rule_multipliers("affine_matrix", "module") == (1.0, 0.0)
    assert rule_multipliers("_plus12_loc_pred_conv_bias", "module", lr_mult=2.0) == (2.0, 0.0)
    assert rule_multipliers("x_weight", "module", wd_mult=0.5) == (1.0, 0.5)
    for name in ("conv0_weight", "bn0_beta", "_plus12_cls_pred_conv_bias"):
        assert rule_multipliers(name, "multi_solver", lr_mult=2.0) == (1.0, 1.0)
    with pytest.raises(ValueError):
        rule_multipliers("conv0_weight", "adam")


def test_head_biases_carry_lr_mult_2(stub_prior):
    g = build("resnet-50").g
    twos = sorted(p.name for p in g.param_order if p.lr_mult != 1.0)
    heads = sorted(p.name for p in g.param_order if p.name.endswith(("_loc_pred_conv_bias", "_cls_pred_conv_bias")))
    assert twos == heads and len(heads) == 12
    assert all(g.params[n].lr_mult == 2.0 for n in twos)
    assert all(p.wd_mult == 1.0 for p in g.param_order)


# ---------------------------------------------------------------- segment tables
def _rows_for(params, frozen, rules="multi_solver"):
    return sgd_segments([(o, s) + rule_multipliers(n, rules, 2.0 if n.endswith(("_loc_pred_conv_bias",
                                                                                  "_cls_pred_conv_bias")) else 1.0)
                         for n, o, s in params if n not in frozen])


def _covered(rows):
    return set().union(*[set(range(o, o + n, 4)) for o, n, _, _ in rows]) if rows else set()


@pytest.mark.parametrize("pattern", [r"^(bn_data|conv0|bn0|stage1_)", r"^stage3_", r"^$"])
@pytest.mark.parametrize("rules", ["multi_solver", "module"])
def test_segment_tables_cover_exactly_the_trainable_ranges(pattern, rules):
    import re
    params, owner, total, _ = golden()
    frozen = {n for n, _, _ in params if re.match(pattern, n)}
    rows = _rows_for(params, frozen, rules)
    assert all(o % 4 == 0 and n % 4 == 0 and n > 0 for o, n, _, _ in rows)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(rows, rows[1:]))           # sorted, disjoint
    # merged: two neighbouring rows either leave a gap or differ in a multiplier
    assert all(a[0] + a[1] < b[0] or a[2:] != b[2:] for a, b in zip(rows, rows[1:]))
    want = set().union(*[set(range(o, o + s, 4)) for n, o, s in params if n not in frozen])
    assert _covered(rows) == want
    for n, o, s in params:
        row = [r for r in rows if r[0] <= o < r[0] + r[1]]
        if n in frozen:
            assert not row
        else:
            assert row[0][2:] == rule_multipliers(n, rules, 2.0 if n.endswith(("_loc_pred_conv_bias",
                                                                               "_cls_pred_conv_bias")) else 1.0)
    if rules == "multi_solver":          # one row per run of trainable parameters
        runs = sum(1 for i, (n, _, _) in enumerate(params) if n not in frozen and (i == 0 or params[i - 1][0] in frozen))
        assert len(rows) == runs
    if not frozen and rules == "multi_solver":
        assert rows == [(0, total, 1.0, 1.0)]


def test_segment_table_upload_checks_rows():
    rows = [(0, 8, 1.0, 1.0), (12, 4, 2.0, 0.0)]
    dev, nseg, total4 = fn.sgd_segment_table(rows, 16, torch.device("cpu"))
    assert (nseg, total4) == (2, 3) and dev.dtype == torch.uint8 and dev.numel() == 2 * 24
    tab = dev.numpy().view(np.dtype(fn.SGD_SEGMENT_FIELDS))
    assert list(tab["offset"]) == [0, 12] and list(tab["lr_mult"]) == [1.0, 2.0]
    for bad in ([(0, 8, 1, 1), (4, 4, 1, 1)],          # overlap
                [(2, 8, 1, 1)],                         # unaligned offset
                [(0, 6, 1, 1)],                         # unaligned length
                [(8, 4, 1, 1), (0, 4, 1, 1)],           # unsorted
                [(0, 20, 1, 1)],                        # outside the arena
                []):
        with pytest.raises(ValueError):
            fn.sgd_segment_table(bad, 16, torch.device("cpu"))


def test_segmented_entry_point_validates_without_a_gpu():
    lib = _lib.lib()
    assert "dspn_sgd_momentum_segments_f32" in _lib.SIGNATURES
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # null pointers, an empty or oversized table, total4 <= 0: refused before anything is launched
    assert lib.dspn_sgd_momentum_segments_f32(None, p, p, p, 1, 4, 0.1, 0.9, 0.0, 1.0, None) != 0
    assert b"sgd_momentum_segments" in lib.dspn_last_error()
    assert lib.dspn_sgd_momentum_segments_f32(p, p, p, None, 1, 4, 0.1, 0.9, 0.0, 1.0, None) != 0
    assert lib.dspn_sgd_momentum_segments_f32(p, p, p, p, 0, 4, 0.1, 0.9, 0.0, 1.0, None) != 0
    assert lib.dspn_sgd_momentum_segments_f32(p, p, p, p, fn.SGD_MAX_SEGMENTS + 1, 4, 0.1, 0.9, 0.0, 1.0, None) != 0
    assert lib.dspn_sgd_momentum_segments_f32(p, p, p, p, 1, 0, 0.1, 0.9, 0.0, 1.0, None) != 0


# ---------------------------------------------------------------- buckets
def test_bucket_plan_without_frozen_is_the_golden_layout():
    params, owner, total, doc = golden()
    want = doc["buckets_16mb"]
    for frozen in (None, set(), frozenset()):
        assert [list(b) for b in plan_buckets(params, owner, total, int(16.0 * (1 << 20) / 4), frozen)] == want


@pytest.mark.parametrize("pattern", [r"^(bn_data|conv0|bn0|stage1_)", r"^stage3_", r"^(stage2_|multi_feat_3)"])
def test_bucket_plans_exclude_frozen_ranges(pattern):
    import re
    params, owner, total, _ = golden()
    frozen = {n for n, _, _ in params if re.match(pattern, n)}
    assert frozen
    for mb in (16.0, 4.0):
        buckets = plan_buckets(params, owner, total, int(mb * (1 << 20) / 4), frozen)
        cover = sorted((lo, hi) for lo, hi, _ in buckets)
        assert all(b <= c for (_, b), (c, _) in zip(cover, cover[1:]))            # disjoint
        for n, o, s in params:
            inside = [b for b in cover if b[0] <= o and o + s <= b[1]]
            if n in frozen:
                assert not any(lo < o + s and o < hi for lo, hi in cover), n
            else:
                assert len(inside) == 1, n
        firsts = [f for _, _, f in buckets]
        assert firsts == sorted(firsts, reverse=True)
        for lo, hi, first in buckets:
            assert first == min(owner[n] for n, o, s in params if o < hi and o + s > lo)
        side = side_buckets(buckets, params, owner, {owner[n] for n, _, _ in params if n.startswith("multi_feat_")})
        assert len(side) == len(buckets)


def _worker(rank, world, port, total, params, owner, frozen, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(100 + rank)
    arena = torch.randn(total, generator=g)
    local = arena.clone()
    buckets = plan_buckets(params, owner, total, 6000, frozen)
    red = GradBucketReducer(arena, buckets)
    red.begin()
    for idx in range(max(owner.values()), -1, -1):
        red.node_done(idx)
    red.finish()
    gathered = [torch.zeros(total) for _ in range(world)]
    dist.all_gather(gathered, local)
    summed = sum(gathered)
    ok_frozen = ok_trainable = True
    for n, o, s in params:
        if n in frozen:
            ok_frozen &= torch.equal(arena[o:o + s], local[o:o + s])          # never reduced: this rank's own values
        else:
            ok_trainable &= torch.allclose(arena[o:o + s], summed[o:o + s], rtol=0, atol=1e-5)
    out.put((rank, bool(ok_frozen), bool(ok_trainable), len(red.launched)))
    dist.destroy_process_group()


def test_bucketed_allreduce_world2_gloo_skips_frozen_ranges():
    rng = np.random.default_rng(3)
    params, owner, off = [], {}, 0
    for i in range(31):
        size = int(rng.integers(1, 4000)) // 4 * 4 + 4
        params.append(("p%d" % i, off, size))
        owner["p%d" % i] = i // 2
        off += size
    frozen = {"p0", "p1", "p2", "p9", "p10", "p30"}         # a prefix, a middle run, the last parameter
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, off, params, owner, frozen, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok_frozen, ok_trainable, n in res:
        assert ok_frozen and ok_trainable and n > 3, (rank, ok_frozen, ok_trainable, n)


def test_node_outputs_are_what_its_constructor_made(stub_prior):
    """a tensor made BETWEEN nodes (by a builder) that a node reads is that node's input, not its output"""
    from dspnet_amd import engine as E
    g = E.Graph(torch.device("cpu"))
    g.set_freeze(["c_weight"])
    data = g.tensor((1, 4, 4, 4), "data", requires_grad=False)
    x = g.add(E.InputNCHW(g, g.tensor((1, 3, 4, 4), "img", requires_grad=False))).out
    side = g.tensor((1, 4, 4, 4), "side", requires_grad=True)       # a builder-made tensor that needs a gradient
    out = g.add(E.Add(g, x, side, "sum")).out
    assert out.requires_grad and side.requires_grad and not data.requires_grad
    c = g.add(E.Conv(g, x, "c", 8, 1)).out                             # frozen weight, input without gradient
    assert not c.requires_grad


def test_segmented_update_needs_a_gpu_graph(stub_prior):
    from dspnet_amd.train.solver import MultiTaskSolver
    net = build("resnet-50", freeze_pattern="^conv0")
    net.g.arena = torch.zeros(net.g.param_order[-1].offset + 8)      # (finalize() on a CPU graph: the arena exists)
    s = MultiTaskSolver(net, high_priority=False)
    assert s.sgd_rows and s.sgd_table is None
    with pytest.raises(RuntimeError, match="GPU"):
        s.update()
