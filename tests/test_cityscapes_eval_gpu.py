"""Cityscapes pixel-level evaluation on the device: the two count entry points against the fixtures generated from the
reference's evalPixelLevelSemanticLabeling.py and, at full size, against the numpy restatement of its counting
(tests/cityscapes_cases.py, itself pinned to the fixtures in tests/test_cityscapes_eval.py).  Every comparison is exact:
the device forms integers only, the host scores repeat the script's float64 operations in its order."""
import numpy as np
import pytest

import cityscapes_cases as cc
from test_cityscapes_eval import assert_scores_equal

pytestmark = pytest.mark.gpu
CASES = cc.golden_cases()


def _dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _tables(ce, device):
    return _dev(ce.category_table(), device), _dev(ce.label_of_train_id_table(), device)


def _counts_class_map(fn, pred, gt, inst, cat, out=None):
    conf, table, err = out if out is not None else fn.cityscapes_tables(pred.shape[0], pred.device)
    fn.cityscapes_counts(pred, gt, inst, cat, conf, table, err)
    return conf, table, err


def _assert_counts(got, want):
    conf, table, err = got
    wconf, wrows, werr = want
    np.testing.assert_array_equal(conf.cpu().numpy(), wconf)
    np.testing.assert_array_equal(cc.table_rows(table.cpu().numpy()), wrows)
    assert int(err.item()) == werr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_counts_and_scores(gpu_device, case):
    from dspnet_amd import functional as fn
    from dspnet_amd.evaluate import cityscapes_eval as ce
    cat, _ = _tables(ce, gpu_device)
    conf, table, err = _counts_class_map(fn, _dev(case["pred"], gpu_device), _dev(case["gt_label"], gpu_device),
                                         _dev(case["gt_inst"], gpu_device), cat)
    np.testing.assert_array_equal(conf.cpu().numpy(), case["conf"])
    assert int(err.item()) == 0
    rows, want = cc.table_rows(table.cpu().numpy()), case["inst"]
    np.testing.assert_array_equal(rows[:, :3], want[:, :3])
    walked = want[:, 3] >= 0                     # the others are instances of ignored labels: the script has no figure
    np.testing.assert_array_equal(rows[walked], want[walked])
    np.testing.assert_array_equal(rows, cc.count(case["pred"], case["gt_label"], case["gt_inst"], ce.category_table())[1])
    m = ce.CityscapesPixelMetric(device=gpu_device)
    for n in range(case["pred"].shape[0]):       # image by image, as the script walks them
        m.update(case["pred"][n], case["gt_label"][n], case["gt_inst"][n])
    got = m.get()
    assert_scores_equal(got, case["scores"])
    assert got["confMatrix"] == case["conf"].tolist()
    m.reset()
    m.update(case["pred"], case["gt_label"], case["gt_inst"])      # and as one batch
    assert_scores_equal(m.get(), case["scores"])


def test_full_size_random_scenes_both_entry_points(gpu_device):
    """1024 x 2048, N = 4, ~150 instances per image; the fused call is checked against the class map of
    seg_upsample_argmax (bit exact against the CPU restatement in test_eval_metrics.py) sent through the table"""
    import torch
    from dspnet_amd import functional as fn
    from dspnet_amd.evaluate import cityscapes_eval as ce
    from dspnet_amd.evaluate.multi_eval import label_ids
    g = np.random.Generator(np.random.PCG64(2026))
    N, H, W = 4, 1024, 2048
    pred, gt, inst = cc.random_scene(g, N, H, W, 150)
    cat, lut = _tables(ce, gpu_device)
    want = cc.count(pred, gt, inst, ce.category_table())
    assert want[2] == 0 and len(want[1]) > 400 and np.count_nonzero(want[0]) > 500
    dgt, dinst = _dev(gt, gpu_device), _dev(inst, gpu_device)
    _assert_counts(_counts_class_map(fn, _dev(pred, gpu_device), dgt, dinst, cat), want)
    prob = _dev(cc.softmax_nhwc(g, N, 19, 128, 256, 20), gpu_device)
    out = fn.cityscapes_tables(N, gpu_device)
    fn.cityscapes_counts_prob(prob, 19, lut, dgt, dinst, cat, *out)
    ids = label_ids(fn.seg_upsample_argmax(prob, 19, H, W))
    _assert_counts(out, cc.count(ids.cpu().numpy(), gt, inst, ce.category_table()))
    for a, b in zip(out, _counts_class_map(fn, ids, dgt, dinst, cat)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 19, 16, 32, 128, 256), (1, 19, 9, 13, 37, 51), (3, 5, 7, 7, 7, 7),
                                   (1, 19, 128, 256, 1024, 2048), (1, 3, 4, 4, 1, 1), (2, 6, 5, 9, 33, 64)])
@pytest.mark.parametrize("ld_pad", [0, 1])
def test_fused_equals_upsample_then_class_map(gpu_device, shape, ld_pad):
    """the shapes of test_seg_upsample_argmax_bit_exact; ld_pad = 1 adds a row length with ld % 4 != 0"""
    import torch
    from dspnet_amd import functional as fn
    from dspnet_amd.evaluate import cityscapes_eval as ce
    N, C, h, w, Ho, Wo = shape
    ld = fn.pad4(C) + ld_pad * (1 if fn.pad4(C) != C else 3)
    assert (ld % 4 != 0) == bool(ld_pad)
    g = np.random.Generator(np.random.PCG64(11))
    prob = _dev(cc.softmax_nhwc(g, N, C, h, w, ld), gpu_device)
    _, gt, inst = cc.random_scene(g, N, Ho, Wo, 12 if Ho * Wo > 64 else 0)
    cat, _ = _tables(ce, gpu_device)
    lut_host = np.zeros(256, np.uint8)
    lut_host[:C] = g.permutation(np.arange(34))[:C]                  # any table: here C of the 34 labelIds
    lut = _dev(lut_host, gpu_device)
    dgt, dinst = _dev(gt, gpu_device), _dev(inst, gpu_device)
    fused = fn.cityscapes_tables(N, gpu_device)
    fn.cityscapes_counts_prob(prob, C, lut, dgt, dinst, cat, *fused)
    ids = lut[fn.seg_upsample_argmax(prob, C, Ho, Wo).long()]
    two_step = _counts_class_map(fn, ids, dgt, dinst, cat)
    for a, b in zip(fused, two_step):
        assert torch.equal(a, b)
    assert int(fused[0].sum().item()) == N * Ho * Wo and int(fused[2].item()) == 0
    _assert_counts(fused, cc.count(ids.cpu().numpy(), gt, inst, ce.category_table()))


def test_accumulation_streams_and_graph_replay(gpu_device):
    import torch
    from dspnet_amd import functional as fn
    from dspnet_amd.evaluate import cityscapes_eval as ce
    g = np.random.Generator(np.random.PCG64(5))
    N, H, W = 3, 120, 200
    pred, gt, inst = cc.random_scene(g, N, H, W, 20)
    cat, lut = _tables(ce, gpu_device)
    want = cc.count(pred, gt, inst, ce.category_table())
    d = [_dev(a, gpu_device) for a in (pred, gt, inst)]
    # several calls into one set of tables == one call on the concatenation (each image into its own slice of the table)
    conf, table, err = fn.cityscapes_tables(N, gpu_device)
    for n in range(N):
        fn.cityscapes_counts(d[0][n:n + 1], d[1][n:n + 1], d[2][n:n + 1], cat, conf, table[n:n + 1], err)
    _assert_counts((conf, table, err), want)
    # a call on a stream of its own
    side = torch.cuda.Stream(device=gpu_device)
    out = fn.cityscapes_tables(N, gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn.cityscapes_counts(*d, cat, *out)
    side.synchronize()
    _assert_counts(out, want)
    # recorded in a graph, replayed twice: the tables hold twice the counts of one call (both entry points)
    prob = _dev(cc.softmax_nhwc(g, N, 19, 15, 25, 20), gpu_device)
    out = fn.cityscapes_tables(N, gpu_device)
    out2 = fn.cityscapes_tables(N, gpu_device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn.cityscapes_counts(*d, cat, *out)
        fn.cityscapes_counts_prob(prob, 19, lut, d[1], d[2], cat, *out2)
    for t in out + out2:
        t.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[0].cpu().numpy(), 2 * want[0])
    rows = cc.table_rows(out[1].cpu().numpy())
    np.testing.assert_array_equal(rows[:, :2], want[1][:, :2])
    np.testing.assert_array_equal(rows[:, 2:], 2 * want[1][:, 2:])
    ids = lut[fn.seg_upsample_argmax(prob, 19, H, W).long()].cpu().numpy()
    want2 = cc.count(ids, gt, inst, ce.category_table())
    np.testing.assert_array_equal(out2[0].cpu().numpy(), 2 * want2[0])
    np.testing.assert_array_equal(cc.table_rows(out2[1].cpu().numpy())[:, 2:], 2 * want2[1][:, 2:])


def test_out_of_range_ids_raise_and_leave_the_valid_counts(gpu_device):
    from dspnet_amd import functional as fn
    from dspnet_amd.evaluate import cityscapes_eval as ce
    g = np.random.Generator(np.random.PCG64(9))
    pred, gt, inst = cc.random_scene(g, 2, 64, 100, 10)
    pred[0, 3, 5:9] = 34; pred[1, 60, 1] = 255
    gt[0, 10, 10] = 99
    inst[1, 20, 20:23] = 7001; inst[1, 21, 20] = 34000; inst[0, 5, 5] = 65535
    want = cc.count(pred, gt, inst, ce.category_table())
    assert want[2] == 11
    cat, _ = _tables(ce, gpu_device)
    _assert_counts(_counts_class_map(fn, *[_dev(a, gpu_device) for a in (pred, gt, inst)], cat), want)
    m = ce.CityscapesPixelMetric(device=gpu_device)
    with pytest.raises(ValueError, match="11 pixel"):
        m.update(pred, gt, inst)
    np.testing.assert_array_equal(m.conf.cpu().numpy(), want[0])
    np.testing.assert_array_equal(np.concatenate([np.c_[np.full(len(r), n), r] for n, r in enumerate(m.last_instance_counts)]),
                                  want[1])
    m.update(np.clip(pred, 0, 33), np.clip(gt, 0, 33), np.where(inst > 33999, 0, np.where(inst // 1000 == 7, 7, inst)))


def test_evaluate_net_cityscapes_keys(gpu_device):
    import torch
    from dspnet_amd import synthetic
    from dspnet_amd.evaluate import cityscapes_eval as ce
    from dspnet_amd.evaluate.multi_eval import evaluate_net
    from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
    B, S, R = 2, 128, (96, 200)
    net = get_multi_symbol_train("resnet-50", S, num_classes=8, batch_size=B, device=gpu_device)
    gen = synthetic.rng(233)
    g = np.random.Generator(np.random.PCG64(1))
    batches = []
    for _ in range(2):
        _, gt, inst = cc.random_scene(g, B, R[0], R[1], 8)
        batches.append({"data": torch.from_numpy(synthetic.images(B, S, S, gen)).to(gpu_device),
                        "label_det": torch.from_numpy(synthetic.det_labels(B, gen=gen, height=S, width=S)).to(gpu_device),
                        "label_seg": torch.from_numpy(synthetic.seg_labels(B, S, S, gen=gen)).to(gpu_device),
                        "gt_label_ids": torch.from_numpy(gt), "gt_instance_ids": torch.from_numpy(inst)})
    cls = ["c%d" % i for i in range(8)]
    seg = ["s%d" % i for i in range(19)]
    by_hand = ce.CityscapesPixelMetric(device=gpu_device)
    plain = None
    for b in batches:                               # the metric fed by hand from the same forward passes
        plain = evaluate_net(net, [b], cls, seg)
        by_hand.update_from_prob(net.seg_out.prob.data, b["gt_label_ids"], b["gt_instance_ids"])
    out = evaluate_net(net, batches, cls, seg, cityscapes=True)
    extra = dict(by_hand.get_name_value())
    assert set(out) - set(plain) == set(extra) and set(plain) <= set(out)
    assert {"cityscapes/IoU_class", "cityscapes/iIoU_class", "cityscapes/IoU_category", "cityscapes/iIoU_category",
            "cityscapes/IoU/road", "cityscapes/iIoU/car"} <= set(extra) and len(extra) == 4 + 19 + 8
    for k, v in extra.items():
        assert (np.isnan(v) and np.isnan(out[k])) or out[k] == v, (k, out[k], v)
    assert np.isfinite(out["cityscapes/IoU_class"]) and np.isfinite(out["cityscapes/IoU_category"])
    # without the argument: the keys of the parent commit
    base = evaluate_net(net, batches, cls, seg, full_res=(256, 256))
    assert not [k for k in base if k.startswith("cityscapes")]
    assert set(base) == set(plain) | {"class_maps"} and {"CrossEntropy", "SmoothL1", "accuracy", "mAP", "mIoU"} <= set(base)
    with pytest.raises(ValueError, match="full_res"):
        evaluate_net(net, batches[:1], cls, seg, full_res=(256, 256), cityscapes=True)
