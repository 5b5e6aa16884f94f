"""Cityscapes pixel-level evaluation without a GPU: the label table and the host score arithmetic against fixtures
generated from the reference's own evalPixelLevelSemanticLabeling.py (tests/golden/make_cityscapes_eval_golden.py),
the numpy restatement of the counting that the GPU tests use as their yardstick, and the argument checks of the two
C entry points."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import cityscapes_cases as cc
from dspnet_amd import _lib
from dspnet_amd import functional as fn
from dspnet_amd.evaluate import cityscapes_eval as ce
from dspnet_amd.evaluate.multi_eval import CITYSCAPES_LABEL_IDS

CASES = cc.golden_cases()


def same(a, b):
    """equal floats, NaN in the same places"""
    return (math.isnan(a) and math.isnan(b)) or a == b


def assert_scores_equal(got, want):
    for field in cc.SCORE_FIELDS + ("priors",):
        assert list(got[field]) == list(want[field]), field            # same keys in the same order
        for k in want[field]:
            assert same(got[field][k], want[field][k]), (field, k, got[field][k], want[field][k])
    for field in cc.AVERAGES:
        assert same(got[field], want[field]), (field, got[field], want[field])
    assert got["labels"] == want["labels"]
    for level in ("classes", "categories"):
        assert list(got["instanceStats"][level]) == list(want["instanceStats"][level])
        for k, w in want["instanceStats"][level].items():
            for f in w:
                assert got["instanceStats"][level][k][f] == w[f], (level, k, f, got["instanceStats"][level][k][f], w[f])


def stats_from_rows(rows):
    stats = ce.new_instance_stats()
    for n in np.unique(rows[:, 0]):
        r = rows[rows[:, 0] == n]
        ce.add_image_instances(stats, r[:, 1], r[:, 2], r[:, 3], r[:, 4])
    return stats


def test_label_table_equals_the_scripts():
    with open(os.path.join(cc.GOLDEN, "cityscapes_labels.json")) as f:
        want = json.load(f)
    assert len(ce.CITYSCAPES_LABELS) == len(want["labels"]) == 35
    for mine, ref in zip(ce.CITYSCAPES_LABELS, want["labels"]):
        assert mine._asdict() == {"name": ref["name"], "id": ref["id"], "train_id": ref["trainId"], "category": ref["category"],
                                  "category_id": ref["categoryId"], "has_instances": ref["hasInstances"],
                                  "ignore_in_eval": ref["ignoreInEval"]}, ref["name"]
        assert type(mine.has_instances) is bool and type(mine.ignore_in_eval) is bool
    assert ce.AVG_CLASS_SIZE == want["avgClassSize"] and len(ce.AVG_CLASS_SIZE) == 10


def test_label_table_agrees_with_the_train_id_table():
    by_train = sorted((lab.train_id, lab.id) for lab in ce.CITYSCAPES_LABELS if 0 <= lab.train_id < 255)
    assert tuple(i for _, i in by_train) == CITYSCAPES_LABEL_IDS and [t for t, _ in by_train] == list(range(19))
    lut = ce.label_of_train_id_table()
    assert tuple(lut[:19]) == CITYSCAPES_LABEL_IDS and not lut[19:].any()
    cat = ce.category_table()
    assert set(np.nonzero(cat)[0]) == set(range(24, 34)) and cat[24] == cat[25] != cat[26] and len(set(cat[26:34])) == 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_scores_equal_the_scripts(case):
    """golden confusion matrix + golden per-instance counts -> every golden score with ==: the same float64 operations in
    the same order.  (instances of labels ignored in evaluation carry -1 counts in the fixture: they must be skipped)"""
    got = ce.scores_from_counts(case["conf"], stats_from_rows(case["inst"]))
    assert_scores_equal(got, case["scores"])
    assert got["confMatrix"] == case["conf"].tolist()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_numpy_counting_equals_the_scripts(case):
    conf, rows, errors = cc.count(case["pred"], case["gt_label"], case["gt_inst"], ce.category_table())
    assert errors == 0
    np.testing.assert_array_equal(conf, case["conf"])
    want = case["inst"]
    np.testing.assert_array_equal(rows[:, :3], want[:, :3])             # the same instances with the same sizes
    walked = want[:, 3] >= 0                                            # the script walks these: its own tp / catTp
    assert walked.sum() >= 1
    np.testing.assert_array_equal(rows[walked], want[walked])
    assert_scores_equal(ce.scores_from_counts(conf, stats_from_rows(rows)), case["scores"])


def test_golden_cases_cover_what_they_should():
    by = {c["name"]: c for c in CASES}
    assert by["three_images"]["pred"].shape[0] == 3 and by["width_101"]["pred"].shape[2] % 4 != 0
    r = by["ignored_labels"]["inst"]
    assert (r[:, 4] > r[:, 3]).any()                                    # cat_tp != tp
    assert (by["ignored_instances"]["inst"][:, 3] < 0).any()            # 29xxx / 30xxx instances
    g = by["groups"]
    assert ((g["gt_inst"] < 1000) & (g["gt_inst"] >= 24)).any()
    assert (by["single_pixel_instances"]["inst"][:, 2] == 1).sum() >= 3
    s = by["absent_classes"]["scores"]
    assert math.isnan(s["classScores"]["sidewalk"]) and math.isnan(s["categoryScores"]["human"])
    assert math.isnan(s["classInstScores"]["road"]) and not math.isnan(s["classInstScores"]["car"])
    assert len(set(np.unique(by["one_class_everywhere"]["pred"]))) == 1


def test_numpy_counting_of_out_of_range_ids():
    pred = np.array([[[7, 40, 26, 26]]], np.uint8); gt = np.array([[[7, 7, 200, 26]]], np.uint8)
    inst = np.array([[[7, 7001, 34000, 26001]]], np.int32)
    conf, rows, errors = cc.count(pred, gt, inst, ce.category_table())
    assert errors == 2 and conf.sum() == 2 and conf[7, 7] == 1 and conf[26, 26] == 1
    np.testing.assert_array_equal(rows, [[0, 26001, 1, 1, 1]])


def _calls():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)        # never dereferenced: every call below fails its checks first

    def class_map(pred=p, gt=p, inst=p, N=1, H=8, W=8, cat=p, conf=p, table=p, err=p):
        return lib.dspn_cityscapes_counts_u8(pred, gt, inst, N, H, W, cat, conf, table, err, None)

    def fused(prob=p, N=1, Hin=4, Win=4, C=19, ld=20, lut=p, gt=p, inst=p, Ho=8, Wo=8, cat=p, conf=p, table=p, err=p):
        return lib.dspn_cityscapes_counts_prob_f32(prob, N, Hin, Win, C, ld, lut, gt, inst, Ho, Wo, cat, conf, table, err, None)
    return lib, class_map, fused


def test_class_map_entry_point_rejects_bad_arguments_without_gpu():
    lib, call, _ = _calls()
    for name in ("pred", "gt", "inst", "cat", "conf", "table", "err"):
        assert call(**{name: None}) == -1 and b"cityscapes_counts: null pointer" in lib.dspn_last_error(), name
    for bad in ({"N": 0}, {"N": -1}, {"H": 0}, {"H": -3}, {"W": 0}, {"W": -1}, {"N": 300000}, {"H": 70000, "W": 70000},
                {"N": 2000, "H": 30000, "W": 30000}):
        assert call(**bad) == -1 and b"cityscapes_counts: bad argument" in lib.dspn_last_error(), bad


def test_fused_entry_point_rejects_bad_arguments_without_gpu():
    lib, _, call = _calls()
    for name in ("prob", "lut", "gt", "inst", "cat", "conf", "table", "err"):
        assert call(**{name: None}) == -1 and b"cityscapes_counts_prob: null pointer" in lib.dspn_last_error(), name
    for bad in ({"N": 0}, {"N": -1}, {"Hin": 0}, {"Win": 0}, {"Ho": 0}, {"Wo": -2}, {"C": 0}, {"C": -1}, {"C": 257, "ld": 260},
                {"C": 19, "ld": 18}, {"N": 300000}, {"Ho": 70000, "Wo": 70000}):
        assert call(**bad) == -1 and b"cityscapes_counts_prob: bad argument" in lib.dspn_last_error(), bad


def test_wrappers_check_shapes_before_the_call():
    import torch
    conf, table, err = fn.cityscapes_tables(2, "cpu")
    assert conf.shape == (34, 34) and table.shape == (2, 10, 1000, 3) and err.shape == (1,)
    z = torch.zeros(2, 8, 8, dtype=torch.uint8)
    cat = torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(AssertionError):
        fn.cityscapes_counts(z, z, z, cat, conf, table, err)            # the instance map is 32-bit
    with pytest.raises(AssertionError):
        fn.cityscapes_counts(z, z[:1], z[:1].int(), cat, conf, table, err)
