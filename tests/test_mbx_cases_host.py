"""Host self-checks of the MultiBoxDetection edge cases (mbx_cases.DET_EDGE_CASES): the CPU oracle alone, no GPU.

A case is only worth its GPU time while it still meets the condition it was built for -- an exact number of valid rows, a cut
inside a run of ties that spans two strides, pairs whose IoU has to be divided out.  These tests state those conditions, and
test_case_set_reaches_every_route keeps the case table from quietly losing a route of the operator."""
import numpy as np
import pytest

import mbx_cases as mc

# det_route() fields that the cases must reach between them: every sort, select and grouping route of
# dspn_multibox_detection_f32 / det_decode_sort_kernel / nms_scan_kernel (DESIGN.md lists them)
REQUIRED_ROUTES = {
    "keys:lds", "keys:global",
    "select:on", "select:on+segments",                      # the selected list sorted by one wave / by per-wave segments
    "refused:half", "refused:bytes", "refused:global",
    "sorter:none", "sorter:wave", "sorter:wave@1024", "sorter:workgroup",
    "sorter:segments@128", "sorter:segments@256", "sorter:segments@512", "sorter:segments@1024",
    "grouping:force", "grouping:count", "grouping:count@256", "grouping:sort", "grouping:sort+global",
    "scan_tail",
}


def route_tags(r, C):
    tags = {f"keys:{r.keys}"}
    if r.sorter != "segments":
        tags.add(f"sorter:{r.sorter}")
    if r.select:
        tags.add("select:on+segments" if r.sorter == "segments" else "select:on")
    if r.refused:
        tags.add(f"refused:{r.refused}")
    if r.sorter == "wave" and r.sort_n == mc.K_WAVE_SORT_MAX:
        tags.add("sorter:wave@1024")
    if r.sorter == "segments":
        tags.add(f"sorter:segments@{r.segment}")
    if r.grouping:
        tags.add(f"grouping:{r.grouping}")
        if r.grouping == "count" and C - 1 == mc.K_COUNT_CLS:
            tags.add("grouping:count@256")
        if r.grouping == "sort" and r.keys == "global":
            tags.add("grouping:sort+global")
    if r.scan_tail:
        tags.add("scan_tail")
    return tags


def test_case_set_reaches_every_route():
    reached = set()
    for cid, (name, _) in mc.DET_EDGE_CASES.items():
        C = mc.det_inputs(name)[1].shape[1]
        for r in mc.det_case_routes(cid):
            reached |= route_tags(r, C)
    assert REQUIRED_ROUTES - reached == set()
    assert reached - REQUIRED_ROUTES == set()          # (a tag nobody requires is a typo here, not a new route)


def test_route_model_at_the_dispatch_edges():
    """det_route against the rules of multibox.hip, worked by hand"""
    r = mc.det_route(6132, 9, 6132, 4096, .5)           # selcap 4096: 2 x 4096 == n2cap, 96 KiB: selected, segments of 256
    assert (r.select, r.sort_n, r.sorter, r.segment) == (True, 4096, "segments", 256)
    r = mc.det_route(6132, 9, 6132, 4097, .5)           # selcap 8192 > n2cap / 2
    assert (r.select, r.refused, r.sort_n, r.segment) == (False, "half", 8192, 512)
    r = mc.det_route(12264, 9, 12264, 1024, .5)         # 8 (16384 + 1024) = 139264 <= 143360
    assert (r.select, r.sort_n, r.sorter) == (True, 1024, "wave")
    r = mc.det_route(12264, 9, 12264, 1025, .5)         # 8 (16384 + 2048) = 147456 > 143360
    assert (r.select, r.refused, r.sort_n, r.segment) == (False, "bytes", 16384, 1024)
    r = mc.det_route(12264, 9, 1000, 1025, .5)          # the list is not cut: nothing to refuse
    assert (r.select, r.refused, r.sorter) == (False, None, "wave")
    assert mc.det_route(16384, 9, 16384, -1, .5).keys == "lds" and mc.det_route(16385, 9, 5, -1, .5).keys == "global"
    assert mc.det_route(16385, 9, 5, 3, .5)[:5] == ("global", False, "global", 8, "workgroup")
    assert mc.det_route(268, 257, 200, -1, .5).grouping == "count" and mc.det_route(268, 258, 200, -1, .5).grouping == "sort"
    assert mc.det_route(268, 258, 200, -1, .5, force_suppress=True).grouping == "force"
    assert mc.det_route(268, 4, 200, -1, -1.).sorter == "none" and mc.det_route(268, 4, 0, -1, .5).sorter == "none"
    # blocks 0 .. 129 are 130 blocks: the first row's words 1 .. 128 are preloaded, word 129 is the tail
    assert mc.det_route(12264, 9, 129 * 64, -1, .5, force_suppress=True).scan_tail is False
    assert mc.det_route(12264, 9, 129 * 64 + 1, -1, .5, force_suppress=True).scan_tail is True
    assert mc.det_route(12264, 9, 9000, -1, .5).scan_tail is None
    assert mc.det_route(12264, 9, 9000, -1, .5, segment=(63, 129 * 64 + 1)).scan_tail is True


def oracle_valid(out):
    """valid rows per sample of an oracle output: the rows it wrote (empty rows are -1 throughout, a score never is)"""
    return (out[:, :, 1] != -1).sum(axis=1)


def suppressed(out):
    return ((out[:, :, 0] == -1) & (out[:, :, 1] != -1)).sum(axis=1)


@pytest.mark.parametrize("name,cid,Vs", [("ladderA", "A-topk-1", mc.LADDER_A), ("ladderB", "B-topk-1", mc.LADDER_B),
                                         ("ladderC", "C-topk-1-force0", mc.LADDER_C)])
def test_ladders_have_exactly_the_valid_rows(name, cid, Vs):
    _, prob, _ = mc.det_inputs(name)
    assert oracle_valid(mc.det_expected(cid)).tolist() == list(Vs)
    assert mc.valid_counts(prob, 0.01).tolist() == list(Vs)


@pytest.mark.parametrize("cid", ["E-offrange-topk-1", "E-threshold-edge", "F-257classes-topk-1", "F-299classes-topk-1",
                                 "H-wild-clip0-force0", "C-299classes"])
def test_valid_count_model_agrees_with_the_oracle(cid):
    """det_case_routes takes V from mc.valid_counts: NaN, -0, inf and the threshold edge included"""
    name, kw = mc.DET_EDGE_CASES[cid]
    _, prob, _ = mc.det_inputs(name)
    assert mc.valid_counts(prob, kw.get("threshold", 0.01)).tolist() == oracle_valid(mc.det_expected(cid)).tolist()


def test_wide_anchor_table_is_one_past_the_lds_capacity():
    assert mc.wide_anchors_16385().shape == (1, mc.K_LDS_KEY_CAP + 1, 4)


# ---- D: ties at the cut
def compacted_scores(prob):
    return prob[1:].max(axis=0)          # (every row of the tie inputs is valid)


@pytest.mark.parametrize("k", [400, 1024, 2500])
def test_tie_levels_cut_inside_a_run_across_strides(k):
    _, prob, _ = mc.det_inputs("tiesLevels")
    assert mc.valid_counts(prob, 0.01).tolist() == [6132, 6132]
    assert mc.det_route(6132, 9, 6132, k, .5).select
    for b in range(prob.shape[0]):
        s = compacted_scores(prob[b])
        T, nless, kk, ties = mc.cut_of(s, k)
        assert 0 < kk < ties and nless > 0
        stride = np.arange(len(s)) // mc.K_TB
        touched = np.unique(stride[s == T])
        assert len(touched) >= 2
        # the first kk members of the run are not all in one stride either: `taken` is carried over
        assert len(np.unique(stride[np.flatnonzero(s == T)[:kk]])) >= 2
        for st in touched:
            assert (s[stride == st] > T).any()


def test_tie_levels_cut_at_the_end_of_a_run():
    _, prob, _ = mc.det_inputs("tiesLevels")
    k = mc.DET_EDGE_CASES["D-levels-cut-at-run-end"][1]["nms_topk"]
    assert mc.det_route(6132, 9, 6132, k, .5).select
    for b in range(prob.shape[0]):
        T, nless, kk, ties = mc.cut_of(compacted_scores(prob[b]), k)
        assert kk == ties >= 2 and nless > 0


def test_all_equal_scores_cut_inside_the_only_run():
    _, prob, _ = mc.det_inputs("tiesAll")
    T, nless, kk, ties = mc.cut_of(compacted_scores(prob[0]), 400)
    assert (nless, kk, ties) == (0, 400, 6132)


# ---- E: scores outside softmax's range
def test_offrange_scores_keep_negative_rows_and_special_values():
    _, prob, _ = mc.det_inputs("offrange")
    for cid in ("E-offrange-topk100", "E-offrange-topk-1"):
        out = mc.det_expected(cid)
        kept = out[:, :, 0] >= 0
        assert (kept & (out[:, :, 1] < 0)).sum(axis=1).min() >= 10
        score = out[:, :, 1]
        assert np.isinf(score[0]).sum() == 1 and not np.isnan(score).any()
        bits = np.ascontiguousarray(score).view(np.uint32)
        assert (bits == 0x80000000).sum() >= 10 and ((bits == 0) & (out[:, :, 2] != -1)).sum() >= 10      # -0 and +0 rows
        if cid.endswith("topk-1"):      # (under nms_topk 100 the sorted head overwrites rows 10 .. 12, where they entered)
            assert ((score != 0) & (np.abs(score) < 1.17e-38)).sum() == 3                                  # the denormals
    A = prob.shape[2]
    assert oracle_valid(mc.det_expected("E-offrange-topk-1")).tolist() == [A, A - 1]       # the all-NaN anchor is no row


def test_threshold_edge_keeps_the_equal_score_and_drops_the_one_below():
    score = mc.det_expected("E-threshold-edge")[0, :, 1]
    assert (score == np.float32(0.25)).sum() == 1
    assert (score == np.nextafter(np.float32(0.25), np.float32(0))).sum() == 0
    assert score[score != -1].min() == np.float32(0.25)


# ---- F: class grouping
@pytest.mark.parametrize("cid", ["F-299classes-topk-1", "F-299classes-topk400", "C-299classes", "C-299classes-topk-1"])
def test_skewed_classes_fill_long_segments(cid):
    out = mc.det_expected(cid)
    assert suppressed(out).min() >= 100
    name, kw = mc.DET_EDGE_CASES[cid]
    prob = mc.det_inputs(name)[1]
    for b in range(out.shape[0]):
        ids = prob[b, 1:].argmax(axis=0)[prob[b, 1:].max(axis=0) >= 0.01]      # class id (0-based) of each valid row
        counts = np.bincount(ids, minlength=299)
        assert counts[298] > 0 and (counts > 64).sum() >= 3
        assert (counts[[c - 1 for c in mc.BOOSTED]] > 128).all()               # the boosted segments span tile boundaries


@pytest.mark.parametrize("n", [256, 257])
def test_class_table_edge_has_the_last_class(n):
    prob = mc.det_inputs(f"cls{n}")[1]
    assert prob.shape[1] == n + 1
    assert mc.valid_counts(prob, 0.01).min() > 64


# ---- G: IoU at the threshold
def pair_outcome(out, n):
    """rows n .. 2n-1 of the oracle's output are the small boxes in pair order (score 0.8 behind the 0.9 of the big ones)"""
    assert (out[0, :n, 1] == np.float32(0.9)).all() and (out[0, n:, 1] == np.float32(0.8)).all()
    assert (out[0, :n, 0] == 0).all()
    return out[0, n:, 0] == -1


@pytest.mark.parametrize("idx", range(len(mc.PAIR_THRESHOLDS)))
@pytest.mark.parametrize("force", [0, 1])
def test_threshold_pairs_need_the_division_on_both_sides(idx, force):
    t = mc.PAIR_THRESHOLDS[idx]
    anc, _, _ = mc.det_inputs(f"pairs{idx}")
    n = anc.shape[1] // 2
    assert n == 97
    out = mc.det_expected(f"G-pairs-t{idx}-force{force}")
    # the decode is exact: the rows are the anchors, bit for bit (big boxes first, each group in pair order)
    rows = np.concatenate([anc[0, 0::2], anc[0, 1::2]])
    np.testing.assert_array_equal(out[0, :, 2:6].view(np.uint32), rows.view(np.uint32))
    gone = pair_outcome(out, n)
    undecided, i, u = mc.pair_decisions(anc, t)
    assert (undecided & gone).sum() >= 8 and (undecided & ~gone).sum() >= 8
    assert gone[0] and not gone[-1]                  # (H ascends: IoU falls from above the threshold to below it)
    # what the kernel concludes without dividing agrees with the oracle's division
    t32, eps = np.float32(t), np.float32(2.0 ** -20)
    assert gone[i >= t32 * (np.float32(1) + eps) * u].all() and not gone[i <= t32 * (np.float32(1) - eps) * u].any()


@pytest.mark.parametrize("scale,lo,hi", [("1e-16", 1e-33, 1e-30), ("1e-20", 1e-45, 1.17e-38), ("1e-23", 0.0, 0.0)])
def test_scaled_pairs_have_tiny_denormal_and_vanishing_areas(scale, lo, hi):
    anc, _, _ = mc.det_inputs(f"pairs0s{scale}")
    _, i, u = mc.pair_decisions(anc, 0.5)
    assert (u >= np.float32(lo)).all() and (u <= np.float32(hi)).all()
    gone = mc.det_expected(f"G-pairs-scale{scale}")[0, 97:, 0] == -1
    if hi == 0.0:
        assert not gone.any()                        # u <= 0: no suppression at all
    else:
        assert gone.any() and not gone.all()


def test_border_collapse_has_zero_area_rows():
    out = mc.det_expected("G-border-collapse")[0]
    zero_area = (out[:, 2] == 1) & (out[:, 4] == 1)
    assert zero_area.sum() == 32 and (out[zero_area, 0] == 0).all()      # collapsed boxes suppress nothing, nor are they
    assert suppressed(out[None])[0] >= 10


# ---- H: non-finite and huge coordinates
def test_wild_locs_decode_to_non_finite_and_huge_rows():
    out = mc.det_expected("H-wild-clip0-force0")
    assert oracle_valid(out).min() > 6000
    bad = (~np.isfinite(out[:, :, 2:])).any(axis=2).sum(axis=1)
    assert bad[0] >= 20 and bad[1] == 1 and bad[2] == 0
    with np.errstate(invalid="ignore"):
        huge = (np.isfinite(out[0, :, 2:6]) & (np.abs(out[0, :, 2:6]) > 1e15)).any(axis=1)
    assert huge.sum() >= 2
    assert np.isnan(out[0]).any() and np.isinf(out[0]).any()


# ---- I: expf
def test_expf_probe_covers_both_cut_offs_and_the_denormals():
    out = mc.det_expected("I-expf")[0]
    x = mc.expf_probe_inputs()[3]
    assert out.shape[0] == len(x) and 6000 <= len(x) <= 6200
    assert (out[:, 0] == 0).all()                    # NMS off: every row, in anchor order
    e = out[:, 4]
    assert np.isinf(e).sum() >= 1000 and (e == 0).sum() >= 50 and np.isnan(e).sum() == 1
    assert ((e != 0) & (np.abs(e) < 1.17e-38)).sum() >= 1000
    # the finite, not-overflowing part is libm's expf itself
    mid = np.abs(x) <= 1
    np.testing.assert_allclose(e[mid], np.exp(x[mid].astype(np.float64)), rtol=2e-7)
    np.testing.assert_array_equal(out[:, 5].view(np.uint32), np.ascontiguousarray(e[::-1]).view(np.uint32))
