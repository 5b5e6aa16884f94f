"""Host self-checks of the MultiBoxDetection and MultiBoxTarget edge cases (mbx_cases.DET_EDGE_CASES, TGT_EDGE_CASES): the CPU
oracle alone, no GPU.

A case is only worth its GPU time while it still meets the condition it was built for -- an exact number of valid rows, a cut
inside a run of ties that spans two strides, pairs whose IoU has to be divided out.  These tests state those conditions, and
test_case_set_reaches_every_route keeps the case table from quietly losing a route of the operator."""
import numpy as np
import pytest

import mbx_cases as mc
from oracle import multibox as om

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


# =====================================================================================================================
# MultiBoxTarget: mbx_cases.TGT_EDGE_CASES.  The same two questions: does each case still meet the condition it was built
# for, and does the table reach every value of every field of mbx_cases.target_route on both stores.
# =====================================================================================================================
TGT_IDS = list(mc.TGT_EDGE_CASES)
TGT_EXITS = ("all_negatives", "none", "every_candidate", "short", "radix_all_ties", "radix_tie_scan")
TGT_REQUIRED = {f"{store}:{tag}" for store in ("reg", "global") for tag in
                ("g_zero", "g_full", "g_partial", "bad_terminator", "G>64", "G>256", "G=1024", "greedy", "rounds", "chain>=3",
                 "thr_pos", "tie_strides", "tie_one_stride") + tuple(f"exit:{e}" for e in TGT_EXITS)} | {"reg:at_once"}


def tgt_route_tags(r):
    tags = {"g_zero"} if r.g_zero else {"g_full" if r.g_full else "g_partial"}
    tags |= {t for t, on in (("bad_terminator", r.bad_terminator), ("G>64", r.G > 64), ("G>256", r.G > 256),
                             ("G=1024", r.G == mc.K_MAX_LABELS), ("rounds", r.rounds > 0), ("chain>=3", r.chain >= 3),
                             ("thr_pos", r.thr_pos > 0)) if on}
    if r.match:
        tags.add(r.match)
    if r.exit:
        tags.add(f"exit:{r.exit}")
    if r.exit in ("radix_all_ties", "radix_tie_scan") and r.ties > 1:
        tags.add("tie_strides" if r.tie_strides else "tie_one_stride")
    return {f"{r.store}:{t}" for t in tags}


def test_target_case_set_reaches_every_route():
    reached = set()
    for cid in TGT_IDS:
        for r in mc.tgt_case_routes(cid):
            reached |= tgt_route_tags(r)
    assert TGT_REQUIRED - reached == set()
    assert reached - TGT_REQUIRED == set()


def test_target_route_model_at_the_dispatch_edges():
    """target_route and negative_count against the rules of multibox.hip, worked by hand"""
    anc = mc.grid_anchors(8)
    lab = -np.ones((3, 6), np.float32)
    lab[0] = [1, *anc[2], .5]
    pred = np.zeros((2, 8), np.float32)
    r = mc.target_route(8, 3, lab, pred, anc, negative_mining_ratio=3)       # 3 of 7 equal keys: inside the only run
    assert r[:6] == ("reg", 1, False, False, False, "at_once") and (r.exit, r.T, r.kk, r.ties) == ("radix_tie_scan", 0x3f000000, 3, 7)
    assert mc.target_route(8, 3, lab, pred, anc, negative_mining_ratio=7).exit == "every_candidate"
    assert mc.target_route(8, 3, lab, pred, anc, negative_mining_ratio=0.5).exit == "none"
    assert mc.target_route(8, 3, lab, pred, anc, negative_mining_ratio=-1).exit == "all_negatives"
    assert mc.target_route(8, 3, lab, pred, anc, negative_mining_ratio=7, negative_mining_thresh=1e-9).exit == "every_candidate"
    big = mc.pad_anchors(anc, mc.K_REG_ANCHORS)
    assert mc.target_route(len(big), 3, lab, np.zeros((2, len(big)), np.float32), big).store == "reg"
    big = mc.pad_anchors(anc, mc.K_REG_ANCHORS + 1)
    r = mc.target_route(len(big), 3, lab, np.zeros((2, len(big)), np.float32), big)
    assert (r.store, r.match) == ("global", "greedy")
    # the negative count: the clamp first, in float32
    assert mc.negative_count(3, mc.THIRD, 300) == 1 and mc.negative_count(3, 2.9999998, 300) == 8
    assert mc.negative_count(314, 1e7, 6132) == 6132 - 314                   # (x86's conversion gave INT_MIN: no negatives)
    assert mc.negative_count(1, 2.0 ** 31, 300) == 299 and mc.negative_count(1, 2.0 ** 31 - 128, 300) == 299
    assert mc.negative_count(4, 73.5, 300) == 294 and mc.negative_count(4, 74.0, 300) == 296 and mc.negative_count(0, 1e30, 9) == 0


@pytest.mark.parametrize("cid", TGT_IDS)
def test_target_route_model_agrees_with_the_oracle(cid):
    """positives, negatives and return code of every sample, as the route says; the log bar is one value per entry"""
    anc, lab, pred, kw = mc.tgt_inputs(cid)
    (_, _, ct), rc, matched, seconds = mc.tgt_expected(cid)
    A = anc.shape[1]
    print(f"{cid}: oracle {seconds:.3f} s")
    assert seconds < 3.0
    assert mc.ambiguous_log_brackets(anc, lab, matched, kw.get("variances", (0.1, 0.1, 0.2, 0.2))) == 0
    routes = mc.tgt_case_routes(cid)
    assert (rc == -2) == any(r.bad_terminator for r in routes)
    assert (rc == -3) == (any(r.exit == "short" for r in routes) and rc != -2)
    for b, r in enumerate(routes):
        npos = int((matched[b] >= 0).sum())
        bipartite = npos - r.thr_pos
        assert 0 <= bipartite <= r.G
        with np.errstate(invalid="ignore"):
            nneg = int(((ct[b] == 0) & (matched[b] < 0)).sum()) if kw.get("ignore_label", -1.0) != 0 else None
        if r.g_zero:
            assert npos == 0 and (matched[b] < 0).all()
        elif nneg is not None:
            want = mc.negative_count(npos, kw.get("negative_mining_ratio", -1.0), A)
            expect = {"all_negatives": A - npos, "none": 0, "every_candidate": want, "radix_all_ties": want,
                      "radix_tie_scan": want}.get(r.exit)
            if r.exit == "short":
                assert nneg < want
            else:
                assert nneg == expect
        if r.exit == "none":
            assert mc.negative_count(npos, kw["negative_mining_ratio"], A) <= 0


# ---- A: label counts
@pytest.mark.parametrize("G", [1, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_label_count_cases_decide_something_in_the_last_row(G):
    anc, lab, _, _ = mc.tgt_inputs(f"A-G{G}")
    r = mc.tgt_case_routes(f"A-G{G}")[-1]
    matched = mc.tgt_expected(f"A-G{G}")[2][-1]
    assert r.G == G and lab.shape[1] == mc.K_MAX_LABELS
    assert (matched == G - 1).sum() == 1                                   # the last valid row is some anchor's ground truth
    if G >= 63:
        assert (r.match, r.rounds) == ("greedy", 1)                        # the register store runs the greedy loop too
        assert matched[10] == G - 1 and 0 <= matched[11] < G - 1            # the loser recomputed onto anchor 11
    if G > 64:
        assert len(np.unique(matched[matched >= 64] // 64)) >= min((G - 1) // 64, 8)   # picks from several 64-row trips


def test_all_matchable_case_matches_every_row():
    matched = mc.tgt_expected("A-G1024-all-matchable")[2][0]
    assert sorted(matched[matched >= 0].tolist()) == list(range(1024))
    assert mc.tgt_case_routes("A-G1024-all-matchable")[0].match == "at_once"


def test_rows_behind_the_terminator_are_ignored():
    anc, lab, pred, kw = mc.tgt_inputs("A-garbage-behind-terminator")
    G = mc.valid_gt(lab[0])[0]
    assert G == 63 and (lab[0, G + 1:, 0] >= 0).all() and (lab[0, G] == -1).all()
    clean = lab.copy()
    clean[0, G:] = -1
    exp = mc.tgt_expected("A-garbage-behind-terminator")[0]
    for a, b in zip(exp, om.multibox_target(anc, clean, pred, **kw)):
        np.testing.assert_array_equal(a, b)


def test_label_rows_and_mining_ratio_are_refused_as_arguments():
    """L = 1025 and a non-finite negative_mining_ratio: the argument checks, which run ahead of any device work"""
    from dspnet_amd import _lib
    L = _lib.lib()
    var = _lib.floats((.1, .1, .2, .2))

    def call(labels, ratio):
        return L.dspn_multibox_target_f32(None, None, None, 1, 300, labels, 6, 3, 0.5, -1.0, ratio, 0.5, 0, var,
                                          None, None, None, None, 0, None)
    assert call(mc.K_MAX_LABELS + 1, 3.0) != 0 and b"at most 1024 label rows" in L.dspn_last_error()
    assert call(mc.K_MAX_LABELS, 3.0) != 0 and b"null pointer" in L.dspn_last_error()      # 1024 passes that check
    for ratio in (float("inf"), float("-inf"), float("nan")):
        assert call(8, ratio) != 0 and b"negative_mining_ratio must be finite" in L.dspn_last_error()
        anc, lab, pred, _ = mc.tgt_inputs("D-one")
        assert om.multibox_target(anc, lab, pred, negative_mining_ratio=ratio, return_code=True)[1] == -1


# ---- B: the IoU cuts
def cut_distances(cid, t):
    """per (anchor, its ground truth): distance of the IoU from t in floats, for the anchors within 8 floats of it"""
    anc, lab, _, _ = mc.tgt_inputs(cid)
    G = mc.valid_gt(lab[0])[0]
    iou = mc.target_iou_f32(anc[0], lab[0, :G, 1:5])
    with np.errstate(invalid="ignore"):
        j, k = np.nonzero((iou > 0) & (iou < 1))
    d = mc.bits_from(iou[j, k], t)
    near = np.abs(d) <= 8
    return j[near], d[near]


@pytest.mark.parametrize("i,t", list(enumerate((0.5, mc.THIRD, 0.7))))
def test_overlap_cut_cases_walk_across_the_threshold(i, t):
    j, d = cut_distances(f"B-overlap-t{i}", t)
    assert set(range(-mc.WALK, mc.WALK + 1)) <= set(d.tolist())
    ct = mc.tgt_expected(f"B-overlap-t{i}")[0][2][0]
    assert (ct[j[d > 0]] > 0).all() and (ct[j[d <= 0]] == 0).all()         # strictly above: positive; equal: not
    assert (d == 0).sum() >= 1


@pytest.mark.parametrize("i,t,thr", [(0, 0.5, 0.7), (1, 0.3, 0.7), (2, 0.5, 0.5)])
def test_mining_cut_cases_walk_across_the_threshold_and_leave_limbo(i, t, thr):
    j, d = cut_distances(f"B-mining-t{i}", t)
    assert set(range(-mc.WALK, mc.WALK + 1)) <= set(d.tolist())
    (_, _, ct), rc, _, _ = mc.tgt_expected(f"B-mining-t{i}")
    ct = ct[0]
    if thr > t:
        assert (ct[j[d < 0]] == 0).all() and (ct[j[d >= 0]] == -1).all()   # strictly below: candidate; equal: limbo
    else:                       # one threshold for both: above it positive, at it limbo, below it negative
        assert (ct[j[d < 0]] == 0).all() and (ct[j[d == 0]] == -1).all() and (ct[j[d > 0]] > 0).all()
    assert (d == 0).sum() >= 1 and (ct == -1).sum() >= 3 and rc == -3      # the limbo anchors exist: fewer candidates than asked


def test_match_cut_case_walks_across_1e_6():
    j, d = cut_distances("B-match-cut", mc.K_MATCH_CUT)
    assert set(range(-mc.WALK, mc.WALK + 1)) <= set(d.tolist())
    ct = mc.tgt_expected("B-match-cut")[0][2][0]
    assert (ct[j[d > 0]] > 0).all() and (ct[j[d <= 0]] == 0).all()


def test_skipped_threshold_stage_and_wild_boxes():
    outs = [mc.tgt_expected(f"B-threshold-{n}")[0] for n in ("zero", "minus-zero", "negative")]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a, b)
    assert all(r.thr_pos == 0 for n in ("zero", "minus-zero", "negative") for r in mc.tgt_case_routes(f"B-threshold-{n}"))
    anc, lab, _, _ = mc.tgt_inputs("B-wild")
    iou = mc.target_iou_f32(anc[0], lab[0, :mc.valid_gt(lab[0])[0], 1:5])
    bits = iou.view(np.uint32)
    assert np.isnan(iou).any() and (bits == 0x80000000).any() and (bits == 0).any()
    with np.errstate(invalid="ignore"):
        assert ((iou > 0) & (iou < 1e-30)).sum() == 1                      # 2^-120: enters the column maxima, never matched
    a, g = anc[0, 50], lab[0, 2, 1:5]
    assert (a == g).all() and a[0] == a[2] and iou[50, 2] == 0             # union 0
    for cid in ("B-wild", "B-wild-all-negatives"):
        assert [int((m >= 0).sum()) for m in mc.tgt_expected(cid)[2]] == [2, 2]


# ---- C: matching order
def test_equal_ious_go_to_the_lower_anchor_then_the_lower_ground_truth():
    matched = mc.tgt_expected("C-equal")[2][0]
    assert (matched[20], matched[100], matched[200]) == (0, 1, 0)          # 200: threshold stage, first of two equal rows
    assert (matched[30], matched[40]) == (3, 2) and (matched >= 0).sum() == 5
    r = mc.tgt_case_routes("C-equal")[0]
    assert (r.rounds, r.thr_pos) == (1, 1)


@pytest.mark.parametrize("cid,n", [("C-identical70", 70), ("C-identical300", 300), ("C-identical70-global", 70)])
def test_identical_boxes_take_the_anchors_in_order(cid, n):
    matched = mc.tgt_expected(cid)[2][0]
    assert matched[:n].tolist() == list(range(n)) and (matched[n:] < 0).all()
    r = mc.tgt_case_routes(cid)[0]
    assert (r.match, r.rounds) == ("greedy", n - 1) and n > 64


@pytest.mark.parametrize("cid", ["C-chain", "C-chain-global"])
def test_chain_case_has_depth_three(cid):
    r = mc.tgt_case_routes(cid)[0]
    assert (r.match, r.rounds, r.chain) == ("greedy", 9, 3)
    matched = mc.tgt_expected(cid)[2][0]
    for c in range(3):                                                     # a0 a1 a2 to the better ones, a3 to the loser
        assert matched[4 * c:4 * c + 4].tolist() == [4 * c + 1, 4 * c + 2, 4 * c + 3, 4 * c]


def test_sub_cut_ground_truths_share_a_best_anchor_with_a_matchable_one():
    anc, lab, _, _ = mc.tgt_inputs("C-subcut")
    iou = mc.target_iou_f32(anc[0], lab[0, :6, 1:5])
    for k in (0, 2, 4):
        assert 0 < iou[:, k].max() <= mc.K_MATCH_CUT and iou[:, k].argmax() == iou[:, k + 1].argmax()
        assert iou[:, k + 1].max() > 0.5
    reg, glob = mc.tgt_case_routes("C-subcut")[0], mc.tgt_case_routes("C-subcut-global")[0]
    assert reg.match == "at_once" and (glob.match, glob.rounds >= 1) == ("greedy", True)
    a, b = mc.tgt_expected("C-subcut")[0], mc.tgt_expected("C-subcut-global")[0]
    np.testing.assert_array_equal(a[2][0, :300] > 0, b[2][0, :300] > 0)
    assert (mc.tgt_expected("C-subcut")[2][0] >= 0).sum() == 3


# ---- D: the negative count
@pytest.mark.parametrize("cid,nneg,exit_", [
    ("D-third-of-3", 1, "radix_all_ties"), ("D-below-3", 2, "radix_all_ties"), ("D-below-9", 8, "radix_all_ties"),
    ("D-none", 0, "none"), ("D-one", 1, "radix_all_ties"), ("D-candidates-1", 289, "radix_all_ties"),
    ("D-candidates+0", 290, "every_candidate"), ("D-candidates+1", 290, "short"), ("D-above-all", 296, "every_candidate"),
    ("D-product-2p31-minus-128", 299, "every_candidate"), ("D-product-2p31", 299, "every_candidate"),
    ("D-product-3e9", 100, "every_candidate"), ("D-product-2p31-global", 8189, "short")])
def test_negative_count_cases(cid, nneg, exit_):
    (_, _, ct), rc, _, _ = mc.tgt_expected(cid)
    assert int((ct == 0).sum()) == nneg and mc.tgt_case_routes(cid)[0].exit == exit_
    assert rc == (-3 if exit_ == "short" else 0)


def test_large_products_are_the_out_of_range_ones():
    f = np.float32
    assert float(f(1) * f(2.0 ** 31 - 128)) == 2.0 ** 31 - 128 and float(f(1) * f(2.0 ** 31)) == 2.0 ** 31
    assert float(f(300) * f(1e7)) > 2.0 ** 31
    assert float(f(3) * f(mc.THIRD)) == 1.0 and float(f(3) * f(2.9999998)) < 9.0


# ---- E: the radix select
def candidate_keys(cid):
    anc, lab, pred, _ = mc.tgt_inputs(cid)
    matched = mc.tgt_expected(cid)[2][0]
    keys = om.bg_prob(pred)[0].view(np.uint32)
    return keys, matched < 0


@pytest.mark.parametrize("b", range(4))
def test_digit_cases_differ_in_one_byte_and_cut_in_its_first_and_last_bin(b):
    pk, _ = mc.digit_keys(b)
    assert len(pk) >= (150 if b < 3 else 48)
    assert len(np.unique(pk.astype(np.uint64) >> np.uint64(8 * (b + 1)))) == 1          # the bytes above are shared
    digit = (pk >> np.uint32(8 * b)) & 255
    assert len(np.unique(digit)) == len(pk) and digit.min() == 0                       # one key per bin, bin 0x00 among them
    for cut, want in (("first", pk.min()), ("mid", np.sort(pk)[len(pk) // 2 - 1]), ("last", pk.max())):
        r = mc.tgt_case_routes(f"E-byte{b}-{cut}")[0]
        assert (r.exit, r.T, r.kk, r.ties) == ("radix_all_ties", int(want), 1, 1)
        keys, cand = candidate_keys(f"E-byte{b}-{cut}")
        assert np.isin(pk, keys[cand]).all() and (keys[cand & ~np.isin(keys, pk)] == 0x3f800000).all()
    if b == 0:
        assert (np.diff(np.sort(pk)) == 1).mean() > 0.9                    # consecutive logits gave consecutive keys


@pytest.mark.parametrize("run", [1500, 2100])
def test_tie_cases_cut_the_run_where_they_say(run):
    for kk in (1, 1023, 1024, 1025, run - 1, run):
        r = mc.tgt_case_routes(f"E-ties{run}-kk{kk}")[0]
        assert (r.exit, r.T, r.kk, r.ties) == ("radix_all_ties" if kk == run else "radix_tie_scan", 0x3f000000, kk, run)
        assert r.tie_strides
    keys, cand = candidate_keys(f"E-ties{run}-kk1")
    members = np.flatnonzero(cand & (keys == 0x3f000000))
    assert len(members) == run and set((members // mc.K_TB).tolist()) == {0, 1, 2}
    assert (members >= 2048 + 64).any() and members[-1] == 2149             # in the last, partial wave; the last anchor
    assert int((keys[cand] < 0x3f000000).sum()) == mc.TIE_BELOW
    # the kk-th member of the run lies in the second stride for 1023 .. 1025: `taken` is carried across a stride
    assert members[1022] // mc.K_TB >= 1 or members[1024] // mc.K_TB >= 1
    r = mc.tgt_case_routes("E-ties1500-kk1025-global")[0]
    assert (r.store, r.exit, r.kk, r.ties) == ("global", "radix_tie_scan", 1025, 1500)


def test_flat_key_cases_cut_at_zero_at_one_and_among_denormals():
    r = mc.tgt_case_routes("E-zeros")[0]
    assert (r.exit, r.T, r.kk, r.ties, r.tie_strides) == ("radix_tie_scan", 0, 700, 1500, True)
    _, _, pred, _ = mc.tgt_inputs("E-zeros")
    assert np.isneginf(pred[0, 0]).sum() == 750 and (pred[0, 1] == 200).sum() == 750 and np.isfinite(pred[0, 1]).all()
    r = mc.tgt_case_routes("E-zeros-all")[0]
    assert (r.exit, r.T, r.kk, r.ties) == ("radix_all_ties", 0, 1500, 1500)
    r = mc.tgt_case_routes("E-ones")[0]
    assert (r.exit, r.T, r.ties) == ("radix_tie_scan", 0x3f800000, 1500) and 0 < r.kk < 1500
    r = mc.tgt_case_routes("E-denormal")[0]
    assert r.exit.startswith("radix") and 0 < r.T < 0x00800000
    keys, cand = candidate_keys("E-denormal")
    assert (keys[cand] < 0x00800000).all() and len(np.unique(keys[cand])) > 1000
    for cid in TGT_IDS:                                                    # +inf and NaN logits are excluded: NaN keys
        p = mc.tgt_inputs(cid)[2]
        assert not np.isnan(p).any() and not np.isposinf(p).any()


# ---- F: the encode
def test_encode_cases_hold_every_quotient_in_both_columns():
    anc, lab, _, _ = mc.tgt_inputs("F-variances1")
    matched = mc.tgt_expected("F-variances1")[2]
    _, q = mc.log_columns(anc, lab, matched)
    n = len(mc.ENCODE_QUOTIENTS)
    assert len(q) == 2 * n
    for col in (0, 1):
        assert set(np.array(mc.ENCODE_QUOTIENTS).view(np.uint32).tolist()) <= set(np.ascontiguousarray(q[:, col]).view(np.uint32).tolist())
    assert mc.ENCODE_QUOTIENTS[1] == np.nextafter(np.float32(1), np.float32(2)) and min(mc.ENCODE_QUOTIENTS) > mc.K_MATCH_CUT
    ct = mc.tgt_expected("F-variances1")[0][2][0]
    assert (ct == 2.0 ** 24).sum() >= 4 and ((ct == -1) & (matched[0] >= 0)).sum() >= 4 and ((ct == 1) & (matched[0] >= 0)).sum() >= 4
    lt = mc.tgt_expected("F-variances3")[0][0]                              # variance 0
    assert np.isnan(lt).sum() >= 10 and np.isposinf(lt).sum() >= 10 and np.isneginf(lt).sum() >= 10
    lt = mc.tgt_expected("F-variances2")[0][0]                              # a denormal variance: overflow, not NaN
    assert np.isinf(lt).sum() >= 20
    ct = mc.tgt_expected("F-ignore-nan")[0][2][0]
    assert np.isnan(ct).sum() == len(ct) - 60
    ct = mc.tgt_expected("F-ignore-minus-zero")[0][2][0]
    assert (ct.view(np.uint32) == 0x80000000).sum() == len(ct) - 60


def test_log_bar_catches_a_one_ulp_error_and_passes_the_rounded_double():
    """the bar of the two log columns, on the CPU: the correctly rounded result passes, its float neighbours do not (glibc's
    logf is such a neighbour for some quotients: the oracle's own column is NOT what the kernel is held to)"""
    anc, lab, _, kw = mc.tgt_inputs("F-variances1")
    exp, _, matched, _ = mc.tgt_expected("F-variances1")
    pos, q = mc.log_columns(anc, lab, matched)
    lo, hi = mc.log_bracket(q, (.1, .1, .2, .2))
    good = exp[0].copy().reshape(1, -1, 5)
    good[0, pos[1], 2:4] = lo
    mc.assert_log_columns(good.reshape(1, -1), anc, lab, matched)
    for step in (-np.inf, np.inf):
        bad = good.copy()
        bad[0, pos[1][3], 2] = np.nextafter(good[0, pos[1][3], 2], np.float32(step))
        with pytest.raises(AssertionError, match="log columns"):
            mc.assert_log_columns(bad.reshape(1, -1), anc, lab, matched)
    bad = good.copy()
    bad[0, -1, 3] = 1e-30                                                   # an anchor that is not positive
    with pytest.raises(AssertionError, match="not positive"):
        mc.assert_log_columns(bad.reshape(1, -1), anc, lab, matched)
