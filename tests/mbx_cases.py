"""Shared builders for multibox test cases (numpy only)."""
import collections
import functools

import numpy as np

from dspnet_amd import synthetic
from oracle import multibox as om

# resnet-50 preset after the [1:] slice (symbol/multitask_symbol_factory.py:68-81,
# symbol/multitask_symbol_builder.py:503-508)
R50_SIZES = [[.1, .141], [.2, .272], [.37, .447], [.54, .619], [.71, .79], [.88, .961]]
R50_RATIOS = [[1, 2, .5], [1, 2, .5, 3, 1. / 3], [1, 2, .5, 3, 1. / 3], [1, 2, .5, 3, 1. / 3],
              [1, 2, .5], [1, 2, .5]]


def r50_maps(height, width):
    maps = []
    for s in (16, 32):
        maps.append((height // s, width // s))
    h, w = maps[-1]
    for _ in range(4):  # 3x3 stride-2 pad-1 extras
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        maps.append((h, w))
    return maps


def r50_anchors(height=512, width=512):
    parts = [om.multibox_prior(h, w, s, r)
             for (h, w), s, r in zip(r50_maps(height, width), R50_SIZES, R50_RATIOS)]
    return np.concatenate(parts, axis=1)


def small_anchors(h=4, w=5):
    return np.concatenate([om.multibox_prior(h, w, [.2, .3], [1, 2, .5]),
                           om.multibox_prior(2, 2, [.5, .7], [1, 2])], axis=1)


def target_inputs(anchors, batch, num_labels=200, num_classes=8, max_gt=40, seed=233,
                  pred_scale=1.0):
    gen = synthetic.rng(seed)
    lab = synthetic.det_labels(batch, num_labels, num_classes, max_gt, gen=gen)
    A = anchors.shape[1]
    cls_pred = (gen.standard_normal((batch, num_classes + 1, A)) * pred_scale).astype(np.float32)
    return lab, cls_pred


def detection_inputs(anchors, batch, num_classes=8, seed=7, peaky=True):
    gen = synthetic.rng(seed)
    A = anchors.shape[1]
    logits = gen.standard_normal((batch, num_classes + 1, A)).astype(np.float32)
    if peaky:  # make background dominant for most anchors, like a trained net
        logits[:, 0, :] += 3.0
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    loc = (gen.standard_normal((batch, A * 5)) * 0.5).astype(np.float32)
    return prob, loc


def assert_target_equal(got, exp):
    """[loc_target, loc_mask, cls_target]: masks / classes / which anchors are positive must be
    bit-exact; so must dx, dy and dist.  The two log() columns depend on libm's logf (0.818 ulp,
    not reproducible off-host): 1-ulp tolerance there."""
    lt_g, lm_g, ct_g = [np.asarray(x) for x in got]
    lt_e, lm_e, ct_e = [np.asarray(x) for x in exp]
    np.testing.assert_array_equal(ct_g, ct_e)
    np.testing.assert_array_equal(lm_g, lm_e)
    B = lt_g.shape[0]
    g5, e5 = lt_g.reshape(B, -1, 5), lt_e.reshape(B, -1, 5)
    np.testing.assert_array_equal(g5[..., [0, 1, 4]], e5[..., [0, 1, 4]])
    np.testing.assert_allclose(g5[..., 2:4], e5[..., 2:4], rtol=2.5e-7, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------------
# MultiBoxDetection: a model of the operator's dispatch, and the edge cases of tests/test_multibox_edges_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
# Copies of the constants the routes depend on (dspnet_amd/csrc/multibox.hip).  A change there has to be repeated here: the
# coverage test (test_mbx_cases_host.py) then shows whether the cases still reach every route.
K_TB = 1024                  # kTB: threads of det_decode_sort_kernel, the stride of its compaction and of the tie scan
K_LDS_KEY_CAP = 16384        # kLdsKeyCap (det_layout): most keys held in LDS; above, det_decode_sort_kernel<false>
K_DYN_MAX = 140 * 1024       # kDynMax (dspn_multibox_detection_f32): dynamic LDS for the keys plus the selected list
K_COUNT_CLS = 256            # kCountCls: foreground classes the counting sort of the grouping step holds
K_WAVE_SORT_MAX = 1024       # bitonic_sort_keys: `kLds && n2 <= 1024`, the one-wave sort
K_SEGMENT_MIN = 128 * 16     # bitonic_sort_keys: `kLds && n2 >= 128 * kWaves`, per-wave segments of S = n2 / 16 keys
K_SCAN_AHEAD = 8 * 16        # nms_scan_kernel: kScanPre * kScanPhases mask words preloaded per row

DetRoute = collections.namedtuple(
    "DetRoute", "keys select refused sort_n sorter segment grouping group_sort_n scan_tail")


def next_pow2(v):
    n = 1
    while n < v:
        n <<= 1
    return n


def _sorter(keys, n):
    if keys == "global":
        return "workgroup", 0
    if n <= K_WAVE_SORT_MAX:
        return "wave", 0
    assert n >= K_SEGMENT_MIN          # (powers of two: nothing lies between the two rules)
    return "segments", n // 16


def det_route(A, C, V, nms_topk, nms_threshold, force_suppress=False, segment=None):
    """The route one sample with V valid rows takes through dspn_multibox_detection_f32 (A anchors, C scores per anchor
    including the background).  Mirrors the host dispatch and the block-uniform branches of det_decode_sort_kernel:
      keys        lds | global: where the sort keys live
      select      the nms_topk rows are radix-selected ahead of the sort
      refused     why a cut list (nms_topk < V) is NOT selected: half (2 selcap > n2cap), bytes (kDynMax), global; else None
      sort_n      the n2 or n2k actually sorted;  sorter: none | wave | segments | workgroup;  segment: S of `segments`
      grouping    force | count | sort (None without NMS);  group_sort_n: keys of the second sort
      scan_tail   a scan segment of more than 1 + K_SCAN_AHEAD blocks (the words fetched behind the preloaded ones).  Known
                  under force_suppress (one segment, every row) or when `segment` = (first, one past last) grouped position
                  of a class is given; else None."""
    n2cap = next_pow2(A)
    keys = "lds" if n2cap <= K_LDS_KEY_CAP else "global"
    nms = not (nms_threshold <= 0 or nms_threshold > 1)
    if not nms or V < 1:
        return DetRoute(keys, False, None, 0, "none", 0, None, 0, False)
    selcap, refusal = 0, None
    if nms_topk > 0:
        selcap = next_pow2(min(nms_topk, A))
        if keys == "global":
            selcap, refusal = 0, "global"
        elif 2 * selcap > n2cap:
            selcap, refusal = 0, "half"
        elif 8 * (n2cap + selcap) > K_DYN_MAX:
            selcap, refusal = 0, "bytes"
    nkeep = min(V, nms_topk) if nms_topk > 0 else V
    n2, n2k = next_pow2(V), next_pow2(nkeep)
    cut = nkeep < V
    select = keys == "lds" and cut and n2k <= selcap
    sort_n = n2k if select else n2
    sorter, seg = _sorter(keys, sort_n)
    if force_suppress:
        grouping, gsn = "force", 0
    elif C - 1 <= K_COUNT_CLS:
        grouping, gsn = "count", 0
    else:
        grouping, gsn = "sort", n2
    if force_suppress:
        segment = (0, V)
    tail = None
    if segment is not None:
        tail = (((segment[1] - 1) >> 6) + 1) - (segment[0] >> 6) > 1 + K_SCAN_AHEAD
    return DetRoute(keys, select, refusal if cut and not select else None, sort_n, sorter, seg, grouping, gsn, tail)


def valid_counts(prob, threshold):
    """rows that pass the class scan of MultiBoxDetection (multibox_detection.cc:96-106: `t > score` from -1, then
    `score < threshold` drops the row), per sample"""
    with np.errstate(invalid="ignore"):
        fg = np.where(prob[:, 1:] > -1, prob[:, 1:], -np.inf)
        s = fg.max(axis=1) if fg.shape[1] else np.full((prob.shape[0], prob.shape[2]), -np.inf, np.float32)
        return ((s > -1) & ~(s < np.float32(threshold))).sum(axis=1)


def with_valid_rows(prob, Vs, gen):
    """in sample b, the class scores of a random A - Vs[b] anchors times 1e-3: exactly Vs[b] rows pass threshold 0.01 (when
    every row did before)"""
    prob = prob.copy()
    A = prob.shape[2]
    for b, v in enumerate(Vs):
        drop = gen.permutation(A)[:A - v]
        prob[b, 1:, drop] *= np.float32(1e-3)
    return prob


def wide_anchors_16385():
    """one more anchor than kLdsKeyCap: the 512 x 1024 table, then its first 4121 boxes shifted by +0.003"""
    a = r50_anchors(512, 1024)
    return np.concatenate([a, a[:, :4121] + np.float32(0.003)], axis=1)


def skewed_class_inputs(anchors, batch, num_classes, boosted, seed):
    """softmax inputs whose logits of the `boosted` classes are raised by 4: those classes own several hundred rows each,
    the others stay sparse"""
    gen = synthetic.rng(seed)
    A = anchors.shape[1]
    logits = gen.standard_normal((batch, num_classes + 1, A)).astype(np.float32)
    logits[:, list(boosted)] += np.float32(4.0)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    loc = (gen.standard_normal((batch, A * 5)) * 0.5).astype(np.float32)
    return prob, loc


TIE_LEVELS = np.array([0.75, 0.6, 0.45, 0.3, 0.15], np.float32)
TIE_COUNTS = (245, 490, 1226, 1840, 2331)          # rows per level, in every sample (6132 in all)


def tie_level_inputs(anchors, batch, seed):
    """every row valid, its score one of five levels; the populations are the same in every sample, so one nms_topk cuts
    every sample inside (or exactly at the end of) the same run of equal scores"""
    gen = synthetic.rng(seed)
    A = anchors.shape[1]
    assert sum(TIE_COUNTS) == A
    prob = np.full((batch, 9, A), 0.02, np.float32)
    for b in range(batch):
        level = np.repeat(np.arange(5), TIE_COUNTS)[gen.permutation(A)]
        cls = gen.integers(1, 9, A)
        prob[b, cls, np.arange(A)] = TIE_LEVELS[level]
    prob[:, 0] = 1 - prob[:, 1:].sum(axis=1)
    loc = (gen.standard_normal((batch, A * 5)) * 0.5).astype(np.float32)
    return prob, loc


def cut_of(scores, nms_topk):
    """(T, nless, kk, ties) of the nms_topk cut through `scores` (the compacted rows, -0 == +0): the score at the cut, the
    rows above it, the rank of the cut inside the run of rows equal to it, the length of that run"""
    nkeep = min(len(scores), nms_topk)
    T = np.sort(scores)[::-1][nkeep - 1]
    nless, ties = int((scores > T).sum()), int((scores == T).sum())
    return T, nless, nkeep - nless, ties


def offrange_score_inputs(seed=41):
    """class scores no softmax emits (A = 268, 3 foreground classes, for threshold -5): uniform in (-0.99, 1), anchors of
    all -0.0 and of all +0.0, denormals of both signs, one +inf, one anchor of NaNs only and one with a single NaN"""
    gen = synthetic.rng(seed)
    anc = small_anchors(8, 8)
    A = anc.shape[1]
    prob = gen.uniform(-0.99, 1.0, (2, 4, A)).astype(np.float32)
    prob[:, 1:, 3::17] = np.float32(-0.0)
    prob[:, 1:, 5::19] = np.float32(0.0)
    prob[0, 1:, 10:13] = np.float32(-0.5)
    prob[0, 2, 10:13] = np.array([1e-40, -1e-40, 1.4e-45], np.float32)
    prob[0, 2, 40] = np.inf
    prob[1, :, 50] = np.nan
    prob[1, 2, 51] = np.nan
    loc = (gen.standard_normal((2, A * 5)) * 0.5).astype(np.float32)
    return anc, prob, loc


def threshold_edge_inputs():
    """the inputs above with two anchors whose best score is exactly 0.25 and one float below: at threshold 0.25 the first
    is kept and the second dropped"""
    anc, prob, loc = offrange_score_inputs()
    prob = prob.copy()
    prob[0, 1:, 100:102] = np.float32(-0.5)
    prob[0, 1, 100] = np.float32(0.25)
    prob[0, 1, 101] = np.nextafter(np.float32(0.25), np.float32(0))
    return anc, prob, loc


PAIR_THRESHOLDS = (0.5, float(np.float32(1) / np.float32(3)), 0.45, 0.7, 0.95)


def threshold_pairs(t, h=0.75, ulps=48, scale=1.0):
    """2 ulps + 1 pairs of nested boxes whose IoU walks across nms_threshold t.  Pair k sits at x offset 4k: a big box
    [x, 0, x + 1, H_k] scoring 0.9 and a small one [x, 0, x + 1, h] scoring 0.8, H_k the float32 neighbours of float32(h / t),
    so IoU = h / H_k.  With loc_pred 0 and clip off the decode returns the anchors bit for bit (scale 1).  scale multiplies
    every coordinate (tiny, denormal and vanishing areas).  One foreground class."""
    t32, h32 = np.float32(t), np.float32(h)
    centre = np.array([h32 / t32], np.float32)
    H = (centre.view(np.int32) + np.arange(-ulps, ulps + 1, dtype=np.int32)).view(np.float32)
    n = len(H)
    x = (4 * np.arange(n)).astype(np.float32)
    anc = np.zeros((1, 2 * n, 4), np.float32)
    anc[0, 0::2] = np.stack([x, np.zeros(n, np.float32), x + 1, H], axis=1)
    anc[0, 1::2] = np.stack([x, np.zeros(n, np.float32), x + 1, np.full(n, h32)], axis=1)
    anc *= np.float32(scale)
    prob = np.empty((1, 2, 2 * n), np.float32)
    prob[0, 1, 0::2], prob[0, 1, 1::2] = 0.9, 0.8
    prob[0, 0] = 1 - prob[0, 1]
    return anc, prob, np.zeros((1, 2 * n * 5), np.float32)


def pair_decisions(anc, t):
    """per pair, in float32 and in the operation order of nms_mask_kernel: (undecided, i, u) -- undecided: neither
    i >= t_hi u nor i <= t_lo u, the pairs whose IoU is divided out"""
    big, small = anc[0, 0::2], anc[0, 1::2]
    zero = np.float32(0)
    w = np.maximum(zero, np.minimum(big[:, 2], small[:, 2]) - np.maximum(big[:, 0], small[:, 0]))
    hh = np.maximum(zero, np.minimum(big[:, 3], small[:, 3]) - np.maximum(big[:, 1], small[:, 1]))
    i = w * hh
    area = lambda r: (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])  # noqa: E731
    u = area(big) + area(small) - i
    t32, eps = np.float32(t), np.float32(2.0 ** -20)
    t_hi, t_lo = t32 * (np.float32(1) + eps), t32 * (np.float32(1) - eps)
    assert i.dtype == np.float32 and u.dtype == np.float32 and isinstance(t_hi, np.float32)
    return ~(i >= t_hi * u) & ~(i <= t_lo * u), i, u


def border_collapse_inputs(seed=19):
    """boxes clip=True collapses onto the right border (zero area: i = 0, u = 0), boxes straddling it and boxes inside, all
    of one class and overlapping"""
    gen = synthetic.rng(seed)
    n = 96
    x1 = np.concatenate([gen.uniform(1.05, 1.3, n // 3), gen.uniform(0.8, 0.95, n // 3), gen.uniform(0.6, 0.7, n // 3)])
    y1 = gen.uniform(0.1, 0.3, n)
    anc = np.stack([x1, y1, x1 + gen.uniform(0.2, 0.3, n), y1 + gen.uniform(0.3, 0.5, n)], axis=1)
    anc = anc[gen.permutation(n)].astype(np.float32)[None]
    prob = np.empty((1, 2, n), np.float32)
    prob[0, 1] = gen.uniform(0.3, 0.9, n)
    prob[0, 0] = 1 - prob[0, 1]
    return anc, prob, np.zeros((1, n * 5), np.float32)


WILD_LOCS = (np.nan, np.inf, -np.inf, 600.0, -600.0, 1e16, -1e16, 3e19, 4.4e3)


def wild_loc_inputs(seed=53):
    """A = 6132, 3 foreground classes: sample 0 has 60 anchors with one loc_pred entry that is NaN, infinite or huge, sample
    1 exactly one +inf, sample 2 none"""
    gen = synthetic.rng(seed)
    anc = r50_anchors(512, 512)
    A = anc.shape[1]
    prob, loc = detection_inputs(anc, batch=3, num_classes=3, seed=seed + 1, peaky=False)
    loc = loc.reshape(3, A, 5).copy()
    rows = gen.permutation(A)[:60]
    k = np.arange(60)          # (5 entries x 9 values: every value meets every entry of a row)
    loc[0, rows, k % 5] = np.array(WILD_LOCS, np.float32)[k % len(WILD_LOCS)]
    loc[1, int(gen.integers(0, A)), 2] = np.inf
    return anc, prob, loc.reshape(3, A * 5)


def expf_probe_inputs():
    """every anchor [-1, -1, 1, 1], loc_pred (0, 0, x, x', .): with variances (.1, .1, 1, 1), clip and NMS off, row[4] of the
    output is expf(x) * 2 / 2 and row[5] expf(x') * 2 / 2 -- expf itself wherever its double does not overflow.  x: the
    arguments around both cut-offs of expf, the denormal results, the common range and the special values; x' the same
    values in reverse order."""
    f = np.float32
    def around(v):
        c = np.array([v], np.float32).view(np.int32)
        return (c + np.arange(-8, 9, dtype=np.int32)).view(np.float32)
    x = np.concatenate([
        np.linspace(-104.5, -87.0, 3000), np.linspace(87.5, 89.5, 2000), np.linspace(-1.0, 1.0, 1000),
        [0.0, -0.0, np.inf, -np.inf, np.nan, 88.0, -88.0],
        around(float.fromhex("0x1.62e42ep6")), around(float.fromhex("-0x1.9fe368p6")), around(88.0), around(-88.0),
    ]).astype(f)
    A = len(x)
    anc = np.tile(np.array([-1, -1, 1, 1], f), (1, A, 1))
    loc = np.zeros((1, A, 5), f)
    loc[0, :, 2], loc[0, :, 3] = x, x[::-1]
    prob = np.full((1, 2, A), 0.5, f)
    return anc, prob, loc.reshape(1, A * 5), x


# ---- the case table: name -> (inputs, keyword arguments).  Inputs are built once per process and shared read-only.
LADDER_A = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 6132)
LADDER_B = (8192, 8193, 12264, 1)
LADDER_C = (0, 1, 1025, 16384, 16385)
BOOSTED = (1, 130, 257, 299)


@functools.lru_cache(maxsize=None)
def det_inputs(name):
    """(anchors, cls_prob, loc_pred) of an input set, read-only"""
    if name == "ladderA":
        anc = r50_anchors(512, 512)
        prob, loc = detection_inputs(anc, len(LADDER_A), num_classes=8, seed=61, peaky=False)
        prob = with_valid_rows(prob, LADDER_A, synthetic.rng(62))
    elif name == "ladderB":
        anc = r50_anchors(512, 1024)
        prob, loc = detection_inputs(anc, len(LADDER_B), num_classes=8, seed=63, peaky=False)
        prob = with_valid_rows(prob, LADDER_B, synthetic.rng(64))
    elif name == "ladderC":
        anc = wide_anchors_16385()
        prob, loc = detection_inputs(anc, len(LADDER_C), num_classes=8, seed=65, peaky=False)
        prob = with_valid_rows(prob, LADDER_C, synthetic.rng(66))
    elif name == "globalC299":
        anc = wide_anchors_16385()
        prob, loc = skewed_class_inputs(anc, 2, 299, BOOSTED, seed=67)
    elif name == "tiesAll":
        anc = r50_anchors(512, 512)
        prob = np.full((2, 9, anc.shape[1]), 1 / 9, np.float32)
        loc = np.zeros((2, anc.shape[1] * 5), np.float32)
    elif name == "tiesLevels":
        anc = r50_anchors(512, 512)
        prob, loc = tie_level_inputs(anc, 2, seed=68)
    elif name == "offrange":
        anc, prob, loc = offrange_score_inputs()
    elif name == "thresholdEdge":
        anc, prob, loc = threshold_edge_inputs()
    elif name in ("cls256", "cls257"):
        anc = small_anchors(8, 8)
        prob, loc = detection_inputs(anc, 2, num_classes=int(name[3:]), seed=69, peaky=False)
    elif name == "cls299":
        anc = r50_anchors(512, 512)
        prob, loc = skewed_class_inputs(anc, 2, 299, BOOSTED, seed=70)
    elif name.startswith("pairs"):          # pairs<index of the threshold>[s<scale>]
        idx, _, scale = name[5:].partition("s")
        anc, prob, loc = threshold_pairs(PAIR_THRESHOLDS[int(idx)], scale=float(scale or 1))
    elif name == "border":
        anc, prob, loc = border_collapse_inputs()
    elif name == "wildLoc":
        anc, prob, loc = wild_loc_inputs()
    elif name == "expf":
        anc, prob, loc, _ = expf_probe_inputs()
    else:
        raise KeyError(name)
    out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (anc, prob, loc))
    for a in out:
        a.setflags(write=False)
    return out


def _det_edge_cases():
    cases = {}

    def add(cid, inputs, **kw):
        assert cid not in cases
        cases[cid] = (inputs, kw)
    for k in (-1, 1, 1024, 1025, 2048, 2049, 4096, 4097):                                   # A
        add(f"A-topk{k}", "ladderA", nms_topk=k)
    for k in (-1, 1025):
        add(f"A-force-topk{k}", "ladderA", nms_topk=k, force_suppress=True)
    for k in (-1, 1024, 1025):                                                              # B
        add(f"B-topk{k}", "ladderB", nms_topk=k)
    for k in (-1, 400):                                                                     # C
        for force in (False, True):
            add(f"C-topk{k}-force{int(force)}", "ladderC", nms_topk=k, force_suppress=force)
    add("C-299classes", "globalC299", nms_topk=400)
    add("C-299classes-topk-1", "globalC299")
    add("D-all-equal-topk400", "tiesAll", nms_topk=400)                                      # D
    for k in (400, 1024, 2500):
        add(f"D-levels-topk{k}", "tiesLevels", nms_topk=k)
    add("D-levels-cut-at-run-end", "tiesLevels", nms_topk=TIE_COUNTS[0] + TIE_COUNTS[1])
    for k in (100, -1):                                                                     # E
        add(f"E-offrange-topk{k}", "offrange", threshold=-5.0, nms_topk=k)
    add("E-threshold-edge", "thresholdEdge", threshold=0.25)
    for n in (256, 257):                                                                    # F
        for k in (100, -1):
            add(f"F-{n}classes-topk{k}", f"cls{n}", nms_topk=k)
    for k in (-1, 400):
        add(f"F-299classes-topk{k}", "cls299", nms_topk=k)
    for idx, t in enumerate(PAIR_THRESHOLDS):                                               # G
        for force in (False, True):
            add(f"G-pairs-t{idx}-force{int(force)}", f"pairs{idx}", clip=False, nms_threshold=t, force_suppress=force)
    for scale in ("1e-16", "1e-20", "1e-23"):
        add(f"G-pairs-scale{scale}", f"pairs0s{scale}", clip=False, nms_threshold=0.5)
    add("G-border-collapse", "border", clip=True, nms_threshold=0.5)
    for clip in (False, True):                                                              # H
        for force in (False, True):
            add(f"H-wild-clip{int(clip)}-force{int(force)}", "wildLoc", clip=clip, force_suppress=force)
    add("I-expf", "expf", clip=False, nms_threshold=-1.0, variances=(.1, .1, 1., 1.))         # I
    return cases


DET_EDGE_CASES = _det_edge_cases()


@functools.lru_cache(maxsize=None)
def det_expected(cid):
    """the CPU oracle's output for a case, computed once per process, read-only"""
    name, kw = DET_EDGE_CASES[cid]
    anc, prob, loc = det_inputs(name)
    out = om.multibox_detection(prob, loc, anc, **kw)
    out.setflags(write=False)
    return out


def det_case_routes(cid):
    """the route of every sample of a case"""
    name, kw = DET_EDGE_CASES[cid]
    anc, prob, _ = det_inputs(name)
    Vs = valid_counts(prob, kw.get("threshold", 0.01))
    return [det_route(anc.shape[1], prob.shape[1], int(v), kw.get("nms_topk", -1), kw.get("nms_threshold", 0.5),
                      kw.get("force_suppress", False)) for v in Vs]
