"""Shared builders for multibox test cases (numpy only)."""
import collections
import functools
import time

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


# ---------------------------------------------------------------------------------------------------------------------
# MultiBoxTarget: the log() bar, a model of the operator's dispatch, and the edge cases of tests/test_multibox_edges_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def same_bits_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def log_columns(anchors, labels, matched):
    """(pos, q): pos = the (sample, anchor) indices of the positives, q (npos, 2) the float32 quotients gw / aw and gh / ah
    whose logarithms are columns 2 and 3 of loc_target, formed as encode_loc forms them (- and / only: bit-equal)"""
    pos = np.nonzero(matched >= 0)
    a = anchors.reshape(-1, 4)[pos[1]]
    g = labels[pos[0], matched[pos], 1:5]
    with np.errstate(all="ignore"):
        q = np.stack([(g[:, 2] - g[:, 0]) / (a[:, 2] - a[:, 0]), (g[:, 3] - g[:, 1]) / (a[:, 3] - a[:, 1])], axis=1)
    assert q.dtype == np.float32
    return pos, q


def log_bracket(q, variances):
    """(lo, hi) float32, shaped like q (npos, 2): the ends of the admissible results for log(q) / variance.  The kernel forms
    (float)log((double)q) / v.  l = numpy's float64 log; the true double nearest the device's lies within one float64 ulp of
    the exact value for each of the two libraries, so every x in [l - 2 ulp, l + 2 ulp] is admitted; float32(x) and the
    float32 division are monotone in x, so the admissible results are the floats between the images of the two ends.
    Where lo and hi have equal bits the bar is one value.  q == 1 is the exact case of every log: +0, no bracket."""
    v = np.array(variances[2:4], np.float32)
    with np.errstate(all="ignore"):
        l = np.log(q.astype(np.float64))
        lo, hi = l, l
        for _ in range(2):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        lo, hi = np.where(q == 1, 0.0, lo), np.where(q == 1, 0.0, hi)
        return lo.astype(np.float32) / v, hi.astype(np.float32) / v


def glibc_log_candidates(q, variances):
    """the three float32 results from libm's logf(q) (the oracle's) and its two float neighbours, each divided by the variance"""
    v = np.array(variances[2:4], np.float32)
    l = om.logf(q)
    with np.errstate(all="ignore"):
        return [np.nextafter(l, np.float32(-np.inf)) / v, l / v, np.nextafter(l, np.float32(np.inf)) / v]


def ambiguous_log_brackets(anchors, labels, matched, variances=(0.1, 0.1, 0.2, 0.2)):
    """how many log-column entries of these inputs have a bracket of more than one float (the bar is then not a single
    value); measured 0 of 500 000 sampled quotients"""
    _, q = log_columns(anchors, labels, matched)
    lo, hi = log_bracket(q, variances)
    return int((~same_bits_or_nan(lo, hi)).sum())


def assert_log_columns(loc_target, anchors, labels, matched, variances=(0.1, 0.1, 0.2, 0.2), libm=False):
    """columns 2 and 3 of loc_target (B, A * 5) against the double-precision bracket and against glibc's logf +- 1 ulp; no
    tolerance constant.  Anchors that are not positive must hold +0.
    libm: loc_target is the OUTPUT OF A libm logf (the oracle itself against another reading of the reference): logf is
    within one float of the exact logarithm, so the result is the rounded double or one of its two float neighbours, each
    divided by the variance."""
    B = loc_target.shape[0]
    t = np.asarray(loc_target).reshape(B, -1, 5)[..., 2:4]
    pos, q = log_columns(anchors, labels, matched)
    rest = np.ones(t.shape[:2], bool)
    rest[pos] = False
    assert (t[rest].view(np.uint32) == 0).all(), "log columns of anchors that are not positive must be +0"
    got = t[pos]
    lo, hi = log_bracket(q, variances)
    if libm:
        v = np.array(variances[2:4], np.float32)
        with np.errstate(all="ignore"):
            mid = np.log(q.astype(np.float64)).astype(np.float32)
            near = [np.nextafter(mid, np.float32(-np.inf)) / v, mid / v, np.nextafter(mid, np.float32(np.inf)) / v]
        ok = np.zeros(got.shape, bool)
        for c in near:
            ok |= same_bits_or_nan(got, c)
        assert ok.all(), f"log columns: {int((~ok).sum())} of {ok.size} more than one float from the rounded double"
        return
    ok = same_bits_or_nan(got, lo) | same_bits_or_nan(got, hi)
    with np.errstate(invalid="ignore"):
        ok |= (got > lo) & (got < hi)
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"log columns: {int((~ok).sum())} of {ok.size} outside the float64 bracket; first: sample "
                             f"{pos[0][i[0]]} anchor {pos[1][i[0]]} column {2 + i[1]}: q {q[i]!r} got {got[i]!r} "
                             f"admissible [{lo[i]!r}, {hi[i]!r}]")
    near = np.zeros(got.shape, bool)
    for c in glibc_log_candidates(q, variances):
        near |= same_bits_or_nan(got, c)
    if not near.all():
        i = tuple(np.argwhere(~near)[0])
        raise AssertionError(f"log columns: {int((~near).sum())} of {near.size} more than 1 ulp of logf from glibc's; first: "
                             f"q {q[i]!r} got {got[i]!r}")


def assert_target_equal(got, exp, anchors, labels, matched, variances=(0.1, 0.1, 0.2, 0.2), libm=False):
    """[loc_target, loc_mask, cls_target] against the oracle's.  Masks, classes, which anchors are positive, dx, dy and dist
    are bit-exact.  The two log() columns depend on libm's logf (0.818 ulp, not reproducible off-host); the kernel rounds the
    double logarithm instead, and is held to that: assert_log_columns.  matched: the oracle's ground truth per positive
    (oracle.multibox.multibox_target(return_matched=True))."""
    lt_g, lm_g, ct_g = [np.asarray(x) for x in got]
    lt_e, lm_e, ct_e = [np.asarray(x) for x in exp]
    np.testing.assert_array_equal(ct_g, ct_e)
    np.testing.assert_array_equal(lm_g, lm_e)
    B = lt_g.shape[0]
    g5, e5 = lt_g.reshape(B, -1, 5), lt_e.reshape(B, -1, 5)
    np.testing.assert_array_equal(g5[..., [0, 1, 4]], e5[..., [0, 1, 4]])
    assert_log_columns(lt_g, anchors, labels, matched, variances, libm)


def assert_target_parity(got, anchors, labels, cls_pred, **kw):
    """the operator's outputs against the oracle run on the same inputs; returns the oracle's return code"""
    exp, rc, matched = om.multibox_target(anchors, labels, cls_pred, return_matched=True, **kw)
    assert_target_equal(got, exp, anchors, labels, matched, kw.get("variances", (0.1, 0.1, 0.2, 0.2)))
    return rc


# Copies of the constants the routes of MultiBoxTarget depend on (dspnet_amd/csrc/multibox.hip).  A change there has to be
# repeated here: the coverage test (test_mbx_cases_host.py) then shows whether the cases still reach every route.
K_MAX_LABELS = 1024               # kMaxLabels: label rows per sample that target_rows_kernel / MatchLds hold
K_REG_ANCHORS = 8 * K_TB          # dspn_multibox_target_f32: num_anchors <= 8 * kTB takes target_match_reg_kernel<8>
K_MATCH_CUT = np.float32(1e-6)    # target_match_body: `iou > 1e-6f`, the bipartite stage's cut
K_NO_ANCHOR = 0x7fffffff          # the column maximum of a ground truth no anchor overlaps

TgtRoute = collections.namedtuple(
    "TgtRoute", "store G g_zero g_full bad_terminator match rounds chain thr_pos exit T kk ties tie_strides")


def target_iou_f32(anc, gt):
    """(A, 4) x (G, 4) -> (A, G) float32: target_iou of multibox.hip / the oracle, operation for operation (+ - x / and
    comparisons only, `a > b ? a : b` for the extrema: NaN and -0 travel as they do there), so bit-equal"""
    a, g = np.asarray(anc, np.float32)[:, None, :], np.asarray(gt, np.float32)[None, :, :]
    fmax = lambda x, y: np.where(x > y, x, y)          # noqa: E731
    fmin = lambda x, y: np.where(x < y, x, y)          # noqa: E731
    zero = np.float32(0)
    with np.errstate(all="ignore"):
        iw = fmax(zero, fmin(a[..., 2], g[..., 2]) - fmax(a[..., 0], g[..., 0]))
        ih = fmax(zero, fmin(a[..., 3], g[..., 3]) - fmax(a[..., 1], g[..., 1]))
        inter = iw * ih
        uni = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1]) - inter
        out = np.where(uni == zero, zero, inter / uni)
    assert out.dtype == np.float32
    return out


def valid_gt(lab):
    """(G, bad terminator) of one sample's (L, 6) label rows"""
    term = np.flatnonzero(lab[:, 0] == -1)
    G = int(term[0]) if len(term) else len(lab)
    return G, bool(G < len(lab) and (lab[G, 1:5] != -1).any())


def _bipartite_model(iou, reg):
    """the bipartite stage as target_match_body runs it: (match, rounds, chain, positive flags).  rounds: the recomputation
    rounds of the greedy loop (a pick consumed an anchor that was another unmatched ground truth's column maximum); chain:
    the longest run of rounds in which the consumed anchor was itself a recomputed maximum."""
    A, G = iou.shape
    with np.errstate(invalid="ignore"):
        packed = np.where(iou > 0, iou, np.float32(0))         # only IoU > 0 enters the column maxima
    ca, ciou = packed.argmax(axis=0), packed.max(axis=0)       # (argmax: the lowest anchor among equals)
    none = ~(ciou > 0)
    ca, ciou = np.where(none, K_NO_ANCHOR, ca), np.where(none, np.float32(-1), ciou)
    matchable = ciou > K_MATCH_CUT
    flag = np.zeros(A, bool)
    if reg and len(np.unique(ca[matchable])) == matchable.sum():
        flag[ca[matchable]] = True
        return "at_once", 0, 0, flag
    gflag = np.zeros(G, bool)
    rounds, longest, depth = 0, 0, {}
    while True:
        cand = np.flatnonzero(~gflag)
        if not len(cand):
            break
        k = cand[np.lexsort((cand, ca[cand], -ciou[cand]))[0]]           # IoU descending, anchor, ground truth ascending
        if not ciou[k] > K_MATCH_CUT:
            break
        a = int(ca[k])
        flag[a], gflag[k] = True, True
        hit = np.flatnonzero(~gflag & (ca == a))
        if len(hit):
            rounds += 1
            c = 1 + depth.get(a, 0)
            longest = max(longest, c)
            for kk in hit:
                with np.errstate(invalid="ignore"):
                    col = np.where(flag | ~(iou[:, kk] > -1), -np.inf, iou[:, kk])
                j = int(col.argmax())
                ca[kk], ciou[kk] = (j, col[j]) if col[j] > -1 else (K_NO_ANCHOR, np.float32(-1))
                depth[int(ca[kk])] = max(depth.get(int(ca[kk]), 0), c)
    return "greedy", rounds, longest, flag


def negative_count(npos, ratio, A):
    """num_negative of target_match_body: the clamp to A - npos first, in float32, then the conversion"""
    want = np.float32(npos) * np.float32(ratio)
    return A - npos if not want < np.float32(A - npos) else int(want)


def target_route(A, L, labels, cls_pred, anchors=None, overlap_threshold=0.5, negative_mining_ratio=-1.0,
                 negative_mining_thresh=0.5, **_):
    """The route one sample takes through dspn_multibox_target_f32: labels (L, 6), cls_pred (C + 1, A), anchors (A, 4).
      store            reg | global: target_match_reg_kernel<8> or target_match_kernel
      G, g_zero, g_full, bad_terminator
      match            None (G == 0) | at_once | greedy;  rounds, chain: see _bipartite_model
      thr_pos          positives of the threshold stage
      exit             all_negatives | none | every_candidate | short | radix_all_ties | radix_tie_scan (None when G == 0)
      T, kk, ties      of the radix exits: the key at the cut, the rank of the cut in the run of keys equal to it, the run
      tie_strides      the run's members lie in more than one 1024-anchor stride
    The background keys are the oracle's own (oracle.multibox.bg_prob)."""
    assert labels.shape == (L, 6) and cls_pred.shape[1] == A and anchors.shape == (A, 4)
    store = "reg" if A <= K_REG_ANCHORS else "global"
    G, bad = valid_gt(labels)
    if G == 0:
        return TgtRoute(store, 0, True, L == 0, bad, None, 0, 0, 0, None, None, 0, 0, False)
    iou = target_iou_f32(anchors, labels[:G, 1:5])
    match, rounds, chain, flag = _bipartite_model(iou, store == "reg")
    with np.errstate(invalid="ignore"):
        row = np.where(iou > -1, iou, np.float32(-1)).max(axis=1)       # best IoU per anchor, from -1 with a strict `>`
    thr = np.float32(overlap_threshold)
    thr_pos = 0
    if thr > 0:
        more = ~flag & (row > thr)
        thr_pos, flag = int(more.sum()), flag | more
    npos = int(flag.sum())
    head = (store, G, False, G == L, bad, match, rounds, chain, thr_pos)
    if not np.float32(negative_mining_ratio) > 0:
        return TgtRoute(*head, "all_negatives", None, 0, 0, False)
    nneg = negative_count(npos, negative_mining_ratio, A)
    if nneg <= 0:
        return TgtRoute(*head, "none", None, 0, 0, False)
    cand = ~flag & (row < np.float32(negative_mining_thresh))
    ncand = int(cand.sum())
    if ncand < nneg:
        return TgtRoute(*head, "short", None, 0, 0, False)
    if ncand == nneg:
        return TgtRoute(*head, "every_candidate", None, 0, 0, False)
    keys = om.bg_prob(cls_pred[None])[0].view(np.uint32)
    ck = keys[cand]
    T = np.sort(ck)[nneg - 1]
    kk, ties = nneg - int((ck < T).sum()), int((ck == T).sum())
    strides = np.unique(np.flatnonzero(cand & (keys == T)) // K_TB)
    return TgtRoute(*head, "radix_all_ties" if kk == ties else "radix_tie_scan", int(T), kk, ties, len(strides) > 1)


# ---- builders of the MultiBoxTarget edge cases.  Each returns (anchors (1, A, 4), labels (B, L, 6), cls_pred (B, C + 1, A),
# ---- keyword arguments of the operator).  Coordinates are small integers plus short binary fractions wherever a test has
# ---- to know a difference exactly; everything else is judged by the oracle.
def grid_anchors(n, cols=64):
    """n disjoint unit squares [2c, 2r, 2c + 1, 2r + 1], 64 to a row"""
    i = np.arange(n)
    c, r = (i % cols).astype(np.float32), (i // cols).astype(np.float32)
    return np.stack([2 * c, 2 * r, 2 * c + 1, 2 * r + 1], axis=1)


def pad_anchors(anc, total):
    """the anchors followed by zero-area ones far from every box, up to `total` (8193: the global store)"""
    pad = np.full((total - len(anc), 4), -5.0, np.float32)
    return np.concatenate([anc, pad])


def outside_box(k):
    """a ground truth no anchor of this file overlaps"""
    return [k % 5, -100.0 - 2 * k, -100.0, -99.0 - 2 * k, -99.0, 0.1 * (k % 7)]


def _finish(anc, lab, pred, **kw):
    return anc[None].astype(np.float32), np.asarray(lab, np.float32), np.asarray(pred, np.float32), kw


def tgt_label_counts(G, L=1024, A=300, matchable=40, dup=False, garbage=False, bad=False, empty_first=False, ratio=3.0, seed=5):
    """group A: G label rows of L, `matchable` of them on an anchor of their own (spread over the rows, the last row
    included, so the second and later trips of the `k += 64` and `k += 256` loops decide something), the rest outside every
    anchor.  dup: the last two matchable rows share their best anchor, so the register store also takes the greedy loop."""
    gen = synthetic.rng(seed + G)
    n = min(A, 2048)
    anc = pad_anchors(grid_anchors(n), A)
    lab = -np.ones((1, L, 6), np.float32)
    for k in range(G):
        lab[0, k] = outside_box(k)
    rows = np.unique(np.round(np.linspace(0, G - 1, min(G, matchable))).astype(int)) if G else np.array([], int)
    free = np.setdiff1d(np.arange(n), [10, 11, n - 1])
    own = np.concatenate([[n - 1], gen.permutation(free)])[:len(rows)]
    for i, (k, j) in enumerate(zip(rows, own)):
        x, y = anc[j, 0], anc[j, 1]
        lab[0, k] = [i % 7, x, y, x + 1, y + np.float32(0.55 + 0.4 * ((i * 37) % 101) / 101), 0.05 * i]
    if dup:
        x, y = anc[10, 0], anc[10, 1]
        lab[0, rows[-1]] = [3, x, y, x + 1, y + 0.9, 0.3]
        lab[0, rows[-2]] = [4, x, y, x + 2.5, y + 0.8, 0.4]          # loses anchor 10, recomputes onto anchor 11
    if garbage:                                                   # rows behind the terminator: boxes ON anchors, never read
        for k in range(G + 1, L):
            j = int(gen.integers(0, n))
            lab[0, k] = [k % 5, anc[j, 0], anc[j, 1], anc[j, 2], anc[j, 3], 0.5]
    if bad:
        lab[0, G, 2] = 0.25
    if empty_first:
        lab = np.concatenate([-np.ones((1, L, 6), np.float32), lab])
    pred = gen.standard_normal((len(lab), 4, A))
    return _finish(anc, lab, pred, negative_mining_ratio=ratio)


# heights of the group-B ground truths: short binary fractions and full 24-bit mantissas (with the former alone no IoU lands
# one float below 0.5)
CUT_HEIGHTS = tuple(np.float32(h) for h in (0.375, 0.4375, 0.3125, 0.40625)) + tuple(
    synthetic.rng(3).uniform(0.26, 0.47, 10).astype(np.float32))
WALK = 3          # the IoUs walk at least +-3 ulps across each cut


def bits_from(x, t):
    """signed distance in float32 steps from t to x (both positive)"""
    return np.asarray(x, np.float32).view(np.int32).astype(np.int64) - int(np.float32(t).view(np.int32))


def tgt_iou_cuts(t, kind, thr=None, ratio=None):
    """group B.  kind overlap / mining: per height h a ground truth [X, 0, X + 1, h], an anchor equal to it (taken by the
    bipartite stage) and anchors [X, 0, X + 1, H], H the floats around h / t whose IoU with the ground truth lies within
    +-WALK floats of t -- the IoU is computed as the kernel computes it and the anchors are chosen by it.  overlap: t is
    overlap_threshold and every other anchor a negative; mining: t is negative_mining_thresh under overlap_threshold `thr`,
    every candidate is taken, the anchors from t up to thr stay ignored.
    kind match: anchors [X, 0, X + 1, 1] with a ground truth [X, 0, X + 2^-10, h'] inside, IoU within +-WALK floats of 1e-6."""
    ancs, labs = [], []
    if kind == "match":
        centre = np.array([np.float32(1e-6) * 1024], np.float32)
        hs = (centre.view(np.int32) + np.arange(-16, 17, dtype=np.int32)).view(np.float32)
        for i, h in enumerate(hs):
            X = np.float32(4 * i)
            a = np.array([X, 0, X + 1, 1], np.float32)
            g = np.array([X, 0, X + np.float32(2.0 ** -10), h], np.float32)
            if abs(int(bits_from(target_iou_f32(a[None], g[None])[0, 0], K_MATCH_CUT))) <= WALK + 2:
                ancs.append(a)
                labs.append([len(labs) % 5, *g, 0.2])
        kw = dict(overlap_threshold=0.5, negative_mining_ratio=-1.0)
    else:
        t32 = np.float32(t)
        for i, h in enumerate(CUT_HEIGHTS):
            X = np.float32(4 * i)
            g = np.array([X, 0, X + 1, h], np.float32)
            centre = np.array([h / t32], np.float32)
            Hs = (centre.view(np.int32) + np.arange(-24, 25, dtype=np.int32)).view(np.float32)
            cand = np.stack([np.full_like(Hs, X), np.zeros_like(Hs), np.full_like(Hs, X + 1), Hs], axis=1)
            d = bits_from(target_iou_f32(cand, g[None])[:, 0], t32)
            ancs.append(g.copy())
            ancs.extend(cand[np.abs(d) <= WALK])
            labs.append([i % 5, *g, 0.1 * i])
        if kind == "overlap":
            kw = dict(overlap_threshold=t, negative_mining_ratio=-1.0 if ratio is None else ratio)
        else:
            kw = dict(overlap_threshold=thr, negative_mining_thresh=t, negative_mining_ratio=1e4)
    anc = np.concatenate([np.array(ancs, np.float32), grid_anchors(40) + np.float32(1000)])
    gen = synthetic.rng(17)
    anc = anc[gen.permutation(len(anc))]
    lab = -np.ones((1, len(labs) + 3, 6), np.float32)
    lab[0, :len(labs)] = labs
    return _finish(anc, lab, gen.standard_normal((1, 3, len(anc))), **kw)


def tgt_wild(ratio=3.0, thr=0.5):
    """group B: unions of zero, zero-area and inverted boxes on both sides (IoU 0 and -0), an IoU that underflows and one
    that is positive but far below every cut, NaN and infinite label coordinates; two ordinary ground truths beside them"""
    anc = grid_anchors(300)
    x, y = anc[50, 0], anc[50, 1]
    anc[50] = [x, y, x, y]                                   # a point
    anc[51] = [anc[51, 2], anc[51, 3], anc[51, 0], anc[51, 1]]  # inverted on both axes
    anc[52, 2] = anc[52, 0]                                  # zero width
    inf, nan = np.inf, np.nan
    p = anc[0, :2]                                           # the origin: 2^-60 survives the addition
    rows = [
        [0, *anc[3, :2], anc[3, 2], anc[3, 1] + 0.75, 0.3], [1, *anc[70, :2], anc[70, 0] + 0.875, anc[70, 3], 0.6],
        [2, x, y, x, y, 0.1],                                # on the point anchor: union 0
        [3, *anc[5, 2:], *anc[5, :2], 0.1],                  # inverted, over anchor 5
        [4, anc[6, 0], anc[6, 1], anc[6, 0], anc[6, 3], 0.1],  # zero width, on the edge of anchor 6
        [1, anc[8, 0] + 3, anc[8, 1], anc[8, 0], anc[8, 3], 0.1],  # inverted on one axis, area -3: unions below 0, IoU -0
        [0, p[0], p[1], p[0] + 2.0 ** -60, p[1] + 2.0 ** -60, 0.1],   # IoU 2^-120 > 0
        [1, p[0], p[1], p[0] + 2.0 ** -80, p[1] + 2.0 ** -80, 0.1],   # intersection underflows to 0
        [2, nan, 0, 1, 1, 0.1], [2, 0, nan, 1, 1, 0.1], [2, 0, 0, nan, 1, 0.1], [2, 0, 0, 1, nan, 0.1],
        [3, nan, nan, nan, nan, nan],
        [4, 0, 0, inf, inf, 0.1], [4, -inf, -inf, inf, inf, 0.1], [4, inf, inf, inf, inf, 0.1], [4, -inf, 0, 1, 1, 0.1],
        [0, 0, 0, 1, inf, 0.2],
    ]
    lab = -np.ones((2, 24, 6), np.float32)
    lab[0, :len(rows)] = rows
    lab[1, :6] = rows[:6]
    gen = synthetic.rng(23)
    return _finish(anc, lab, gen.standard_normal((2, 3, 300)), negative_mining_ratio=ratio, overlap_threshold=thr)


def tgt_matching(kind, A=0, ratio=3.0):
    """group C (A: pad with zero-area anchors up to A, the global store):
      equal      three identical anchors and two identical ground truths on them, beside two ground truths with one IoU on
                 two different anchors: order is anchor ascending, then ground truth ascending
      identicalN N identical ground truths over a block of anchors with one common IoU: N - 1 recomputation rounds
      chain      per cluster, a ground truth whose maximum is taken three times in a row by a better one: each recomputed
                 maximum lands on the maximum of another unmatched ground truth
      subcut     ground truths with 0 < IoU <= 1e-6 whose best anchor is also a matchable one's"""
    gen = synthetic.rng(29)
    if kind == "equal":
        anc = grid_anchors(300)
        anc[100] = anc[200] = anc[20]
        x, y = anc[20, :2]
        rows = [[1, x, y, x + 1, y + 0.75, 0.1], [2, x, y, x + 1, y + 0.75, 0.2]]
        for j, c in ((40, 3), (30, 4)):                       # equal IoU 0.5 on anchors 40 and 30: 30 is picked first
            rows.append([c, anc[j, 0], anc[j, 1], anc[j, 0] + 0.5, anc[j, 3], 0.3])
    elif kind.startswith("identical"):
        n = int(kind[9:])
        anc = grid_anchors(320)
        rows = [[k % 7, 0, 0, 127, 9, 0.01 * k] for k in range(n)]
    elif kind == "chain":
        unit = np.array([[0, 0, 1, 1], [1, 0, 2, 1], [0, 1, 1, 2], [1, 1, 2, 2]], np.float32)
        anc = np.concatenate([unit + np.float32(8 * c) * np.array([1, 0, 1, 0], np.float32) for c in range(3)]
                             + [grid_anchors(288) + np.float32(100)])
        rows = []
        for c in range(3):
            o = 8.0 * c
            rows += [[0, o + 0.3, 0.4, o + 1.25, 1.2, 0.1],                      # loses a0, a1, a2 in turn, ends on a3
                     [1, o, 0, o + 1, 0.95, 0.2], [2, o + 1, 0, o + 2, 0.9, 0.3], [3, o, 1, o + 1, 1.85, 0.4]]
    elif kind == "subcut":
        anc = grid_anchors(300)
        rows = []
        for j, e in ((17, -11), (90, -12), (299, -13)):
            x, y = anc[j, :2]
            s = 2.0 ** e
            rows += [[1, x + 0.5, y + 0.5, x + 0.5 + s, y + 0.5 + s, 0.1], [2, x, y, x + 1, y + 0.875, 0.2]]
    else:
        raise KeyError(kind)
    if A:
        anc = pad_anchors(anc, A)
    lab = -np.ones((1, max(len(rows) + 2, 8), 6), np.float32)
    lab[0, :len(rows)] = rows
    return _finish(anc, lab, gen.standard_normal((1, 3, len(anc))), negative_mining_ratio=ratio)


def tgt_neg_counts(npos, ratio=None, want=None, limbo=0, A=300):
    """group D: npos ground truths each ON an anchor (IoU 1), `limbo` further anchors at IoU 0.6 (overlap_threshold 0.7,
    negative_mining_thresh 0.5: neither positive nor candidate), every other anchor a candidate.  want: a count relative
    to the candidates (-1, 0, +1), turned into the ratio (want + 0.5) / npos."""
    anc = pad_anchors(grid_anchors(min(A, 400)), A)
    lab = -np.ones((1, npos + 4, 6), np.float32)
    for k in range(npos):
        lab[0, k] = [k % 5, *anc[k], 0.1]
    for i in range(limbo):
        anc[250 + i] = [anc[i % npos, 0], anc[i % npos, 1], anc[i % npos, 2], anc[i % npos, 1] + np.float32(0.6)]
    if want is not None:
        ratio = (A - npos - limbo + want + 0.5) / npos
    gen = synthetic.rng(31)
    return _finish(anc, lab, gen.standard_normal((1, 3, A)), negative_mining_ratio=ratio, overlap_threshold=0.7)


@functools.lru_cache(maxsize=None)
def key_pool():
    """(keys ascending, logit): two-class columns (0, x) and the key -- the bits of the oracle's background probability --
    each gives.  x: 70 000 consecutive floats from 1.0 (consecutive keys, bytes 0 and 1), 200 000 uniform in [-3, 3] (byte
    2), 40 000 from 80 to 104 (tiny and denormal probabilities, and 0 beyond both cut-offs of expf), 12 000 from -20 to 104
    (byte 3: every binade)"""
    gen = synthetic.rng(37)
    run = (np.array([1.0], np.float32).view(np.int32) + np.arange(70000, dtype=np.int32)).view(np.float32)
    x = np.concatenate([run, gen.uniform(-3, 3, 200000), np.linspace(80, 104, 40000), np.linspace(-20, 104, 12000)])
    x = x.astype(np.float32)
    pred = np.zeros((1, 2, len(x)), np.float32)
    pred[0, 1] = x
    keys, first = np.unique(om.bg_prob(pred)[0].view(np.uint32), return_index=True)
    return keys, x[first]


def digit_keys(b, most=200):
    """keys of the pool that share every byte above byte b and differ in byte b, one per value of it -- from the prefix with
    the most values (bin 0x00 among them where the pool has it)"""
    keys, x = key_pool()
    nz = keys > 0
    keys, x = keys[nz], x[nz]
    prefix = (keys.astype(np.uint64) >> np.uint64(8 * (b + 1))).astype(np.int64)
    digit = (keys >> np.uint32(8 * b)) & np.uint32(255)
    _, first = np.unique(prefix * 256 + digit, return_index=True)          # one key per (prefix, digit)
    pk, count = np.unique(prefix[first], return_counts=True)
    score = count + 1000 * np.isin(pk, prefix[first][digit[first] == 0])
    sel = first[prefix[first] == pk[score.argmax()]]
    if len(sel) > most:
        sel = np.concatenate([sel[:most // 2], sel[-(most - most // 2):]])
    return keys[sel], x[sel]


ONE_KEY_LOGIT = np.float32(-200.0)      # expf(-200) == 0: background probability exactly 1, key 0x3f800000
RADIX_POS = (5, 1030, 2050, 2100)       # the four positives of the long tables


def _radix_case(A, x1, x0=None, pos=(0, 100, 200, 299), k=1, pad=0):
    anc = grid_anchors(A)
    lab = -np.ones((1, 6, 6), np.float32)
    for i, j in enumerate(pos):
        lab[0, i] = [i, *anc[j], 0.1 * i]
    if pad:
        anc = pad_anchors(anc, pad)
        x1 = np.concatenate([x1, np.full(pad - A, ONE_KEY_LOGIT)])
        x0 = None if x0 is None else np.concatenate([x0, np.zeros(pad - A, np.float32)])
    pred = np.zeros((1, 2, len(anc)), np.float32)
    pred[0, 1] = x1
    if x0 is not None:
        pred[0, 0] = x0
    return _finish(anc, lab, pred, negative_mining_ratio=(k + 0.5) / len(pos))


def tgt_radix_digit(b, cut, pad=0):
    """group E: the candidates' keys differ in byte b alone among those that share the bytes above it (one key per value of
    the byte); the other candidates hold the key of probability 1, above them all.  cut: first / mid / last -- the cut falls
    in the lowest, a middle, the last occupied bin of that digit"""
    A, gen = 300, synthetic.rng(41 + b)
    _, x = digit_keys(b)
    x1 = np.full(A, ONE_KEY_LOGIT)
    where = np.setdiff1d(np.arange(A), (0, 100, 200, 299))
    x1[gen.permutation(where)[:len(x)]] = x
    return _radix_case(A, x1, k={"first": 1, "mid": len(x) // 2, "last": len(x)}[cut], pad=pad)


def tgt_radix_flat(kind, k, pad=0):
    """group E, 2150 anchors: zeros -- 1500 keys equal to 0, half from a background logit of -inf, half from a gap beyond
    both cut-offs of expf; ones -- 1500 keys of probability 1; denormal -- every key a denormal probability (or 0)"""
    A, gen = 2150, synthetic.rng(43)
    x1 = gen.uniform(-3, 3, A).astype(np.float32)
    x0 = np.zeros(A, np.float32)
    flat = gen.permutation(np.setdiff1d(np.arange(A), RADIX_POS))[:1500]
    if kind == "zeros":
        x0[flat[:750]] = -np.inf
        x1[flat[750:]] = 200.0
    elif kind == "ones":
        x1[flat] = ONE_KEY_LOGIT
    elif kind == "denormal":
        x1 = gen.uniform(87.5, 104.5, A).astype(np.float32)
    return _radix_case(A, x1, x0, pos=RADIX_POS, k=k, pad=pad)


def tgt_radix_one_stride(k, pad=0):
    """group E: 296 equal keys in the first 300 anchors, the cut inside them: a tie scan that ends within one stride"""
    return _radix_case(300, np.zeros(300, np.float32), k=k, pad=pad)


TIE_BELOW = 20


def tgt_radix_ties(run, kk, pad=0):
    """group E, 2150 anchors (two full strides and 102 anchors: one full wave and a partial one): `run` candidates with the
    key of probability 0.5 -- anchors 1023, 1024, 2048 and the last one among them --, TIE_BELOW keys below it, the rest
    above; the cut takes kk of the run"""
    A, gen = 2150, synthetic.rng(47 + run)
    fixed = np.array([1023, 1024, 2048, A - 1])
    rest = gen.permutation(np.setdiff1d(np.arange(A), np.concatenate([fixed, RADIX_POS])))
    x1 = -gen.uniform(0.5, 3, A).astype(np.float32)                 # probability above 0.5
    x1[np.concatenate([fixed, rest[:run - len(fixed)]])] = 0.0
    x1[rest[run - len(fixed):][:TIE_BELOW]] = gen.uniform(0.5, 3, TIE_BELOW).astype(np.float32)
    return _radix_case(A, x1, pos=RADIX_POS, k=TIE_BELOW + kk, pad=pad)


def _ulps(v, k):
    return (np.array([v], np.float32).view(np.int32) + np.int32(k)).view(np.float32)[0]


ENCODE_QUOTIENTS = tuple([np.float32(1)] + [_ulps(1, k) for k in (1, 2, 3, -1, -2, -3)]
                         + [np.float32(v) for v in (1.001, 0.999, 1e-4, 1e4, 2.0 ** -19, 1.5e-6, 0.5, 3.0)])


def tgt_encode(**kw):
    """group F: positives whose width quotient gw / aw (first family: anchors [0, 2i, 1, 2i + 1], so gw / aw is the ground
    truth's right edge itself) or height quotient (second family, transposed, from x = 10) is each of ENCODE_QUOTIENTS; the
    other quotient is 0.75 or 1.  A quotient below the bipartite cut cannot be a positive's (IoU <= either quotient), so
    2^-19 and 1.5e-6 are the smallest here and a denormal quotient is unreachable.  Class ids 0, 2^24 and -2."""
    ancs, rows = [], []
    classes = (0.0, 2.0 ** 24, -2.0, 3.0)
    for i, q in enumerate(ENCODE_QUOTIENTS):
        o = np.float32(2 * i + 2)
        other = np.float32(0.75 if i % 2 else 1.0)
        ancs += [[0, o, 1, o + 1], [o + 10, 0, o + 11, 1]]
        rows += [[classes[i % 4], 0, o, q, o + other, 0.07 * i], [classes[(i + 1) % 4], o + 10, 0, o + 10 + other, q, 0.9 - 0.05 * i]]
    anc = np.concatenate([np.array(ancs, np.float32), grid_anchors(64) + np.float32(20000)])
    lab = -np.ones((1, len(rows) + 1, 6), np.float32)
    lab[0, :len(rows)] = rows
    gen = synthetic.rng(53)
    return _finish(anc, lab, gen.standard_normal((1, 3, len(anc))), negative_mining_ratio=1.0, **kw)


TGT_BUILDERS = {"label_counts": tgt_label_counts, "iou_cuts": tgt_iou_cuts, "wild": tgt_wild, "matching": tgt_matching,
                "neg_counts": tgt_neg_counts, "radix_digit": tgt_radix_digit, "radix_flat": tgt_radix_flat,
                "radix_ties": tgt_radix_ties, "radix_one_stride": tgt_radix_one_stride, "encode": tgt_encode}
THIRD = float(np.float32(1) / np.float32(3))
GLOBAL_A = K_REG_ANCHORS + 1


def _tgt_edge_cases():
    cases = {}

    def add(cid, builder, **kw):
        assert cid not in cases
        cases[cid] = (builder, kw)
    for G in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024):                                  # A
        add(f"A-G{G}", "label_counts", G=G, dup=G >= 63, empty_first=G == 1)
    for G in (0, 65, 257, 1024):
        add(f"A-G{G}-global", "label_counts", G=G, A=GLOBAL_A, dup=G >= 63, empty_first=G == 65)
    add("A-G1024-all-matchable", "label_counts", G=1024, A=2048, matchable=1024, ratio=0.5)
    add("A-G-equals-L-1024", "label_counts", G=1024, dup=True)
    add("A-G7-equals-L-global", "label_counts", G=7, L=7, A=GLOBAL_A)
    add("A-garbage-behind-terminator", "label_counts", G=63, garbage=True)
    add("A-bad-terminator", "label_counts", G=70, bad=True, dup=True)
    add("A-bad-terminator-global", "label_counts", G=70, bad=True, A=GLOBAL_A)
    for i, t in enumerate((0.5, THIRD, 0.7)):                                                # B
        add(f"B-overlap-t{i}", "iou_cuts", t=t, kind="overlap")
    add("B-overlap-mined", "iou_cuts", t=0.5, kind="overlap", ratio=2.0)
    for i, (t, thr) in enumerate(((0.5, 0.7), (0.3, 0.7), (0.5, 0.5))):
        add(f"B-mining-t{i}", "iou_cuts", t=t, kind="mining", thr=thr)
    add("B-match-cut", "iou_cuts", t=1e-6, kind="match")
    for name, thr in (("zero", 0.0), ("minus-zero", -0.0), ("negative", -0.25)):
        add(f"B-threshold-{name}", "wild", thr=thr, ratio=-1.0)
    add("B-wild", "wild")
    add("B-wild-all-negatives", "wild", ratio=-1.0)
    for kind in ("equal", "identical70", "identical300", "chain", "subcut"):                 # C
        add(f"C-{kind}", "matching", kind=kind)
    for kind in ("equal", "identical70", "chain", "subcut"):
        add(f"C-{kind}-global", "matching", kind=kind, A=GLOBAL_A)
    add("C-chain-all-negatives-global", "matching", kind="chain", A=GLOBAL_A, ratio=-1.0)
    add("D-third-of-3", "neg_counts", npos=3, ratio=THIRD)                                   # D
    add("D-below-3", "neg_counts", npos=1, ratio=2.9999998)
    add("D-below-9", "neg_counts", npos=3, ratio=2.9999998)
    add("D-none", "neg_counts", npos=1, ratio=0.5)
    add("D-one", "neg_counts", npos=1, ratio=1.0)
    for w in (-1, 0, 1):
        add(f"D-candidates{w:+d}", "neg_counts", npos=4, want=w, limbo=6)
    add("D-above-all", "neg_counts", npos=4, ratio=1e4)
    add("D-none-global", "neg_counts", npos=1, ratio=0.5, A=GLOBAL_A)
    for w in (-1, 0, 1):
        add(f"D-candidates{w:+d}-global", "neg_counts", npos=4, want=w, limbo=6, A=GLOBAL_A)
    add("D-product-2p31-minus-128", "neg_counts", npos=1, ratio=2.0 ** 31 - 128)
    add("D-product-2p31", "neg_counts", npos=1, ratio=2.0 ** 31)
    add("D-product-3e9", "neg_counts", npos=300, ratio=1e7, A=400)
    add("D-product-2p31-global", "neg_counts", npos=1, ratio=2.0 ** 31, A=GLOBAL_A, limbo=3)
    for b in range(4):                                                                       # E
        for cut in ("first", "mid", "last"):
            add(f"E-byte{b}-{cut}", "radix_digit", b=b, cut=cut)
    add("E-byte1-mid-global", "radix_digit", b=1, cut="mid", pad=GLOBAL_A)
    add("E-zeros", "radix_flat", kind="zeros", k=700)
    add("E-zeros-all", "radix_flat", kind="zeros", k=1500)
    add("E-ones", "radix_flat", kind="ones", k=1400)
    add("E-denormal", "radix_flat", kind="denormal", k=900)
    for run in (1500, 2100):
        for kk in (1, 1023, 1024, 1025, run - 1, run):
            add(f"E-ties{run}-kk{kk}", "radix_ties", run=run, kk=kk)
    add("E-ties1500-kk1025-global", "radix_ties", run=1500, kk=1025, pad=GLOBAL_A)
    add("E-one-stride", "radix_one_stride", k=100)
    add("E-one-stride-global", "radix_one_stride", k=295, pad=GLOBAL_A)
    for i, v in enumerate(((1, 1, 1, 1), (.1, .1, .2, .2), (1e-40,) * 4, (0.0,) * 4)):        # F
        add(f"F-variances{i}", "encode", variances=v)
    for name, v in (("minus-zero", -0.0), ("255", 255.0), ("nan", float("nan"))):
        add(f"F-ignore-{name}", "encode", ignore_label=v)
    return cases


TGT_EDGE_CASES = _tgt_edge_cases()


@functools.lru_cache(maxsize=None)
def tgt_inputs(cid):
    """(anchors, labels, cls_pred, keyword arguments) of a case; the arrays read-only"""
    builder, kw = TGT_EDGE_CASES[cid]
    anc, lab, pred, okw = TGT_BUILDERS[builder](**kw)
    for a in (anc, lab, pred):
        a.setflags(write=False)
    return anc, lab, pred, okw


@functools.lru_cache(maxsize=None)
def tgt_expected(cid):
    """the CPU oracle on a case, once per process: ([loc_target, loc_mask, cls_target], return code, matched, seconds)"""
    anc, lab, pred, kw = tgt_inputs(cid)
    t0 = time.perf_counter()
    exp, rc, matched = om.multibox_target(anc, lab, pred, return_matched=True, **kw)
    dt = time.perf_counter() - t0
    for a in (*exp, matched):
        a.setflags(write=False)
    return exp, rc, matched, dt


@functools.lru_cache(maxsize=None)
def tgt_case_routes(cid):
    """the route of every sample of a case"""
    anc, lab, pred, kw = tgt_inputs(cid)
    return [target_route(anc.shape[1], lab.shape[1], lab[b], pred[b], anc[0], **kw) for b in range(lab.shape[0])]
