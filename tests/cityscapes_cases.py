"""Shared by the Cityscapes evaluation tests: the golden cases (tests/golden/cityscapes_pixel_eval.npz, generated from
the reference's evalPixelLevelSemanticLabeling.py), a plain numpy restatement of the counting of its evaluatePair, and
random full-size scenes."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
L = 34
SCORE_FIELDS = ("classScores", "classInstScores", "categoryScores", "categoryInstScores")
AVERAGES = ("averageScoreClasses", "averageScoreInstClasses", "averageScoreCategories", "averageScoreInstCategories")


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "cityscapes_pixel_eval.npz"))
    out = []
    for k in range(int(z["count"])):
        out.append({"name": str(z["name_%d" % k]), "pred": z["pred_%d" % k], "gt_label": z["gt_label_%d" % k],
                    "gt_inst": z["gt_inst_%d" % k], "conf": z["conf_%d" % k].astype(np.int64), "inst": z["inst_%d" % k],
                    "scores": json.loads(str(z["scores_json_%d" % k]))})
    return out


def count(pred, gt_label, gt_inst, category):
    """The counting of evaluatePair (:583-635), per pixel instead of per mask.  pred, gt_label (N, H, W) uint8, gt_inst
    (N, H, W) int; category (256,) labelId -> category number (0: none).
    -> conf (34, 34) int64 [gt][pred]; rows (M, 5) int64 (image, instance id, size, tp, cat_tp) image-major, ascending id,
    for every instance id > 1000 of a label 24..33; errors: pixels with gt or pred >= 34 (not in conf) or an instance id
    > 1000 of another label (not in rows)."""
    pred = np.asarray(pred).astype(np.int64); gt = np.asarray(gt_label).astype(np.int64); inst = np.asarray(gt_inst).astype(np.int64)
    bad = (pred >= L) | (gt >= L)
    conf = np.bincount((gt * L + pred)[~bad], minlength=L * L).reshape(L, L)
    has = inst > 1000
    lab = inst // 1000
    known = has & (lab >= 24) & (lab <= 33)
    errors = int(np.count_nonzero(bad | (has & ~known)))
    rows = []
    for n in range(pred.shape[0]):
        ids, inverse = np.unique(inst[n][known[n]], return_inverse=True)
        p = pred[n][known[n]]
        l_of = ids[inverse] // 1000
        size = np.bincount(inverse, minlength=len(ids))
        tp = np.bincount(inverse, weights=(p == l_of), minlength=len(ids)).astype(np.int64)
        c = category[l_of]
        cat = np.bincount(inverse, weights=(c != 0) & (category[p] == c), minlength=len(ids)).astype(np.int64)
        rows += [(n, int(i), int(s), int(t), int(ct)) for i, s, t, ct in zip(ids, size, tp, cat)]
    return conf, np.asarray(rows, np.int64).reshape(-1, 5), errors


def table_rows(table):
    """the dense device table (N, 10, 1000, 3) -> rows like count()'s"""
    table = np.asarray(table)
    n, lab, k = np.nonzero(table[..., 0])
    c = table[n, lab, k].astype(np.int64)
    return np.concatenate([n[:, None], ((lab + 24) * 1000 + k)[:, None], c], 1).astype(np.int64).reshape(-1, 5)


def random_scene(g, N, H, W, n_inst, noise=0.1):
    """ground truth of vertical bands and rectangles with `n_inst` elliptic instances per image, prediction = ground
    truth with `noise` of its pixels replaced and a few wrong rectangles; all labelIds 0..33 occur"""
    gt = np.zeros((N, H, W), np.uint8); inst = np.zeros((N, H, W), np.int32)
    for n in range(N):
        edges = np.sort(g.choice(np.arange(1, W), size=min(23, W - 1), replace=False))
        for s, a, b in zip(g.permutation(24), np.r_[0, edges], np.r_[edges, W]):
            gt[n, :, a:b] = s
        inst[n] = gt[n]
        counter = {}
        for _ in range(n_inst):
            lab = int(g.integers(24, 34))
            k = counter.get(lab, 0); counter[lab] = k + 1
            cy, cx = int(g.integers(0, H)), int(g.integers(0, W))
            ry, rx = int(g.integers(1, max(2, H // 8))), int(g.integers(1, max(2, W // 12)))
            y0, y1, x0, x1 = max(0, cy - ry), min(H, cy + ry + 1), max(0, cx - rx), min(W, cx + rx + 1)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
            gt[n, y0:y1, x0:x1][m] = lab
            inst[n, y0:y1, x0:x1][m] = lab * 1000 + (k if g.random() < 0.9 else 999 - k % 100)
        if n_inst:                                   # a group region: bare labelId
            gt[n, :3, :7] = 26; inst[n, :3, :7] = 26
    pred = gt.copy()
    m = g.random(gt.shape) < noise
    pred[m] = g.integers(0, L, int(m.sum()), dtype=np.uint8)
    for n in range(N):
        for _ in range(6):
            y, x = int(g.integers(0, H)), int(g.integers(0, W))
            pred[n, y:y + int(g.integers(1, H // 4 + 2)), x:x + int(g.integers(1, W // 4 + 2))] = g.integers(0, L)
    return pred, gt, inst


def softmax_nhwc(g, N, C, h, w, ld):
    """class probabilities in the graph's layout (N, h, w, ld), pad channels poisoned; one exact tie"""
    logits = g.standard_normal((N, C, h, w)).astype(np.float32) * 2
    e = np.exp(logits - logits.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32)
    prob[0, :, 0, 0] = 1.0 / C
    nhwc = np.zeros((N, h, w, ld), np.float32)
    nhwc[..., :C] = prob.transpose(0, 2, 3, 1)
    nhwc[..., C:] = 9.0
    return nhwc
