"""Generates tests/golden/cityscapes_labels.json and tests/golden/cityscapes_pixel_eval.npz from the REFERENCE's own
Cityscapes evaluation script, data/cityscapes/Scripts/evaluation/evalPixelLevelSemanticLabeling.py, imported unmodified
from the reference checkout at generation time (Python 3 with numpy and Pillow; the script's cython module is not built,
so it counts on its pure-Python path).

Run with:  python tests/golden/make_cityscapes_eval_golden.py [path of the reference checkout, default /root/reference]

`PIL.PILLOW_VERSION` -- the alias of `PIL.__version__` that Pillow < 7 exported and helpers/csHelpers.py:16 imports to
check that PIL is Pillow -- is restored before the import; nothing else about Pillow or numpy is touched.

Per case the script's own functions are called on small PNG files written to a temporary directory: generateMatrix,
generateInstanceStats, evaluatePair per image, then getIouScoreForLabel / getInstanceIouScoreForLabel /
getIouScoreForCategory / getInstanceIouScoreForCategory and createResultDict, as evaluateImgLists (:460-546) strings
them together.  Per image the instance statistics are also taken on their own (a fresh generateInstanceStats), which
is where the per-instance expectations come from.

cityscapes_pixel_eval.npz holds inputs and expected outputs only, per case k:
  name_k; pred_k, gt_label_k (N, H, W) uint8; gt_inst_k (N, H, W) int32; conf_k (34, 34) uint64;
  inst_k (M, 5) int64 rows (image, instance id, size, tp, cat_tp) of every instance > 1000 the script walks or skips,
  image-major then ascending id (tp / cat_tp of the instances the script walks are its own figures -- an image's
  statistics are rebuilt from these rows by the tests and must equal scores_json_k's 'instanceStats');
  scores_json_k: createResultDict's dict (without confMatrix) plus 'instanceStats', as JSON with NaN spelled NaN.
cityscapes_labels.json: the fields of the script's `labels` tuple, and args.avgClassSize."""
import json
import os
import sys
import tempfile

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

PIL.PILLOW_VERSION = PIL.__version__                # Pillow < 7: `from PIL import PILLOW_VERSION`
sys.path.insert(0, os.path.join(REFERENCE, "data", "cityscapes", "Scripts", "evaluation"))
import evalPixelLevelSemanticLabeling as ev         # noqa: E402  (the reference's script)

assert not ev.CSUPPORT
ev.args.quiet = True

EVALUATED = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
STUFF = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23]


def scene(rng, H, W, n_inst, inst_labels, stuff=STUFF, void=(), groups=()):
    """bands of `stuff` labels, rectangles of `void` labels, then instance blobs (ellipses; later ones cover earlier
    ones) numbered per label, and `groups` regions whose instance id is the bare labelId"""
    lab = np.zeros((H, W), np.uint8)
    inst = np.zeros((H, W), np.int32)
    edges = np.sort(rng.choice(np.arange(1, W), size=min(len(stuff), W - 1) - 1, replace=False))
    for s, (a, b) in zip(rng.permutation(stuff), zip(np.r_[0, edges], np.r_[edges, W])):
        lab[:, a:b] = s
    yy, xx = np.mgrid[:H, :W]

    def blob():
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(2, max(3, H // 4)), rng.integers(2, max(3, W // 5))
        return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0

    for v in void:
        y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
        lab[y:y + rng.integers(3, 20), x:x + rng.integers(3, 30)] = v
    inst[:] = lab
    counter = {}
    for _ in range(n_inst):
        L = int(rng.choice(inst_labels))
        k = counter.get(L, 0)
        counter[L] = k + 1
        m = blob()
        lab[m] = L
        inst[m] = L * 1000 + k
    for L in groups:
        m = blob()
        lab[m] = L
        inst[m] = L
    return lab, inst


def noisy(rng, gt, frac, choices):
    pred = gt.copy()
    m = rng.random(gt.shape) < frac
    pred[m] = rng.choice(choices, size=int(m.sum()))
    # coherent wrong regions as well: whole rectangles of one label
    for _ in range(3):
        y, x = rng.integers(0, gt.shape[0] - 4), rng.integers(0, gt.shape[1] - 4)
        pred[y:y + rng.integers(2, 24), x:x + rng.integers(2, 40)] = rng.choice(choices)
    return pred


def run_reference(preds, gts, insts):
    """-> conf (34, 34), instance rows, result dict, as the script computes them for the image list"""
    conf = ev.generateMatrix(ev.args)
    stats = ev.generateInstanceStats(ev.args)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for n, (p, g, i) in enumerate(zip(preds, gts, insts)):
            pf = os.path.join(tmp, "pred_%03d.png" % n)
            gf = os.path.join(tmp, "city_%06d_000019_gtFine_labelIds.png" % n)
            Image.fromarray(p).save(pf)
            Image.fromarray(g).save(gf)
            Image.fromarray(i.astype(np.uint16)).save(gf.replace("labelIds", "instanceIds"))
            ev.evaluatePair(pf, gf, conf, stats, {}, ev.args)
            # the same image once per instance, alone in its instance map: the script's own tp / catTp of that instance
            for iid in np.unique(i[i > 1000]):
                label = ev.id2label[int(iid) // 1000]
                size = int(np.count_nonzero(i == iid))
                if label.ignoreInEval:
                    # the script skips it (:605-606); what the device counts for it is checked against the restatement
                    rows.append((n, int(iid), size, -1, -1))
                    continue
                one = ev.generateInstanceStats(ev.args)
                Image.fromarray(np.where(i == iid, i, 0).astype(np.uint16)).save(gf.replace("labelIds", "instanceIds"))
                ev.evaluatePair(pf, gf, ev.generateMatrix(ev.args), one, {}, ev.args)
                c, k = one["classes"][label.name], one["categories"][label.category]
                assert c["tp"] + c["fn"] == size and k["tp"] + k["fn"] == size
                rows.append((n, int(iid), size, int(c["tp"]), int(k["tp"])))
    assert int(conf.sum()) == sum(p.size for p in preds)
    cls = {ev.id2label[l].name: ev.getIouScoreForLabel(l, conf, ev.args) for l in ev.args.evalLabels}
    cls_i = {ev.id2label[l].name: ev.getInstanceIouScoreForLabel(l, conf, stats, ev.args) for l in ev.args.evalLabels}
    cat = {c: ev.getIouScoreForCategory(c, conf, ev.args) for c in ev.category2labels.keys()}
    cat_i = {c: ev.getInstanceIouScoreForCategory(c, conf, stats, ev.args) for c in ev.category2labels.keys()}
    result = ev.createResultDict(conf, cls, cls_i, cat, cat_i, {}, ev.args)
    del result["confMatrix"]
    result["instanceStats"] = stats
    return conf, np.asarray(rows, np.int64).reshape(-1, 5), result


def plain(o):
    if isinstance(o, (bool, np.bool_)):
        return bool(o)
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    if isinstance(o, (np.floating, float)):
        return float(o)
    if isinstance(o, (np.integer, int)):
        return int(o)
    return o


def main():
    rng = np.random.default_rng(20260117)
    H, W = 96, 192
    cases = {}
    k = 0

    def add(name, preds, gts, insts):
        nonlocal k
        preds = [np.ascontiguousarray(p, np.uint8) for p in preds]
        gts = [np.ascontiguousarray(g, np.uint8) for g in gts]
        insts = [np.ascontiguousarray(i, np.int32) for i in insts]
        conf, rows, result = run_reference(preds, gts, insts)
        cases["name_%d" % k] = np.array(name)
        cases["pred_%d" % k] = np.stack(preds)
        cases["gt_label_%d" % k] = np.stack(gts)
        cases["gt_inst_%d" % k] = np.stack(insts)
        cases["conf_%d" % k] = conf.astype(np.uint64)
        cases["inst_%d" % k] = rows
        cases["scores_json_%d" % k] = np.array(json.dumps(plain(result)))      # repr-exact floats, NaN as NaN
        print("%-28s images %d instances %3d mIoU %.4f iIoU %.4f" % (name, len(preds), len(rows), result["averageScoreClasses"],
                                                                    result["averageScoreInstClasses"]))
        k += 1

    inst_eval = [24, 25, 26, 27, 28, 31, 32, 33]
    g, i = scene(rng, H, W, 14, inst_eval)
    add("blobs_noise_5pct", [noisy(rng, g, 0.05, EVALUATED)], [g], [i])
    g, i = scene(rng, H, W, 25, inst_eval)
    add("blobs_noise_40pct", [noisy(rng, g, 0.40, EVALUATED)], [g], [i])
    trio = [scene(rng, H, W, n, inst_eval) for n in (6, 12, 18)]
    add("three_images", [noisy(rng, g, 0.15, EVALUATED) for g, _ in trio], [g for g, _ in trio], [i for _, i in trio])
    g, i = scene(rng, H, W, 10, inst_eval)
    add("one_class_everywhere", [np.full_like(g, 26)], [g], [i])
    # only four labels in prediction and ground truth: every other class and whole categories score NaN
    g, i = scene(rng, H, W, 5, [26], stuff=[7, 21, 23])
    add("absent_classes", [noisy(rng, g, 0.1, [7, 21, 23, 26])], [g], [i])
    # ignoreInEval regions in the ground truth, ignoreInEval labelIds predicted (29 / 30 inside vehicles: cat_tp != tp)
    g, i = scene(rng, H, W, 12, [26, 27, 28, 24], void=(0, 1, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18))
    p = noisy(rng, g, 0.1, EVALUATED + [0, 4, 9, 18, 29, 30])
    veh = np.isin(g, [26, 27, 28])
    p[veh & (rng.random(g.shape) < 0.3)] = 29
    p[veh & (rng.random(g.shape) < 0.15)] = 30
    add("ignored_labels", [p], [g], [i])
    # instances OF ignoreInEval labels (29xxx caravan, 30xxx trailer), which the script skips
    g, i = scene(rng, H, W, 14, [29, 30, 26, 33, 25])
    add("ignored_instances", [noisy(rng, g, 0.2, EVALUATED + [29, 30])], [g], [i])
    # group regions: the instance id is the bare labelId (< 1000), no instance
    g, i = scene(rng, H, W, 8, inst_eval, groups=(24, 26, 26, 33))
    add("groups", [noisy(rng, g, 0.1, EVALUATED)], [g], [i])
    # single-pixel instances: one predicted right, one wrong, one as another label of its category
    g, i = scene(rng, H, W, 4, inst_eval)
    p = noisy(rng, g, 0.05, EVALUATED)
    for (y, x, L, kk, pl) in ((3, 5, 24, 900, 24), (50, 100, 27, 901, 8), (95, 191, 32, 999, 26), (0, 0, 33, 0, 33)):
        g[y, x] = L; i[y, x] = L * 1000 + kk; p[y, x] = pl
    add("single_pixel_instances", [p], [g], [i])
    # a width that is not a multiple of 4 (and an odd height), two images
    duo = [scene(rng, 57, 101, 9, inst_eval, void=(0, 3)) for _ in range(2)]
    add("width_101", [noisy(rng, g, 0.2, EVALUATED + [29]) for g, _ in duo], [g for g, _ in duo], [i for _, i in duo])

    cases["count"] = np.int64(k)
    cases["numpy_version"] = np.array(np.__version__)
    out = os.path.join(HERE, "cityscapes_pixel_eval.npz")
    np.savez_compressed(out, **cases)
    print("wrote", out, k, "cases,", os.path.getsize(out), "bytes")

    table = {"labels": [lab._asdict() for lab in ev.labels], "avgClassSize": dict(ev.args.avgClassSize)}
    out = os.path.join(HERE, "cityscapes_labels.json")
    with open(out, "w") as f:
        json.dump(plain(table), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
