"""Cityscapes pixel-level scores (IoU and instance-weighted iIoU, per class and per category) at full resolution.

The reference writes labelId maps as PNGs (multi_eval.py:352-356) and leaves the scores to the dataset's own script,
data/cityscapes/Scripts/evaluation/evalPixelLevelSemanticLabeling.py.  Here the script's counting (evaluatePair,
:583-635: ~100 passes over the 2 M pixels of an image) is one device pass -- dspn_cityscapes_counts_u8 over a labelId
map, or dspn_cityscapes_counts_prob_f32 straight from the class probabilities -- and the script's score arithmetic
(:229-351, a few hundred float64 operations per image) runs on the host in the script's statement order, so that the
scores are the script's to the last bit (tests/golden/cityscapes_pixel_eval.npz holds its outputs).

The label table below states the facts of the dataset (labelId, trainId, category, which labels have instances, which
are ignored in evaluation) in this project's own words; tests/golden/cityscapes_labels.json pins it to the script's."""
import math
from collections import namedtuple

import numpy as np
import torch

from .. import functional as fn

CityscapesLabel = namedtuple("CityscapesLabel", "name id train_id category category_id has_instances ignore_in_eval")

_CATEGORY_IDS = {"void": 0, "flat": 1, "construction": 2, "object": 3, "nature": 4, "sky": 5, "human": 6, "vehicle": 7}


def _table():
    rows = []
    evaluated = iter(range(19))                         # trainIds go to the evaluated labels in labelId order

    def add(category, names, first_id, has_instances=False, ignored=()):
        for k, name in enumerate(names):
            ign = name in ignored
            rows.append(CityscapesLabel(name, first_id + k, 255 if ign else next(evaluated), category,
                                        _CATEGORY_IDS[category], has_instances, ign))

    void = ("unlabeled", "ego vehicle", "rectification border", "out of roi", "static", "dynamic", "ground")
    add("void", void, 0, ignored=void)
    add("flat", ("road", "sidewalk", "parking", "rail track"), 7, ignored=("parking", "rail track"))
    add("construction", ("building", "wall", "fence", "guard rail", "bridge", "tunnel"), 11,
        ignored=("guard rail", "bridge", "tunnel"))
    add("object", ("pole", "polegroup", "traffic light", "traffic sign"), 17, ignored=("polegroup",))
    add("nature", ("vegetation", "terrain"), 21)
    add("sky", ("sky",), 23)
    add("human", ("person", "rider"), 24, has_instances=True)
    add("vehicle", ("car", "truck", "bus", "caravan", "trailer", "train", "motorcycle", "bicycle"), 26, has_instances=True,
        ignored=("caravan", "trailer"))
    # the one label without an id: it never appears in a ground-truth image and has no row in the confusion matrix
    rows.append(CityscapesLabel("license plate", -1, -1, "vehicle", _CATEGORY_IDS["vehicle"], False, True))
    return tuple(rows)


CITYSCAPES_LABELS = _table()
# mean size in pixels of an instance of each class over the training set: the numerator of an instance's iIoU weight
AVG_CLASS_SIZE = {
    "bicycle": 4672.3249222261, "caravan": 36771.8241758242, "motorcycle": 6298.7200839748, "rider": 3930.4788056518,
    "bus": 35732.1511111111, "train": 67583.7075812274, "car": 12794.0202738185, "person": 3462.4756337644,
    "truck": 27855.1264367816, "trailer": 16926.9763313609,
}

NUM_LABELS = fn.CITYSCAPES_LABELS                       # rows of the confusion matrix: labelIds 0..33
_BY_ID = {lab.id: lab for lab in CITYSCAPES_LABELS}
_EVAL_IDS = [lab.id for lab in CITYSCAPES_LABELS if lab.id >= 0]
_CATEGORIES = {}                                         # category -> its labels, both in table order
for _lab in CITYSCAPES_LABELS:
    _CATEGORIES.setdefault(_lab.category, []).append(_lab)
# categories with instance scores: every label (that has an id) has instances.  -> the ids of those labels
_INST_CATEGORIES = {c: [lab.id for lab in labs if lab.id >= 0] for c, labs in _CATEGORIES.items()
                    if all(lab.has_instances for lab in labs if lab.id >= 0)}


def label_of_train_id_table():
    """(256,) uint8: trainId -> labelId of the evaluated labels, 0 elsewhere (the LUT of multi_eval.py:352-353)"""
    lut = np.zeros(256, np.uint8)
    for lab in CITYSCAPES_LABELS:
        if 0 <= lab.train_id < 255:
            lut[lab.train_id] = lab.id
    return lut


def category_table():
    """(256,) uint8: labelId -> category number for the categories with instance scores, 0 elsewhere"""
    cat = np.zeros(256, np.uint8)
    for c, ids in _INST_CATEGORIES.items():
        cat[ids] = _CATEGORY_IDS[c]
    assert all(_CATEGORY_IDS[c] > 0 for c in _INST_CATEGORIES)
    return cat


def new_instance_stats():
    """the script's generateInstanceStats (:184-215): float sums per class / category with instance scores"""
    zero = lambda: {"tp": 0.0, "tpWeighted": 0.0, "fn": 0.0, "fnWeighted": 0.0}  # noqa: E731
    stats = {"classes": {lab.name: zero() for lab in CITYSCAPES_LABELS if lab.has_instances and not lab.ignore_in_eval},
             "categories": {}}
    for c, ids in _INST_CATEGORIES.items():
        stats["categories"][c] = dict(zero(), labelIds=list(ids))
    return stats


def add_image_instances(stats, inst_ids, size, tp, cat_tp):
    """One image's instances into stats, as evaluatePair :601-635 does: in ascending instance id,
    weight = avgClassSize / size, weighted and plain tp / fn sums per class and per category; instances of labels
    ignored in evaluation are skipped.  inst_ids ascending, the others their pixel counts."""
    for iid, n, t, ct in zip(inst_ids, size, tp, cat_tp):
        iid, n, t, ct = int(iid), int(n), int(t), int(ct)
        label = _BY_ID[iid // 1000]
        if label.ignore_in_eval:
            continue
        fneg = n - t
        weight = AVG_CLASS_SIZE[label.name] / float(n)
        tp_w = float(t) * weight
        fn_w = float(fneg) * weight
        s = stats["classes"][label.name]
        s["tp"] += t
        s["fn"] += fneg
        s["tpWeighted"] += tp_w
        s["fnWeighted"] += fn_w
        if label.category in stats["categories"]:
            cat_fn = n - ct
            cat_tp_w = float(ct) * weight
            cat_fn_w = float(cat_fn) * weight
            s = stats["categories"][label.category]
            s["tp"] += ct
            s["fn"] += cat_fn
            s["tpWeighted"] += cat_tp_w
            s["fnWeighted"] += cat_fn_w


def _not_ignored(skip):
    return [i for i in _EVAL_IDS if not _BY_ID[i].ignore_in_eval and not skip(i)]


def _ratio(tp, fp, fneg):
    denom = tp + fp + fneg
    if denom == 0:
        return float("nan")
    return float(tp) / denom


def _average(scores):
    """the script's getScoreAverage (:286-295): mean over the entries that are not NaN, summed in dict order"""
    valid, total = 0, 0.0
    for v in scores.values():
        if not math.isnan(v):
            valid += 1
            total += v
    return total / valid if valid else float("nan")


def scores_from_counts(conf, stats):
    """conf (34, 34) integer confusion matrix [gt][pred], stats as add_image_instances leaves them -> the dict of the
    script's createResultDict (:355-376) plus 'instanceStats'.  Statement order of :229-351 in float64 / Python ints."""
    conf = np.asarray(conf).astype(np.int64)
    assert conf.shape == (NUM_LABELS, NUM_LABELS)
    class_scores, class_inst = {}, {}
    for i in _EVAL_IDS:
        lab = _BY_ID[i]
        if lab.ignore_in_eval:
            class_scores[lab.name] = class_inst[lab.name] = float("nan")
            continue
        tp = int(conf[i, i])
        fneg = int(conf[i, :].sum()) - tp
        fp = int(conf[_not_ignored(lambda j: j == i), i].sum())        # other labels' pixels, ignored rows left out
        class_scores[lab.name] = _ratio(tp, fp, fneg)
        if lab.name in stats["classes"]:
            s = stats["classes"][lab.name]
            class_inst[lab.name] = _ratio(s["tpWeighted"], fp, s["fnWeighted"])
        else:
            class_inst[lab.name] = float("nan")
    cat_scores, cat_inst = {}, {}
    for c, labs in _CATEGORIES.items():
        outside = _not_ignored(lambda j: _BY_ID[j].category == c)
        ids = [lab.id for lab in labs if not lab.ignore_in_eval and lab.id >= 0]
        if ids:
            tp = int(conf[ids, :][:, ids].sum())
            fneg = int(conf[ids, :].sum()) - tp
            fp = int(conf[outside, :][:, ids].sum())
            cat_scores[c] = _ratio(tp, fp, fneg)
        else:
            cat_scores[c] = float("nan")
        if c in stats["categories"]:
            s = stats["categories"][c]
            fp = int(conf[outside, :][:, s["labelIds"]].sum())
            cat_inst[c] = _ratio(s["tpWeighted"], fp, s["fnWeighted"])
        else:
            cat_inst[c] = float("nan")
    total = int(conf.sum())
    return {
        "confMatrix": conf.tolist(),
        "priors": {_BY_ID[i].name: (float(conf[i, :].sum()) / total if total else float("nan")) for i in _EVAL_IDS},
        "labels": {_BY_ID[i].name: i for i in _EVAL_IDS},
        "classScores": class_scores, "classInstScores": class_inst,
        "categoryScores": cat_scores, "categoryInstScores": cat_inst,
        "averageScoreClasses": _average(class_scores), "averageScoreInstClasses": _average(class_inst),
        "averageScoreCategories": _average(cat_scores), "averageScoreInstCategories": _average(cat_inst),
        "instanceStats": stats,
    }


class CityscapesPixelMetric:
    """IoU / iIoU of evalPixelLevelSemanticLabeling.py over the images fed to update / update_from_prob.

    The confusion matrix stays on the device until get().  The instance table (fn.cityscapes_tables: 120 kB per image)
    is zeroed and filled per call and READ BACK ONCE PER update CALL -- that is where a call waits for the device --
    and its non-empty entries are folded into the float64 instance statistics in image order, ascending instance id.
    A pixel the script would stop on (label or prediction > 33, an instance id of a label without instances) raises
    ValueError after the counts of the call's other pixels have been added."""

    def __init__(self, device=None):
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.category = torch.from_numpy(category_table()).to(self.device)
        self.label_of_train_id = torch.from_numpy(label_of_train_id_table()).to(self.device)
        self.conf = torch.zeros(NUM_LABELS, NUM_LABELS, dtype=torch.int64, device=self.device)
        self.errors = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.reset()

    def reset(self):
        self.conf.zero_()
        self.errors.zero_()
        self.stats = new_instance_stats()
        self.num_images = 0
        self.last_instance_counts = None

    def _inputs(self, gt_label_ids, gt_instance_ids):
        gt = torch.as_tensor(gt_label_ids).to(self.device, torch.uint8).contiguous()
        inst = torch.as_tensor(gt_instance_ids).to(self.device, torch.int32).contiguous()
        if gt.dim() == 2:
            gt, inst = gt[None], inst[None]
        return gt, inst

    def _fold(self, table):
        host = table.cpu().numpy()                                    # the one wait of an update call
        errors = int(self.errors.item())
        per_image = []
        for b in range(host.shape[0]):
            lab, k = np.nonzero(host[b, :, :, 0])                     # row-major: ascending instance id
            ids = (lab + fn.CITYSCAPES_INST_LABEL0) * 1000 + k
            cnt = host[b, lab, k].astype(np.int64)
            add_image_instances(self.stats, ids, cnt[:, 0], cnt[:, 1], cnt[:, 2])
            per_image.append(np.concatenate([ids[:, None].astype(np.int64), cnt], 1))
        self.num_images += host.shape[0]
        self.last_instance_counts = per_image     # per image (n_inst, 4): instance id, size, tp, cat_tp
        if errors:
            self.errors.zero_()
            raise ValueError("CityscapesPixelMetric: %d pixel(s) with a label or prediction outside 0..%d, or with an "
                             "instance id of a label without instances" % (errors, NUM_LABELS - 1))

    def update(self, pred_label_ids, gt_label_ids, gt_instance_ids):
        """pred_label_ids, gt_label_ids: (N, H, W) or (H, W) labelId maps; gt_instance_ids: the *_instanceIds.png values"""
        gt, inst = self._inputs(gt_label_ids, gt_instance_ids)
        pred = torch.as_tensor(pred_label_ids).to(self.device, torch.uint8).contiguous()
        pred = pred[None] if pred.dim() == 2 else pred
        table = fn.cityscapes_tables(gt.shape[0], self.device)[1]
        fn.cityscapes_counts(pred, gt, inst, self.category, self.conf, table, self.errors)
        self._fold(table)

    def update_from_prob(self, seg_prob, gt_label_ids, gt_instance_ids, num_classes=19):
        """seg_prob: (N, h, w, ld) NHWC class probabilities as the graph holds them; the prediction at the ground truth's
        resolution is prob_upsampling's class map sent through the trainId -> labelId table, formed inside the kernel"""
        gt, inst = self._inputs(gt_label_ids, gt_instance_ids)
        table = fn.cityscapes_tables(gt.shape[0], self.device)[1]
        fn.cityscapes_counts_prob(seg_prob.contiguous(), num_classes, self.label_of_train_id, gt, inst, self.category,
                                  self.conf, table, self.errors)
        self._fold(table)

    def get(self):
        return scores_from_counts(self.conf.cpu().numpy(), self.stats)

    def get_name_value(self):
        """flat (name, value) pairs: the four averages as cityscapes/IoU_class, cityscapes/iIoU_class,
        cityscapes/IoU_category, cityscapes/iIoU_category, then cityscapes/IoU/<class> for every evaluated class and
        cityscapes/iIoU/<class> for those with instances"""
        r = self.get()
        out = [("cityscapes/IoU_class", r["averageScoreClasses"]), ("cityscapes/iIoU_class", r["averageScoreInstClasses"]),
               ("cityscapes/IoU_category", r["averageScoreCategories"]),
               ("cityscapes/iIoU_category", r["averageScoreInstCategories"])]
        for lab in CITYSCAPES_LABELS:
            if lab.id >= 0 and not lab.ignore_in_eval:
                out.append(("cityscapes/IoU/" + lab.name, r["classScores"][lab.name]))
        for name in r["instanceStats"]["classes"]:
            out.append(("cityscapes/iIoU/" + name, r["classInstScores"][name]))
        return out
