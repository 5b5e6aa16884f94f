"""Cityscapes label and instance maps from the dataset's polygon files (`*_gtFine_polygons.json`) on the device: the
step of data/cityscapes/Scripts/preparation (json2labelImg.py, json2instanceImg.py, createTrainIdLabelImgs.py,
createTrainIdInstanceImgs.py) that paints every object's polygon with PIL.ImageDraw.polygon, one object after the other,
once per encoding; and the boxes of dataset/cs_json2xml.py.

One rasterisation per image gives an owner map (which object painted each pixel last); the four encodings are looked
up from it.  The fill rule is Pillow's (tests/ref_polygon.py holds it, equal to Pillow pixel for pixel): everything in
it that divides, or that depends on the order of a polygon's edges, is computed here on the host in numpy float32 and
handed to the kernels as a table (include/dspn_polygon.h)."""
import json
import os

import numpy as np
import torch

from .. import functional as fn
from ..evaluate.cityscapes_eval import CITYSCAPES_LABELS
from .distance_labels import round_half_away

KINDS = ("labelIds", "labelTrainIds", "instanceIds", "instanceTrainIds")
_BY_NAME = {lab.name: lab for lab in CITYSCAPES_LABELS}
_COORD_LIMIT = 1 << 20            # |coordinate| below this: every float32 step of the rule is then exact where Pillow's is
_NAN = np.float32(np.nan)


def load_annotation(path_or_dict):
    """a polygon file (path, or its parsed dict) -> {"imgWidth", "imgHeight", "objects": [{"label", "polygon", "deleted"}]}
    with the polygon as a list of integer (x, y): Pillow's binding truncates coordinates toward zero"""
    if isinstance(path_or_dict, dict):
        d = path_or_dict
    else:
        with open(path_or_dict) as f:
            d = json.load(f)
    objects = []
    for o in d["objects"]:
        objects.append({"label": str(o["label"]), "polygon": [(int(p[0]), int(p[1])) for p in o["polygon"]],
                        "deleted": bool(int(o.get("deleted", 0)))})
    return {"imgWidth": int(d["imgWidth"]), "imgHeight": int(d["imgHeight"]), "objects": objects}


def drawn_objects(annotation):
    """-> [(polygon, (labelId, labelTrainId, instanceId, instanceTrainId))] of the objects the scripts draw, in file
    order: deleted objects are skipped, `<label>group` of an unknown label is the label without instance numbers, any
    other unknown label is an error, instances of a has_instances class are numbered per class in file order, and an
    object whose id is negative is not drawn (it still takes its number)"""
    counts = {}
    out = []
    for o in annotation["objects"]:
        if o["deleted"]:
            continue
        label, group = o["label"], False
        if label not in _BY_NAME and label.endswith("group"):
            label, group = label[:-len("group")], True
        if label not in _BY_NAME:
            raise ValueError("Label '%s' not known." % label)
        lab = _BY_NAME[label]
        inst, inst_train = lab.id, lab.train_id
        if lab.has_instances and not group:
            n = counts.get(label, 0)
            counts[label] = n + 1
            inst, inst_train = lab.id * 1000 + n, lab.train_id * 1000 + n
        if lab.id < 0:
            continue
        if len(o["polygon"]) < 2:
            raise ValueError("polygon of '%s' has %d point(s): Pillow refuses fewer than 2" % (o["label"], len(o["polygon"])))
        out.append((o["polygon"], (lab.id, lab.train_id, inst, inst_train)))
    return out


def _round_half_up(f):
    return np.where(f >= 0, np.floor(f + np.float32(0.5)), -np.floor(np.abs(f) + np.float32(0.5))).astype(np.int64)


def _crossing(y, y0, dx, x0):
    return (y - y0).astype(np.float32) * dx + x0.astype(np.float32)        # two float32 roundings, as Pillow's C


def polygon_tables(polygons, images, orders, H, W, wave_entries):
    """polygons: list of integer point lists; images / orders: per polygon.  -> (edges (E, 8), polys (P, 4), jobs (J, 5))
    int32 arrays of include/dspn_polygon.h and the number of scratch floats the spilling jobs address"""
    P = len(polygons)
    counts = np.array([len(p) for p in polygons], np.int64)
    if P == 0 or int(counts.sum()) == 0:
        return np.zeros((0, 8), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 5), np.int32), 0
    if counts.min() < 2:
        raise ValueError("a polygon needs at least 2 points")
    pts = np.concatenate([np.asarray(p, np.int64).reshape(-1, 2) for p in polygons])
    if np.abs(pts).max() >= _COORD_LIMIT:
        raise ValueError("polygon coordinate beyond +-%d" % _COORD_LIMIT)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    poly = np.repeat(np.arange(P), counts)
    idx = np.arange(len(pts))
    nxt = idx + 1
    last = start + counts - 1
    nxt[last] = start
    keep = np.ones(len(pts), bool)
    keep[last] = (pts[last] != pts[start]).any(axis=1)                      # the closing edge, only if the ends differ
    a, b, poly = pts[keep], pts[nxt[keep]], poly[keep]
    E = len(a)
    per_poly = np.bincount(poly, minlength=P)
    e_begin = np.concatenate([[0], np.cumsum(per_poly)[:-1]])
    x0, y0, x1, y1 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    ymin, ymax = np.minimum(y0, y1), np.maximum(y0, y1)
    flat = y0 == y1
    dx = np.zeros(E, np.float32)
    dx[~flat] = (x1 - x0)[~flat].astype(np.float32) / (y1 - y0)[~flat].astype(np.float32)

    # the corner rule: per edge and end, the first earlier slanted edge of the polygon with the same vertex at that end
    slanted = ~flat & (dx != 0)
    entries = {}
    e_idx = np.arange(E)
    down = y0 < y1
    for off in (1, -1):
        upper_is_a = down == (off == 1)
        vx, vy = np.where(upper_is_a, x0, x1), np.where(upper_is_a, y0, y1)
        entry = np.full(E, _NAN, np.float32)
        cand = e_idx[slanted]
        if len(cand):
            _, inv = np.unique(np.stack([poly[cand], vx[cand], vy[cand]], 1), axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            first = np.full(inv.max() + 1, E, np.int64)
            np.minimum.at(first, inv, cand)
            k = first[inv]
            sel = (k < cand) & ((dx[k] > 0) == (dx[cand] > 0))
            c, k = cand[sel], k[sel]
            row = vy[c] + off
            ca, cb = _crossing(row, y0[c], dx[c], x0[c]), _crossing(row, y0[k], dx[k], x0[k])
            right = (off == -1) == (dx[c] > 0)
            r = np.where(right, _round_half_up(np.maximum(ca, cb)) + 1, _round_half_up(np.minimum(ca, cb)) - 1)
            ok = np.where(right, r <= vx[c], r >= vx[c])
            entry[c[ok]] = r[ok].astype(np.float32)
        entries[off] = entry
    edges = np.zeros((E, 8), np.int32)
    edges[:, 0], edges[:, 1], edges[:, 2], edges[:, 3] = x0, y0, ymin, ymax
    edges[:, 4], edges[:, 5], edges[:, 6] = dx.view(np.int32), entries[1].view(np.int32), entries[-1].view(np.int32)
    edges[:, 7] = x1

    # rows: Pillow starts from ymin = H - 1, ymax = 0 and clips to 0 .. H; row H is outside the image
    p_ymin = np.full(P, H - 1, np.int64)
    p_ymax = np.zeros(P, np.int64)
    np.minimum.at(p_ymin, poly, ymin)
    np.maximum.at(p_ymax, poly, ymax)
    last_row = np.minimum(p_ymax, H)
    ylo, yhi = np.maximum(p_ymin, 0), np.minimum(p_ymax, H - 1)
    rows = np.maximum(yhi - ylo + 1, 0)
    polys = np.stack([e_begin, e_begin + per_poly, np.asarray(images, np.int64), np.asarray(orders, np.int64)], 1).astype(np.int32)
    J = int(rows.sum())
    if J == 0:
        return edges, polys, np.zeros((0, 5), np.int32), 0
    j_begin = np.concatenate([[0], np.cumsum(rows)[:-1]])
    j_poly = np.repeat(np.arange(P), rows)
    j_y = np.arange(J) - j_begin[j_poly] + ylo[j_poly]
    # an upper bound of each row's entries: active slanted-or-vertical edges, one more for each that ends there
    diff = np.zeros(J + 1, np.int64)
    ends = np.zeros(J, np.int64)
    nf = e_idx[~flat]
    lo, hi = np.maximum(ymin[nf], ylo[poly[nf]]), np.minimum(ymax[nf], yhi[poly[nf]])
    on = lo <= hi
    base = (j_begin - ylo)[poly[nf]]
    np.add.at(diff, (base + lo)[on], 1)
    np.add.at(diff, (base + hi + 1)[on], -1)
    end_on = (ymax[nf] >= ylo[poly[nf]]) & (ymax[nf] <= yhi[poly[nf]])
    np.add.at(ends, (base + ymax[nf])[end_on], 1)
    n = np.cumsum(diff)[:J] + ends
    spill = n > wave_entries
    offs = np.zeros(J, np.int64)
    offs[spill] = np.cumsum(2 * n[spill]) - 2 * n[spill]
    scratch_floats = int((2 * n[spill]).sum())
    if scratch_floats >= 1 << 31:
        raise ValueError("polygon rows with %d entries in all: too many for one call" % (scratch_floats // 2))
    jobs = np.stack([j_poly, j_y, last_row[j_poly], n, offs], 1).astype(np.int32)
    return edges, polys, jobs, scratch_floats


def rasterize(polygons, images, orders, B, H, W, device=None, spill_count=None):
    """integer polygons, each with its image index and order (>= 1) -> owner (B, H, W) int32 on the device"""
    device = torch.device("cuda" if device is None else device)
    edges, polys, jobs, scratch_floats = polygon_tables(polygons, images, orders, H, W, fn.polygon_wave_entries())
    up = [torch.from_numpy(t).to(device) for t in (edges, polys, jobs)]
    if spill_count is None:
        spill_count = torch.zeros(1, dtype=torch.int32, device=device)
    return fn.polygon_rasterize(up[0], up[1], up[2], scratch_floats, B, H, W, spill_count=spill_count)


def label_maps(annotations, device=None):
    """annotations of one image size (load_annotation's dicts, or paths) -> {"labelIds", "labelTrainIds": (B, H, W) uint8,
    "instanceIds", "instanceTrainIds": (B, H, W) int32} device tensors: what createLabelImage / createInstanceImage
    paint for the encodings "ids" and "trainIds"."""
    anns = [load_annotation(a) for a in annotations]
    if not anns:
        raise ValueError("label_maps: no annotation")
    H, W = anns[0]["imgHeight"], anns[0]["imgWidth"]
    unlabeled = _BY_NAME["unlabeled"]
    polygons, images, orders, table, offsets = [], [], [], [], []
    for b, ann in enumerate(anns):
        if (ann["imgHeight"], ann["imgWidth"]) != (H, W):
            raise ValueError("label_maps: images of one size per call, got %dx%d and %dx%d"
                             % (W, H, ann["imgWidth"], ann["imgHeight"]))
        offsets.append(len(table))
        table.append((unlabeled.id, unlabeled.train_id, unlabeled.id, unlabeled.train_id))
        for order, (polygon, values) in enumerate(drawn_objects(ann), 1):
            polygons.append(polygon)
            images.append(b)
            orders.append(order)
            table.append(values)
    device = torch.device("cuda" if device is None else device)
    owner = rasterize(polygons, images, orders, len(anns), H, W, device)
    lab, lab_t, inst, inst_t = fn.polygon_resolve(owner, torch.tensor(table, dtype=torch.int32, device=device),
                                                  torch.tensor(offsets, dtype=torch.int32, device=device))
    return {"labelIds": lab, "labelTrainIds": lab_t, "instanceIds": inst, "instanceTrainIds": inst_t}


def _as_uint16(t, what):
    """(H, W) int32 device map -> uint16 of the same values; a value that does not fit is an error"""
    top = int(t.max().item()) if t.numel() else 0
    if top > 65535 or (t.numel() and int(t.min().item()) < 0):
        raise ValueError("%s: value %d does not fit a 16-bit PNG" % (what, top))
    return t.view(torch.int16)[..., 0::2].contiguous().view(torch.uint16)      # the low half of each little-endian word


def output_path(json_path, kind, out_dir=None):
    """createTrainIdLabelImgs.py's naming: `_polygons.json` -> `_<kind>.png`, beside the JSON or under out_dir"""
    dst = json_path.replace("_polygons.json", "_%s.png" % kind)
    return dst if out_dir is None else os.path.join(out_dir, os.path.basename(dst))


def write_label_images(json_paths, out_dir=None, kinds=KINDS, device=None, batch=8, compress_level=6):
    """polygon files -> the scripts' PNG files, label maps as 8-bit and instance maps as 16-bit grey; returns the paths
    written.  Files of one size are rasterised `batch` at a time."""
    from ..detect import render
    for k in kinds:
        if k not in KINDS:
            raise ValueError("write_label_images: kind %r is none of %s" % (k, ", ".join(KINDS)))
    json_paths = list(json_paths)
    anns = [load_annotation(p) for p in json_paths]
    by_size = {}
    for i, a in enumerate(anns):
        by_size.setdefault((a["imgHeight"], a["imgWidth"]), []).append(i)
    written = []
    for members in by_size.values():
        for s in range(0, len(members), batch):
            chunk = members[s:s + batch]
            maps = label_maps([anns[i] for i in chunk], device)
            paths, tensors = [], []
            for n, i in enumerate(chunk):
                for k in kinds:
                    dst = output_path(json_paths[i], k, out_dir)
                    t = maps[k][n]
                    paths.append(dst)
                    tensors.append(_as_uint16(t, dst) if k.startswith("instance") else t)
            render.save_pngs(paths, tensors, compress_level=compress_level)
            written += paths
    return written


def _half(v):
    """Python 2's int(round(v / 2)): `/` floors on integers, round() takes halves away from zero"""
    return int(v) // 2 if isinstance(v, (int, np.integer)) else round_half_away(v / 2)


def polygon_boxes(path_or_dict):
    """dataset/cs_json2xml.py's <size> and <bndbox> of every object (deleted ones included, as the script's), from the
    raw polygon file: {"width", "height", "boxes": [(label, xmin, ymin, xmax, ymax)]}, all at half size"""
    if isinstance(path_or_dict, dict):
        d = path_or_dict
    else:
        with open(path_or_dict) as f:
            d = json.load(f)
    width, height = _half(d["imgWidth"]), _half(d["imgHeight"])
    boxes = []
    for o in d["objects"]:
        xmin, ymin, xmax, ymax = width, height, 0, 0
        for p in o["polygon"]:
            x, y = _half(p[0]), _half(p[1])
            xmin, xmax, ymin, ymax = min(xmin, x), max(xmax, x), min(ymin, y), max(ymax, y)
        boxes.append((str(o["label"]), xmin, ymin, xmax, ymax))
    return {"width": width, "height": height, "boxes": boxes}
