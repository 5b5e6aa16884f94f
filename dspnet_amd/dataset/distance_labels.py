"""The <distance> tag of the dataset preparation (data/cityscapes/disparity2distance.py:55-73): for every ground-truth
box the distance 2200 * 75 / (median disparity in the box + 1e-3), > 1000 -> 200, rounded to an integer.  The median
is the element of rank n // 2 of the box's pixels (the script ran under Python 2: `roi.shape[1]/2` is a floor division),
taken on the device by dspn_box_rank_select_* (include/dspn_distance.h); the arithmetic after it is the script's, in
Python doubles."""
import math

import numpy as np
import torch

from .. import functional as fn


def resolve_boxes(boxes_px, hh, ww):
    """(K, 4) integer [xmin, ymin, xmax, ymax] -> (K, 4) int32 [x0, x1, y0, y1]: the slices the script cuts
    (disparity2distance.py:61-64): mins clamped at 0, an empty column range widened to one pixel, then numpy's slicing"""
    out = np.zeros((len(boxes_px), 4), np.int32)
    for k, (xmin, ymin, xmax, ymax) in enumerate(np.asarray(boxes_px).reshape(-1, 4).tolist()):
        xmin, ymin = max(0, int(xmin)), max(0, int(ymin))
        xmax, ymax = int(xmax), int(ymax)
        if xmin == xmax:
            xmax = xmin + 1
        out[k, 0:2] = fn.slice_bounds(xmin, xmax, ww)
        out[k, 2:4] = fn.slice_bounds(ymin, ymax, hh)
    return out


def round_half_away(v):
    """Python 2's round(): halves go away from zero (Python 3 rounds them to even)"""
    a = math.floor(abs(v))
    if abs(v) - a >= 0.5:
        a += 1
    return int(math.copysign(a, v))


def distance_from_median(q):
    """disparity2distance.py:67-73 after the selection: the integer the script writes"""
    dist = 2200. * 75. / (float(q) + 1e-3)
    if dist > 1000:
        dist = 200
    return round_half_away(dist)


def box_distances(disparity, boxes_px, device=None):
    """disparity: one (hh, ww) map, uint16 or float32 (numpy array or tensor); boxes_px: (K, 4) integer
    [xmin, ymin, xmax, ymax] -> list of K integers, the <distance> values.  A box whose region is empty raises
    ValueError (the script indexes an empty array there)."""
    t = disparity if hasattr(disparity, "detach") else torch.from_numpy(np.ascontiguousarray(disparity))
    if t.dim() != 2:
        raise ValueError("box_distances: one (hh, ww) map, got %s" % (tuple(t.shape),))
    if t.dtype not in (torch.uint16, torch.float32):
        t = t.to(torch.float32)                              # the script's astype(np.float32)
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    hh, ww = t.shape
    res = resolve_boxes(boxes_px, hh, ww)
    empty = [k for k, (x0, x1, y0, y1) in enumerate(res.tolist()) if x1 == x0 or y1 == y0]
    if empty:
        raise ValueError("box_distances: box %d covers no pixel of the %d x %d map" % (empty[0], hh, ww))
    if len(res) == 0:
        return []
    table = np.concatenate([np.zeros((len(res), 1), np.int32), res], 1)
    q, _ = fn.box_rank_select(t.detach().to(device).contiguous()[None], torch.from_numpy(table).to(device))
    return [distance_from_median(v) for v in q.cpu().tolist()]


def save_maps(paths, maps, compress_level=6, device_deflate=False):
    """writes a batch of (hh, ww) uint16 disparity or distance maps (device or host; a (B, hh, ww) tensor or a list) as
    16-bit greyscale PNG files, the format the dataset keeps them in: one device filter call for the batch (png_encode);
    device_deflate=True keeps the deflate on the device as well (detect.render.save_pngs' keyword)"""
    from ..detect.render import save_pngs
    maps = list(maps)
    bad = [tuple(m.shape) for m in maps if str(m.dtype).replace("torch.", "") != "uint16" or len(m.shape) != 2]
    if bad:
        raise ValueError("save_maps: (hh, ww) uint16 maps, got %s among them" % (bad[0],))
    save_pngs(paths, maps, compress_level, device_deflate=device_deflate)
