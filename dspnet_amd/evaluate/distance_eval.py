"""DistanceAccuracyMetric with the per-box selection on the device (include/dspn_distance.h).

The host class (train.metric.DistanceAccuracyMetric, the reference's train/metric.py:135-260) cuts every detection's
box out of the disparity map and takes the element of rank n // 2.  Here the maps stay on the device:
dspn_distance_boxes_f32 turns the detection rows into pixel boxes in the host loop's order, dspn_box_rank_select_*
returns that element q and the pixel count n per box, and after the four bytes of the row count one device-to-host copy
brings (q, n, source row) plus the class id and predicted distance of the rows selected.  Everything after q runs here in
Python doubles, in the host class's order, so sum_metric, num_inst, errors and get() carry the same bits."""
import math

import numpy as np
import torch

from .. import functional as fn
from ..train.metric import DistanceAccuracyMetric


class DeviceDistanceAccuracyMetric(DistanceAccuracyMetric):
    """reset / get / names / values of the host class.  max_boxes: room of the box table of one update.  None (the default)
    sizes it from the detections of the update, B * N rows, which no selection can exceed: the detection output keeps
    valid ids and scores in its rows past nms_topk, so the rows that pass score_thresh are bounded by the anchors only.
    With a number, an update that selects more rows raises DspnError; nothing is truncated."""

    def __init__(self, class_names, name="derror", dump_errors=None, max_boxes=None, device=None):
        self.max_boxes = None if max_boxes is None else int(max_boxes)
        self.device = torch.device(device) if device is not None else None
        self._buf = None
        self.last_boxes = 0
        super().__init__(class_names, name=name, dump_errors=dump_errors)

    def _buffers(self, device, K):
        if self._buf is None or self._buf[0].device != device or self._buf[0].shape[0] < K:
            i32 = dict(dtype=torch.int32, device=device)
            self._buf = (torch.zeros(K, 5, **i32), torch.zeros(K, **i32), torch.zeros(1, **i32),
                         torch.zeros(K, dtype=torch.float32, device=device), torch.zeros(K, **i32))
        return self._buf

    def _maps(self, labels, device):
        """(B, hh, ww) uint16 or float32 device maps from a host array or a tensor (other types are read as float32, the
        host class's astype)"""
        t = labels if hasattr(labels, "detach") else torch.from_numpy(np.ascontiguousarray(labels))
        if t.dtype not in (torch.uint16, torch.float32):
            t = t.to(torch.float32)
        return t.detach().to(device).contiguous()

    def _device_of(self, *tensors):
        if self.device is not None:
            return self.device
        for t in tensors:
            if hasattr(t, "is_cuda") and t.is_cuda:
                return t.device
        return torch.device("cuda", torch.cuda.current_device())

    def _score(self, maps, det, mode, score_thresh, map_index=None):
        """maps (B, hh, ww), det (Bd, N, 7) device tensors; map_index: the map of each det image (None: image b, map b)"""
        room = det.shape[0] * det.shape[1] if self.max_boxes is None else self.max_boxes
        boxes, src, count, q, n = self._buffers(det.device, room)
        _, hh, ww = maps.shape
        fn.distance_boxes(det, hh, ww, score_thresh, mode, room, out=(boxes, src, count), sync=False)
        K = int(count.item())                               # four bytes: all that follows is sized by the rows selected,
        fn.check_box_count(K, room)                         # not by the room of the table
        self.last_boxes = K
        boxes, src = boxes[:K], src[:K].long()
        if map_index is not None:
            boxes[:, 0] = map_index[boxes[:, 0].long()]
        fn.box_rank_select(maps, boxes, out=(q, n))
        rows = det.view(-1, 7)[src]
        f64 = torch.float64
        packed = torch.stack((q[:K].to(f64), n[:K].to(f64), src.to(f64), rows[:, 0].to(f64), rows[:, 6].to(f64)), 1)
        host = packed.cpu().tolist()                        # the one copy of the table: K rows
        error = [[] for _ in range(self.num - 1)]
        for qv, nv, _, cls, pred in host:
            if nv == 0:
                continue
            dist = 2200. * 75. / (qv + 1e-3)
            if dist > 1000:
                dist = 200
            if dist > 199:
                continue
            error[int(cls)].append(math.fabs(pred * 255. - dist) / dist)
        for i in range(self.num - 1):
            self.sum_metric[i] += math.fsum(error[i])
            self.num_inst[i] += len(error[i])
            self.errors += error[i]
        self.sum_metric[self.num - 1] += math.fsum([math.fsum(e) for e in error])
        self.num_inst[self.num - 1] += math.fsum([len(e) for e in error])

    def update(self, labels, preds):
        """the host class's contract: labels (B, hh, ww) maps (numpy array or tensor, uint16 or float32), preds a list of
        (n, N, 7) detections paired with the maps as `zip(labels, preds)` pairs them; rows up to the first id < 0"""
        device = self._device_of(labels, *preds)
        maps = self._maps(labels, device)
        dets, index = [], []
        for i, d in zip(range(maps.shape[0]), preds):
            d = d if hasattr(d, "detach") else torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))
            d = d.detach().to(device=device, dtype=torch.float32)
            d = d.reshape((-1,) + tuple(d.shape[-2:]))
            dets.append(d)
            index += [i] * d.shape[0]
        if not dets:
            return
        N = max(d.shape[1] for d in dets)
        if any(d.shape[1] != N for d in dets):              # short tables end with id < 0 rows, as the loop's break reads them
            dets = [torch.cat([d, d.new_full((d.shape[0], N - d.shape[1], 7), -1.0)], 1) for d in dets]
        det = torch.cat(dets, 0).contiguous()
        identity = index == list(range(len(index)))
        self._score(maps, det, 0, 0.0, None if identity else torch.tensor(index, dtype=torch.int32, device=device))

    def update_filtered(self, disparity, det, score_thresh):
        """what evaluate_net uses: det (B, N, 7) is the network's unfiltered device output, image b against map b; the rows
        with id >= 0 and score > score_thresh are scored (filter_detections followed by the host class's update)"""
        device = self._device_of(det, disparity)
        det = det.detach().to(device=device, dtype=torch.float32).contiguous()
        self._score(self._maps(disparity, device), det, 1, float(score_thresh))
