"""Evaluation loop of multi_eval.py (evaluate_net, :156-425) over this build's graph.

What the reference does per batch, and where it runs here:
  forward of the TRAINING symbol with is_train=True (:312)                 -> net.g.forward() (HIP graph)
  MultiBoxMetric over cls_prob / loc_loss / cls_label (:372-374)           -> train.metric.MultiBoxMetric (device sums)
  CustomAccuracyMetric + IoUMetric over seg_out (:375, :378)               -> dspn_seg_counts_f32 (device counts)
  detections with id >= 0 and score > .1 (:329-335), MApMetric (:376-377)  -> host, a few hundred rows
  seg probabilities upsampled to 1024x2048 + argmax (:28-34, :355)         -> dspn_seg_upsample_argmax_f32 (fused)
  DistanceAccuracyMetric against the disparity maps (:379-384)             -> host, as in the reference; with
      device_depth=True the box medians come from the device (evaluate.distance_eval, dspn_box_rank_select_*)
  (offline, on the PNGs the script writes) Cityscapes IoU / iIoU           -> evaluate.cityscapes_eval (device counts)
  result images (:344-368): the labelId map at full resolution and the 2 x 2 display mosaic, per image
                                                                           -> results_dir=...: label_ids(prob_upsampling)
      and detect.render.display_results (device), written as PNG files (device_png=True: filtered on the device, a batch
      at a time); no window is opened"""
import os

import numpy as np
import torch

from .. import functional as fn
from ..train.metric import CustomAccuracyMetric, DistanceAccuracyMetric, IoUMetric, MultiBoxMetric
from .eval_metric import MApMetric, VOC07MApMetric

# trainId -> labelId table the script applies before writing result images (multi_eval.py:352-353)
CITYSCAPES_LABEL_IDS = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)


def prob_upsampling(seg_prob, target_shape=(1024, 2048), num_classes=19):
    """multi_eval.py:28-34: class map (uint8) of the probabilities sampled bilinearly at target_shape.
    seg_prob: device tensor, NHWC (B, h, w, ld) as the graph holds it, or NCHW (C, h, w) / (B, C, h, w) as the
    reference passes it.  Returns (B, H, W) uint8 on the device (squeezed to (H, W) for a single 3-d input)."""
    squeeze = seg_prob.dim() == 3
    if squeeze:
        seg_prob = seg_prob.unsqueeze(0)
    if seg_prob.shape[1] == num_classes and seg_prob.shape[-1] != fn.pad4(num_classes):        # NCHW
        seg_prob = fn.nchw_to_nhwc(seg_prob.contiguous(), Cp=fn.pad4(num_classes))
    out = fn.seg_upsample_argmax(seg_prob.contiguous(), num_classes, int(target_shape[0]), int(target_shape[1]))
    return out[0] if squeeze else out


def label_ids(class_map):
    """trainId map -> Cityscapes labelId map (the cv2.LUT of multi_eval.py:352-356), on the device"""
    lut = torch.zeros(256, dtype=torch.uint8, device=class_map.device)
    lut[:19] = torch.tensor(CITYSCAPES_LABEL_IDS, dtype=torch.uint8, device=class_map.device)
    return lut[class_map.long()]


def filter_detections(det, score_thresh=0.1):
    """multi_eval.py:329-335: keep rows with id >= 0, then score > score_thresh.  det (B, N, 7) device or host.
    -> host float32 (B, kmax, 7), short images padded with -1 rows (B = 1 reproduces the reference's array)."""
    det = det.detach().cpu().numpy() if hasattr(det, "detach") else np.asarray(det)
    rows = [d[(d[:, 0] >= 0)] for d in det]
    rows = [d[d[:, 1] > score_thresh] for d in rows]
    kmax = max([r.shape[0] for r in rows] + [0])
    out = np.full((det.shape[0], kmax, det.shape[2]), -1.0, np.float32)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


def evaluate_net(net, batches, class_names, seg_class_names, ovp_thresh=0.5, use_difficult=False,
                 voc07_metric=False, full_res=None, score_thresh=0.1, cityscapes=False, device_depth=False,
                 results_dir=None, device_png=False, device_deflate=False):
    """net: training graph (symbol.multitask_symbol_factory.get_multi_symbol_train); batches: iterable of dicts with
    'data' (B,3,H,W), 'label_det' (B,L,6), 'label_seg' (B,H/4,W/4) and optionally 'disparity' (B,hh,ww) host maps.
    -> dict name -> value, plus 'class_maps' (list of uint8 device tensors) when full_res=(H, W) is given.
    cityscapes=True: every batch also carries 'gt_label_ids' (B, H, W) uint8 and 'gt_instance_ids' (B, H, W) int32, the
    *_gtFine_labelIds / *_gtFine_instanceIds images at full resolution (full_res when that is given); the dict gains the
    scores of the dataset's pixel-level evaluation script, 'cityscapes/IoU_class', 'cityscapes/iIoU_class',
    'cityscapes/IoU_category', 'cityscapes/iIoU_category' and the per-class 'cityscapes/IoU/<name>' / 'cityscapes/iIoU/<name>'
    (cityscapes_eval.CityscapesPixelMetric, fed from the probabilities without writing a class map).
    device_depth=True: the distance metric reads the device's unfiltered detections and takes every box median on the
    device (distance_eval.DeviceDistanceAccuracyMetric; 'disparity' may then be a device tensor, uint16 or float32);
    the box table is sized from det_out, B * N rows, so no batch the host path scores can overflow it; the values are
    those of the host metric, which stays the default.
    results_dir: a directory; per image the script's two files (multi_eval.py:355, :366) are written below it:
    results/<name>, the labelId map at full_res (default 1024 x 2048), and output/<name with labelTrainIds -> output>, the
    display_results mosaic.  <name> is the base name of batch['fnames'][i] (the label image's path, as the iterator gives
    it), or '%06d_gtFine_labelTrainIds.png' of the running image index.  None (the default) launches nothing, imports
    nothing and writes nothing.
    device_png=True: the files of a batch are written by one detect.render.save_pngs call (row filters on the device, deflate
    on a thread pool) in place of two Pillow saves per image; same names, same pixels.
    device_deflate=True (with device_png=True; a ValueError without it): that call deflates on the device as well
    (dataset/png_encode.py); same names, same pixels, larger files."""
    if device_deflate and not device_png:
        raise ValueError("evaluate_net: device_deflate=True needs device_png=True (it is a switch of the device PNG writer)")
    render = image_index = None
    if results_dir is not None:
        from ..detect import render
        image_index = 0
        for sub in ("results", "output"):
            os.makedirs(os.path.join(results_dir, sub), exist_ok=True)
    multibox_metric = MultiBoxMetric()
    acc_metric = CustomAccuracyMetric(num_classes=len(seg_class_names))
    if device_depth:
        from .distance_eval import DeviceDistanceAccuracyMetric
        depth_metric = DeviceDistanceAccuracyMetric(class_names=list(class_names), device=net.det.out.data.device)
    else:
        depth_metric = DistanceAccuracyMetric(class_names=list(class_names))
    det_metric = (VOC07MApMetric if voc07_metric else MApMetric)(ovp_thresh, use_difficult, list(class_names))
    seg_metric = IoUMetric(class_names=list(seg_class_names), axis=1)
    class_maps = []
    city_metric = None
    if cityscapes:
        from .cityscapes_eval import CityscapesPixelMetric
        city_metric = CityscapesPixelMetric(device=net.seg_out.prob.data.device)
    for batch in batches:
        net.data.data.copy_(batch["data"])
        net.label_det.data.copy_(batch["label_det"])
        net.label_seg.data.copy_(batch["label_seg"])
        net.g.forward()
        net.det.join()
        multibox_metric.update(net)
        seg_prob = net.seg_out.prob.data                     # (B, h, w, ld) NHWC probabilities
        acc_metric.update([net.label_seg.data], [seg_prob])
        seg_metric.update([net.label_seg.data], [seg_prob])
        pred_det = filter_detections(net.det.out.data, score_thresh)
        det_metric.update([batch["label_det"][:, :, :5]], [pred_det[:, :, :6]])
        if full_res is not None:
            class_maps.append(prob_upsampling(seg_prob, full_res, len(seg_class_names)))
        if render is not None:
            ids = label_ids(class_maps[-1] if full_res is not None else
                            prob_upsampling(seg_prob, (1024, 2048), len(seg_class_names)))
            mosaic = render.display_results(net.data.data, net.label_seg.data, seg_prob, list(pred_det), net.label_det.data,
                                            list(class_names), num_classes=len(seg_class_names))
            paths, images = [], []
            for i in range(mosaic.shape[0]):
                name = (os.path.basename(batch["fnames"][i]) if batch.get("fnames") else
                        "%06d_gtFine_labelTrainIds.png" % image_index)
                paths += [os.path.join(results_dir, "results", name),
                          os.path.join(results_dir, "output", name.replace("labelTrainIds", "output"))]
                images += [ids[i], mosaic[i]]
                image_index += 1
            if device_png:
                render.save_pngs(paths, images, device_deflate=device_deflate)
            else:
                for path, image in zip(paths, images):
                    render.save_png(path, image)
        if city_metric is not None:
            gt_ids = batch["gt_label_ids"]
            if full_res is not None and tuple(gt_ids.shape[-2:]) != tuple(int(v) for v in full_res):
                raise ValueError("evaluate_net: gt_label_ids are %s, full_res is %s" % (tuple(gt_ids.shape[-2:]), tuple(full_res)))
            city_metric.update_from_prob(seg_prob, gt_ids, batch["gt_instance_ids"], num_classes=len(seg_class_names))
        if batch.get("disparity") is not None:
            if device_depth:
                depth_metric.update_filtered(batch["disparity"], net.det.out.data, score_thresh)
            else:
                depth_metric.update(batch["disparity"], list(pred_det[:, None]))
    out = {}
    names, values = multibox_metric.get()
    out.update(zip(names, values))
    name, value = acc_metric.get()
    out[name] = value
    for m in (det_metric, seg_metric, depth_metric):
        names, values = m.get()
        out.update(zip(names, values))
    if full_res is not None:
        out["class_maps"] = class_maps
    if city_metric is not None:
        out.update(city_metric.get_name_value())
    return out
