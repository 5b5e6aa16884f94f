"""Inference wrapper: what `Detector` feeds and reads in the reference.

detect/multitask_detector.py:99-163 loads the saved TRAINING symbol, binds zero `label_det (B,200,6)` and
`seg_out_label`, runs forward(is_train=True) per image and reads outputs[3] (det_out) and outputs[4]
(seg probabilities); rows with id >= 0 are detections (:268-271) and the seg map is the arg-max over
the class axis (:263).  det_out does not depend on MultiBoxTarget, so this forward-only path runs the
test graph (`get_multi_symbol`): same det / seg values, no target / loss kernels.  Image decoding (cv2.imread,
cv2.VideoCapture) stays outside; the demo's picture -- resize, boxes, class colours, legend -- is made on the device
(`visualize_detection` / `detect_and_visualize`, detect/render.py)."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .. import functional as fn
from ..symbol.multitask_symbol_factory import get_multi_symbol

MEAN_RGB = (123.0, 117.0, 104.0)


class Detector:
    def __init__(self, network="resnet-50", data_shape=512, num_classes=8, batch_size=1, mean_pixels=MEAN_RGB,
                 nms_thresh=0.5, force_suppress=False, nms_topk=400, device=None, params=None, seed=0,
                 model_prefix=None, epoch=0, use_global_stats=False, aux_params=None):
        """use_global_stats: every BatchNorm normalises with its moving statistics (the checkpoint's aux states, or
        aux_params), so that a detection does not depend on the other images of the batch; default: batch statistics,
        as the reference's forward(is_train=True).  aux_params ('<bn>_moving_mean' / '<bn>_moving_var') are loaded
        after the checkpoint's."""
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.net = get_multi_symbol(network, data_shape, num_classes=num_classes, batch_size=batch_size,
                                    nms_thresh=nms_thresh, force_suppress=force_suppress, nms_topk=nms_topk,
                                    device=self.device, seed=seed, use_global_stats=use_global_stats)
        if params:
            self.net.g.load_params(params)
        if model_prefix is not None:   # mx.model.load_checkpoint(model_prefix, epoch) (detect/multitask_detector.py:105)
            from ..model import load_checkpoint
            _, args, auxs = load_checkpoint(model_prefix, epoch)
            self.net.g.set_params(args)
            # (a global-statistics net needs every BatchNorm's statistics; a batch-statistics one does not read them)
            self.net.g.set_aux(auxs, allow_missing=not (use_global_stats and aux_params is None))
        if aux_params is not None:
            self.net.g.set_aux(aux_params, allow_missing=not use_global_stats)
        self.mean = torch.tensor(mean_pixels, dtype=torch.float32, device=self.device).view(1, 3, 1, 1)
        self.mean_pixels = tuple(float(m) for m in mean_pixels)

    def forward(self, data=None):
        """data: (B,3,H,W) float32 device tensor, RGB, mean already subtracted (dataset/iterator.py:570-571)"""
        if data is not None:
            self.net.data.data.copy_(data)
        g = self.net.g
        if g.scalars is not None and g.guard["enabled"] and not g.guard["have_stats"]:
            # range guard of the default math (advisor r5): the very first batch of a freshly loaded net has no spans to decide
            # from -- one extra forward measures them (inputs, weights), the next decides from that pass before it runs
            g.forward()
            g.guard["decide_now"] = True
        g.forward()
        self.net.det.join()        # MultiBoxDetection runs on a side stream beside the seg decoder
        return self.net.det.out.data, self.net.seg_out.prob.data

    def detect(self, data, thresh=0.0):
        """-> (list of per-image (k,7) tensors [id, score, xmin, ymin, xmax, ymax, dist] with id >= 0 and
        score > thresh, seg probabilities (B,19,H/4,W/4))"""
        det, _ = self.forward(data)
        det = det.cpu()
        out = []
        for b in range(det.shape[0]):
            rows = det[b]
            out.append(rows[(rows[:, 0] >= 0) & (rows[:, 1] > thresh)])
        return out, fn.nhwc_to_nchw(self.net.seg_out.prob.data, self.net.seg_out.C)

    def visualize_detection(self, img, dets, seg_prob, classes, thresh=0.6):
        """detect/multitask_detector.py:336-399 on the device -> (B, H + H + 30, W, 3) uint8 RGB: the image with boxes and
        tags, the class colours at image size, the legend.  img: device uint8 (B, H, W, 3) RGB frames, or the net's input
        (B, 3, H, W) float32, shown with this detector's mean added back; dets: (B, N, 7) or per-image (k, 7) row tables;
        seg_prob: (B, h, w, ld) NHWC scores as `forward` returns them.  Nothing is displayed or written (render.save_png)."""
        from . import render
        return render.visualize_detection(img, dets, seg_prob, classes, thresh, mean=self.mean_pixels,
                                          num_classes=self.net.seg_out.C)

    def detect_and_visualize(self, frames, classes, thresh=0.6, nms_thresh=0.95):
        """the video branch of detect_and_visualize (:433-456) for a batch of decoded frames: uint8 (B, Hs, Ws, 3) BGR,
        host or device -> (B, H + H + 30, W, 3) uint8 RGB on the device.
        The reference resizes a frame (`resize(img, 600, 1024)`), crops rows [64:576] unless the aspect is 2, and feeds the
        result to a net bound to that size.  Here `frame_warp` composes that rule with the scale onto this net's (H, W)
        -- the identity for the 512 x 1024 model on 16:9 video -- into one affine map, and the existing
        dspn_augment_batch_u8 applies it as a pure scale warp (the `_get_resized` convention: bilinear, border 0, BGR ->
        RGB planes, mean subtracted): one interpolation where the reference chains two.  Then forward, the pixel NMS
        post-filter on [xmin, ymin, xmax, ymax, score] at nms_thresh (:450), and the picture."""
        from ..dataset import iterator as it
        from .nms import nms
        frames = torch.as_tensor(frames)
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
            raise _lib.DspnError("detect_and_visualize: frames are uint8 (B, Hs, Ws, 3)")
        B, _, H, W = self.net.data.data.shape
        if frames.shape[0] != B:
            raise _lib.DspnError("detect_and_visualize: %d frames for a net of batch size %d" % (frames.shape[0], B))
        Hs, Ws = int(frames.shape[1]), int(frames.shape[2])
        frames = frames.to(self.device).contiguous()
        samples = np.zeros(B, it._SAMPLE)
        samples["img_offset"] = np.arange(B, dtype=np.int64) * (Hs * Ws * 3)
        samples["seg_offset"] = -1
        samples["src_h"], samples["src_w"] = Hs, Ws
        samples["minv"] = it.invert_affine(frame_warp(Hs, Ws, H, W))
        desc = torch.from_numpy(samples.view(np.uint8).reshape(-1)).to(self.device)
        data = self.net.data.data
        _lib.check(it._entry()(frames.data_ptr(), None, desc.data_ptr(), B, H, W, it._CMAP_BGR,
                               (ctypes.c_double * 3)(*self.mean_pixels), None, data.data_ptr(), None, fn.stream()),
                   "augment_batch")
        det, seg_prob = self.forward()
        det = det.cpu().numpy()
        rows = []
        for b in range(B):
            d = det[b][det[b][:, 0] >= 0]
            rows.append(d[nms(np.hstack((d[:, 2:6], d[:, 1:2])), nms_thresh)])
        return self.visualize_detection(data, rows, seg_prob, classes, thresh)


def frame_warp(Hs, Ws, H, W, target_size=600, max_size=1024):
    """forward affine map (2 x 3, row major, source -> net input) of the demo's frame preparation:
    `resize(img, 600, 1024)` (:45-62: the short side to 600 unless the long side would pass 1024; the new size is
    cvRound(size * scale)), rows [64:576] unless |width / height - 2| <= .01 (:440-442), then the scale onto (H, W)"""
    scale = float(target_size) / float(min(Hs, Ws))
    if np.round(scale * max(Hs, Ws)) > max_size:
        scale = float(max_size) / float(max(Hs, Ws))
    rh, rw = int(np.rint(Hs * scale)), int(np.rint(Ws * scale))
    top, rows = 0, rh
    if abs(float(rw) / float(rh) - 2.) > .01:
        top, rows = 64, min(576, rh) - 64
    if rows <= 0 or rw <= 0:
        raise _lib.DspnError("frame_warp: a %d x %d frame leaves nothing after the resize and the row crop" % (Hs, Ws))
    sx, sy = W / float(rw), H / float(rows)
    return [scale * sx, 0.0, 0.0, 0.0, scale * sy, -top * sy]
