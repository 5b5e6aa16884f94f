"""MultiTaskRecordIter (dataset/iterator.py:301-603): batches of (data, label_det, seg_out_label) from an indexed
RecordIO file plus per-image label-map PNGs, with the reference's augmentation (flip, rotation, anisotropic scale,
translation) or its plain resize.

Division of labour (MI355X-first):
  host   record lookup, JPEG / PNG decode (Pillow, a small thread pool: the decoders release the GIL), the box
         arithmetic of `_get_augmented` / `_get_resized` (a few dozen boxes per image), the random draws;
         with device_jpeg=True only the serial half of the JPEG decode (markers, Huffman) stays here and the
         coefficients are uploaded instead of pixels (dataset/jpeg.py, include/dspn_jpeg.h);
         with device_png=True only the inflate of the label map stays here and the still filtered rows are uploaded
         (dataset/png.py, include/dspn_png.h);
  device ONE upload of the decoded uint8 pixels of the whole batch and ONE launch pair (dspn_augment_batch_u8,
         include/dspn_augment.h) that does warpAffine (bilinear, OpenCV's fixed point) + flip + BGR->RGB planes + mean
         subtraction for the images and nearest warp + flip + /4 resize + LUT for the label maps.  The reference runs
         four OpenCV passes per sample on the host and uploads float32 planes.
         With color_jitter=... one more launch shifts hue / lightness / saturation and scales the contrast of the decoded
         pixels in front of the warp (dataset/colour_jitter.py, include/dspn_colour_jitter.h; off by default).

The shuffle and the augmentation parameters come from the same MT19937 stream as the reference
(`np.random.seed(233)`, then shuffle / rand in the reference's call order, :381-383, :406-419), so for a given
record file the sample order and every (flip, theta, sx, sy, tx, ty) are identical.

Kept from the reference on purpose: an image without any box returns before the flip (:498-499) -- it is never
flipped even when its draw says so; exactly one surviving box is written to the first SIX label rows (np.squeeze
turns the (1, 6) selection into (6,), :542-544); `iter_next` drops the last partial batch (:421-423)."""
import ctypes as _c
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib
from . import colour_jitter
from . import jpeg
from . import png
from . import recordio
from .staging import Decoded, HostPools

_SAMPLE = _lib.layout("dspn_warp_sample")                       # include/dspn_augment.h
_CMAP_BGR = (_c.c_int * 3)(2, 1, 0)                             # BGR source -> R, G, B planes (:568-569)
_CMAP_RGB = (_c.c_int * 3)(0, 1, 2)                             # Pillow decodes to RGB: identity


def _entry():
    """dspn_augment_batch_u8 (fails loudly when the HIP library is missing)"""
    return _lib.lib().dspn_augment_batch_u8


def seg_lut():
    """:361-366 over dataset/cs_labels.py: ids whose trainId is >= 0 (0..34) map to themselves, the rest to 255"""
    lut = np.full(256, 255, np.uint8)
    lut[:35] = np.arange(35, dtype=np.uint8)
    return lut


def invert_affine(M):
    """the inverse map cv2.warpAffine derives from M (double arithmetic, same statement order)"""
    m = np.array(M, np.float64).reshape(-1).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2] = b1; m[5] = b2
    return m


def _pack_to_top(rows):
    """surviving rows (xmax > -0.5) first, -1 below; a single survivor fills six rows (module note)"""
    keep = rows[rows[:, 3] > -.5]
    rows[:] = -1
    if keep.shape[0] == 1:
        rows[:6] = keep[0]
    else:
        rows[:keep.shape[0]] = keep


def resized_boxes(rows, data_shape):
    """box bookkeeping of `_get_resized` (:447-469) on the (n, 6) label rows, in place"""
    if not (rows[:, 0] >= 0).any():
        return
    area = (rows[:, 3] - rows[:, 1]) * data_shape[2] * (rows[:, 4] - rows[:, 2]) * data_shape[1]
    rows[area < 100] = -1
    _pack_to_top(rows)


def augmented_boxes(rows, data_shape, aug):
    """box bookkeeping of `_get_augmented` (:486-544) on the (n, 6) label rows, in place.
    -> False when the sample has no box (the caller then skips the flip, like the reference's early return)"""
    flip, theta, sx, sy, tx, ty = (float(a) for a in aug)
    W, H = data_shape[2], data_shape[1]
    sel = np.where(rows[:, 0] >= 0)[0]
    if sel.size < 1:
        return False
    dist = rows[sel, 5].copy()
    box = rows[sel, 1:5] * np.array([W, H, W, H], np.float64)
    A = np.array([[sx * math.cos(theta), -sy * math.sin(theta)], [sx * math.sin(theta), sy * math.cos(theta)]])
    t = np.array([tx, ty])
    p0 = box[:, :2] @ A.T + t                                   # cv2.transform of the (xmin, ymin) corners
    p1 = box[:, 2:] @ A.T + t                                   # ... and of the (xmax, ymax) corners
    if flip > .5:
        p0[:, 0] = W - p0[:, 0]
        p1[:, 0] = W - p1[:, 0]
    scale = np.array([1.0 / W, 1.0 / H])
    p0 = p0 * scale
    p1 = p1 * scale
    new = np.hstack((p0, p1))
    if flip > .5:
        new[:, [0, 2]] = new[:, [2, 0]]
    vis = new[:, 2] > -.5
    new[vis] = np.clip(new[vis], 0, 1)
    rows[sel, 1:5] = new
    rows[sel, 5] = dist / math.sqrt(sx * sy)
    area = (rows[:, 3] - rows[:, 1]) * W * (rows[:, 4] - rows[:, 2]) * H
    rows[area < 100] = -1
    rows[rows[:, 3] < .01] = -1
    rows[rows[:, 1] > .99] = -1
    rows[rows[:, 4] < .01] = -1
    rows[rows[:, 2] > .99] = -1
    _pack_to_top(rows)
    return True


class DataBatch(object):
    def __init__(self, data, label):
        self.data, self.label = data, label


class MultiTaskRecordIter(object):
    """see the module docstring; constructor arguments as in the reference (unused ones accepted and ignored).
    device_jpeg=True: baseline JPEG records are Huffman-decoded on the host and reconstructed on the device in front of
    the augmentation (same pixels as Pillow's, byte for byte); any other record takes the Pillow path, counted in
    `jpeg_fallbacks` (records of delivered batches since construction).
    device_entropy=True (with device_jpeg): records whose JPEG carries restart intervals of at most
    jpeg.DEVICE_MAX_INTERVAL MCUs (what im2rec writes with --restart-interval) are Huffman-decoded on the device as well: a
    worker thread only indexes the scan, the compressed scan is uploaded instead of the coefficients, and
    `jpeg_device_entropy` counts such records.  Before a batch is handed out its status words are read with one small
    copy, and a scan the device could not decode raises DspnError naming the record: the host pass falls back to Pillow
    for a corrupt scan, this pass cannot, because by then the batch is on the device.
    device_png=True: 8-bit greyscale / palette label maps are inflated on the host and unfiltered on the device in front of
    the augmentation (same bytes as Pillow's); any other label map takes the Pillow path, counted in `png_fallbacks`.
    color_jitter: a colour_jitter.ColorJitter (or a dict with its keys); with enable_aug and some probability in it not
    zero, every epoch draws a table of per-slot parameters from a private RandomState(jitter_seed) beside `aug_params`,
    and one launch jitters the decoded pixels in front of the warp.  The flat jitter keys that `**cfg.train` brings stay
    among the ignored **kwargs: only this argument switches the feature on."""

    def __init__(self, path_imgrec, batch_size, data_shape, path_imglist="", label_width=-1, label_pad_width=-1,
                 label_pad_value=-1, resize_mode="force", mean_pixels=(123.68, 116.779, 103.939), enable_aug=True,
                 device=None, decode_threads=8, prefetch=True, cache_decoded=False, device_jpeg=False, device_png=False,
                 color_jitter=None, jitter_seed=0, device_entropy=False, **kwargs):
        if device_jpeg and cache_decoded:
            raise ValueError("device_jpeg=True with cache_decoded=True: the cache exists to avoid the host decode that "
                             "device_jpeg removes; choose one")
        if device_entropy and not device_jpeg:
            raise ValueError("device_entropy=True needs device_jpeg=True: it moves the rest of that decode to the device")
        if device_png and cache_decoded:
            raise ValueError("device_png=True with cache_decoded=True: the cache exists to avoid the host decode that "
                             "device_png removes; choose one")
        path_imgidx = path_imgrec.replace(".rec", ".idx")
        path_imglst = path_imgrec.replace(".rec", ".lst")
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.enable_aug = enable_aug
        self.batch_size = batch_size
        self.data_shape = tuple(data_shape)
        assert self.data_shape[0] == 3 and self.data_shape[1] % 4 == 0 and self.data_shape[2] % 4 == 0
        self.mean_pixels = list(mean_pixels)
        self.angle_range = (-5, 5)
        self.scale_range = (.5, 2.)
        self.ratio_range = (.8, 1.2)
        self.lut = seg_lut()
        self._lut_dev = torch.from_numpy(self.lut).to(self.device)
        with open(path_imgidx, "r") as f:
            self.num_samples = sum(1 for _ in f)
        self.index_table = np.arange(self.num_samples)
        self._rs = np.random.RandomState(233)                  # np.random.seed(233) (:381)
        self._jitter = colour_jitter.config(color_jitter) if enable_aug else None
        self._jitter_rs = np.random.RandomState(jitter_seed) if self._jitter is not None else None
        self._rs.shuffle(self.index_table)
        self._reset_aug_params()
        self.curr_index = 0
        self.imglst = {}
        dirname = os.path.dirname(path_imglst)
        with open(path_imglst, "r") as fp:
            for line in fp:
                patch = line.rstrip("\n").split()
                if not patch:
                    continue
                segfile = patch[-1].replace("leftImg8bit.jpg", "gtFine_labelTrainIds.png")
                segfile = segfile.replace("JPEGImages", "SegmentationClass")
                self.imglst[patch[0]] = os.path.join(dirname, "cityscapes", segfile)
        self.rec = recordio.MXIndexedRecordIO(path_imgidx, path_imgrec, "r")
        self.provide_data = [("data", [self.batch_size] + list(self.data_shape))]
        self.provide_label = None
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(decode_threads)))
        self._producer = ThreadPoolExecutor(max_workers=1)
        self.prefetch, self._ahead = bool(prefetch), None
        # cache_decoded: keep the decoded uint8 pixels of every record in host memory (Cityscapes train: 2975 x 8.4 MB =
        # 25 GB); from the second epoch on the host phase is a memcpy instead of a JPEG + PNG decode
        self._cache = {} if cache_decoded else None
        self._pools = [HostPools(torch.device(self.device).type == "cuda") for _ in range(2)]
        self.device_jpeg, self.jpeg_fallbacks = bool(device_jpeg), 0
        self.device_entropy, self.jpeg_device_entropy = bool(device_entropy), 0
        self.device_png, self.png_fallbacks = bool(device_png), 0
        self._get_batch()
        if not self.provide_label:
            raise RuntimeError("Invalid ImageDetRecordIter: " + path_imgrec)
        self.reset()
        self.jpeg_fallbacks = self.png_fallbacks = self.jpeg_device_entropy = 0    # the batch above was not delivered

    # ---- epoch control (:401-434) -------------------------------------------------------------------------------
    def reset(self):
        self._drop_ahead()                                     # a batch prepared ahead belongs to the old order
        self._rs.shuffle(self.index_table)
        self.curr_index = 0
        self._reset_aug_params()

    def _reset_aug_params(self):
        n, r = self.num_samples, self._rs
        p = np.zeros((n, 6))                                   # flip, theta, sx, sy, tx, ty
        p[:, 0] = r.rand(n) > .5
        p[:, 1] = np.radians(self.angle_range[0] + r.rand(n) * (self.angle_range[1] - self.angle_range[0]))
        p[:, 2] = self.scale_range[0] + r.rand(n) * (self.scale_range[1] - self.scale_range[0])
        p[:, 3] = p[:, 2] * (self.ratio_range[0] + r.rand(n) * (self.ratio_range[1] - self.ratio_range[0]))
        p[:, 4] = -r.rand(n) * self.data_shape[2] * (p[:, 2] - 1.)
        p[:, 5] = -r.rand(n) * self.data_shape[1] * (p[:, 3] - 1.)
        self.aug_params = p
        # a stream of its own: _rs, and with it the order and the geometry, is the same with the feature on or off
        self.jitter_params = colour_jitter.draw(self._jitter, n, self._jitter_rs) if self._jitter is not None else None

    def iter_next(self):
        return (self.curr_index + self.batch_size) <= self.num_samples

    def next(self):
        if self.iter_next():
            self._get_batch()
            return self._batch, self._fnames
        raise StopIteration

    __next__ = next

    def __iter__(self):
        return self

    # ---- one batch (:550-603) -----------------------------------------------------------------------------------
    # host phase (_prepare: records, decode straight into a pinned pool, boxes, descriptors; may run ahead of the
    # consumer on the producer thread) and device phase (_finish: one upload, one launch pair, on the caller's stream)
    def _peek(self, item):
        """header, label row and the lazily opened image(s) of one record: sizes are known before any pixel is decoded
        (from the markers / IHDR where the device will decode).  With cache_decoded the images come back as arrays from
        the second time a record is seen."""
        header, payload = recordio.unpack(item)
        hdr = np.array([header.label.shape[0]] + header.label.tolist())
        seg_path = self.imglst[str(header.id)]
        hit = self._cache.get(header.id) if self._cache is not None else None
        if hit is not None:
            return hdr, Decoded(hit[0]), (None if hit[1] is None else Decoded(hit[1])), seg_path, header.id
        im = jpeg.open_image(payload, self.device_jpeg)
        seg_im = None
        if os.path.exists(seg_path):
            with open(seg_path, "rb") as f:
                seg_im = png.open_label(f.read(), self.device_png)
        if self.enable_aug:
            assert seg_im is not None, seg_path + " not found."
        if seg_im is not None:
            assert seg_im.size == im.size, "label map and image differ in size: " + seg_path
        return hdr, im, seg_im, seg_path, header.id

    def _decode(self, job):
        """one record into its slices of the pools (worker thread; the decoders and numpy's copy loops release the GIL)
        -> (the device reconstructs the image, the device unfilters the label map; None: there is no label map)"""
        im, seg_im, img_dst, seg_dst, coef_dst, raw_dst, rec_id, index = job
        if isinstance(im, Decoded):                            # cached pixels: one memcpy each
            img_dst[...] = im.a
            if seg_im is not None:
                seg_dst[...] = seg_im.a
            return False, (None if seg_im is None else False)
        answer = (jpeg.decode_image(im, img_dst, coef_dst, index),
                  None if seg_im is None else png.decode_label(seg_im, seg_dst, raw_dst))
        if self._cache is not None:
            self._cache[rec_id] = (img_dst.copy(), None if seg_im is None else seg_dst.copy())
        return answer

    def _prepare(self, start, serial):
        B, (C, H, W) = self.batch_size, self.data_shape
        items = [self.rec.read_idx(self.rec.key_type(self.index_table[s])) for s in range(start, start + B)]
        peeked = [self._peek(item) for item in items]
        img_sizes = [im.size[0] * im.size[1] * 3 for _, im, _, _, _ in peeked]
        seg_sizes = [(sm.size[0] * sm.size[1] if sm is not None else 0) for _, _, sm, _, _ in peeked]
        img_offsets, seg_offsets = np.cumsum([0] + img_sizes).tolist(), np.cumsum([0] + seg_sizes).tolist()
        jbatch = jpeg.CodedBatch([im.info if isinstance(im, jpeg.Coded) else None for _, im, _, _, _ in peeked],
                                 img_offsets, self.device_entropy)
        pbatch = png.CodedBatch([sm.info if isinstance(sm, png.CodedLabel) else None for _, _, sm, _, _ in peeked],
                                seg_offsets)
        pools = self._pools[serial % 2]                        # two sets of pinned staging buffers, used alternately
        pixels = pools.take("pixels", img_offsets[-1], torch.uint8)
        labels = pools.take("labels", seg_offsets[-1], torch.uint8)
        coefs = pools.take("coefs", jbatch.host_count, torch.int16, floor=jbatch.FLOOR)
        raw = pools.take("raw", pbatch.count, torch.uint8)
        ip, sp = pixels.numpy(), labels.numpy()
        label = np.ones((B, 1206)) * -1
        label[:, :3] = np.array(list(self.data_shape))
        samples = np.zeros(B, _SAMPLE)
        jobs, fnames = [], []
        coef_dsts, raw_dsts, indexers = jbatch.slices(coefs.numpy()), pbatch.slices(raw.numpy()), jbatch.indexers()
        for b, (hdr, im, seg_im, seg_path, rec_id) in enumerate(peeked):
            ww, hh = im.size
            slot = start + b
            io_, so = img_offsets[b], seg_offsets[b]
            rows = hdr[3:].reshape((-1, 6))                     # view: the edits land in hdr
            if self.enable_aug:
                flip, theta, sx, sy, tx, ty = self.aug_params[slot]
                sx2, sy2 = sx * (W / float(ww)), sy * (H / float(hh))
                M = [sx2 * math.cos(theta), -sy2 * math.sin(theta), tx, sx2 * math.sin(theta), sy2 * math.cos(theta), ty]
                has_box = augmented_boxes(rows, self.data_shape, self.aug_params[slot])
                flip_img, ib, sb = bool(flip > .5) and has_box, 128, 255
            else:
                M = [1. * (W / float(ww)), -0.0, 0, 0.0, 1. * (H / float(hh)), 0]
                resized_boxes(rows, self.data_shape)
                flip_img, ib, sb = False, 0, 0
            s = samples[b]
            s["img_offset"], s["src_h"], s["src_w"] = io_, hh, ww
            s["seg_offset"] = so if seg_im is not None else -1
            s["flip"], s["img_border"], s["seg_border"] = int(flip_img), ib, sb
            s["minv"] = invert_affine(M)
            jobs.append((im, seg_im, ip[io_:io_ + img_sizes[b]].reshape(hh, ww, 3),
                         sp[so:so + seg_sizes[b]].reshape(hh, ww) if seg_im is not None else None,
                         coef_dsts[b], raw_dsts[b], rec_id, indexers[b]))
            label[b, 3:3 + hdr.shape[0]] = hdr
            fnames.append(seg_path)
        answers = list(self._pool.map(self._decode, jobs))
        jbatch.answered([a for a, _ in answers])
        pbatch.answered([a for _, a in answers])
        return {"pools": pools, "pixels": pixels[:max(img_offsets[-1], 1)], "labels": labels[:max(seg_offsets[-1], 1)],
                "coefs": coefs, "raw": raw, "jpeg": jbatch, "png": pbatch, "samples": samples, "label": label,
                "fnames": fnames, "start": start, "records": ["record %s" % p[4] for p in peeked],
                "jitter": None if self.jitter_params is None else self.jitter_params[start:start + B]}

    def _finish(self, prep):
        B, (C, H, W) = self.batch_size, self.data_shape
        dev = self.device
        jbatch, pbatch = prep["jpeg"], prep["png"]
        # pool copies, then the set's event, then descriptors and launches: the reason is in dataset/staging.py
        img_dev = jbatch.upload(prep["coefs"], dev, prep["pixels"])
        seg_dev = pbatch.upload(prep["raw"], dev, prep["labels"])
        prep["pools"].uploaded(torch.cuda.current_stream(dev))
        desc_dev = torch.from_numpy(prep["samples"].view(np.uint8).reshape(-1)).to(dev)
        coded_keep = jbatch.launch(img_dev) + pbatch.launch(seg_dev)    # the coded records' bytes, in front of the warp
        jbatch.check(prep["records"])                          # the device entropy pass's status words, if it ran
        if self.device_jpeg:
            self.jpeg_fallbacks += jbatch.fallbacks
            self.jpeg_device_entropy += jbatch.device_entropy
        if self.device_png:
            self.png_fallbacks += pbatch.fallbacks
        if prep["jitter"] is not None:                         # on the decoded pixels, in front of the warp
            s = prep["samples"]
            coded_keep += colour_jitter.apply(img_dev, prep["jitter"], s["img_offset"],
                                              np.stack([s["src_h"], s["src_w"]], axis=1))
        data = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        seg_out = torch.empty(B, H // 4, W // 4, dtype=torch.float32, device=dev)
        _lib.check(_entry()(img_dev.data_ptr(), seg_dev.data_ptr(), desc_dev.data_ptr(), B, H, W, _CMAP_RGB,
                            (_c.c_double * 3)(*[float(m) for m in self.mean_pixels]), self._lut_dev.data_ptr(),
                            data.data_ptr(), seg_out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "augment_batch")
        label = prep["label"]
        if self.provide_label is None:
            first = label[0]
            self.label_header_width = int(first[4])
            self.label_object_width = int(first[5])
            assert self.label_object_width >= 5, "object width must >=5"
            self.label_start = 4 + self.label_header_width
            self.max_objects = (first.size - self.label_start) // self.label_object_width
            self.label_shape = (B, self.max_objects, self.label_object_width)
            self.label_end = self.label_start + self.max_objects * self.label_object_width
            self.provide_label = [("label_det", self.label_shape), ("seg_out_label", tuple(seg_out.shape))]
        det = label[:, self.label_start:self.label_end].reshape((B, self.max_objects, self.label_object_width))
        det_dev = torch.from_numpy(det.astype(np.float32)).to(dev)
        self._batch = DataBatch(data=[data], label=[det_dev, seg_out])
        self._fnames = prep["fnames"]
        self._keepalive = (img_dev, seg_dev, desc_dev) + coded_keep    # until the next batch replaces them

    def _drop_ahead(self):
        fut, self._ahead = getattr(self, "_ahead", None), None
        if fut is not None:
            fut.result()                                        # let it finish: it writes into a pinned pool

    def _get_batch(self):
        fut, self._ahead = getattr(self, "_ahead", None), None
        prep = fut.result() if fut is not None else None
        if prep is None or prep["start"] != self.curr_index:    # nothing prepared ahead (or the order changed)
            self._serial = getattr(self, "_serial", 0) + 1
            prep = self._prepare(self.curr_index, self._serial)
        self.curr_index += self.batch_size
        self._finish(prep)
        if self.prefetch and self.iter_next():                  # the next batch's host phase overlaps the consumer
            self._serial += 1
            self._ahead = self._producer.submit(self._prepare, self.curr_index, self._serial)
