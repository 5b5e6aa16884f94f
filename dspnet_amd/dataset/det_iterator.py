"""DetIter (dataset/iterator.py:113-297): batches of (data, label) for a detection-only net from an image database, with
the SSD augmentation -- a random crop constrained by ground-truth overlap or a zoom-out padding (rand_sampler.py), one of
five interpolations drawn per image, mirror -- and ListImdb, the database of an image list written by `Imdb.save_imglist`.

Division of labour, as in MultiTaskRecordIter:
  host   file read, decode on a thread pool into one pinned pool (with device_jpeg=True only the entropy pass of a
         baseline JPEG stays here, dataset/jpeg.py, with device_png=True only the inflate of a PNG, dataset/png.py, with
         Pillow for everything else), the samplers and the box
         arithmetic, the window (`crop_window`) and the resize tap tables (`resize_taps`): pure functions;
  device ONE upload of the pixels, ONE upload of descriptors and tables, ONE launch (dspn_det_augment_batch_u8,
         include/dspn_det_augment.h) that does crop / pad + resize + mirror + mean + planes for the whole batch.  The
         reference runs these per sample on the host with OpenCV.

The random draws come from the global `np.random` stream in the reference's order (per sample: every sampler in list
order, the pick only when some crop exists, the interpolation always, the mirror only when training with rand_mirror).

Kept from the reference on purpose: `if rand_seed:` -- a seed of 0 does not seed (:169); the constructor builds one batch
before the first next(), so it consumes draws (:179); there is no shuffle until reset() (:192-195); the tail batch is
padded from the middle of the epoch (:229); when not training the interpolation draw still happens (:285) and slots past
the end stay zero images (:226-227).

The resize follows OpenCV's as this project understands it; PARITY STATUS: unpinned (include/dspn_det_augment.h lists the
two known differences).

The colour-jitter settings of config/config.py (`ColorJitter`: hue, saturation, illumination, contrast), which in the
reference only MXNet's C++ detection augmenter reads, are available here as DetIter(color_jitter=..., jitter_seed=...):
one more launch on the decoded pixels in front of the crop (dataset/colour_jitter.py, include/dspn_colour_jitter.h), with
parameters from a RandomState of their own, so the global stream above is the same with the feature on or off.

Out of scope: DetRecordIter (:10-111), a wrapper of MXNet's C++ ImageDetRecordIter whose text is not in the reference."""
import ctypes as _c
import functools
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib
from ..detect.render import nearest_tables
from . import colour_jitter
from . import jpeg
from . import png
from .im2rec import read_list
from .rand_sampler import RandSampler
from .staging import HostPools, upload_decoded

# the reference's list order (:281-282)
LINEAR, CUBIC, AREA, NEAREST, LANCZOS4 = range(5)
METHODS = (LINEAR, CUBIC, AREA, NEAREST, LANCZOS4)
MAX_TAPS = 64                                                  # what one launch takes per axis
COEF_BITS = 11                                                 # coefficients are integers of 1 / 2048
_ONE = 1 << COEF_BITS
_FLT_EPSILON = 1.1920928955078125e-07

SAMPLE = _lib.layout("dspn_det_sample")                        # include/dspn_det_augment.h
FILL = 128                                                     # :277


def _entry():
    """dspn_det_augment_batch_u8 (fails loudly when the HIP library is missing)"""
    return _lib.lib().dspn_det_augment_batch_u8


# ---- host planning: pure functions ----------------------------------------------------------------------------------
def crop_window(crop_box, width, height):
    """the pixel window of a sampler's (left, top, right, bottom) box on a width x height image (:263-278)
    -> (x0, y0, w, h, padded).  The int() truncations (toward zero, also for negative origins) are the reference's.
    Crop mode when the window lies inside the image; otherwise padding mode: a w x h canvas of 128 with the image at
    (-x0, -y0), which must contain the image -- ValueError where the reference's slice assignment would have failed (and
    for an empty window, which its fixed_crop / imresize refuse)."""
    xmin = int(crop_box[0] * width)
    ymin = int(crop_box[1] * height)
    xmax = int(crop_box[2] * width)
    ymax = int(crop_box[3] * height)
    w, h = xmax - xmin, ymax - ymin
    if w < 1 or h < 1:
        raise ValueError("crop box %r gives an empty %d x %d window on a %d x %d image" % (tuple(crop_box), w, h, width, height))
    if xmin >= 0 and ymin >= 0 and xmax <= width and ymax <= height:
        return xmin, ymin, w, h, False
    if xmin > 0 or ymin > 0 or xmax < width or ymax < height:
        raise ValueError("crop box %r neither lies inside the %d x %d image nor contains it: the window is x %d..%d, y %d..%d"
                         % (tuple(crop_box), width, height, xmin, xmax, ymin, ymax))
    return xmin, ymin, w, h, True


def _quantise(c):
    """(n, K) double coefficients -> int16 of 1 / 2048, round-half-even, the residual of a row added to its first largest
    tap so that every row sums to exactly 2048"""
    q = np.rint(c * _ONE).astype(np.int64)
    rows = np.arange(q.shape[0])
    q[rows, np.argmax(q, axis=1)] += _ONE - q.sum(axis=1)
    assert (q.sum(axis=1) == _ONE).all() and np.abs(q).max() < 32768
    return q.astype(np.int16)


def _area_box_taps(n_src, n_dst, s):
    """fractional-coverage box average of [d s, min((d + 1) s, n_src)): the weight of a source pixel is its overlap over the
    interval length; partial covers below 1e-3 are dropped; short rows are zero-padded to the longest"""
    firsts, rows = [], []
    for d in range(n_dst):
        a, b = d * s, min((d + 1) * s, float(n_src))
        length = b - a
        p1, p2 = int(math.ceil(a)), int(math.floor(b))         # whole pixels: p1 .. p2 - 1
        if p1 > p2:                                            # the interval lies inside one pixel
            firsts.append(int(math.floor(a)))
            rows.append([1.0])
            continue
        first, row = p1, []
        if p1 - a > 1e-3:
            first = p1 - 1
            row.append((p1 - a) / length)
        row.extend([1.0 / length] * (p2 - p1))
        if b - p2 > 1e-3:
            row.append((b - p2) / length)
        if not row:
            first, row = min(p1, n_src - 1), [1.0]
        firsts.append(first)
        rows.append(row)
    K = max(len(r) for r in rows)
    c = np.zeros((n_dst, K))
    for d, r in enumerate(rows):
        c[d, :len(r)] = r
    return np.asarray(firsts, np.int64), c


def resize_coefficients(n_src, n_dst, method, area_box):
    """the table of resize_taps before quantisation: (first int64[n_dst], c float64[n_dst, K])"""
    s = n_src / n_dst
    d = np.arange(n_dst, dtype=np.float64)
    if method == NEAREST:
        first = nearest_tables(n_src, 1, n_dst, 1)[0].astype(np.int64)
        c = np.ones((n_dst, 1))
    elif method == AREA and area_box:
        if s < 1:
            raise ValueError("the box average of the area method needs a shrinking axis, got %d -> %d" % (n_src, n_dst))
        first, c = _area_box_taps(n_src, n_dst, s)
    elif method == AREA:
        i = np.floor(d * s)
        t = (d + 1) - (i + 1) / s
        t = np.where(t <= 0, 0.0, t - np.floor(t))
        first, c = i.astype(np.int64), np.stack([1 - t, t], axis=1)
    elif method in (LINEAR, CUBIC, LANCZOS4):
        f = (d + .5) * s - .5
        i = np.floor(f)
        t = f - i
        if method == LINEAR:
            low, high = i < 0, i >= n_src - 1
            i = np.where(low, 0, np.where(high, n_src - 1, i))
            t = np.where(low | high, 0.0, t)
            first, c = i.astype(np.int64), np.stack([1 - t, t], axis=1)
        elif method == CUBIC:
            A = -0.75
            c0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
            c1 = ((A + 2) * t - (A + 3)) * t * t + 1
            c2 = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1
            first, c = i.astype(np.int64) - 1, np.stack([c0, c1, c2, 1 - c0 - c1 - c2], axis=1)
        else:
            j = np.arange(8, dtype=np.float64)
            y = (t[:, None] + 3 - j[None, :]) * (math.pi / 4)
            unit = t < _FLT_EPSILON
            y[unit] = 1.0                                      # not used: those rows are unit taps
            c = np.where(j % 2 == 0, 1.0, -1.0)[None, :] * np.sin(y) / (y * y)
            c[unit] = (j == 3).astype(np.float64)
            c = c / c.sum(axis=1, keepdims=True)
            first = i.astype(np.int64) - 3
    else:
        raise ValueError("method is 0 (linear), 1 (cubic), 2 (area), 3 (nearest) or 4 (lanczos4), got %r" % (method,))
    return first, c


@functools.lru_cache(maxsize=256)
def _resize_taps(n_src, n_dst, method, area_box):
    first, c = resize_coefficients(n_src, n_dst, method, area_box)
    if c.shape[1] > MAX_TAPS:
        raise _lib.DspnError("resize %d -> %d needs %d taps per output, more than the %d one launch takes"
                             % (n_src, n_dst, c.shape[1], MAX_TAPS))
    first, coef = first.astype(np.int32), _quantise(c)
    first.setflags(write=False)
    coef.setflags(write=False)
    return first, coef


def resize_taps(n_src, n_dst, method, area_box=None):
    """the tap table of one axis of a resize n_src -> n_dst: (first int32[n_dst], coef int16[n_dst, K]), read-only.  Tap j
    of output d reads canvas index clamp(first[d] + j, 0, n_src - 1) with weight coef[d][j] / 2048; every row sums to 2048.
    method: LINEAR, CUBIC, AREA, NEAREST, LANCZOS4 (the reference's list order).  area_box says which rule the AREA method
    uses: the box average (both axes of the sample shrink) or the two-tap rule (either axis grows; BOTH axes then use it);
    None decides by this axis alone.  Everything is computed in double from s = n_src / n_dst.  DspnError when a row
    needs more than 64 taps."""
    n_src, n_dst, method = int(n_src), int(n_dst), int(method)
    if n_src < 1 or n_dst < 1:
        raise ValueError("sizes must be positive, got %d -> %d" % (n_src, n_dst))
    if method != AREA:
        area_box = False
    elif area_box is None:
        area_box = n_src >= n_dst
    return _resize_taps(n_src, n_dst, method, bool(area_box))


def sample_taps(canvas_w, canvas_h, W, H, method):
    """the x and y tables of one sample: the AREA method takes the box average only when both axes shrink"""
    box = canvas_w >= W and canvas_h >= H
    return resize_taps(canvas_w, W, method, box), resize_taps(canvas_h, H, method, box)


def _table_ints(first, coef):
    """one table as the launch reads it: the first-indices, then the coefficients as int16, two to an int"""
    flat = coef.reshape(-1)
    if flat.size % 2:
        flat = np.concatenate([flat, np.zeros(1, np.int16)])
    return np.concatenate([first.astype("<i4"), np.ascontiguousarray(flat, "<i2").view("<i4")])


def pack_batch(plans, H, W):
    """plans: per sample a dict with src_w, src_h, img_offset, window (x0, y0, w, h), method, mirror and optionally fill
    -> (descriptors as a SAMPLE array, the tables as one int32 array).  Samples with the same table share it.  Refuses
    (DspnError, through resize_taps) more than 64 taps on either axis, before anything is uploaded or launched."""
    samples = np.zeros(len(plans), SAMPLE)
    chunks, where, used = [], {}, 0

    def place(key, first, coef):
        nonlocal used
        if key not in where:
            ints = _table_ints(first, coef)
            where[key] = used
            chunks.append(ints)
            used += ints.size
        return where[key]

    for k, p in enumerate(plans):
        x0, y0, cw, ch = (int(v) for v in p["window"])
        if cw < 1 or ch < 1 or p["src_w"] < 1 or p["src_h"] < 1:
            raise ValueError("sample %d: empty image or window" % k)
        method = int(p["method"])
        box = cw >= W and ch >= H
        (fx, cx), (fy, cy) = sample_taps(cw, ch, W, H, method)
        s = samples[k]
        s["img_offset"], s["src_h"], s["src_w"] = p["img_offset"], p["src_h"], p["src_w"]
        s["x0"], s["y0"], s["canvas_h"], s["canvas_w"] = x0, y0, ch, cw
        s["fill"], s["mirror"] = int(p.get("fill", FILL)), int(bool(p["mirror"]))
        s["kx"], s["ky"] = cx.shape[1], cy.shape[1]
        s["xtab"] = place((cw, W, method, box), fx, cx)
        s["ytab"] = place((ch, H, method, box), fy, cy)
    if used >= 2 ** 31:
        raise _lib.DspnError("the tap tables of this batch take %d ints, past what the descriptors index" % used)
    tables = np.concatenate(chunks) if chunks else np.zeros(1, "<i4")
    return samples, tables


def augment_on_device(images, samples, tables, H, W, mean, out=None, stream=None):
    """dspn_det_augment_batch_u8: images a uint8 device pool, samples a uint8 device tensor of descriptors, tables an int32
    device tensor -> (B, 3, H, W) float32 (written into `out` when given)"""
    dev = images.device
    B = samples.numel() // SAMPLE.itemsize
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == B * 3 * H * W
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_entry()(images.data_ptr(), samples.data_ptr(), tables.data_ptr(), B, H, W,
                        (_c.c_double * 3)(*[float(m) for m in mean]), out.data_ptr(), st), "det_augment_batch")
    return out


# ---- the database of an image list ----------------------------------------------------------------------------------
class ListImdb(object):
    """the image list `Imdb.save_imglist` writes (dataset/imdb.py:81-82): per line the index, the header width 2, the object
    width, the flattened label, the path relative to `root`.  Labels are padded with -1 rows to pad_rows (default: the
    largest object count in the list).  label_width=6 on a 5-column list appends a 0.0 distance column to the valid rows
    (MultiBoxTarget here takes 6 columns); pad rows stay -1."""

    def __init__(self, lst_path, root, label_width=None, pad_rows=None):
        self.root = root
        self._paths, labels = [], []
        for index, cols, rel in read_list(lst_path):
            if len(cols) < 2 or int(cols[0]) != 2:
                raise ValueError("%s: index %d: a header of width 2 (2, object width) is expected" % (lst_path, index))
            width = int(cols[1])
            body = np.asarray(cols[2:], np.float64)
            if width < 5 or body.size % width:
                raise ValueError("%s: index %d: %d label values do not make rows of %d" % (lst_path, index, body.size, width))
            labels.append(body.reshape(-1, width))
            self._paths.append(rel)
        if not labels:
            raise RuntimeError("No image in " + lst_path)
        widths = set(l.shape[1] for l in labels)
        if len(widths) != 1:
            raise ValueError("%s: object widths differ: %s" % (lst_path, sorted(widths)))
        width = widths.pop()
        out_width = width if label_width is None else int(label_width)
        if out_width != width and not (width == 5 and out_width == 6):
            raise ValueError("label_width=%d on a list of width %d: only 5 -> 6 is defined" % (out_width, width))
        rows = max(l.shape[0] for l in labels) if pad_rows is None else int(pad_rows)
        self._labels = []
        for l in labels:
            if l.shape[0] > rows:
                raise ValueError("a label of %d objects does not fit pad_rows=%d" % (l.shape[0], rows))
            full = -np.ones((rows, out_width))
            full[:l.shape[0], :width] = l
            if out_width != width:
                full[:l.shape[0], width:] = 0.0
            self._labels.append(full)
        self.num_images = len(self._paths)

    def image_path_from_index(self, index):
        return os.path.join(self.root, self._paths[index])

    def label_from_index(self, index):
        return self._labels[index]


# ---- the iterator ---------------------------------------------------------------------------------------------------
def _decode_image(im, dst, coef_dst, raw_dst, index=None):
    """worker thread: one image's host half (with `index`, a JPEG's scan index only: jpeg.decode_image) -> "jpeg" or
    "png" when that format's launch finishes the image, False when Pillow's pixels are in dst"""
    if isinstance(im, png.CodedRgb):
        return "png" if png.decode_rgb(im, dst, raw_dst) else False
    return "jpeg" if jpeg.decode_image(im, dst, coef_dst, index) else False


class DataBatch(object):
    def __init__(self, data, label, pad=0, index=None):
        self.data, self.label, self.pad, self.index = data, label, pad, index


class _FitView(object):
    """what train.solver.fit consumes: (batch, indices) with batch.label == [label, None]"""

    def __init__(self, it):
        self._it = it

    def reset(self):
        self._it.reset()

    def iter_next(self):
        return self._it.iter_next()

    def next(self):
        b = self._it.next()
        return DataBatch(b.data, [b.label[0], None], b.pad, b.index), list(self._it.batch_indices)

    __next__ = next

    def __iter__(self):
        return self


class DetIter(object):
    """see the module docstring; constructor arguments as in the reference.  imdb: any object with num_images,
    image_path_from_index(i) and label_from_index(i) -> (rows, 5+) array with -1 rows below the valid ones.
    device_jpeg=True: baseline JPEGs are Huffman-decoded on the host and reconstructed on the device in front of the
    augmentation (same pixels as Pillow's, byte for byte); any other file takes the Pillow path, counted in
    `jpeg_fallbacks`.
    device_entropy=True (with device_jpeg): JPEGs with restart intervals of at most jpeg.DEVICE_MAX_INTERVAL MCUs are
    Huffman-decoded on the device as well -- a worker thread only indexes the scan, the compressed scan goes up instead of
    the coefficients --, counted in `jpeg_device_entropy`.  The status words of a batch are read with one small copy before
    it is handed out, and a scan the device could not decode raises DspnError naming the image: the host pass falls back
    to Pillow for a corrupt scan, this pass cannot, because by then the batch is on the device.
    device_png=True: PNG files of every non-interlaced format but 16-bit greyscale are inflated on the host and turned into
    RGB on the device in front of the augmentation (same pixels as Pillow's convert("RGB"), byte for byte); a PNG file that
    is unsupported, malformed or does not inflate takes the Pillow path, counted in `png_fallbacks`.  With both switches on,
    an image the device decodes in either format is no fallback of the other.
    color_jitter: a colour_jitter.ColorJitter (or a dict with its keys); when training and some probability in it is not
    zero, every batch draws per-sample parameters from np.random.RandomState(jitter_seed) and one launch jitters the
    decoded pixels in front of the crop.  None, or all probabilities zero: no draw, no launch."""

    def __init__(self, imdb, batch_size, data_shape, mean_pixels=[128, 128, 128], rand_samplers=[], rand_mirror=False,
                 shuffle=False, rand_seed=None, is_train=True, max_crop_trial=50, device=None, decode_threads=8,
                 device_jpeg=False, color_jitter=None, jitter_seed=0, device_png=False, device_entropy=False):
        if device_entropy and not device_jpeg:
            raise ValueError("device_entropy=True needs device_jpeg=True: it moves the rest of that decode to the device")
        self._imdb = imdb
        self.batch_size = batch_size
        if isinstance(data_shape, int):
            data_shape = (data_shape, data_shape)
        else:
            assert len(data_shape) == 3 and data_shape[0] == 3
            data_shape = (data_shape[1], data_shape[2])
        self._data_shape = data_shape
        if isinstance(mean_pixels, (int, float)):
            mean_pixels = [mean_pixels] * 3
        self._mean_pixels = [float(m) for m in mean_pixels]
        assert len(self._mean_pixels) == 3
        if not rand_samplers:
            self._rand_samplers = []
        else:
            if not isinstance(rand_samplers, list):
                rand_samplers = [rand_samplers]
            assert isinstance(rand_samplers[0], RandSampler), "Invalid rand sampler"
            self._rand_samplers = rand_samplers
        self.is_train = is_train
        self._rand_mirror = rand_mirror
        self._shuffle = shuffle
        if rand_seed:                                          # :169 a seed of 0 does not seed
            np.random.seed(rand_seed)
        self._max_crop_trial = max_crop_trial
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._pool = ThreadPoolExecutor(max_workers=max(1, int(decode_threads)))
        self.device_jpeg, self.jpeg_fallbacks = bool(device_jpeg), 0
        self.device_entropy, self.jpeg_device_entropy = bool(device_entropy), 0
        self.device_png, self.png_fallbacks = bool(device_png), 0
        self._pools = HostPools(self.device.type == "cuda")
        self._jitter = colour_jitter.config(color_jitter) if is_train else None
        self._jitter_rs = np.random.RandomState(jitter_seed) if self._jitter is not None else None

        self._current = 0
        self._size = imdb.num_images
        self._index = np.arange(self._size)

        self._data = None
        self._label = None
        self.batch_indices = []
        self._get_batch()                                      # :179
        self.jpeg_fallbacks = self.png_fallbacks = self.jpeg_device_entropy = 0    # that batch was not delivered

    @property
    def provide_data(self):
        return [("data", tuple(self._data.shape))]

    @property
    def provide_label(self):
        if self.is_train:
            return [("label", tuple(self._label.shape))]
        return []

    def reset(self):
        self._current = 0
        if self._shuffle:
            np.random.shuffle(self._index)

    def iter_next(self):
        return self._current < self._size

    def next(self):
        if self.iter_next():
            self._get_batch()
            batch = DataBatch(data=[self._data], label=[self._label], pad=self.getpad(), index=self.getindex())
            self._current += self.batch_size
            return batch
        raise StopIteration

    __next__ = next

    def __iter__(self):
        return self

    def getindex(self):
        return self._current // self.batch_size

    def getpad(self):
        pad = self._current + self.batch_size - self._size
        return 0 if pad < 0 else pad

    def fit_view(self):
        """the iterator as train.solver.fit reads one: reset / iter_next / next -> (batch, indices), with
        batch.label == [label, None] (a detection-only net has no input for the second)"""
        return _FitView(self)

    # ---- one batch (:218-297) -----------------------------------------------------------------------------------
    def _plan(self, width, height, label):
        """the draws of `_data_augmentation` for one image of width x height, in its order, and what they decide
        -> (window (x0, y0, w, h), method, mirror, label)"""
        window = (0, 0, width, height)
        if self.is_train and self._rand_samplers:
            rand_crops = []
            for rs in self._rand_samplers:
                rand_crops += rs.sample(label)
            num_rand_crops = len(rand_crops)
            if num_rand_crops > 0:
                index = int(np.random.uniform(0, 1) * num_rand_crops)
                window = crop_window(rand_crops[index][0], width, height)[:4]
                label = rand_crops[index][1]
        methods = METHODS if self.is_train else (LINEAR,)
        method = methods[int(np.random.uniform(0, 1) * len(methods))]
        mirror = False
        if self.is_train and self._rand_mirror:
            if np.random.uniform(0, 1) > 0.5:
                mirror = True
                valid_mask = np.where(label[:, 0] > -1)[0]      # :290 the pad rows stay -1
                tmp = 1.0 - label[valid_mask, 1]
                label[valid_mask, 1] = 1.0 - label[valid_mask, 3]
                label[valid_mask, 3] = tmp
        return window, method, mirror, label

    def _prepare(self):
        """host phase: indices, files, draws, decode, descriptors and tables"""
        B, (H, W) = self.batch_size, self._data_shape
        opened, plans, labels, indices, is_png = [], [], [], [], []
        offset = 0
        for i in range(B):
            if (self._current + i) >= self._size:
                if not self.is_train:
                    continue
                idx = (self._current + i + self._size // 2) % self._size      # :229 padding from the middle of the epoch
                index = self._index[idx]
            else:
                index = self._index[self._current + i]
            with open(self._imdb.image_path_from_index(index), "rb") as fp:
                content = fp.read()
            is_png.append(content[:8] == png.SIGNATURE)
            im = png.open_rgb(content) if self.device_png else None
            if im is None:
                im = jpeg.open_image(content, self.device_jpeg)      # sizes before any pixel is decoded
            width, height = im.size
            gt = self._imdb.label_from_index(index).copy() if self.is_train else None
            window, method, mirror, label = self._plan(width, height, gt)
            plans.append({"src_w": width, "src_h": height, "img_offset": offset, "window": window, "method": method,
                          "mirror": mirror})
            offset += width * height * 3
            opened.append(im)
            labels.append(label)
            indices.append(int(index))
        samples, tables = pack_batch(plans, H, W)
        jitter = colour_jitter.draw(self._jitter, len(plans), self._jitter_rs) if self._jitter is not None else None
        jbatch = jpeg.CodedBatch([im.info if isinstance(im, jpeg.Coded) else None for im in opened],
                                 [p["img_offset"] for p in plans], self.device_entropy)
        pbatch = png.RgbBatch([im.info if isinstance(im, png.CodedRgb) else None for im in opened],
                              [p["img_offset"] for p in plans])
        pixels = self._pools.take("pixels", offset, torch.uint8)
        coefs = self._pools.take("coefs", jbatch.host_count, torch.int16, floor=jbatch.FLOOR)
        raw = self._pools.take("raw", pbatch.count, torch.uint8, floor=pbatch.FLOOR)
        pnp = pixels.numpy()
        dsts = [pnp[p["img_offset"]:p["img_offset"] + p["src_w"] * p["src_h"] * 3].reshape(p["src_h"], p["src_w"], 3)
                for p in plans]
        answers = list(self._pool.map(_decode_image, opened, dsts, jbatch.slices(coefs.numpy()), pbatch.slices(raw.numpy()),
                                      jbatch.indexers()))
        # per format: True -- its launch finishes the image; None -- the other format's does; False -- the host decoded it
        jbatch.answered([a == "jpeg" or (None if a else False) for a in answers])
        pbatch.answered([a == "png" or (None if a else False) for a in answers])
        return {"count": len(plans), "pixels": pixels, "pixel_bytes": offset, "samples": samples, "tables": tables,
                "labels": labels, "indices": indices, "coefs": coefs, "jpeg": jbatch, "jitter": jitter, "raw": raw,
                "png": pbatch, "png_on_host": sum(1 for a, f in zip(answers, is_png) if f and not a)}

    def _device_batch(self, prep):
        """device phase: one upload of pixels (or coefficients), one of descriptors and tables, one launch
        -> (B, 3, H, W) float32; slots past the samples of `prep` stay zero"""
        B, (H, W), dev = self.batch_size, self._data_shape, self.device
        n, jbatch, pbatch = prep["count"], prep["jpeg"], prep["png"]
        data = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if n == B else \
            torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev)
        if n == 0:
            return data
        # pool copies, then the pools' event, then descriptors and launches: the reason is in dataset/staging.py
        jbatch.upload(prep["coefs"], dev)
        pbatch.upload(prep["raw"], dev)
        img_dev = upload_decoded(prep["pixels"][:max(prep["pixel_bytes"], 1)], dev, jbatch.on_device + pbatch.on_device,
                                 jbatch.fallbacks)
        self._pools.uploaded(torch.cuda.current_stream(dev))
        desc = np.concatenate([prep["samples"].view(np.uint8).reshape(-1), prep["tables"].view(np.uint8)])
        desc_dev = torch.from_numpy(desc).to(dev)              # descriptors and tables in one upload (56 B each: 4-aligned)
        ndesc = n * SAMPLE.itemsize
        keep = jbatch.launch(img_dev) + pbatch.launch(img_dev)
        jbatch.check(["image %d" % i for i in prep["indices"]])     # the device entropy pass's status words, if it ran
        if self.device_jpeg:
            self.jpeg_fallbacks += jbatch.fallbacks
            self.jpeg_device_entropy += jbatch.device_entropy
        if self.device_png:
            self.png_fallbacks += prep["png_on_host"]
        if prep["jitter"] is not None:                         # on the decoded pixels, in front of the crop
            s = prep["samples"]
            keep += colour_jitter.apply(img_dev, prep["jitter"], s["img_offset"], np.stack([s["src_h"], s["src_w"]], axis=1))
        augment_on_device(img_dev, desc_dev[:ndesc], desc_dev[ndesc:].view(torch.int32), H, W, self._mean_pixels,
                          out=data[:n])
        self._keepalive = (img_dev, desc_dev) + keep           # until the next batch replaces them
        return data

    def _get_batch(self):
        prep = self._prepare()
        self._data = self._device_batch(prep)
        self.batch_indices = prep["indices"]
        if self.is_train:
            self._label = torch.from_numpy(np.array(prep["labels"]).astype(np.float32)).to(self.device)
        else:
            self._label = None
