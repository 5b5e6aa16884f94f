"""JPEG decode split between host and device (include/dspn_jpeg.h): the host parses the markers and Huffman-decodes the
scan into quantised DCT coefficients (serial work; ctypes releases the GIL around it, so a thread pool runs it in
parallel), the device dequantises, inverts the DCT, upsamples the chroma and converts to RGB for a whole batch in one
call.  The pixels equal Pillow's (libjpeg-turbo, accurate integer IDCT, fancy upsampling) byte for byte.

`probe` and `decode_batch` are the public use; the iterators (device_jpeg=True) go through `open_image`, `decode_image`
and `CodedBatch` with their own pools (dataset/staging.py)."""
import ctypes as _c
import io

import numpy as np
import torch

from .. import _lib
from . import staging

# dspn_jpeg_info / dspn_jpeg_sample (include/dspn_jpeg.h)
INFO = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("restart_interval", "<i4"),
                 ("hsamp", "<i4", (3,)), ("vsamp", "<i4", (3,)), ("blocks_w", "<i4", (3,)), ("blocks_h", "<i4", (3,)),
                 ("supported", "<i4"), ("reason", "<i4"), ("coef_count", "<i8"), ("coef_offset", "<i8", (3,)),
                 ("quant", "u1", (3, 64))])
assert INFO.itemsize == 296
SAMPLE = np.dtype([("coef_offset", "<i8", (3,)), ("img_offset", "<i8"), ("width", "<i4"), ("height", "<i4"),
                   ("ncomp", "<i4"), ("skip", "<i4"), ("hsamp", "<i4"), ("vsamp", "<i4"), ("blocks_w", "<i4", (3,)),
                   ("blocks_h", "<i4", (3,)), ("quant", "u1", (3, 64))])
assert SAMPLE.itemsize == 272
REASONS = ("ok", "progressive", "extended sequential", "arithmetic coding", "lossless or hierarchical",
           "sample precision is not 8 bits", "neither 1 nor 3 components", "unsupported sampling factors",
           "more than one scan", "colour transform is not YCbCr", "16-bit quantisation table")
MAX_BATCH = 1024                                               # kMaxB of csrc/jpeg.hip: descriptors of one reconstruct call

_lib.register({
    "dspn_jpeg_probe": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "dspn_jpeg_entropy_decode": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p]),
    "dspn_jpeg_reconstruct_workspace_bytes": (_c.c_size_t, [_c.c_longlong]),
    "dspn_jpeg_reconstruct_batch_u8": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_void_p, _c.c_int, _c.c_void_p,
                                                  _c.c_longlong, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    # include/dspn_jpeg_encode.h (dataset/jpeg_encode.py is its front end)
    "dspn_jpeg_quant_tables": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_void_p]),
    "dspn_jpeg_encode_geometry": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_void_p]),
    "dspn_jpeg_encode_workspace_bytes": (_c.c_size_t, [_c.c_longlong]),
    "dspn_jpeg_encode_blocks_batch_u8": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                                    _c.c_longlong, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "dspn_jpeg_entropy_encode": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
})


def probe_info(payload):
    """-> (status, info record): dspn_jpeg_probe on a bytes object; status != 0: malformed (message in dspn_last_error)"""
    info = np.zeros(1, INFO)
    rc = _lib.lib().dspn_jpeg_probe(_c.c_char_p(payload), len(payload), info.ctypes.data)
    return rc, info[0]


def probe(payload):
    """what the markers up to SOS say: a dict with the fields of dspn_jpeg_info, `quant` as a (3, 64) array and
    `reason` as text.  Raises DspnError on a malformed stream."""
    rc, info = probe_info(payload)
    _lib.check(rc, "jpeg_probe")
    out = {k: (info[k].copy() if info[k].ndim else int(info[k])) for k in INFO.names}
    out["supported"] = bool(out["supported"])
    out["reason_code"] = out["reason"]
    out["reason"] = REASONS[out["reason_code"]]
    return out


def entropy_decode(payload, info, coef_out):
    """dspn_jpeg_entropy_decode into the int16 array coef_out (info["coef_count"] values); -> status"""
    assert coef_out.dtype == np.int16 and coef_out.flags.c_contiguous and coef_out.size >= int(info["coef_count"])
    rec = np.array([info], INFO)
    return _lib.lib().dspn_jpeg_entropy_decode(_c.c_char_p(payload), len(payload), rec.ctypes.data, coef_out.ctypes.data)


def fill_sample(s, info, coef_base, img_offset):
    """the device descriptor of a probed stream whose coefficients start at int16 index coef_base of the batch's pool"""
    s["coef_offset"] = info["coef_offset"] + coef_base
    s["img_offset"] = img_offset
    s["width"], s["height"], s["ncomp"], s["skip"] = info["width"], info["height"], info["ncomp"], 0
    s["hsamp"], s["vsamp"] = info["hsamp"][0], info["vsamp"][0]
    s["blocks_w"], s["blocks_h"], s["quant"] = info["blocks_w"], info["blocks_h"], info["quant"]


def reconstruct(coefs, samples, images_out, stream=None):
    """dspn_jpeg_reconstruct_batch_u8: coefs an int16 device tensor, samples a uint8 device tensor of B descriptors,
    images_out the uint8 device pool.  -> the workspace tensor (keep it alive until the stream has run the call)"""
    dev = coefs.device
    n = coefs.numel()
    ws_bytes = _lib.lib().dspn_jpeg_reconstruct_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_jpeg_reconstruct_batch_u8(coefs.data_ptr(), n, samples.data_ptr(),
                                                         samples.numel() // SAMPLE.itemsize, images_out.data_ptr(),
                                                         images_out.numel(), ws.data_ptr(), ws_bytes, st),
               "jpeg_reconstruct")
    return ws


class Coded(object):
    """a JPEG payload the device will reconstruct: the probed header, with the `size` a batch layout reads from a PIL
    image"""

    def __init__(self, payload, info):
        self.payload, self.info = payload, info
        self.size = (int(info["width"]), int(info["height"]))


def open_image(content, device_jpeg):
    """sizes before any pixel is decoded: a Coded for a baseline JPEG the device decode supports (device_jpeg only), else
    a lazily opened Pillow image"""
    from PIL import Image
    if device_jpeg:
        rc, info = probe_info(content)
        if rc == 0 and info["supported"]:
            return Coded(content, info)
    return Image.open(io.BytesIO(content))


def decode_image(im, dst, coef_dst):
    """worker thread (ctypes and Pillow's decoders release the GIL): the coefficients of a Coded into coef_dst, or the
    pixels of anything else into the (h, w, 3) array dst.  -> True when the device reconstructs the image"""
    if isinstance(im, Coded):
        if entropy_decode(im.payload, im.info, coef_dst) == 0:
            return True
        from PIL import Image
        im = Image.open(io.BytesIO(im.payload))                 # a corrupt scan: Pillow decodes or raises
    dst[...] = np.asarray(im if im.mode == "RGB" else im.convert("RGB"))
    return False


class CodedBatch(staging.CodedBatch):
    """staging.CodedBatch over dspn_jpeg_sample: int16 coefficients in, RGB bytes out.  The pool is cut to at least 64
    values because the reconstruct entry refuses a count that is zero or not a multiple of 64."""
    SAMPLE, FLOOR = SAMPLE, 64

    def _describe(self, s, info, coef_base, img_offset):
        fill_sample(s, info, coef_base, img_offset)
        return int(info["coef_count"])

    def _launch(self, coef_dev, desc_dev, images_out):
        return (reconstruct(coef_dev, desc_dev, images_out),)   # the workspace


def decode_batch(payloads, device):
    """decode a list of JPEG byte strings -> list of (h, w, 3) uint8 RGB tensors on `device`, views of one pool.
    ValueError (naming the reason) for a stream outside the supported set, DspnError for a malformed one."""
    payloads = list(payloads)
    if len(payloads) > MAX_BATCH:                               # before any stream is decoded: the entry would refuse it after all of them
        raise ValueError("decode_batch: %d streams, the batch limit of one call is %d" % (len(payloads), MAX_BATCH))
    infos = []
    for i, p in enumerate(payloads):
        rc, info = probe_info(p)
        _lib.check(rc, "jpeg_probe (stream %d)" % i)
        if not info["supported"]:
            raise ValueError("stream %d is not decodable on the device: %s" % (i, REASONS[int(info["reason"])]))
        infos.append(info)
    if not infos:
        return []
    sizes = [int(i["width"]) * int(i["height"]) * 3 for i in infos]
    batch = CodedBatch(infos, np.cumsum([0] + sizes[:-1]))
    coefs = torch.empty(batch.count, dtype=torch.int16).pin_memory()
    for k, (p, info, dst) in enumerate(zip(payloads, infos, batch.slices(coefs.numpy()))):
        _lib.check(entropy_decode(p, info, dst), "jpeg_entropy_decode (stream %d)" % k)
    batch.answered([True] * len(infos))
    pool = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
    batch.upload(coefs, device)
    batch.launch(pool)
    torch.cuda.current_stream(device).synchronize()            # the pinned buffer and the workspace go out of scope here
    return [img.view(int(i["height"]), int(i["width"]), 3) for img, i in zip(pool.split(sizes), infos)]
