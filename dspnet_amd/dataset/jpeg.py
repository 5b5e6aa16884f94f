"""JPEG decode split between host and device (include/dspn_jpeg.h): the host parses the markers and Huffman-decodes the
scan into quantised DCT coefficients (serial work; ctypes releases the GIL around it, so a thread pool runs it in
parallel), the device dequantises, inverts the DCT, upsamples the chroma and converts to RGB for a whole batch in one
call.  The pixels equal Pillow's (libjpeg-turbo, accurate integer IDCT, fancy upsampling) byte for byte.

A stream with restart intervals (what `jpeg_encode.encode_batch(..., restart_interval=n)` and `im2rec` write, and Pillow
with `restart_marker_blocks=n`) can leave the host pass out: the host only finds the restart markers (`scan_index`), the
device Huffman-decodes one interval per lane in front of the reconstruction (`device_entropy=True`, off by default),
and the upload is the compressed scan instead of the coefficients.

`probe`, `scan_index` and `decode_batch` are the public use; the iterators (device_jpeg=True) go through `open_image`,
`decode_image` and `CodedBatch` with their own pools (dataset/staging.py)."""
import ctypes as _c
import io

import numpy as np
import torch

from .. import _lib
from . import staging

INFO = _lib.layout("dspn_jpeg_info")                           # include/dspn_jpeg.h
SAMPLE = _lib.layout("dspn_jpeg_sample")
SCAN = _lib.layout("dspn_jpeg_scan")                           # the device entropy pass's descriptor of a stream with restart intervals
DEVICE_MAX_INTERVAL = _lib.DEFINES["DSPN_JPEG_DEVICE_MAX_INTERVAL"]
STATUS_SEGMENTS = (1 << 27) - 1                                # DSPN_JPEG_STATUS_SEGMENTS
STATUS_CODES = ("ok", "a Huffman code that is not in its table", "a coefficient index past 63",
                "a DC difference of more than 11 bits or an AC value of more than 10", "data that ends inside a block",
                "unread data before the segment's end", "a DC value out of range",
                "a segment table or Huffman table that contradicts itself")
REASONS = ("ok", "progressive", "extended sequential", "arithmetic coding", "lossless or hierarchical",
           "sample precision is not 8 bits", "neither 1 nor 3 components", "unsupported sampling factors",
           "more than one scan", "colour transform is not YCbCr", "16-bit quantisation table")
MAX_BATCH = 1024                                               # kMaxB of csrc/jpeg.hip: descriptors of one reconstruct call


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


def scan_segments(info):
    """restart intervals of a probed stream (dspn_jpeg_scan_segments); 0 without a restart interval"""
    rec = np.array([info], INFO)
    return int(_lib.lib().dspn_jpeg_scan_segments(rec.ctypes.data))


def device_entropy_ok(info):
    """whether the device entropy pass takes the probed stream: supported, with a restart interval of at most
    DEVICE_MAX_INTERVAL MCUs (what dspn_jpeg_scan_index accepts, told from the header alone)"""
    return bool(info["supported"]) and 0 < int(info["restart_interval"]) <= DEVICE_MAX_INTERVAL


def scan_index_into(payload, info, scan, seg_offsets):
    """dspn_jpeg_scan_index into the SCAN record `scan` and the uint32 array seg_offsets; -> status"""
    assert seg_offsets.dtype == np.uint32 and seg_offsets.flags.c_contiguous
    rec, out = np.array([info], INFO), np.zeros(1, SCAN)
    rc = _lib.lib().dspn_jpeg_scan_index(_c.c_char_p(payload), len(payload), rec.ctypes.data, out.ctypes.data,
                                         seg_offsets.ctypes.data, seg_offsets.size)
    for name in SCAN.names:
        scan[name] = out[0][name]
    return rc


def scan_index(payload, info):
    """the restart intervals of a probed stream, found without any Huffman work -> (SCAN record, uint32 offsets): where
    the data of each interval starts, relative to scan["data_offset"] (the first byte of entropy-coded data in
    `payload`), plus one closing offset, scan["data_bytes"].  Raises DspnError, naming the reason, for a stream the
    device entropy pass does not take (no restart interval, or one above DEVICE_MAX_INTERVAL: it stays on the host pass)
    and for restart markers that are missing, misnumbered or too many."""
    seg = np.zeros(scan_segments(info) + 1, np.uint32)
    scan = np.zeros(1, SCAN)
    _lib.check(scan_index_into(payload, info, scan[0], seg), "jpeg_scan_index")
    return scan[0], seg


def status_parts(word):
    """a status word of the device entropy pass -> (code, first bad segment)"""
    word = int(word)
    return word & 7, STATUS_SEGMENTS - (word >> 3)


def entropy_decode_segments(pool, sample, scan, seg_offsets, coefs):
    """dspn_jpeg_entropy_decode_segments: the device's decode built for the host, over ONE sample whose descriptors
    index the uint8 array `pool`, the uint32 array seg_offsets and the int16 array coefs -> the status word"""
    assert pool.dtype == np.uint8 and seg_offsets.dtype == np.uint32 and coefs.dtype == np.int16
    s, sc, st = np.array([sample], SAMPLE), np.array([scan], SCAN), _c.c_int(0)
    _lib.check(_lib.lib().dspn_jpeg_entropy_decode_segments(pool.ctypes.data, pool.size, s.ctypes.data, sc.ctypes.data,
                                                            seg_offsets.ctypes.data, seg_offsets.size, coefs.ctypes.data,
                                                            coefs.size, _c.byref(st)), "jpeg_entropy_decode_segments")
    return st.value


def entropy_decode_device(pool, samples, scans, seg_offsets, coefs, status, stream=None):
    """dspn_jpeg_entropy_decode_batch: pool the uint8 device byte pool, samples and scans uint8 device tensors of B
    descriptors each, seg_offsets an int32 device tensor (the uint32 table), coefs the int16 device pool, status an int32
    device tensor of B words (zeroed by the call)"""
    B = samples.numel() // SAMPLE.itemsize
    assert scans.numel() == B * SCAN.itemsize and status.numel() >= B and status.dtype == torch.int32
    st = torch.cuda.current_stream(coefs.device).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_jpeg_entropy_decode_batch(pool.data_ptr(), pool.numel(), samples.data_ptr(), scans.data_ptr(),
                                                         B, seg_offsets.data_ptr(), seg_offsets.numel(), coefs.data_ptr(),
                                                         coefs.numel(), status.data_ptr(), st),
               "jpeg_entropy_decode_batch")


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


def decode_image(im, dst, coef_dst, index=None):
    """worker thread (ctypes and Pillow's decoders release the GIL): the coefficients of a Coded into coef_dst -- or, with
    `index` (CodedBatch.indexers: the sample's entropy pass runs on the device), only the index of its scan --, or the
    pixels of anything else into the (h, w, 3) array dst.  -> True when the device reconstructs the image"""
    if isinstance(im, Coded):
        if (index(im.payload) if index is not None else entropy_decode(im.payload, im.info, coef_dst) == 0):
            return True
        from PIL import Image
        im = Image.open(io.BytesIO(im.payload))                 # a corrupt scan: Pillow decodes or raises
    dst[...] = np.asarray(im if im.mode == "RGB" else im.convert("RGB"))
    return False


class CodedBatch(staging.CodedBatch):
    """staging.CodedBatch over dspn_jpeg_sample: int16 coefficients in, RGB bytes out.  The pool is cut to at least 64
    values because the reconstruct entry refuses a count that is zero or not a multiple of 64.

    device_entropy=True: the samples `device_entropy_ok` accepts get their coefficients from the device entropy pass.
    Their slices of the pool lie behind the host's and are never uploaded; what goes up for them is the compressed scan,
    the segment table and one dspn_jpeg_scan each, and one launch in front of the reconstruction decodes them.  The
    worker of such a sample calls its entry of `indexers()` instead of the host entropy pass.  After `launch`, `check`
    reads the status words."""
    SAMPLE, FLOOR = SAMPLE, 64

    def __init__(self, infos, out_offsets, device_entropy=False):
        side = [device_entropy and info is not None and device_entropy_ok(info) for info in infos]
        staging.CodedBatch.__init__(self, infos, out_offsets, side)
        self._infos, self._side = infos, side
        self.scans = np.zeros(len(infos), SCAN)
        counts = [scan_segments(info) + 1 if d else 0 for info, d in zip(infos, side)]
        self._seg_at = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.segments = np.zeros(max(int(self._seg_at[-1]), 1), np.uint32)
        self._payloads = [None] * len(infos)
        self.device_entropy = 0                                 # samples whose entropy pass the device runs (after `answered`)
        self.scan_bytes = 0                                     # bytes of compressed scan uploaded for them (after `upload`)
        self._status_dev = None

    def _describe(self, s, info, coef_base, img_offset):
        fill_sample(s, info, coef_base, img_offset)
        return int(info["coef_count"])

    def _index(self, k, payload):
        seg = self.segments[self._seg_at[k]:self._seg_at[k + 1]]
        if scan_index_into(payload, self._infos[k], self.scans[k], seg) != 0:
            self.scans[k]["segments"] = 0
            return False
        self.scans[k]["first_segment"] = self._seg_at[k]
        self._payloads[k] = payload
        return True

    def indexers(self):
        """per sample: the callable (payload) -> bool that indexes the sample's scan for the device entropy pass (thread-safe:
        each writes its own slices), or None where the host pass is due"""
        return [(lambda payload, k=k: self._index(k, payload)) if d else None for k, d in enumerate(self._side)]

    def answered(self, answers):
        staging.CodedBatch.answered(self, answers)
        for k, a in enumerate(answers):
            if not a:
                self.scans[k]["segments"] = 0                   # nothing for the entropy launch either
        self.device_entropy = sum(1 for a, d in zip(answers, self._side) if a and d)

    def upload(self, coded, device, decoded=None):
        if self.device_entropy:                                 # the compressed scans, back to back
            parts, at = [], 0
            for k, sc in enumerate(self.scans):
                if sc["segments"]:
                    a, n = int(sc["data_offset"]), int(sc["data_bytes"])
                    parts.append(np.frombuffer(self._payloads[k], np.uint8, n, a))
                    sc["data_offset"] = at
                    at += n
            self.scan_bytes = at
            pool = np.concatenate(parts) if at else np.zeros(1, np.uint8)
            self._scan_dev = torch.from_numpy(pool).to(device, non_blocking=True)
        return staging.CodedBatch.upload(self, coded, device, decoded)

    def _descriptors(self):
        d = self.samples.view(np.uint8).reshape(-1)
        if not self.device_entropy:
            return d
        return np.concatenate([d, self.scans.view(np.uint8).reshape(-1), self.segments.view(np.uint8)])

    def _launch(self, coef_dev, desc_dev, images_out):
        keep = ()
        if self.device_entropy:
            a, b = len(self.samples) * SAMPLE.itemsize, len(self.samples) * (SAMPLE.itemsize + SCAN.itemsize)
            self._status_dev = torch.empty(len(self.samples), dtype=torch.int32, device=coef_dev.device)
            entropy_decode_device(self._scan_dev, desc_dev[:a], desc_dev[a:b], desc_dev[b:].view(torch.int32), coef_dev,
                                  self._status_dev)
            keep = (self._scan_dev, self._status_dev)
            desc_dev = desc_dev[:a]
        return keep + (reconstruct(coef_dev, desc_dev, images_out),)   # the workspace

    def check(self, names=None):
        """after `launch`: reads the status words of the device entropy pass (one small copy; it waits for the stream) and
        raises DspnError naming the first sample whose scan the device could not decode.  The host pass falls back to
        Pillow for such a stream; this pass cannot, the batch is on the device by then."""
        if self._status_dev is None:
            return
        status = self._status_dev.cpu().numpy()
        for k in np.flatnonzero(status):
            code, seg = status_parts(status[k])
            raise _lib.DspnError("jpeg_entropy_decode_batch: %s: %s in restart interval %d (status code %d)"
                                 % (names[k] if names is not None else "stream %d" % k, STATUS_CODES[code], seg, code))


def decode_batch(payloads, device, device_entropy=False):
    """decode a list of JPEG byte strings -> list of (h, w, 3) uint8 RGB tensors on `device`, views of one pool.
    device_entropy=True: every stream `scan_index` accepts (restart intervals of at most DEVICE_MAX_INTERVAL MCUs, all
    markers in place) is decoded entirely on the device -- only its compressed scan is uploaded --, the others take the
    host entropy pass as before.
    ValueError (naming the reason) for a stream outside the supported set, DspnError for a malformed one (naming the
    stream; for the device entropy pass also the status code)."""
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
    batch = CodedBatch(infos, np.cumsum([0] + sizes[:-1]), device_entropy)
    coefs = torch.empty(max(batch.host_count, 1), dtype=torch.int16).pin_memory()
    for k, (p, info, dst, index) in enumerate(zip(payloads, infos, batch.slices(coefs.numpy()), batch.indexers())):
        if index is not None:
            _lib.check(0 if index(p) else -1, "jpeg_scan_index (stream %d)" % k)
        else:
            _lib.check(entropy_decode(p, info, dst), "jpeg_entropy_decode (stream %d)" % k)
    batch.answered([True] * len(infos))
    pool = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
    batch.upload(coefs, device)
    batch.launch(pool)
    torch.cuda.current_stream(device).synchronize()            # the pinned buffer and the workspace go out of scope here
    batch.check()
    return [img.view(int(i["height"]), int(i["width"]), 3) for img, i in zip(pool.split(sizes), infos)]
