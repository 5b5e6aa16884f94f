"""JPEG encode split between device and host (include/dspn_jpeg_encode.h), the mirror image of dataset/jpeg.py: the device
converts the colours, downsamples the chroma, runs the forward DCT and quantises for a whole batch of images of mixed sizes
in one call of two launches; the host does the serial rest -- markers and Huffman coding -- per image on a thread pool
(ctypes releases the GIL around it), or, with device_entropy=True, the device codes the scans as well and the host is left
with the marker segments and a join.  The files equal what Pillow writes for the same pixels and settings
(`Image.fromarray(x).save(f, format="JPEG", quality=q, subsampling=s)`: libjpeg-turbo, standard Huffman tables) byte for byte.

`encode_batch` and `quant_tables` are the public use; `fill_sample`, `encode_blocks` and `entropy_encode` are the three C
entry points one by one, `entropy_scan_batch`, `entropy_write_batch` and `headers` those of the device entropy pass."""
import ctypes as _c
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib

SAMPLE = _lib.layout("dspn_jpeg_enc_sample")                  # include/dspn_jpeg_encode.h
SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}      # luma sampling, h x v
CHANNEL_ORDER = {"rgb": (0, 1, 2), "bgr": (2, 1, 0)}                   # where R, G and B sit in a pixel
MAX_SIDE = 65500                                                       # libjpeg's, and so Pillow's
_TOO_SMALL = -2


def quant_tables(quality):
    """-> (luminance, chrominance): the (64,) uint8 tables of a quality 1..100 in natural (row-major) order, as libjpeg
    scales Annex K's"""
    lum, chrom = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    _lib.check(_lib.lib().dspn_jpeg_quant_tables(int(quality), lum.ctypes.data, chrom.ctypes.data), "jpeg_quant_tables")
    return lum, chrom


def fill_sample(s, width, height, ncomp, sampling, tables, coef_base, img_offset):
    """fills the descriptor `s` (a SAMPLE record) of one image whose coefficients start at int16 index coef_base of the
    batch's pool and whose pixels start at byte img_offset of the image pool; -> its number of coefficients"""
    s["width"], s["height"], s["ncomp"], s["skip"] = width, height, ncomp, 0
    s["hsamp"], s["vsamp"] = sampling
    s["img_offset"] = img_offset
    s["quant"] = np.stack([tables[0], tables[1], tables[1]])
    n = _c.c_longlong(0)
    rec = np.array([s], SAMPLE)
    _lib.check(_lib.lib().dspn_jpeg_encode_geometry(rec.ctypes.data, int(coef_base), _c.byref(n)), "jpeg_encode_geometry")
    for key in ("coef_offset", "hsamp", "vsamp", "blocks_w", "blocks_h"):
        s[key] = rec[0][key]
    return n.value


def encode_blocks(images, samples, coefs, channel_order="rgb", stream=None):
    """dspn_jpeg_encode_blocks_batch_u8: images the uint8 device pool, samples a uint8 device tensor of B descriptors,
    coefs the int16 device tensor that receives the coefficients.  -> the workspace tensor (keep it alive until the
    stream has run the call)"""
    dev = coefs.device
    n = coefs.numel()
    ws_bytes = _lib.lib().dspn_jpeg_encode_workspace_bytes(n)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    cmap = (_c.c_int * 3)(*CHANNEL_ORDER[channel_order])
    _lib.check(_lib.lib().dspn_jpeg_encode_blocks_batch_u8(images.data_ptr(), images.numel(), cmap, samples.data_ptr(),
                                                           samples.numel() // SAMPLE.itemsize, coefs.data_ptr(), n,
                                                           ws.data_ptr(), ws_bytes, st),
               "jpeg_encode_blocks")
    return ws


def entropy_encode(coefs, sample, capacity=None, restart_interval=0):
    """dspn_jpeg_entropy_encode_restart: the file of one image as bytes.  coefs: the int16 host array
    sample["coef_offset"] indexes; capacity: a first guess of the file's size (the call is repeated with the size it names
    if that was short); restart_interval: MCUs between restart markers (Pillow's restart_marker_blocks), 0: none"""
    assert coefs.dtype == np.int16 and coefs.flags.c_contiguous
    nc = int(sample["ncomp"])
    last = max(int(sample["coef_offset"][c]) + 64 * int(sample["blocks_w"][c]) * int(sample["blocks_h"][c]) for c in range(nc))
    assert coefs.size >= last, "the coefficient array is shorter than the descriptor says"
    rec = np.array([sample], SAMPLE)
    lib = _lib.lib()
    n = _c.c_size_t(0)
    ri = int(restart_interval)
    cap = int(capacity) if capacity else 1024 + last // 2
    for _ in range(2):
        out = np.empty(cap, np.uint8)
        rc = lib.dspn_jpeg_entropy_encode_restart(coefs.ctypes.data, rec.ctypes.data, ri, out.ctypes.data, cap, _c.byref(n))
        if rc != _TOO_SMALL:
            break
        cap = n.value
    _lib.check(rc, "jpeg_entropy_encode")
    return out[:n.value].tobytes()


def headers(sample, restart_interval=0):
    """dspn_jpeg_encode_headers: SOI through the SOS header of entropy_encode's file, as bytes"""
    rec = np.array([sample], SAMPLE)
    lib = _lib.lib()
    n = _c.c_size_t(0)
    out = np.empty(1024, np.uint8)                             # 623 bytes for colour with a DRI segment
    _lib.check(lib.dspn_jpeg_encode_headers(rec.ctypes.data, int(restart_interval), out.ctypes.data, out.size, _c.byref(n)),
               "jpeg_encode_headers")
    return out[:n.value].tobytes()


def entropy_scan_batch(coefs, samples, intervals, stream=None):
    """dspn_jpeg_entropy_encode_scan_batch: coefs the int16 device pool, samples a uint8 device tensor of B descriptors,
    intervals an int32 device tensor of B restart intervals in MCUs.  -> (scan_bytes int64 (B,), status int32 (B,), workspace),
    all on the device; the workspace goes to entropy_write_batch as it is"""
    dev = coefs.device
    B = samples.numel() // SAMPLE.itemsize
    ws_bytes = _lib.lib().dspn_jpeg_entropy_encode_workspace_bytes(coefs.numel(), B)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    sizes = torch.empty(B, dtype=torch.int64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_jpeg_entropy_encode_scan_batch(coefs.data_ptr(), coefs.numel(), samples.data_ptr(), intervals.data_ptr(), B,
                                                              sizes.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, st),
               "jpeg_entropy_encode_scan")
    return sizes, status, ws


def entropy_write_batch(coef_count, offsets, out, ws, stream=None):
    """dspn_jpeg_entropy_encode_write_batch: offsets an int64 device tensor of B byte offsets into the uint8 device tensor
    out, ws the workspace of entropy_scan_batch over coef_count coefficients"""
    st = torch.cuda.current_stream(out.device).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_jpeg_entropy_encode_write_batch(int(coef_count), offsets.numel(), offsets.data_ptr(), out.data_ptr(),
                                                               out.numel(), ws.data_ptr(), ws.numel(), st),
               "jpeg_entropy_encode_write")


def mcus_per_row(sample):
    """MCUs in one row of the image a filled descriptor describes"""
    hs = int(sample["hsamp"]) if int(sample["ncomp"]) == 3 else 1
    return (int(sample["width"]) + 8 * hs - 1) // (8 * hs)


def _interval_of(sample, restart_interval, restart_rows):
    """the restart interval of one image in MCUs; libjpeg caps an interval given in rows at 65535 MCUs"""
    return min(int(restart_rows) * mcus_per_row(sample), 65535) if restart_rows else int(restart_interval)


def _device_scans(samples, desc, coefs, restart_interval, restart_rows):
    """encode_batch's device_entropy=True: the coefficients stay on the device, the coded scans come down"""
    dev = coefs.device
    ris = [_interval_of(s, restart_interval, restart_rows) for s in samples]
    intervals = torch.tensor(ris, dtype=torch.int32).to(dev)
    sizes, status, ws = entropy_scan_batch(coefs, desc, intervals)
    sizes, status = sizes.cpu().numpy(), status.cpu().numpy()  # the one small copy: 12 bytes per image
    for k in np.flatnonzero(status == 2):                      # the host pass words the refusal
        s = samples[k]
        lo = min(int(s["coef_offset"][c]) for c in range(int(s["ncomp"])))
        hi = max(int(s["coef_offset"][c]) + 64 * int(s["blocks_w"][c]) * int(s["blocks_h"][c]) for c in range(int(s["ncomp"])))
        local = s.copy()
        local["coef_offset"][:int(s["ncomp"])] -= lo
        entropy_encode(coefs[lo:hi].cpu().numpy(), local, restart_interval=ris[k])
    if status.any():
        raise _lib.DspnError("jpeg_encode: the device entropy pass refused images %s (status %s)"
                             % (np.flatnonzero(status).tolist(), status[status != 0].tolist()))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scans = torch.empty(max(int(offsets[-1]), 1), dtype=torch.uint8, device=dev)
    entropy_write_batch(coefs.numel(), torch.from_numpy(offsets[:-1].copy()).to(dev), scans, ws)
    host = torch.empty(scans.numel(), dtype=torch.uint8).pin_memory()
    host.copy_(scans, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    data = host.numpy()
    return [headers(s, ri) + data[a:b].tobytes() + b"\xff\xd9" for s, ri, a, b in zip(samples, ris, offsets[:-1], offsets[1:])]


def encode_batch(images, quality=95, subsampling="4:2:0", channel_order="rgb", threads=8, restart_interval=0, restart_rows=0,
                 device_entropy=False):
    """list of uint8 device tensors, (h, w, 3) or (h, w), of any mix of sizes -> list of JPEG files as bytes, each equal
    to Pillow's `Image.fromarray(x).save(f, format="JPEG", quality=quality, subsampling=subsampling)` (x in RGB order;
    channel_order="bgr" reads OpenCV's order instead; a (h, w) image is greyscale, for which subsampling says nothing).
    One upload of descriptors, two launches, one copy of the coefficients into pinned memory, and the entropy pass of
    the images on `threads` threads.
    restart_interval=n writes a restart marker every n MCUs (Pillow's restart_marker_blocks=n), restart_rows=r every r
    MCU rows of each image (restart_marker_rows=r); at most one of the two.  Such files decode entirely on the device
    (dataset/jpeg.py, device_entropy=True) when the interval is at most jpeg.DEVICE_MAX_INTERVAL MCUs.
    device_entropy=True: the scans are Huffman-coded on the device too (dspn_jpeg_entropy_encode_scan_batch / _write_batch):
    the sizes come down (12 bytes per image), then the coded scans in one copy instead of the coefficients; the host
    writes the marker segments around them.  The files are the same bytes."""
    if restart_interval and restart_rows:
        raise ValueError("restart_interval and restart_rows: at most one of the two")
    if not 0 <= int(restart_interval) <= 65535 or int(restart_rows) < 0:
        raise ValueError("restart_interval is 0..65535 MCUs and restart_rows >= 0, got %r and %r" % (restart_interval, restart_rows))
    if subsampling not in SUBSAMPLING:
        raise ValueError("subsampling is one of %s, got %r" % (sorted(SUBSAMPLING), subsampling))
    if channel_order not in CHANNEL_ORDER:
        raise ValueError("channel_order is 'rgb' or 'bgr', got %r" % (channel_order,))
    images = list(images)
    if not images:
        return []
    if len(images) > 1024:
        return sum((encode_batch(images[k:k + 1024], quality, subsampling, channel_order, threads, restart_interval, restart_rows,
                                 device_entropy)
                    for k in range(0, len(images), 1024)), [])
    tables = quant_tables(quality)
    dev = images[0].device
    for k, im in enumerate(images):
        if not (torch.is_tensor(im) and im.is_cuda and im.device == dev and im.dtype == torch.uint8):
            raise ValueError("image %d: uint8 tensors on one device, got %s" % (k, getattr(im, "dtype", type(im))))
        if not (im.dim() == 2 or (im.dim() == 3 and im.shape[2] == 3)) or min(im.shape[:2]) < 1 or max(im.shape[:2]) > MAX_SIDE:
            raise ValueError("image %d: (h, w, 3) or (h, w) with sides 1..%d, got %s" % (k, MAX_SIDE, tuple(im.shape)))
    samples = np.zeros(len(images), SAMPLE)
    co = io = 0
    for k, im in enumerate(images):
        ncomp = 3 if im.dim() == 3 else 1
        co += fill_sample(samples[k], int(im.shape[1]), int(im.shape[0]), ncomp, SUBSAMPLING[subsampling], tables, co, io)
        io += im.numel()
    with torch.cuda.device(dev):
        pool = images[0].contiguous().view(-1) if len(images) == 1 else torch.cat([im.reshape(-1) for im in images])
        desc = torch.from_numpy(samples.view(np.uint8).reshape(-1)).to(dev)
        coefs = torch.empty(co, dtype=torch.int16, device=dev)
        ws = encode_blocks(pool, desc, coefs, channel_order)
        if device_entropy:
            return _device_scans(samples, desc, coefs, restart_interval, restart_rows)
        host = torch.empty(co, dtype=torch.int16).pin_memory()
        host.copy_(coefs, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()           # pool, descriptors and workspace go out of scope after this
    del ws
    cnp = host.numpy()
    def one(s):
        return entropy_encode(cnp, s, restart_interval=_interval_of(s, restart_interval, restart_rows))

    if threads <= 1 or len(images) == 1:
        return [one(s) for s in samples]
    with ThreadPoolExecutor(min(int(threads), len(images))) as tp:
        return list(tp.map(one, samples))
