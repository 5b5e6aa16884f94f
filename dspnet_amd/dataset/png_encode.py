"""PNG encode split between device and host (include/dspn_png_encode.h), the mirror image of dataset/png.py: the device
picks a filter type for every row of every image of a batch and rewrites the rows under it, in one call of one launch; the
host does the serial rest -- deflate and the chunks around it -- per image on a thread pool (`zlib` releases the GIL around
the compression).  The filtered stream inside a file equals the one inside the file Pillow writes for the same pixels
(`Image.fromarray(x).save(f, format="PNG")`, no optimize) byte for byte; the deflate is Python's zlib with Pillow's settings
(level 6, Z_FILTERED), whose output may differ from Pillow's own zlib build by a few bytes, so the files are not compared.

Formats: 8-bit grey from (H, W) uint8, 8-bit RGB from (H, W, 3) uint8, 16-bit grey from (H, W) uint16; not interlaced, no
ancillary chunks.  `encode_batch` and `filter_batch` are the public use; `filter_into` is the C entry point.

`encode_batch(..., device_deflate=True)` keeps the deflate on the device as well (dspn_png_deflate_batch: matches of distance 1
only, dynamic Huffman codes per block of 32768 bytes, the rule in include/dspn_png_encode.h): only the compressed bytes cross
to the host, which adds the chunks and their CRC-32.  `deflate_batch` is that deflate alone over any byte streams,
`deflate_host` the same encoder on the host (the same bytes, no GPU)."""
import ctypes
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib
from . import png as _dp

SAMPLE = _lib.layout("dspn_png_enc_sample")                   # include/dspn_png_encode.h
MAX_ROW_BYTES = (1 << 24) - 1                                 # DSPN_PNG_ENC_MAX_ROW_BYTES
FORMATS = {1: (8, 0), 2: (16, 0), 3: (8, 2)}                  # bytes per pixel -> IHDR bit depth, colour type
_THREADS = 8                                                  # jpeg_encode.encode_batch's default


def filtered_bytes(width, height, bytes_per_pixel):
    """dspn_png_filtered_bytes: height * (1 + width * bytes_per_pixel), or 0 outside the supported sizes and formats"""
    return _lib.lib().dspn_png_filtered_bytes(int(width), int(height), int(bytes_per_pixel))


def _geometry(k, im):
    """(height, width, bytes per pixel) of image k, a tensor or an array; DspnError naming what was given otherwise"""
    dtype, shape = str(getattr(im, "dtype", type(im).__name__)).replace("torch.", ""), tuple(getattr(im, "shape", ()))
    if dtype == "uint8" and len(shape) == 2:
        bpp = 1
    elif dtype == "uint16" and len(shape) == 2:
        bpp = 2
    elif dtype == "uint8" and len(shape) == 3 and shape[2] == 3:
        bpp = 3
    else:
        raise _lib.DspnError("png_encode: image %d: (H, W) uint8, (H, W) uint16 or (H, W, 3) uint8, got %s %s" % (k, dtype, shape))
    if min(shape) < 1 or shape[1] * bpp > MAX_ROW_BYTES:
        raise _lib.DspnError("png_encode: image %d: sizes from 1 and rows of at most %d bytes, got %s %s" % (k, MAX_ROW_BYTES, dtype, shape))
    return int(shape[0]), int(shape[1]), bpp


def _on_device(images):
    """the images as contiguous device tensors of one device; host tensors and arrays are uploaded to the device of the first
    device tensor, or to the current one"""
    dev = next((im.device for im in images if torch.is_tensor(im) and im.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    out = []
    for k, im in enumerate(images):
        t = im.detach() if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
        if t.is_cuda and t.device != dev:
            raise _lib.DspnError("png_encode: image %d is on %s, the batch on %s" % (k, t.device, dev))
        out.append(t.to(dev).contiguous())
    return dev, out


def filter_into(samples, src, out, stream=None):
    """dspn_png_filter_batch: samples a HOST array of SAMPLE records, src the uint8 device pool of pixels, out the uint8
    device pool that receives the filtered streams.  -> the workspace tensor (keep it alive until the stream has run the call)"""
    assert samples.dtype == SAMPLE and samples.flags.c_contiguous
    lib = _lib.lib()
    ws_bytes = lib.dspn_png_filter_workspace_bytes(len(samples))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=out.device)
    st = torch.cuda.current_stream(out.device).cuda_stream if stream is None else stream
    _lib.check(lib.dspn_png_filter_batch(samples.ctypes.data, len(samples), src.data_ptr(), src.numel(), out.data_ptr(),
                                         out.numel(), ws.data_ptr(), ws_bytes, st), "png_filter")
    return ws


def _filter_to_host(images):
    """-> (uint8 host array of all filtered streams, back to back in pinned memory; list of (offset, bytes, height, width,
    bytes per pixel)): one filter call and one device-to-host copy for the whole batch"""
    geometry = [_geometry(k, im) for k, im in enumerate(images)]
    dev, tensors = _on_device(images)
    samples = np.zeros(len(images), SAMPLE)
    spans = []
    so = oo = 0
    for s, t, (h, w, bpp) in zip(samples, tensors, geometry):
        s["src_offset"], s["out_offset"], s["width"], s["height"], s["bytes_per_pixel"], s["src_pitch"] = so, oo, w, h, bpp, w * bpp
        n = h * (1 + w * bpp)
        spans.append((oo, n, h, w, bpp))
        so += h * w * bpp
        oo += n
    with torch.cuda.device(dev):
        flat = [t.reshape(-1).view(torch.uint8) for t in tensors]
        src = flat[0] if len(flat) == 1 else torch.cat(flat)
        out = torch.empty(oo, dtype=torch.uint8, device=dev)
        ws = filter_into(samples, src, out)
        host = torch.empty(oo, dtype=torch.uint8).pin_memory()
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()           # pixels, workspace and device streams go out of scope after this
    del ws
    return host.numpy(), spans


def filter_batch(images):
    """list of images (see encode_batch) -> list of bytes: per image its height rows of 1 + row_bytes bytes, each a filter
    type followed by the filtered row -- what zlib.decompress of the file's IDAT data gives, for callers that compress
    themselves"""
    images = list(images)
    if not images:
        return []
    host, spans = _filter_to_host(images)
    return [host[o:o + n].tobytes() for o, n, _, _, _ in spans]


def _chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def assemble(filtered, width, height, bytes_per_pixel, compress_level=6):
    """the file around one filtered stream (a bytes-like of height * (1 + row_bytes) bytes): signature, IHDR, one IDAT, IEND"""
    depth, colour = FORMATS[bytes_per_pixel]
    z = zlib.compressobj(compress_level, zlib.DEFLATED, 15, 8, zlib.Z_FILTERED)
    idat = z.compress(filtered) + z.flush()
    return b"".join((_dp.SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, 0)),
                     _chunk(b"IDAT", idat), _chunk(b"IEND")))


def deflate_bound(nbytes):
    """dspn_png_deflate_bound: the most a zlib stream of the device deflate takes for nbytes input bytes (0 below 1)"""
    return _lib.lib().dspn_png_deflate_bound(int(nbytes))


def deflate_host(data):
    """dspn_png_deflate_host: a bytes-like of at least one byte -> the zlib stream the device deflate writes for it, as bytes,
    formed on the host by the same encoder"""
    src = np.frombuffer(data, np.uint8)
    if src.size < 1:
        raise _lib.DspnError("png_deflate: a stream of 0 bytes")
    lib = _lib.lib()
    out = np.empty(lib.dspn_png_deflate_bound(src.size), np.uint8)
    length = ctypes.c_longlong(0)
    _lib.check(lib.dspn_png_deflate_host(src.ctypes.data, src.size, out.ctypes.data, out.size, ctypes.addressof(length)), "png_deflate_host")
    return out[:length.value].tobytes()


def deflate_into(spans, pool, out, result, stream=None):
    """dspn_png_deflate_batch: spans a list of (offset, bytes) into the uint8 device pool, out the uint8 device pool of at
    least the sum of the bounds, result a device int64 tensor of 2 * len(spans) -> the workspace tensor (keep it alive until
    the stream has run the call)"""
    lib = _lib.lib()
    offsets = np.ascontiguousarray([o for o, _ in spans], np.int64)
    sizes = np.ascontiguousarray([n for _, n in spans], np.int64)
    ws_bytes = lib.dspn_png_deflate_workspace_bytes(len(spans), int(sizes.sum()))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=out.device)
    st = torch.cuda.current_stream(out.device).cuda_stream if stream is None else stream
    _lib.check(lib.dspn_png_deflate_batch(offsets.ctypes.data, sizes.ctypes.data, len(spans), pool.data_ptr(), pool.numel(),
                                          out.data_ptr(), out.numel(), result.data_ptr(), ws.data_ptr(), ws_bytes, st), "png_deflate")
    return ws


def _deflate_to_host(spans, pool):
    """the zlib streams of the spans of a device pool -> (uint8 host array in pinned memory, list of (offset, bytes)): the
    launches, one small copy of `result`, one copy of the used prefix of the output"""
    dev = pool.device
    with torch.cuda.device(dev):
        out = torch.empty(sum(deflate_bound(n) for _, n in spans), dtype=torch.uint8, device=dev)
        result = torch.empty(2 * len(spans), dtype=torch.int64, device=dev)
        ws = deflate_into(spans, pool, out, result)
        placed = result.cpu().numpy().reshape(-1, 2)            # waits for the launches
        used = int(placed[-1, 0] + placed[-1, 1])
        host = torch.empty(used, dtype=torch.uint8).pin_memory()
        host.copy_(out[:used], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    del ws
    return host.numpy(), [(int(o), int(n)) for o, n in placed]


def deflate_batch(streams):
    """list of byte streams of at least one byte each -- 1-d uint8 device tensors, or host tensors / arrays / bytes-likes,
    which are uploaded first -- -> list of zlib streams as bytes, each equal to deflate_host's for the same input.  One call
    of dspn_png_deflate_batch for the batch, one small copy of its result table and one copy of the used prefix of its output
    into pinned memory."""
    streams = list(streams)
    if not streams:
        return []
    dev = next((s.device for s in streams if torch.is_tensor(s) and s.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    flat = []
    for k, s in enumerate(streams):
        t = s.detach() if torch.is_tensor(s) else torch.from_numpy(np.frombuffer(s, np.uint8).copy())
        if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < 1:
            raise _lib.DspnError("png_deflate: stream %d: a 1-d uint8 stream of at least one byte, got %s %s" % (k, t.dtype, tuple(t.shape)))
        if t.is_cuda and t.device != dev:
            raise _lib.DspnError("png_deflate: stream %d is on %s, the batch on %s" % (k, t.device, dev))
        flat.append(t.to(dev).contiguous())
    spans, at = [], 0
    for t in flat:
        spans.append((at, t.numel()))
        at += t.numel()
    with torch.cuda.device(dev):
        pool = flat[0] if len(flat) == 1 else torch.cat(flat)
    host, placed = _deflate_to_host(spans, pool)
    return [host[o:o + n].tobytes() for o, n in placed]


def _filter_and_deflate(images):
    """-> (uint8 host array of the zlib streams, list of (offset, bytes, height, width, bytes per pixel)): the filter call and
    the deflate call on one stream; the filtered streams stay on the device"""
    geometry = [_geometry(k, im) for k, im in enumerate(images)]
    dev, tensors = _on_device(images)
    samples = np.zeros(len(images), SAMPLE)
    spans = []
    so = oo = 0
    for s, (h, w, bpp) in zip(samples, geometry):
        s["src_offset"], s["out_offset"], s["width"], s["height"], s["bytes_per_pixel"], s["src_pitch"] = so, oo, w, h, bpp, w * bpp
        n = h * (1 + w * bpp)
        spans.append((oo, n))
        so += h * w * bpp
        oo += n
    with torch.cuda.device(dev):
        flat = [t.reshape(-1).view(torch.uint8) for t in tensors]
        src = flat[0] if len(flat) == 1 else torch.cat(flat)
        filtered = torch.empty(oo, dtype=torch.uint8, device=dev)
        ws = filter_into(samples, src, filtered)
        host, placed = _deflate_to_host(spans, filtered)
    del ws
    return host, [(o, n, h, w, bpp) for (o, n), (h, w, bpp) in zip(placed, geometry)]


def wrap(idat, width, height, bytes_per_pixel):
    """the file around one finished zlib stream: signature, IHDR, one IDAT, IEND"""
    depth, colour = FORMATS[bytes_per_pixel]
    return b"".join((_dp.SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, 0)),
                     _chunk(b"IDAT", idat), _chunk(b"IEND")))


def encode_batch(images, compress_level=6, threads=None, device_deflate=False):
    """list of images of any mix of sizes -- (H, W) uint8, (H, W) uint16 or (H, W, 3) uint8 RGB; device tensors, or host
    tensors / arrays, which are uploaded first -- -> list of PNG files as bytes (modes L, I;16 and RGB).  One filter call,
    one copy of the filtered streams into pinned memory, then deflate (compress_level, Z_FILTERED: Pillow's settings) and the
    chunks of each image on `threads` threads (default 8, never more than images).  DspnError names a dtype or shape outside
    the three formats.

    device_deflate=True: the filter call's output feeds dspn_png_deflate_batch on the same stream, the filtered streams are
    not copied to the host, and the threads only form the CRC-32 and the chunks.  compress_level is not used on this path.
    The files hold the same pixels and the same filtered stream; they are larger than the default path's (about
    1.6 times for label maps, under 1 % for photo-like images), which is why it is opt-in.  It is for large photo-like
    images, where the host deflate is nearly all of the call."""
    images = list(images)
    if not images:
        return []
    threads = _THREADS if threads is None else int(threads)
    if device_deflate:
        host, spans = _filter_and_deflate(images)

        def one(span):
            o, n, h, w, bpp = span
            return wrap(memoryview(host[o:o + n]), w, h, bpp)
    else:
        host, spans = _filter_to_host(images)

        def one(span):
            o, n, h, w, bpp = span
            return assemble(memoryview(host[o:o + n]), w, h, bpp, compress_level)

    if threads <= 1 or len(images) == 1:
        return [one(s) for s in spans]
    with ThreadPoolExecutor(min(threads, len(images))) as tp:
        return list(tp.map(one, spans))
