"""PNG decode split between host and device (include/dspn_png.h): the host walks the chunks and inflates the concatenated
IDAT data (serial work; `zlib` releases the GIL around it, so a thread pool runs it in parallel), the device undoes the
row filters (Sub / Up / Average / Paeth) for a whole batch in one call.  The samples equal Pillow's byte for byte.

Supported: greyscale 8-bit, palette 8-bit (the indices are the samples: what np.asarray of a mode-"P" image gives) and
greyscale 16-bit, not interlaced, without tRNS and without animation.

`probe` and `decode_batch` are the public use (ground-truth id maps, instance-id maps, disparity maps held as PNG bytes);
MultiTaskRecordIter(device_png=True) goes through `open_label`, `decode_label` and `CodedBatch` with its own pools
(dataset/staging.py).

Colour images: `probe_rgb` and `decode_rgb_batch` give the bytes of Pillow's `Image.open(...).convert("RGB")` for every
non-interlaced format but 16-bit greyscale (which convert("RGB") clips; it stays with `decode_batch`): RGB, RGBA and
grey + alpha at 8 and 16 bits, greyscale and palette at 1, 2, 4 and 8 bits, with or without tRNS (convert("RGB") ignores
it).  The device reconstructs the rows at the format's stride and then makes the RGB bytes (dspn_png_rgb_batch).
im2rec's `_decode` uses `decode_rgb_batch`; DetIter(device_png=True) goes through `open_rgb`, `decode_rgb` and `RgbBatch`."""
import io
import struct
import zlib

import numpy as np
import torch

from .. import _lib
from . import staging

SAMPLE = _lib.layout("dspn_png_sample")                        # include/dspn_png.h
REASONS = ("ok", "bit depth below 8", "colour type is RGB, RGBA or grey + alpha", "Adam7 interlace", "tRNS chunk",
           "acTL chunk (APNG)", "not a bit depth / colour type / method of the PNG specification")
OK, LOW_DEPTH, COLOUR, INTERLACE, TRNS, APNG, NONSTANDARD = range(7)
RGB_SAMPLE = _lib.layout("dspn_png_rgb_sample")
PALETTE_BYTES = _lib.DEFINES["DSPN_PNG_PALETTE_BYTES"]
# probe_rgb's reasons (REASONS above is probe's alone)
RGB_REASONS = ("ok", "16-bit greyscale (convert(\"RGB\") clips it; decode_batch keeps the 16 bits)", "Adam7 interlace",
               "acTL chunk (APNG)", "not a bit depth / colour type / method of the PNG specification",
               "palette image without a PLTE chunk of 1 to 256 entries before IDAT")
RGB_OK, RGB_GREY16, RGB_INTERLACE, RGB_APNG, RGB_NONSTANDARD, RGB_NO_PLTE = range(6)
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}      # colour type -> legal bit depths
# inflate_into's statuses
INFLATE_OK, INFLATE_ZLIB, INFLATE_LENGTH, INFLATE_FILTER = 0, 1, 2, 3


def _malformed(what):
    return _lib.DspnError("png_probe: " + what)


def _walk(payload):
    """the chunk list of a stream -> (the IHDR fields, the (offset, length) of every IDAT chunk's data, the set of tRNS / acTL
    seen, the (offset, length) of the first PLTE chunk's data if it comes before IDAT, else None).  The CRC of every critical
    chunk is checked.  Raises DspnError on a malformed stream."""
    data = memoryview(payload)
    n = len(data)
    if n < 8 or bytes(data[:8]) != SIGNATURE:
        raise _malformed("bad signature")
    at, ihdr, idat, flags, plte, ended = 8, None, [], set(), None, False
    while not ended:
        if n - at < 12:
            raise _malformed("a chunk header runs past the end (no IEND)" if n > at else "no IEND chunk")
        length, kind = struct.unpack_from(">I4s", data, at)
        if length > n - at - 12:
            raise _malformed("chunk %r of %d bytes runs past the end" % (kind, length))
        body = at + 8
        if kind in _CRITICAL:
            (crc,) = struct.unpack_from(">I", data, body + length)
            if zlib.crc32(data[at + 4:body + length]) != crc:
                raise _malformed("bad CRC on chunk %r" % kind)
        if ihdr is None:
            if kind != b"IHDR" or length != 13:
                raise _malformed("the first chunk is not a 13-byte IHDR")
            ihdr = struct.unpack_from(">IIBBBBB", data, body)
        elif kind == b"IDAT":
            idat.append((body, length))
        elif kind == b"IEND":
            ended = True
        elif kind in (b"tRNS", b"acTL"):
            flags.add(kind)
        elif kind == b"PLTE" and plte is None and not idat:
            plte = (body, length)
        at = body + length + 4
    if not idat:
        raise _malformed("no IDAT chunk")
    if ihdr[0] == 0 or ihdr[1] == 0:
        raise _malformed("zero width or height")
    return ihdr, idat, flags, plte


def _standard(ihdr):
    width, height, depth, colour, compression, filtering, interlace = ihdr
    return colour in _DEPTHS and depth in _DEPTHS[colour] and not compression and not filtering and interlace <= 1 and \
        width <= 0x7fffffff and height <= 0x7fffffff


def probe(payload):
    """what the chunk list says, before any pixel work: a dict with width, height, bit_depth, colour_type, interlace,
    bytes_per_pixel, row_bytes, raw_bytes (= height * (row_bytes + 1), the inflated size), supported, reason (text),
    reason_code and idat (the (offset, length) of every IDAT chunk's data, for inflate_into).  The CRC of every critical
    chunk is checked.  Raises DspnError on a malformed stream: bad signature, bad CRC on a critical chunk, a chunk running
    past the end, no IHDR / IDAT / IEND, zero width or height."""
    ihdr, idat, flags, _ = _walk(payload)
    width, height, depth, colour, compression, filtering, interlace = ihdr
    if not _standard(ihdr):
        code = NONSTANDARD
    elif colour in (2, 4, 6):
        code = COLOUR
    elif depth < 8:
        code = LOW_DEPTH
    elif interlace:
        code = INTERLACE
    elif b"tRNS" in flags:
        code = TRNS
    elif b"acTL" in flags:
        code = APNG
    else:
        code = OK
    bpp = depth // 8 if code == OK else 0
    return {"width": width, "height": height, "bit_depth": depth, "colour_type": colour, "interlace": interlace,
            "bytes_per_pixel": bpp, "row_bytes": width * bpp, "raw_bytes": height * (width * bpp + 1) if bpp else 0,
            "supported": code == OK, "reason": REASONS[code], "reason_code": code, "idat": idat}


def probe_rgb(payload):
    """`probe` for the RGB path (decode_rgb_batch): the same dict, classified by RGB_REASONS, with bytes_per_pixel the
    filter stride (1 for the packed depths), row_bytes = ceil(width * channels * bit_depth / 8), and one more entry,
    `palette`: the PLTE chunk's data of a supported palette image (else None).  Raises DspnError as `probe` does."""
    ihdr, idat, flags, plte = _walk(payload)
    width, height, depth, colour, compression, filtering, interlace = ihdr
    if not _standard(ihdr):
        code = RGB_NONSTANDARD
    elif colour == 0 and depth == 16:
        code = RGB_GREY16
    elif interlace:
        code = RGB_INTERLACE
    elif b"acTL" in flags:
        code = RGB_APNG
    elif colour == 3 and (plte is None or plte[1] == 0 or plte[1] % 3 or plte[1] > PALETTE_BYTES):
        code = RGB_NO_PLTE
    else:
        code = RGB_OK
    ok = code == RGB_OK
    bits = _CHANNELS[colour] * depth if ok else 0
    row_bytes = (width * bits + 7) // 8
    palette = bytes(memoryview(payload)[plte[0]:plte[0] + plte[1]]) if ok and colour == 3 else None
    return {"width": width, "height": height, "bit_depth": depth, "colour_type": colour, "interlace": interlace,
            "bytes_per_pixel": max(1, bits // 8) if ok else 0, "row_bytes": row_bytes, "raw_bytes": height * (row_bytes + 1) if ok else 0,
            "supported": ok, "reason": RGB_REASONS[code], "reason_code": code, "idat": idat, "palette": palette}


def inflate_into(payload, info, dst):
    """inflate the concatenated IDAT data of a probed (`probe` or `probe_rgb`), supported stream into the uint8 array dst
    (info["raw_bytes"] bytes); every row keeps its filter-type byte in front, info["row_bytes"] + 1 bytes from the last one.  -> 0, or a non-zero status (never an exception) on a zlib error, an
    inflated length other than raw_bytes, or a filter type above 4; dst may then hold anything, nothing around it does."""
    want = info["raw_bytes"]
    assert info["supported"] and dst.dtype == np.uint8 and dst.ndim == 1 and dst.size == want
    data = memoryview(payload)
    spans = info["idat"]
    stream = data[spans[0][0]:spans[0][0] + spans[0][1]] if len(spans) == 1 else b"".join(data[o:o + n] for o, n in spans)
    try:
        z = zlib.decompressobj()
        raw = z.decompress(stream, want + 1)                     # one byte more than wanted shows a stream that is too long
    except zlib.error:
        return INFLATE_ZLIB
    if len(raw) != want or not z.eof:
        return INFLATE_LENGTH
    raw = np.frombuffer(raw, np.uint8)
    if raw[0::info["row_bytes"] + 1].max() > 4:
        return INFLATE_FILTER
    dst[:] = raw
    return INFLATE_OK


def fill_sample(s, info, raw_offset, out_offset, skip=0):
    """the device descriptor of a probed stream whose inflated rows start at byte raw_offset of the batch's raw pool"""
    s["raw_offset"], s["out_offset"] = raw_offset, out_offset
    s["width"], s["height"], s["bytes_per_pixel"], s["skip"] = info["width"], info["height"], info["bytes_per_pixel"], skip


def unfilter(raw_dev, samples_dev, out_dev, stream=None):
    """dspn_png_unfilter_batch: raw_dev the uint8 device pool of inflated rows, samples_dev a uint8 device tensor of
    descriptors, out_dev the uint8 device pool the samples go to"""
    dev = raw_dev.device
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_png_unfilter_batch(raw_dev.data_ptr(), raw_dev.numel(), samples_dev.data_ptr(),
                                                  samples_dev.numel() // SAMPLE.itemsize, out_dev.data_ptr(),
                                                  out_dev.numel(), st), "png_unfilter")


class CodedLabel(object):
    """a label-map PNG the device will unfilter: the probed chunk list, with the `size` a batch layout reads from a PIL
    image"""

    def __init__(self, payload, info):
        self.payload, self.info = payload, info
        self.size = (info["width"], info["height"])


def open_label(content, device_png):
    """sizes before anything is inflated: a CodedLabel for an 8-bit greyscale / palette stream the device decode supports
    (device_png only), else a lazily opened Pillow image"""
    from PIL import Image
    if device_png:
        try:
            info = probe(content)
            if info["supported"] and info["bytes_per_pixel"] == 1:
                return CodedLabel(content, info)
        except _lib.DspnError:
            pass                                                # malformed: Pillow decodes or raises as it always did
    return Image.open(io.BytesIO(content))


def decode_label(im, dst, raw_dst):
    """worker thread (zlib and Pillow's decoders release the GIL): the filtered rows of a CodedLabel into raw_dst, or the
    samples of anything else into the (h, w) array dst.  -> True when the device unfilters the label map"""
    if isinstance(im, CodedLabel):
        if inflate_into(im.payload, im.info, raw_dst) == 0:
            return True
        from PIL import Image
        im = Image.open(io.BytesIO(im.payload))                 # corrupt data: Pillow decodes or raises
    dst[...] = np.asarray(im if im.mode in ("L", "P") else im.convert("L"))
    return False


class CodedBatch(staging.CodedBatch):
    """staging.CodedBatch over dspn_png_sample: inflated rows with their filter bytes in, samples out"""
    SAMPLE, FLOOR = SAMPLE, 1

    def _describe(self, s, info, raw_offset, out_offset):
        fill_sample(s, info, raw_offset, out_offset)
        return info["raw_bytes"]

    def _launch(self, raw_dev, desc_dev, out_dev):
        unfilter(raw_dev, desc_dev, out_dev)
        return ()


def decode_batch(payloads, device):
    """decode a list of PNG byte strings -> list of (h, w) tensors on `device`, torch.uint8 for the 8-bit formats and
    torch.uint16 (native byte order) for 16-bit greyscale, views of one pool.  ValueError (naming the reason) for a stream
    outside the supported set, DspnError for a malformed one."""
    infos = []
    for i, p in enumerate(payloads):
        try:
            info = probe(p)
        except _lib.DspnError as e:
            raise _lib.DspnError("%s (stream %d)" % (e, i)) from None
        if not info["supported"]:
            raise ValueError("stream %d is not decodable on the device: %s" % (i, info["reason"]))
        infos.append(info)
    if not infos:
        return []
    sizes = [-(-i["height"] * i["row_bytes"] // 16) * 16 for i in infos]    # every image 16-byte aligned in the pool
    batch = CodedBatch(infos, np.cumsum([0] + sizes[:-1]))
    raw = torch.empty(batch.count, dtype=torch.uint8).pin_memory()
    for k, (p, info, dst) in enumerate(zip(payloads, infos, batch.slices(raw.numpy()))):
        status = inflate_into(p, info, dst)
        if status:
            raise _lib.DspnError("png_inflate (stream %d): %s" % (k, ("", "zlib error", "inflated length is not height * "
                                 "(row_bytes + 1)", "filter type above 4")[status]))
    batch.answered([True] * len(infos))
    pool = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
    batch.upload(raw, device)
    batch.launch(pool)
    torch.cuda.current_stream(device).synchronize()             # the pinned buffer goes out of scope here
    out = []
    for s, info in zip(batch.samples, infos):
        h, w, o = info["height"], info["width"], int(s["out_offset"])
        img = pool[o:o + h * info["row_bytes"]]
        out.append((img.view(torch.uint16) if info["bytes_per_pixel"] == 2 else img).view(h, w))
    return out


# ---- colour images to RGB (dspn_png_rgb_batch) ------------------------------------------------------------------------------
def rgb_workspace_bytes(samples):
    """dspn_png_rgb_workspace_bytes of an RGB_SAMPLE array on the host (no HIP call)"""
    samples = np.ascontiguousarray(samples, RGB_SAMPLE)
    return int(_lib.lib().dspn_png_rgb_workspace_bytes(samples.ctypes.data, samples.size))


def to_rgb(raw_dev, samples_dev, palettes_dev, out_dev, ws_dev, stream=None):
    """dspn_png_rgb_batch: raw_dev the uint8 device pool of inflated rows, samples_dev a uint8 device tensor of descriptors,
    palettes_dev a uint8 device tensor of 768-byte tables (may be empty), out_dev the uint8 device pool the RGB bytes go
    to, ws_dev the uint8 device scratch (may be empty)"""
    dev = raw_dev.device
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(_lib.lib().dspn_png_rgb_batch(raw_dev.data_ptr(), raw_dev.numel(), samples_dev.data_ptr(),
                                             samples_dev.numel() // RGB_SAMPLE.itemsize,
                                             palettes_dev.data_ptr() if palettes_dev.numel() else None,
                                             palettes_dev.numel() // PALETTE_BYTES, out_dev.data_ptr(), out_dev.numel(),
                                             ws_dev.data_ptr() if ws_dev.numel() else None, ws_dev.numel(), st), "png_rgb")


class RgbBatch(staging.CodedBatch):
    """staging.CodedBatch over dspn_png_rgb_sample: inflated rows with their filter bytes in, (h, w, 3) RGB bytes out.  The
    palettes travel behind the descriptors, in the same upload; the reconstructed rows of everything but RGB 8-bit pass
    through a device workspace laid out here (every image 16-byte aligned)."""
    SAMPLE, FLOOR = RGB_SAMPLE, 1

    def __init__(self, infos, out_offsets):
        self._palettes, self._recon = [], 0
        super().__init__(infos, out_offsets)

    def _describe(self, s, info, raw_offset, out_offset):
        s["raw_offset"], s["recon_offset"], s["out_offset"] = raw_offset, self._recon, out_offset
        s["width"], s["height"], s["bit_depth"], s["colour_type"] = info["width"], info["height"], info["bit_depth"], info["colour_type"]
        if info["colour_type"] == 3:
            s["palette_index"] = len(self._palettes)
            self._palettes.append(info["palette"].ljust(PALETTE_BYTES, b"\0"))
        if not (info["colour_type"] == 2 and info["bit_depth"] == 8):
            self._recon += -(-info["height"] * info["row_bytes"] // 16) * 16
        return info["raw_bytes"]

    def _descriptors(self):
        return np.concatenate([self.samples.view(np.uint8).reshape(-1), np.frombuffer(b"".join(self._palettes), np.uint8)])

    def _launch(self, raw_dev, desc_dev, out_dev):
        n = self.samples.size * RGB_SAMPLE.itemsize
        ws = torch.empty(rgb_workspace_bytes(self.samples), dtype=torch.uint8, device=out_dev.device)
        to_rgb(raw_dev, desc_dev[:n], desc_dev[n:], out_dev, ws)
        return (ws,)


def decode_rgb_batch(payloads, device):
    """decode a list of PNG byte strings -> list of (h, w, 3) torch.uint8 RGB tensors on `device`, views of one pool: the
    bytes of np.array(Image.open(p).convert("RGB")).  ValueError (naming the reason and the stream) for a stream `probe_rgb`
    does not support, DspnError for a malformed one or one that does not inflate."""
    infos = []
    for i, p in enumerate(payloads):
        try:
            info = probe_rgb(p)
        except _lib.DspnError as e:
            raise _lib.DspnError("%s (stream %d)" % (e, i)) from None
        if not info["supported"]:
            raise ValueError("stream %d is not decodable to RGB on the device: %s" % (i, info["reason"]))
        infos.append(info)
    if not infos:
        return []
    sizes = [i["height"] * i["width"] * 3 for i in infos]
    batch = RgbBatch(infos, np.cumsum([0] + sizes[:-1]))
    raw = torch.empty(batch.count, dtype=torch.uint8).pin_memory()
    for k, (p, info, dst) in enumerate(zip(payloads, infos, batch.slices(raw.numpy()))):
        status = inflate_into(p, info, dst)
        if status:
            raise _lib.DspnError("png_inflate (stream %d): %s" % (k, ("", "zlib error", "inflated length is not height * "
                                 "(row_bytes + 1)", "filter type above 4")[status]))
    batch.answered([True] * len(infos))
    pool = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
    batch.upload(raw, device)
    batch.launch(pool)
    torch.cuda.current_stream(device).synchronize()             # the pinned buffer and the workspace go out of scope here
    return [img.view(i["height"], i["width"], 3) for img, i in zip(pool.split(sizes), infos)]


class CodedRgb(object):
    """a colour PNG the device will turn into RGB: the probed chunk list, with the `size` a batch layout reads from a PIL
    image"""

    def __init__(self, payload, info):
        self.payload, self.info = payload, info
        self.size = (info["width"], info["height"])


def open_rgb(content):
    """-> a CodedRgb for a PNG stream `probe_rgb` supports; None for anything else (also a malformed PNG: whoever opens it
    next decodes it or raises as it always did)"""
    if content[:8] != SIGNATURE:
        return None
    try:
        info = probe_rgb(content)
    except _lib.DspnError:
        return None
    return CodedRgb(content, info) if info["supported"] else None


def decode_rgb(im, dst, raw_dst):
    """worker thread: the filtered rows of a CodedRgb into raw_dst -> True (the device finishes the image); when they do not
    inflate, Pillow's pixels (or its exception) into the (h, w, 3) array dst -> False"""
    if inflate_into(im.payload, im.info, raw_dst) == 0:
        return True
    from PIL import Image
    dst[...] = np.asarray(Image.open(io.BytesIO(im.payload)).convert("RGB"))
    return False
