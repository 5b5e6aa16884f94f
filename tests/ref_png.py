"""PNG streams for the tests of dspnet_amd/dataset/png.py: a writer that is told the filter type of every row (Pillow's
encoder chooses its own), and a plain numpy reading of the PNG specification's reconstruction.  tests/test_png_host.py pins
the reading to Pillow; the GPU tests compare the device with Pillow directly."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy


def chunk(kind, data=b""):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(rows, filters, bpp):
    """(h, row_bytes) uint8 stream-order bytes -> the filtered rows, each with its type byte in front, as bytes"""
    h, rb = rows.shape
    out = np.zeros((h, rb + 1), np.uint8)
    zero = np.zeros(rb, np.int64)
    for y in range(h):
        ft = int(filters[y])
        cur = rows[y].astype(np.int64)
        up = rows[y - 1].astype(np.int64) if y else zero
        a = np.concatenate([zero[:bpp], cur[:-bpp]]) if rb > bpp else zero[:rb]
        c = np.concatenate([zero[:bpp], up[:-bpp]]) if rb > bpp else zero[:rb]
        if ft == 0:
            pred = zero
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        else:
            pa, pb, pc = abs(up - c), abs(a - c), abs(a + up - 2 * c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def stream_rows(arr):
    """(h, w) uint8 or uint16 samples -> ((h, row_bytes) uint8 in PNG's byte order, bytes per pixel)"""
    if arr.dtype == np.uint16:
        return arr.astype(">u2").view(np.uint8).reshape(arr.shape[0], -1), 2
    assert arr.dtype == np.uint8
    return np.ascontiguousarray(arr), 1


def assemble(width, height, depth, colour, raw, idat_chunks=3, interlace=0, palette=None, before_idat=(), level=6, compressed=None):
    """a PNG file around the filtered bytes `raw` (or around `compressed`, an already deflated IDAT stream)"""
    z = zlib.compress(raw, level) if compressed is None else compressed
    n = max(1, min(idat_chunks, len(z)))
    cuts = [len(z) * k // n for k in range(n + 1)]
    parts = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, interlace))]
    if colour == 3:
        pal = palette if palette is not None else bytes((i * 7 + k * 50) & 255 for i in range(256) for k in range(3))
        parts.append(chunk(b"PLTE", pal))
    parts += list(before_idat)
    parts += [chunk(b"IDAT", z[cuts[k]:cuts[k + 1]]) for k in range(n)]
    parts.append(chunk(b"IEND"))
    return b"".join(parts)


def write(arr, filters, palette=False, **kw):
    """arr: (h, w) uint8 (greyscale, or palette indices with palette=True) or uint16 (greyscale); filters: one type per row"""
    rows, bpp = stream_rows(arr)
    assert len(filters) == arr.shape[0] and not (palette and bpp == 2)
    return assemble(arr.shape[1], arr.shape[0], 8 * bpp, 3 if palette else 0, filter_rows(rows, filters, bpp), **kw)


def write_interlaced(arr, **kw):
    """Adam7, every row of every pass with filter type 0"""
    rows, bpp = stream_rows(arr)
    raw = b""
    for x0, y0, dx, dy in ADAM7:
        sub = rows.reshape(arr.shape[0], arr.shape[1], bpp)[y0::dy, x0::dx]
        if sub.size:
            sub = sub.reshape(sub.shape[0], -1)
            raw += filter_rows(sub, [0] * sub.shape[0], bpp)
    return assemble(arr.shape[1], arr.shape[0], 8 * bpp, 0, raw, interlace=1, **kw)


def write_rgb(arr, filters, **kw):
    """(h, w, 3) uint8"""
    rows = np.ascontiguousarray(arr).reshape(arr.shape[0], -1)
    return assemble(arr.shape[1], arr.shape[0], 8, 2, filter_rows(rows, filters, 3), **kw)


def unfilter(raw, height, row_bytes, bpp):
    """the specification's reconstruction of `height` rows of 1 + row_bytes bytes -> (height, row_bytes) uint8"""
    raw = np.frombuffer(raw, np.uint8).reshape(height, row_bytes + 1)
    out = np.zeros((height, row_bytes), np.uint8)
    up = [0] * row_bytes
    for y in range(height):
        ft, x = int(raw[y, 0]), raw[y, 1:].tolist()
        cur = [0] * row_bytes
        for i in range(row_bytes):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            b = up[i]
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[ft]
            cur[i] = (x[i] + pred) & 255
        out[y] = cur
        up = cur
    return out


def chunks(payload):
    at = 8
    while at < len(payload):
        n, kind = struct.unpack_from(">I4s", payload, at)
        yield kind, payload[at + 8:at + 8 + n]
        at += 12 + n


def decode(payload):
    """a non-interlaced greyscale or palette stream of 8 or 16 bits -> (h, w) uint8 / uint16, by `unfilter`"""
    parts = list(chunks(payload))
    w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", parts[0][1])
    assert colour in (0, 3) and depth in (8, 16) and not interlace
    bpp = depth // 8
    raw = zlib.decompress(b"".join(d for k, d in parts if k == b"IDAT"))
    rows = unfilter(raw, h, w * bpp, bpp)
    return rows.view(">u2").astype(np.uint16) if bpp == 2 else rows


def pillow(payload):
    """Pillow's samples as they come: uint8 for modes L and P (the indices), uint16 for 16-bit greyscale"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(payload)))


def random_image(g, h, w, bpp):
    """uniformly random bytes: wrap-around, the 9-bit average and Paeth ties all occur"""
    return g.integers(0, 256, (h, w), dtype=np.uint8) if bpp == 1 else g.integers(0, 65536, (h, w), dtype=np.uint16)


def filters_for(g, h, kind):
    """kind 0..4: every row that type; "mix": random types"""
    return [kind] * h if kind != "mix" else g.integers(0, 5, h).tolist()
