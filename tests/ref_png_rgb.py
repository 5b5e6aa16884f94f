"""Colour PNG streams for the tests of the RGB path of dspnet_amd/dataset/png.py: a writer for every (colour type, bit
depth) pair that is told the filter type of every row, the PLTE length and whether a tRNS chunk goes in, and a plain numpy
reading of what Pillow's convert("RGB") makes of such a stream (tests/ref_png.py's `unfilter` at the format's row length
and stride, then the sample-to-RGB table of include/dspn_png.h).  tests/test_png_rgb_host.py pins the reading to Pillow."""
import io
import struct
import zlib

import numpy as np

import ref_png as rp

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# every legal pair; 16-bit greyscale is the one the RGB path leaves out
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]


def geometry(width, colour, depth):
    """-> (row_bytes, filter stride)"""
    bits = CHANNELS[colour] * depth
    return (width * bits + 7) // 8, max(1, bits // 8)


def pack_rows(samples, depth):
    """(h, w, channels) sample values below 2 ** depth -> (h, row_bytes) uint8 in stream order: 16-bit samples high byte
    first, 1-, 2- and 4-bit samples packed from the most significant bits, every row starting on a byte"""
    h, w, ch = samples.shape
    if depth == 16:
        return samples.astype(">u2").view(np.uint8).reshape(h, w * ch * 2)
    if depth == 8:
        return samples.astype(np.uint8).reshape(h, w * ch)
    assert ch == 1
    per = 8 // depth
    padded = np.zeros((h, -(-w // per) * per), np.uint8)
    padded[:, :w] = samples[:, :, 0]
    shifts = (8 - depth * (1 + np.arange(per))).astype(np.uint8)
    return (padded.reshape(h, -1, per) << shifts).sum(axis=2).astype(np.uint8)


def default_palette(entries):
    return bytes((i * 37 + k * 91 + 5) & 255 for i in range(entries) for k in range(3))


def write(samples, colour, depth, filters, plte_entries=None, trns=False, **kw):
    """samples: (h, w, channels) integers below 2 ** depth; filters: one type per row; plte_entries: length of the PLTE chunk
    of a palette stream (default 2 ** depth); trns: put a tRNS chunk in front of IDAT"""
    h, w, ch = samples.shape
    assert ch == CHANNELS[colour] and len(filters) == h
    rows = pack_rows(samples, depth)
    rb, bpp = geometry(w, colour, depth)
    assert rows.shape == (h, rb)
    before = []
    if trns:
        body = {0: struct.pack(">H", 1), 2: struct.pack(">HHH", 1, 2, 3), 3: b"\x80"}.get(colour)
        if body is not None:                                    # the specification allows none with an alpha channel
            before.append(rp.chunk(b"tRNS", body))
    palette = default_palette(2 ** depth if plte_entries is None else plte_entries) if colour == 3 else None
    return rp.assemble(w, h, depth, colour, rp.filter_rows(rows, filters, bpp), palette=palette, before_idat=before, **kw)


def random_samples(g, h, w, colour, depth, values=None):
    """uniformly random samples, or a draw from `values` (constant and two-valued images make Paeth ties)"""
    ch = CHANNELS[colour]
    if values is not None:
        return np.asarray(values)[g.integers(0, len(values), (h, w, ch))]
    return g.integers(0, 2 ** depth, (h, w, ch))


def to_rgb(rows, width, colour, depth, palette=None):
    """(h, row_bytes) reconstructed stream bytes -> (h, width, 3) uint8, the table of include/dspn_png.h"""
    h = rows.shape[0]
    if depth >= 8:
        px, sb = CHANNELS[colour] * depth // 8, depth // 8
        first = rows.reshape(h, width, px)[:, :, ::sb]          # the high byte of every sample
        v = first[:, :, 0]
        if colour in (2, 6):
            return np.ascontiguousarray(first[:, :, :3])
    else:
        bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(h, width, depth)
        v = (bits << np.arange(depth - 1, -1, -1)).sum(axis=2)
        if colour == 0:
            v = v * {1: 255, 2: 85, 4: 17}[depth]
    if colour == 3:
        table = np.zeros((256, 3), np.uint8)
        table[:len(palette) // 3] = np.frombuffer(palette, np.uint8).reshape(-1, 3)
        return table[v]
    return np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2)


def header(payload):
    """-> (width, height, depth, colour, palette bytes or None, inflated IDAT data)"""
    parts = list(rp.chunks(payload))
    w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", parts[0][1])
    assert not interlace
    palette = next((d for k, d in parts if k == b"PLTE"), None)
    return w, h, depth, colour, palette, zlib.decompress(b"".join(d for k, d in parts if k == b"IDAT"))


def decode(payload):
    """a non-interlaced stream of any pair but 16-bit greyscale -> (h, w, 3) uint8, by `rp.unfilter` and `to_rgb`"""
    w, h, depth, colour, palette, raw = header(payload)
    rb, bpp = geometry(w, colour, depth)
    return to_rgb(rp.unfilter(raw, h, rb, bpp), w, colour, depth, palette)


def pillow(payload):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(payload)).convert("RGB"))
