"""The filter half of the PNG encode for the tests of dspnet_amd/dataset/png_encode.py: a plain numpy restatement of the rule
in include/dspn_png_encode.h, what Pillow writes for the same pixels, and the case list both test files share.
tests/test_png_encode_host.py pins the restatement to Pillow; the GPU tests compare the device with Pillow directly."""
import io
import zlib

import numpy as np

import ref_png

STAGE = 16384                     # kStage of dspnet_amd/csrc/png_encode.hip: longer rows take the kernel's other path
FILTERS = (0, 2, 1, 4)            # the order the candidates are tried in: None, Up, Sub, Paeth


def stream_rows(a):
    """(h, w) uint8 / uint16 or (h, w, 3) uint8 -> ((h, row_bytes) uint8 in PNG's byte order, bytes per pixel)"""
    if a.ndim == 3:
        assert a.dtype == np.uint8 and a.shape[2] == 3
        return np.ascontiguousarray(a).reshape(a.shape[0], -1), 3
    return ref_png.stream_rows(a)


def filter_image(a):
    """the filtered stream of an image as bytes: height rows of a filter type and the filtered row"""
    rows, bpp = stream_rows(a)
    h, rb = rows.shape
    out = np.zeros((h, rb + 1), np.uint8)
    zero = np.zeros(rb, np.int64)
    for y in range(h):
        x = rows[y].astype(np.int64)
        up = rows[y - 1].astype(np.int64) if y else zero
        left, ul = zero.copy(), zero.copy()
        left[bpp:], ul[bpp:] = x[:-bpp], up[:-bpp]
        pa, pb, pc = abs(up - ul), abs(left - ul), abs(left + up - 2 * ul)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        rows_by_type = {0: x, 2: (x - up) & 255, 1: (x - left) & 255, 4: (x - paeth) & 255}
        best = None
        for ft in FILTERS:
            v = rows_by_type[ft]
            score = int(np.where(v < 128, v, 256 - v).sum())
            if best is None or score < best:
                best, out[y, 0], out[y, 1:] = score, ft, v
    return out.tobytes()


def pillow_file(a):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(a).save(f, format="PNG")
    return f.getvalue()


def idat(payload):
    """the inflated IDAT data of a file"""
    return zlib.decompress(b"".join(d for k, d in ref_png.chunks(payload) if k == b"IDAT"))


def pillow_filtered(a):
    return idat(pillow_file(a))


def filter_types(filtered, a):
    rows, _ = stream_rows(a)
    return np.frombuffer(filtered, np.uint8).reshape(rows.shape[0], rows.shape[1] + 1)[:, 0].tolist()


def _shape(h, w, bpp):
    return (h, w, 3) if bpp == 3 else (h, w)


def noise(g, h, w, bpp):
    return g.integers(0, 65536 if bpp == 2 else 256, _shape(h, w, bpp), dtype=np.uint16 if bpp == 2 else np.uint8)


def mixed(g, h, w, bpp):
    """noise, then the same row again (Up scores 0), a ramp along the row (Sub), the ramp moved on by one pixel and one
    level (Paeth), and so on: every filter has a row to win"""
    a = noise(g, h, w, bpp).astype(np.int64)
    step = 257 if bpp == 2 else 3
    ramp = (np.arange(w) * step)[:, None] + np.arange(3)[None, :] * 40 if bpp == 3 else np.arange(w) * step
    for y in range(h):
        if y % 4 == 1:
            a[y] = a[y - 1]
        elif y % 4 == 2:
            a[y] = ramp + 11 * y
        elif y % 4 == 3:
            a[y] = np.roll(a[y - 1], 1, axis=0) + step
    return (a % (65536 if bpp == 2 else 256)).astype(np.uint16 if bpp == 2 else np.uint8)


def cases():
    """[(name, array)]: the smallest shapes at which the filter kernel can go wrong"""
    g = np.random.Generator(np.random.PCG64(2024))
    out = []
    for bpp in (1, 2, 3):
        tag = {1: "L", 2: "I16", 3: "RGB"}[bpp]
        out.append(("1x1_" + tag, noise(g, 1, 1, bpp)))
        out.append(("h1_w300_" + tag, np.ascontiguousarray(mixed(g, 3, 300, bpp)[2:])))                 # only None and Sub can be taken
        out.append(("w1_h40_" + tag, noise(g, 40, 1, bpp)))                       # left is always 0
        # rows of 63, 64, 65, 255, 256, 257 bytes, or the nearest the format has: wave, chunk and alignment edges
        for w in {1: (63, 64, 65, 255, 256, 257), 2: (31, 32, 33, 127, 128, 129), 3: (21, 22, 23, 85, 86, 87)}[bpp]:
            out.append(("rb%d_%s" % (w * bpp, tag), mixed(g, 6, w, bpp)))
        out.append(("zeros_" + tag, np.zeros(_shape(5, 37, bpp), noise(g, 1, 1, bpp).dtype)))      # every row stays None
        out.append(("noise_" + tag, noise(g, 9, 50, bpp)))                         # None wins rows
    out.append(("const128_L", np.full((4, 33), 128, np.uint8)))                    # 256 - 128 = 128: the edge of the score
    out.append(("const128_RGB", np.full((4, 11, 3), 128, np.uint8)))
    out.append(("const_0x8080_I16", np.full((4, 17), 0x8080, np.uint16)))
    out.append(("repeated_rows_L", np.tile(noise(g, 1, 77, 1), (5, 1))))           # Up scores 0
    out.append(("hramp_L", ((np.arange(90) * 2 + 5)[None, :] + np.arange(4)[:, None] * 50).astype(np.uint8)))     # Sub
    yy, xx = np.mgrid[0:12, 0:70]
    out.append(("dramp_L", ((xx * 5 + yy * 9) % 256).astype(np.uint8)))            # Paeth
    out.append(("dramp_RGB", np.stack([(xx * 5 + yy * 9) % 256, (xx * 3 + yy * 7 + 40) % 256, (xx * 7 + yy * 2) % 256], -1).astype(np.uint8)))
    # Up, Sub and Paeth all score 40 on the second row, None 100: Up, the first of them, is taken
    out.append(("tie_up_sub_L", np.array([[0, 10, 20, 30], [10, 20, 30, 40]], np.uint8)))
    # Sub scores 40 on the second row, Up and None 100, Paeth 40 as well: it does not replace Sub
    out.append(("tie_sub_paeth_L", np.array([[0, 0, 0, 0], [10, 20, 30, 40]], np.uint8)))
    out.append(("arange_I16", (np.arange(6 * 45, dtype=np.int64) * 257 + 3).astype(np.uint16).reshape(6, 45)))     # high != low byte
    out.append(("noise_I16_odd", noise(g, 7, 31, 2)))
    out.append(("mosaic_row_RGB", mixed(g, 8, 4096, 3)))                           # a caller's real row: 2 * 2048 * 3 bytes
    out.append(("stage_exact_L", mixed(g, 3, STAGE, 1)))                           # the last length the kernel stages
    out.append(("past_stage_L", mixed(g, 3, STAGE + 1, 1)))                        # ... and rows it reads from global memory
    out.append(("past_stage_I16", mixed(g, 3, STAGE // 2 + 9, 2)))
    out.append(("past_stage_RGB", mixed(g, 5, STAGE // 3 + 40, 3)))
    return out


# the filter types the two hand-built cases must give on their second row
TIE_TYPES = {"tie_up_sub_L": 2, "tie_sub_paeth_L": 1}
