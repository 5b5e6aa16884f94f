"""Seeded images and Pillow's files for tests/test_jpeg_encode_host.py and tests/test_jpeg_encode_gpu.py: sizes x chroma
layouts x qualities x contents, and the coefficients of a Pillow stream cut down to the real block grids the encoder works on."""
import functools
import zlib

import numpy as np

import jpeg_cases as jc
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import jpeg_encode as je

SIZES = [(1, 1), (8, 8), (16, 16), (24, 40), (21, 37), (9, 15), (64, 200)]          # (height, width)
LAYOUTS = ["4:2:0", "4:2:2", "4:4:4", "grey"]
QUALITIES = [95, 30]
CONTENTS = ["noise", "smooth"]
CASES = [(h, w, layout, q, content) for (h, w) in SIZES for layout in LAYOUTS for q in QUALITIES for content in CONTENTS]
_PILLOW_SS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def name(case):
    return "%dx%d-%s-q%d-%s" % case


@functools.lru_cache(maxsize=None)
def pixels(case):
    """the image of a case: (h, w, 3) RGB, or (h, w) for grey (treated as read-only)"""
    h, w, layout, _, content = case
    return jc.image(zlib.crc32(name(case).encode()), h, w, content, 1 if layout == "grey" else 3)


@functools.lru_cache(maxsize=None)
def pillow_file(case):
    """what Pillow writes for the case: the yardstick"""
    layout, q = case[2], case[3]
    kw = {} if layout == "grey" else {"subsampling": _PILLOW_SS[layout]}
    return jc.encode(pixels(case), quality=q, **kw)


def sample_of(case, coef_base=0, img_offset=0):
    """-> (descriptor record, number of coefficients) of a case"""
    h, w, layout, q, _ = case
    s = np.zeros(1, je.SAMPLE)
    n = je.fill_sample(s[0], w, h, 1 if layout == "grey" else 3, je.SUBSAMPLING.get(layout, (1, 1)), je.quant_tables(q), coef_base,
                       img_offset)
    return s[0], n


@functools.lru_cache(maxsize=None)
def pillow_real_blocks(case):
    """the coefficients of Pillow's stream, read back with the decoder's host half and cut to the real grids, in the layout
    sample_of(case) describes (coef_base 0); int16, read-only"""
    data = pillow_file(case)
    rc, info = dj.probe_info(data)
    assert rc == 0 and info["supported"], name(case)
    padded = np.zeros(int(info["coef_count"]), np.int16)
    assert dj.entropy_decode(data, info, padded) == 0, name(case)
    s, n = sample_of(case)
    assert (int(info["width"]), int(info["height"]), int(info["ncomp"])) == (int(s["width"]), int(s["height"]), int(s["ncomp"]))
    out = np.zeros(n, np.int16)
    for c in range(int(s["ncomp"])):
        pw, ph = int(info["blocks_w"][c]), int(info["blocks_h"][c])
        bw, bh = int(s["blocks_w"][c]), int(s["blocks_h"][c])
        assert bw <= pw and bh <= ph
        np.testing.assert_array_equal(info["quant"][c], s["quant"][c], err_msg=name(case))
        plane = padded[int(info["coef_offset"][c]):][:64 * pw * ph].reshape(ph, pw, 64)
        o = int(s["coef_offset"][c])
        out[o:o + 64 * bw * bh] = plane[:bh, :bw].reshape(-1)
    out.setflags(write=False)
    return out
