"""Seeded JPEG streams for tests/test_jpeg_host.py and tests/test_jpeg_gpu.py, all made with Pillow in the test run:
the matrix of sizes x subsampling x quality x optimised tables x content, the restart-interval streams, greyscale."""
import functools
import io
import zlib

import numpy as np
from PIL import Image

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (37, 53), (50, 31), (64, 200)]         # (height, width)


def image(seed, h, w, content, channels=3):
    """`smooth`: ramps with a different slope per channel; `noise`: uniform bytes (at quality 100 it drives the clamps)"""
    g = np.random.Generator(np.random.PCG64(seed))
    if content == "noise":
        a = g.integers(0, 256, (h, w, channels))
    else:
        yy, xx = np.mgrid[:h, :w]
        a = np.stack([(xx * g.uniform(1, 6) + yy * g.uniform(1, 6) + g.uniform(0, 255)) % 256 for _ in range(channels)], -1)
        a = np.abs(a - 128) * 2                                  # triangle wave: smooth, full range
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a if channels == 3 else a[:, :, 0]


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _cases():
    out = []
    for (h, w) in SIZES:
        for ss in (0, 1, 2):
            for q in (30, 90, 100):
                for opt in (False, True):
                    for content in ("smooth", "noise"):
                        out.append(("%dx%d-ss%d-q%d-%s-%s" % (h, w, ss, q, "opt" if opt else "std", content), (h, w), 3, content,
                                    dict(subsampling=ss, quality=q, optimize=opt)))
        for k, content in enumerate(("smooth", "noise")):
            for q in (30, 90, 100):
                out.append(("%dx%d-grey-q%d-%s" % (h, w, q, content), (h, w), 1, content, dict(quality=q, optimize=bool((k + q) % 2))))
    for ss in (0, 1, 2):
        for (h, w) in ((37, 53), (64, 200)):
            out.append(("%dx%d-ss%d-rstblocks3" % (h, w, ss), (h, w), 3, "noise", dict(subsampling=ss, quality=90, restart_marker_blocks=3)))
            out.append(("%dx%d-ss%d-rstrows1" % (h, w, ss), (h, w), 3, "smooth", dict(subsampling=ss, quality=90, restart_marker_rows=1)))
    out.append(("16x16-ss2-rstblocks1", (16, 16), 3, "noise", dict(subsampling=2, quality=90, restart_marker_blocks=1)))
    out.append(("50x31-grey-rstblocks3", (50, 31), 1, "noise", dict(quality=90, restart_marker_blocks=3)))
    out.append(("64x200-grey-rstrows1", (64, 200), 1, "smooth", dict(quality=100, restart_marker_rows=1, optimize=True)))
    return out


CASES = _cases()
GROUPS = ["%dx%d-" % s for s in SIZES]


def group(prefix):
    return [c[0] for c in CASES if c[0].startswith(prefix)]


_BY_NAME = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def stream(name):
    _, (h, w), ch, content, kw = _BY_NAME[name]
    return encode(image(zlib.crc32(name.encode()), h, w, content, ch), **kw)


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
