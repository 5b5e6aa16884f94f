"""Seeded JPEG streams for tests/test_jpeg_host.py and tests/test_jpeg_gpu.py, all made with Pillow in the test run:
the matrix of sizes x subsampling x quality x optimised tables x content, the restart-interval streams, greyscale.
Below them the streams of tests/test_pipeline_edges_gpu.py (EDGE_CASES) and the low-level harness of the device half."""
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


# ------------------------------------------------------------------------------------------------------------------
# Streams of tests/test_pipeline_edges_gpu.py: rows wider than the pixels one workgroup covers per unit, the largest
# sides, and the eight small streams a 1024-descriptor call repeats.  CASES above stays as it is (its tests deal it in
# thirds and assert its size).
EDGE_LAYOUTS = [("ss0", 3, dict(subsampling=0)), ("ss1", 3, dict(subsampling=1)), ("ss2", 3, dict(subsampling=2)), ("grey", 1, {})]
CHUNK_WIDTHS = [1021, 1024, 1025, 1027, 1028, 2047, 2049, 3073]
CHUNK_HEIGHTS = [1, 2, 3, 17]
MAX_SIDE = 65500                                               # libjpeg's JPEG_MAX_DIMENSION: Pillow neither writes nor reads more
BATCH_SHAPES = [((56, 72), "ss0"), ((40, 88), "ss1"), ((48, 80), "ss2"), ((72, 56), "grey"), ((33, 95), "ss0"), ((71, 49), "ss2"),
                ((64, 64), "ss1"), ((47, 91), "grey")]


def _edge_cases():
    layouts = {l[0]: l for l in EDGE_LAYOUTS}
    chunk, extent, batch = [], [], []
    for k, (lname, ch, kw) in enumerate(EDGE_LAYOUTS):
        for i, w in enumerate(CHUNK_WIDTHS):                    # every layout meets every width; the heights are dealt round
            h = CHUNK_HEIGHTS[(i + k) % len(CHUNK_HEIGHTS)]
            chunk.append(("chunk-%dx%d-%s" % (h, w, lname), (h, w), ch, "noise", dict(quality=90, **kw)))
    for (h, w) in ((1, MAX_SIDE), (MAX_SIDE, 1)):
        for lname in ("ss2", "grey"):
            _, ch, kw = layouts[lname]
            extent.append(("extent-%dx%d-%s" % (h, w, lname), (h, w), ch, "noise", dict(quality=90, **kw)))
    for (h, w), lname in BATCH_SHAPES:
        _, ch, kw = layouts[lname]
        batch.append(("batch-%dx%d-%s" % (h, w, lname), (h, w), ch, "noise", dict(quality=90, **kw)))
    # chroma planes of one, two and three columns: libjpeg-turbo upsamples the first two by repetition (found by the
    # 65 500 x 1 extent above; CASES has no subsampled image under 8 pixels wide other than 1 x 1)
    narrow = [("narrow-%dx%d-%s" % (h, w, lname), (h, w), 3, "noise", dict(quality=90, **layouts[lname][2]))
              for lname in ("ss1", "ss2") for w in (1, 2, 3, 4, 5, 6) for h in (1, 5, 18)]
    return chunk, extent, batch, narrow


_CHUNK, _EXTENT, _BATCH, _NARROW = _edge_cases()
EDGE_CASES = _CHUNK + _EXTENT + _BATCH + _NARROW
CHUNK_NAMES, EXTENT_NAMES, BATCH_NAMES, NARROW_NAMES = ([c[0] for c in part] for part in (_CHUNK, _EXTENT, _BATCH, _NARROW))
_EDGE_BY_NAME = {c[0]: c for c in EDGE_CASES}


def edge_size(name):
    """(height, width) of an edge case"""
    return _EDGE_BY_NAME[name][1]


@functools.lru_cache(maxsize=None)
def edge_stream(name):
    _, (h, w), ch, content, kw = _EDGE_BY_NAME[name]
    return encode(image(zlib.crc32(name.encode()), h, w, content, ch), **kw)


@functools.lru_cache(maxsize=None)
def edge_pillow_pixels(name):
    """Pillow's pixels of an edge stream, computed once (read-only)"""
    a = pillow_pixels(edge_stream(name))
    a.setflags(write=False)
    return a


def kernel_constants(source, names):
    """`constexpr int NAME = <integer or product/quotient of earlier names and integers>;` read from the text of
    dspnet_amd/csrc/<source> -> {name: value}"""
    import os
    import re
    import dspnet_amd
    text = open(os.path.join(os.path.dirname(dspnet_amd.__file__), "csrc", source)).read()
    found = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([\w */]+);", text):
        assert re.fullmatch(r"\w+( [*/] \w+)*", expr), "%s: cannot read `%s = %s`: update this reader" % (source, name, expr)
        toks = expr.split()
        val = lambda t: int(t) if t.isdigit() else found[t]  # noqa: E731
        v = val(toks[0])
        for op, t in zip(toks[1::2], toks[2::2]):
            v = v * val(t) if op == "*" else v // val(t)
        found[name] = v
    missing = [n for n in names if n not in found]
    assert not missing, "%s: %s not found: update this reader" % (source, missing)
    return {n: found[n] for n in names}


@functools.lru_cache(maxsize=None)
def _coded(payload):
    """host half of one stream: (probed info, coefficients), computed once per distinct stream (read-only)"""
    from dspnet_amd.dataset import jpeg as dj
    rc, info = dj.probe_info(payload)
    assert rc == 0 and info["supported"]
    c = np.zeros(int(info["coef_count"]), np.int16)
    assert dj.entropy_decode(payload, info, c) == 0
    c.setflags(write=False)
    return info, c


def describe_batch(coded, skip, guard=64):
    """descriptors of one dspn_jpeg_reconstruct_batch_u8 call over `coded` (a list of (info, coefficients)) with `guard`
    bytes in front of and behind every sample's output -> (samples, regions as (offset, bytes), bytes of the output pool)"""
    from dspnet_amd.dataset import jpeg as dj
    samples = np.zeros(len(coded), dj.SAMPLE)
    co, io_, regions = 0, 0, []
    for k, (info, c) in enumerate(coded):
        io_ += guard
        dj.fill_sample(samples[k], info, co, io_)
        samples[k]["skip"] = int(k in skip)
        n = int(info["width"]) * int(info["height"]) * 3
        regions.append((io_, n))
        co += c.size
        io_ += n + guard
    return samples, regions, io_


def launch_guarded(coded, skip, dev, guard=64, spoil=None):
    """one dspn_jpeg_reconstruct_batch_u8 call with `guard` bytes of 0xA5 around every sample's output -> (pool, regions)"""
    import torch
    from dspnet_amd.dataset import jpeg as dj
    samples, regions, size = describe_batch(coded, skip, guard)
    if spoil:
        spoil(samples)
    pool = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
    cdev = torch.from_numpy(np.concatenate([c for _, c in coded])).to(dev)
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    dj.reconstruct(cdev, desc, pool)
    torch.cuda.synchronize(dev)
    return pool.cpu().numpy(), regions


def low_level_batch(payloads, skip, dev, guard=64, spoil=None):
    """launch_guarded over streams: the host half runs once per distinct stream"""
    return launch_guarded([_coded(p) for p in payloads], skip, dev, guard, spoil)
