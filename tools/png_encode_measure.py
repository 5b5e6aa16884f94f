"""Measurements of the device PNG encode (include/dspn_png_encode.h), written into DESIGN.md and profiles/ by hand from this
script's output.  Everything is generated from seeds; it fails without a GPU.

    python tools/png_encode_measure.py [--out FILE]

File sizes against Pillow's over the case list of tests/ref_png_encode.py and over 32 labelId maps (1024 x 2048) and 32
evaluation mosaics (2048 x 4096 x 3); encode_batch end to end against the path it replaces (`.cpu()` and `Image.save` per
image), the two alternated; the device call and the copy to the host by device events; one image's deflate on one thread.
Then encode_batch(device_deflate=True) (dspn_png_deflate_batch) against encode_batch at 8 and 16 threads, alternated the same
way; its split into filter, deflate launches, copies (device events) and host CRC-32 and chunks; its sizes against level 6
and against zlib's Z_RLE."""
import io
import os
import statistics
import sys
import time
import zlib

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_png_encode as ref  # noqa: E402
from dspnet_amd.dataset import png_encode as pe  # noqa: E402
from dspnet_amd.evaluate.multi_eval import CITYSCAPES_LABEL_IDS  # noqa: E402
from dspnet_amd.detect.render import PALETTE  # noqa: E402

log = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if log:
        log.write(line + "\n")
        log.flush()


dev = torch.device("cuda", 0)
g = np.random.Generator(np.random.PCG64(7))
B = 32


def train_id_map(h, w):
    m = np.zeros((h, w), np.uint8)
    for _ in range(400):
        y, x = int(g.integers(0, h)), int(g.integers(0, w))
        hh, ww = int(g.integers(8, h // 3)), int(g.integers(8, w // 4))
        m[y:y + hh, x:x + ww] = g.integers(0, 19)
    # ragged class borders, as an argmax of upsampled scores leaves them
    jitter = g.integers(0, 3, (h, 1))
    return np.take_along_axis(m, (np.arange(w)[None, :] + jitter) % w, 1)


def photo(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / 97.0 + c) * np.cos(yy / 61.0 - c) for c in range(3)], -1)
    return np.clip(base + g.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


lut = np.array(CITYSCAPES_LABEL_IDS, np.uint8)
pal = np.array(PALETTE, np.uint8)
H, W = 1024, 2048
bases = [train_id_map(H, W) for _ in range(4)]
ids = [np.roll(lut[bases[i % 4]], 37 * i, 1) for i in range(B)]
ph = [photo(H, W) for _ in range(2)]
mosaics = []
for i in range(B):
    a, b = bases[i % 4], bases[(i + 1) % 4]
    p = np.roll(ph[i % 2], 53 * i, 1)
    mosaics.append(np.concatenate([np.concatenate([p, pal[a]], 1), np.concatenate([p, pal[b]], 1)], 0))
say("labelId maps", ids[0].shape, "mosaics", mosaics[0].shape, "batch", B, "cpus allowed", len(os.sched_getaffinity(0)),
    "OMP_NUM_THREADS", os.environ.get("OMP_NUM_THREADS"))


def pillow_path(tensors):
    out = []
    for t in tensors:
        f = io.BytesIO()
        Image.fromarray(t.cpu().numpy()).save(f, format="PNG")
        out.append(f.getvalue())
    return out


def timed(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return r, ts


def report(name, ts):
    say("  %-44s min %8.1f ms  median %8.1f ms  (%s)" % (name, min(ts) * 1e3, statistics.median(ts) * 1e3,
                                                        " ".join("%.1f" % (t * 1e3) for t in ts)))


# ---- sizes over the case list
say("== file size, device path / Pillow, case list")
cases = ref.cases()
files = pe.encode_batch([torch.from_numpy(a).to(dev) for _, a in cases])
ratios = []
for (name, a), f in zip(cases, files):
    p = ref.pillow_file(a)
    assert ref.idat(f) == ref.idat(p), name
    ratios.append((len(f) / len(p), name, len(f), len(p)))
for r in sorted(ratios):
    say("  %.4f %-20s %8d %8d" % r)
say("  case list: min %.4f max %.4f" % (min(ratios)[0], max(ratios)[0]))

for label, arrays in (("labelId 1024x2048", ids), ("mosaic 2048x4096x3", mosaics)):
    say("== " + label)
    tensors = [torch.from_numpy(a).to(dev) for a in arrays]
    nbytes = sum(a.nbytes for a in arrays)
    # warm-up of every path at the timed shapes
    mine = pe.encode_batch(tensors)
    theirs = pillow_path(tensors)
    rr = [len(m) / len(t) for m, t in zip(mine, theirs)]
    for m, t, a in zip(mine[:3], theirs[:3], arrays[:3]):
        assert ref.idat(m) == ref.idat(t)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(m))), a)
    say("  size ratio device path / Pillow over %d files: min %.4f max %.4f; mean file %.0f bytes, raw %.0f bytes" %
        (len(rr), min(rr), max(rr), sum(map(len, mine)) / len(mine), nbytes / len(arrays)))
    # alternate the paths
    deflated = pe.encode_batch(tensors, device_deflate=True)
    t_dev8, t_dev16, t_pil, t_filter, t_dd = [], [], [], [], []
    for _ in range(3):
        _, t = timed(lambda: pe.encode_batch(tensors, device_deflate=True), 1); t_dd += t
        _, t = timed(lambda: pe.encode_batch(tensors), 1); t_dev8 += t
        _, t = timed(lambda: pillow_path(tensors), 1); t_pil += t
        _, t = timed(lambda: pe.encode_batch(tensors, threads=16), 1); t_dev16 += t
        _, t = timed(lambda: pe._filter_to_host(tensors), 1); t_filter += t
    report("encode_batch, device_deflate=True", t_dd)
    report("encode_batch, 8 threads (default)", t_dev8)
    report("encode_batch, 16 threads", t_dev16)
    report(".cpu() + Image.save per image (parent path)", t_pil)
    report("  of encode_batch: pool + filter + copy to host", t_filter)
    # the device part alone, by events
    samples = np.zeros(len(tensors), pe.SAMPLE)
    so = oo = 0
    for s, a in zip(samples, arrays):
        h, w = a.shape[:2]
        bpp = 3 if a.ndim == 3 else a.itemsize
        s["src_offset"], s["out_offset"], s["width"], s["height"], s["bytes_per_pixel"], s["src_pitch"] = so, oo, w, h, bpp, w * bpp
        so += a.nbytes
        oo += h * (1 + w * bpp)
    src = torch.cat([t.reshape(-1) for t in tensors])
    out = torch.empty(oo, dtype=torch.uint8, device=dev)
    host = torch.empty(oo, dtype=torch.uint8).pin_memory()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf, tc = [], []
    for k in range(6):
        ev[0].record()
        ws = pe.filter_into(samples, src, out)
        ev[1].record()
        host.copy_(out, non_blocking=True)
        ev[2].record()
        torch.cuda.synchronize()
        if k:
            tf.append(ev[0].elapsed_time(ev[1]) / 1e3)
            tc.append(ev[1].elapsed_time(ev[2]) / 1e3)
    report("device: table copy + filter launch (events)", tf)
    report("device -> pinned host copy (events)", tc)
    say("  filter: %.0f GB/s of pixels read once and written once; copy %.1f GB/s" % (2 * nbytes / min(tf) / 1e9, oo / min(tc) / 1e9))
    # the deflate alone on one thread, per image
    hn = host.numpy()
    t0 = time.perf_counter()
    for s, a in list(zip(samples, arrays))[:4]:
        o, n = int(s["out_offset"]), a.shape[0] * (1 + int(s["src_pitch"]))
        pe.assemble(memoryview(hn[o:o + n]), a.shape[1], a.shape[0], int(s["bytes_per_pixel"]))
    say("  deflate + chunks, one thread: %.1f ms per image" % ((time.perf_counter() - t0) / 4 * 1e3))
    # ---- the device deflate: sizes, then the split of the call
    for m, a in zip(deflated[:3], arrays[:3]):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(m))), a)
    rle = []
    for s, a in list(zip(samples, arrays))[:4]:
        o, n = int(s["out_offset"]), a.shape[0] * (1 + int(s["src_pitch"]))
        z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        rle.append(len(z.compress(memoryview(hn[o:o + n])) + z.flush()))
    r6 = [len(d) / len(m) for d, m in zip(deflated, mine)]
    idat = [len(d) - 57 for d in deflated[:4]]              # signature, IHDR, IEND and the IDAT chunk's 12 bytes
    say("  device_deflate size / level 6 over %d files: min %.4f max %.4f mean %.4f; / Z_RLE over 4 streams: %s" %
        (len(r6), min(r6), max(r6), sum(r6) / len(r6), " ".join("%.4f" % (i / r) for i, r in zip(idat, rle))))
    spans, at = [], 0
    for s, a in zip(samples, arrays):
        n = a.shape[0] * (1 + int(s["src_pitch"]))
        spans.append((at, n))
        at += n
    zout = torch.empty(sum(pe.deflate_bound(n) for _, n in spans), dtype=torch.uint8, device=dev)
    result = torch.empty(2 * len(spans), dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    tf, td, tc, th = [], [], [], []
    for k in range(6):
        ev[0].record()
        ws = pe.filter_into(samples, src, out)
        ev[1].record()
        ws2 = pe.deflate_into(spans, out, zout, result)
        ev[2].record()
        placed = result.cpu().numpy().reshape(-1, 2)
        used = int(placed[-1].sum())
        zhost = torch.empty(used, dtype=torch.uint8).pin_memory()
        zhost.copy_(zout[:used], non_blocking=True)
        ev[3].record()
        torch.cuda.synchronize()
        zn = zhost.numpy()
        t0 = time.perf_counter()
        for (o, n), a in zip(placed, arrays):
            pe.wrap(memoryview(zn[o:o + n]), a.shape[1], a.shape[0], 3 if a.ndim == 3 else a.itemsize)
        t1 = time.perf_counter()
        if k:
            tf.append(ev[0].elapsed_time(ev[1]) / 1e3)
            td.append(ev[1].elapsed_time(ev[2]) / 1e3)
            tc.append(ev[2].elapsed_time(ev[3]) / 1e3)
            th.append(t1 - t0)
    report("device_deflate: filter (events)", tf)
    report("device_deflate: table copy + 5 deflate launches", td)
    report("device_deflate: result + %d bytes to the host" % used, tc)
    report("device_deflate: CRC-32 + chunks, one thread", th)
    say("  deflate: %.1f GB/s of filtered bytes" % (oo / min(td) / 1e9))
    del tensors, src, out, host, zout
say("done")
