"""Measurements of the device PNG decode (include/dspn_png.h), written to profiles/png_device_decode.txt by hand from this
script's output.  Everything is generated from seeds.

    python tools/png_measure.py host                       # 1: probe + inflate against Pillow's full decode, per image
    python tools/png_measure.py device                     # 2: unfilter of B = 32 at 1024 x 2048, device events
    python tools/png_measure.py iterator --workdir DIR     # 3: MultiTaskRecordIter batches/s, device_jpeg alone and with device_png

`host` needs no GPU; `device` and `iterator` fail without one.  The record file of `iterator` is the one of
tools/jpeg_measure.py (profiles/jpeg_device_decode.txt, section 3), so the first setting repeats that section's best one."""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W = 1024, 2048


def label_map(seed):
    """a street scene's statistics at the size that matters here: a few dozen filled polygons of class ids over a background"""
    from PIL import Image, ImageDraw
    g = np.random.Generator(np.random.PCG64(seed))
    im = Image.new("L", (W, H), 255)
    draw = ImageDraw.Draw(im)
    for _ in range(60):
        cx, cy, r = g.uniform(0, W), g.uniform(0, H), g.uniform(30, 500)
        k = int(g.integers(3, 9))
        ang = np.sort(g.uniform(0, 2 * np.pi, k))
        rad = g.uniform(.4, 1, k) * r
        draw.polygon([(float(cx + a * np.cos(t)), float(cy + a * np.sin(t))) for a, t in zip(rad, ang)], fill=int(g.integers(0, 19)))
    return np.asarray(im)


def png_bytes(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def paeth_rows(arr):
    """the inflated form of `arr` with every row filtered by type 4 (the worst case for the kernel's arithmetic)"""
    cur = arr.astype(np.int64)
    a = np.zeros_like(cur); a[:, 1:] = cur[:, :-1]
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, 1:] = cur[:-1, :-1]
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    raw = np.empty((arr.shape[0], arr.shape[1] + 1), np.uint8)
    raw[:, 0] = 4
    raw[:, 1:] = (cur - pred) & 255
    return raw.reshape(-1)


def host(args):
    from dspnet_amd.dataset import png as dp
    n = args.images
    streams = [png_bytes(label_map(1000 + i)) for i in range(n)]
    infos = [dp.probe(s) for s in streams]
    bufs = [np.empty(infos[0]["raw_bytes"], np.uint8) for _ in range(16)]
    hist = np.zeros(5, np.int64)
    for s, info in zip(streams, infos):
        assert dp.inflate_into(s, info, bufs[0]) == 0
        hist += np.bincount(bufs[0][0::W + 1], minlength=5)

    def inflate(k):
        assert dp.inflate_into(streams[k], dp.probe(streams[k]), bufs[k % 16]) == 0

    def pillow(k):
        pillow_decode(streams[k])

    print("%d label maps of %d x %d, 8-bit greyscale, written by Pillow: mean %.1f KB; filter types over all rows: "
          "None %d, Sub %d, Up %d, Average %d, Paeth %d" % ((n, H, W, np.mean([len(s) for s in streams]) / 1e3) + tuple(hist)))
    for k in range(2):
        inflate(k); pillow(k)
    t = {"pillow": [], "inflate": []}
    for k in range(n):                                          # single thread, alternated per image
        for name, fn in (("pillow", pillow), ("inflate", inflate)):
            t0 = time.perf_counter(); fn(k); t[name].append(time.perf_counter() - t0)
    p, e = np.median(t["pillow"]) * 1e3, np.median(t["inflate"]) * 1e3
    print("   1 thread : Pillow full decode %.2f ms/image, probe + inflate_into %.2f ms/image (median of %d), ratio %.2f, "
          "difference %.2f ms" % (p, e, n, p / e, p - e))
    for threads in (8, 16):
        with ThreadPoolExecutor(threads) as pool:
            wall = {"pillow": [], "inflate": []}
            for rep in range(3):                                # alternated per pass over the set
                for name, fn in (("pillow", pillow), ("inflate", inflate)):
                    t0 = time.perf_counter(); list(pool.map(fn, range(n))); wall[name].append(time.perf_counter() - t0)
        p, e = min(wall["pillow"]), min(wall["inflate"])
        print("  %2d threads: Pillow %.0f images/s, probe + inflate_into %.0f images/s (best of 3 passes over %d images, %d CPUs "
              "visible), ratio %.2f; host time a batch of 32 sheds: %.2f ms" % (threads, n / p, n / e, n, os.cpu_count(), p / e,
                                                                                32 * (p - e) / n * 1e3))


def device(args):
    import ctypes as c
    import torch
    from dspnet_amd import _lib
    from dspnet_amd.dataset import iterator as it
    from dspnet_amd.dataset import png as dp
    dev = torch.device("cuda", 0)
    B = 32
    maps = [label_map(2000 + i) for i in range(8)]
    streams = [png_bytes(m) for m in maps]
    infos = [dp.probe(s) for s in streams]
    per = infos[0]["raw_bytes"]
    raws = {"Pillow-chosen filters": np.empty(B * per, np.uint8), "every row Paeth": np.empty(B * per, np.uint8)}
    samples, warp = np.zeros(B, dp.SAMPLE), np.zeros(B, it._SAMPLE)
    paeth = [paeth_rows(m) for m in maps]
    for b in range(B):
        assert dp.inflate_into(streams[b % 8], infos[b % 8], raws["Pillow-chosen filters"][b * per:(b + 1) * per]) == 0
        raws["every row Paeth"][b * per:(b + 1) * per] = paeth[b % 8]
        dp.fill_sample(samples[b], infos[b % 8], b * per, b * H * W)
        warp[b] = (b * H * W * 3, b * H * W, H, W, 0, 0, 0, 0, it.invert_affine([.5, 0, 0, 0, .5, 0]))
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    wdesc = torch.from_numpy(warp.view(np.uint8).reshape(-1).copy()).to(dev)
    seg = torch.empty(B * H * W, dtype=torch.uint8, device=dev)
    img = torch.zeros(B * H * W * 3, dtype=torch.uint8, device=dev)
    data = torch.empty(B, 3, H // 2, W // 2, device=dev)
    seg_out = torch.empty(B, H // 8, W // 8, device=dev)
    lut = torch.from_numpy(it.seg_lut()).to(dev)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    mean = (c.c_double * 3)(123.68, 116.779, 103.939)

    def augment():
        _lib.check(it._entry()(img.data_ptr(), seg.data_ptr(), wdesc.data_ptr(), B, H // 2, W // 2, it._CMAP_RGB, mean, lut.data_ptr(),
                               data.data_ptr(), seg_out.data_ptr(), st))

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for k in range(reps):
            fn(); ev[k + 1].record()
        torch.cuda.synchronize(dev)
        ts = [ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]
        return np.median(ts), min(ts), max(ts)

    print("dspn_png_unfilter_batch, B = %d at %d x %d, one byte per sample; device events around each call after 3 warm-up "
          "calls, 20 calls" % (B, H, W))
    for name, raw in raws.items():
        rdev = torch.from_numpy(raw).to(dev)

        def unfilter():
            _lib.check(lib.dspn_png_unfilter_batch(rdev.data_ptr(), rdev.numel(), desc.data_ptr(), B, seg.data_ptr(), seg.numel(), st))

        seg.fill_(0xA5)
        unfilter()
        torch.cuda.synchronize(dev)
        got = seg.view(B, H, W).cpu().numpy()
        assert all((got[b] == maps[b % 8]).all() for b in range(B)), "samples differ from the source label maps"
        med, lo, hi = timed(unfilter)
        print("  %-22s: %.3f ms per call (median; min %.3f, max %.3f), %.1f us per image; samples equal the source maps" %
              (name, med, lo, hi, med * 1e3 / B))
    med, lo, hi = timed(augment)
    print("dspn_augment_batch_u8 of the same batch (images and label maps) to (%d, 3, %d, %d) / (%d, %d, %d): %.3f ms per call "
          "(median; min %.3f, max %.3f)" % (B, H // 2, W // 2, B, H // 8, W // 8, med, lo, hi))


def iterator(args):
    import torch
    from jpeg_measure import _write_records
    from dspnet_amd.dataset import iterator as it
    dev = torch.device("cuda", 0)
    B, n = 32, args.records
    path = _write_records(args.workdir, n)
    print("MultiTaskRecordIter, B = %d, data shape (3, 512, 1024), %d records of %d x %d JPEG (quality 92, 4:2:0) + label PNG, "
          "%d timed batches after the constructor's warm-up batch, window closed by a device synchronise" % (B, n, H, W, args.batches))
    for threads in (8, 16):
        rates, fb = {False: [], True: []}, []
        for rep in range(2):
            for png_on in (False, True):                        # alternated
                itr = it.MultiTaskRecordIter(path, B, (3, 512, 1024), device=dev, decode_threads=threads, device_jpeg=True,
                                             device_png=png_on)
                torch.cuda.synchronize(dev)
                done, t0 = 0, time.perf_counter()
                while done < args.batches:
                    if not itr.iter_next():
                        itr.reset()
                    itr.next()
                    done += 1
                torch.cuda.synchronize(dev)
                rates[png_on].append(done / (time.perf_counter() - t0))
                fb.append((itr.jpeg_fallbacks, itr.png_fallbacks))
                itr._drop_ahead()
                del itr
        off, on = np.mean(rates[False]), np.mean(rates[True])
        print("  decode_threads %2d: device_jpeg alone %.2f batches/s (%.0f images/s; runs %s), with device_png %.2f batches/s "
              "(%.0f images/s; runs %s), ratio %.2f, (jpeg, png) fallbacks per run %s" %
              (threads, off, off * B, ["%.2f" % r for r in rates[False]], on, on * B, ["%.2f" % r for r in rates[True]], on / off, fb))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "device", "iterator"])
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--records", type=int, default=128)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if a.what == "iterator" and not a.workdir:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix="png_measure_")
    {"host": host, "device": device, "iterator": iterator}[a.what](a)
