"""Measurements of the colour PNG decode (dspn_png_rgb_batch, include/dspn_png.h), written to
profiles/png_rgb_device_decode.txt by hand from this script's output.  Everything is generated from seeds.

    python tools/png_rgb_measure.py device [--only rgba16] [--reps 20]   # 1: B = 16 at 2048 x 1024 per format, device events
    python tools/png_rgb_measure.py im2rec                               # 2: im2rec._decode + encode_batch, new against parent

Both fail without a GPU.  `device --only F` under a kernel trace gives the two launches' times apart."""
import argparse
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, B = 1024, 2048, 16
FORMATS = {"rgb8": (2, 8), "rgba8": (6, 8), "rgb16": (2, 16), "rgba16": (6, 16)}


def scene(seed, channels=3):
    """natural-image statistics at the size that matters here: smooth structure at several scales, edges, sensor noise"""
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    out = []
    for _ in range(channels):
        v = 120 + 60 * np.sin(xx / g.uniform(40, 200) + g.uniform(0, 6)) * np.cos(yy / g.uniform(40, 200))
        v += 25 * np.sin(xx / g.uniform(4, 12)) * np.sin(yy / g.uniform(4, 12))
        v += 30 * ((xx * g.uniform(.2, 1) + yy) % g.uniform(150, 400) < 60)
        out.append(v + g.normal(0, 2.5, (H, W)))
    return np.clip(np.stack(out, -1), 0, 255).astype(np.uint8)


def filtered(rows, filters, bpp):
    """(h, row_bytes) stream bytes -> the inflated form, row y filtered by type filters[y]"""
    cur = rows.astype(np.int16)
    a = np.zeros_like(cur); a[:, bpp:] = cur[:, :-bpp]
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, bpp:] = cur[:-1, :-bpp]
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    preds = [np.zeros_like(cur), a, b, (a + b) >> 1, np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))]
    f = np.asarray(filters)
    raw = np.empty((rows.shape[0], rows.shape[1] + 1), np.uint8)
    raw[:, 0] = f
    for t in range(5):
        raw[f == t, 1:] = ((cur - preds[t])[f == t] & 255).astype(np.uint8)
    return raw.reshape(-1)


def device(args):
    import torch
    from dspnet_amd import _lib
    from dspnet_amd.dataset import png as dp
    dev = torch.device("cuda", 0)
    lib, st = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    g = np.random.Generator(np.random.PCG64(5))
    scenes = [scene(3000 + i, 4) for i in range(4)]
    print("dspn_png_rgb_batch, B = %d at %d x %d, row filters drawn uniformly from the five types; device events around each call "
          "after 3 warm-up calls, %d calls; steps = row_bytes / 4 + 1023" % (B, W, H, args.reps))
    for name, (colour, depth) in FORMATS.items():
        if args.only and name != args.only:
            continue
        ch, sb = (3 if colour == 2 else 4), depth // 8
        rb = W * ch * sb
        raws, wants = [], []
        for s in scenes:
            px = s[:, :, :ch]
            if sb == 2:                                         # high byte the scene, low byte noise
                px = np.stack([px, g.integers(0, 256, px.shape, dtype=np.uint8)], -1)
            raws.append(filtered(px.reshape(H, rb), g.integers(0, 5, H), ch * sb))
            wants.append(s[:, :, :3])
        per = raws[0].size
        samples = np.zeros(B, dp.RGB_SAMPLE)
        for b in range(B):
            samples[b] = (b * per, b * H * rb, b * H * W * 3, W, H, depth, colour, 0, 0)
        raw = torch.from_numpy(np.concatenate([raws[b % 4] for b in range(B)])).to(dev)
        desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
        ws = torch.empty(max(dp.rgb_workspace_bytes(samples), 1), dtype=torch.uint8, device=dev)
        out = torch.full((B * H * W * 3,), 0xA5, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.dspn_png_rgb_batch(raw.data_ptr(), raw.numel(), desc.data_ptr(), B, None, 0, out.data_ptr(), out.numel(),
                                              ws.data_ptr(), ws.numel(), st))

        call()
        torch.cuda.synchronize(dev)
        got = out.view(B, H, W, 3).cpu().numpy()
        assert all((got[b] == wants[b % 4]).all() for b in range(B)), "RGB bytes differ from the source scenes"
        for _ in range(3):
            call()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
        ev[0].record()
        for k in range(args.reps):
            call(); ev[k + 1].record()
        torch.cuda.synchronize(dev)
        ts = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.reps)]
        steps = rb // 4 + H - 1
        print("  %-6s stride %d, %5d steps: %.3f ms per call (median; min %.3f, max %.3f), %.3f us per step if the call were the "
              "reconstruction alone; RGB bytes equal the source scenes" % (name, ch * sb, steps, np.median(ts), min(ts), max(ts),
                                                                           np.median(ts) * 1e3 / steps))


def im2rec(args):
    import torch
    from PIL import Image
    from dspnet_amd.dataset import im2rec as ir
    from dspnet_amd.dataset import jpeg_encode
    from dspnet_amd.dataset import png as dp
    dev = torch.device("cuda", 0)
    files = []
    for i in range(B):
        buf = io.BytesIO()
        Image.fromarray(scene(4000 + i)).save(buf, format="PNG", compress_level=6)
        files.append(buf.getvalue())
    hist = np.zeros(5, np.int64)
    for f in files:
        info = dp.probe_rgb(f)
        rows = np.empty(info["raw_bytes"], np.uint8)
        assert info["supported"] and dp.inflate_into(f, info, rows) == 0
        hist += np.bincount(rows[0::info["row_bytes"] + 1], minlength=5)
    print("%d RGB 8-bit PNG files of %d x %d written by Pillow at zlib level 6: mean %.2f MB; filter types over all rows: None %d, "
          "Sub %d, Up %d, Average %d, Paeth %d" % ((B, W, H, np.mean([len(f) for f in files]) / 1e6) + tuple(hist)))
    real = dp.open_rgb

    def run(new):
        dp.open_rgb = real if new else (lambda content: None)   # the parent's _decode: every PNG through Pillow
        try:
            t0 = time.perf_counter()
            pixels = ir._decode(files, dev)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            coded = jpeg_encode.encode_batch(pixels, quality=95, subsampling="4:2:0")
            torch.cuda.synchronize(dev)
            return t1 - t0, time.perf_counter() - t0, pixels, coded
        finally:
            dp.open_rgb = real

    _, _, pa, ca = run(True)
    _, _, pb, cb = run(False)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb)) and ca == cb, "the two paths differ"
    del pa, pb
    t = {True: [], False: []}
    for rep in range(args.reps):                                # alternated
        for new in (False, True):
            t[new].append(run(new)[:2])
    for new, name in ((False, "parent (Pillow decode, pixel upload)"), (True, "new (host inflate, device RGB)")):
        dec, tot = np.array(t[new]).T * 1e3
        print("  %-38s: _decode %.1f ms (median; min %.1f, max %.1f), _decode + encode_batch %.1f ms (median; min %.1f, max %.1f) "
              "per batch of %d, %d repetitions" % (name, np.median(dec), dec.min(), dec.max(), np.median(tot), tot.min(), tot.max(),
                                                   B, args.reps))
    print("  pixels and JPEG files of the two paths are equal")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["device", "im2rec"])
    ap.add_argument("--only", choices=sorted(FORMATS), default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    {"device": device, "im2rec": im2rec}[a.what](a)
