"""Measurements of the device JPEG decode (include/dspn_jpeg.h), written to profiles/jpeg_device_decode.txt by hand from
this script's output.  Everything is generated from seeds.

    python tools/jpeg_measure.py host                      # 1: entropy pass against Pillow's full decode, per image
    python tools/jpeg_measure.py device                    # 2: reconstruction of B = 32 at 1024 x 2048, device events
    python tools/jpeg_measure.py iterator --workdir DIR    # 3: MultiTaskRecordIter batches/s, device_jpeg off and on

`host` needs no GPU; `device` and `iterator` fail without one."""
import argparse
import io
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 1024, 2048


def picture(seed):
    """smooth structure plus noise, like a photograph's statistics at the sizes that matter here"""
    g = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:H, :W]
    chans = [127 + 100 * np.sin(xx / g.uniform(20, 90) + g.uniform(0, 3)) * np.cos(yy / g.uniform(20, 90)) for _ in range(3)]
    return np.clip(np.stack(chans, -1) + g.normal(0, 8, (H, W, 3)), 0, 255).astype(np.uint8)


def jpeg_bytes(arr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def host(args):
    from dspnet_amd.dataset import jpeg as dj
    n = args.images
    for quality in (75, 92):
        streams = [jpeg_bytes(picture(1000 + i), quality) for i in range(n)]
        infos = [dj.probe_info(s)[1] for s in streams]
        bufs = [np.empty(int(i["coef_count"]), np.int16) for i in infos[:16]]

        def entropy(k):
            assert dj.entropy_decode(streams[k], infos[k], bufs[k % 16]) == 0

        def pillow(k):
            pillow_decode(streams[k])

        print("quality %d: %d streams of %d x %d 4:2:0, mean %.0f KB" % (quality, n, H, W, np.mean([len(s) for s in streams]) / 1e3))
        for k in range(2):
            entropy(k); pillow(k)
        t = {"pillow": [], "entropy": []}
        for k in range(n):                                      # single thread, alternated per image
            for name, fn in (("pillow", pillow), ("entropy", entropy)):
                t0 = time.perf_counter(); fn(k); t[name].append(time.perf_counter() - t0)
        p, e = np.median(t["pillow"]) * 1e3, np.median(t["entropy"]) * 1e3
        print("  1 thread : Pillow full decode %.2f ms/image, entropy pass %.2f ms/image (median of %d), ratio %.2f" % (p, e, n, p / e))
        for threads in (8,):
            with ThreadPoolExecutor(threads) as pool:
                wall = {"pillow": [], "entropy": []}
                for rep in range(3):                            # alternated per pass over the set
                    for name, fn in (("pillow", pillow), ("entropy", entropy)):
                        t0 = time.perf_counter(); list(pool.map(fn, range(n))); wall[name].append(time.perf_counter() - t0)
            p, e = min(wall["pillow"]), min(wall["entropy"])
            print("  %d threads: Pillow %.0f images/s, entropy pass %.0f images/s (best of 3 passes over %d images, %d CPUs visible), "
                  "ratio %.2f" % (threads, n / p, n / e, n, os.cpu_count(), p / e))


def device(args):
    import ctypes as c
    import torch
    from dspnet_amd import _lib
    from dspnet_amd.dataset import iterator as it
    from dspnet_amd.dataset import jpeg as dj
    dev = torch.device("cuda", 0)
    B = 32
    streams = [jpeg_bytes(picture(2000 + i % 8), 92) for i in range(8)]
    infos = [dj.probe_info(s)[1] for s in streams]
    per = int(infos[0]["coef_count"])
    coefs = np.empty(B * per, np.int16)
    samples, warp = np.zeros(B, dj.SAMPLE), np.zeros(B, it._SAMPLE)
    for b in range(B):
        assert dj.entropy_decode(streams[b % 8], infos[b % 8], coefs[b * per:(b + 1) * per]) == 0
        dj.fill_sample(samples[b], infos[b % 8], b * per, b * H * W * 3)
        warp[b] = (b * H * W * 3, -1, H, W, 0, 0, 0, 0, it.invert_affine([.5, 0, 0, 0, .5, 0]))
    cdev = torch.from_numpy(coefs).to(dev)
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    wdesc = torch.from_numpy(warp.view(np.uint8).reshape(-1).copy()).to(dev)
    pool = torch.empty(B * H * W * 3, dtype=torch.uint8, device=dev)
    data = torch.empty(B, 3, H // 2, W // 2, device=dev)
    ws = torch.empty(cdev.numel(), dtype=torch.uint8, device=dev)
    lib = _lib.lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    mean = (c.c_double * 3)(123.68, 116.779, 103.939)

    def recon():
        _lib.check(lib.dspn_jpeg_reconstruct_batch_u8(cdev.data_ptr(), cdev.numel(), desc.data_ptr(), B, pool.data_ptr(), pool.numel(),
                                                      ws.data_ptr(), ws.numel(), st))

    def augment():
        _lib.check(it._entry()(pool.data_ptr(), pool.data_ptr(), wdesc.data_ptr(), B, H // 2, W // 2, it._CMAP_RGB, mean, None,
                               data.data_ptr(), None, st))

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for k in range(reps):
            fn(); ev[k + 1].record()
        torch.cuda.synchronize(dev)
        return np.median([ev[k].elapsed_time(ev[k + 1]) for k in range(reps)])

    recon()
    torch.cuda.synchronize(dev)
    got = pool[:H * W * 3].view(H, W, 3).cpu().numpy()
    assert (got == pillow_decode(streams[0])).all(), "pixels differ from Pillow's"
    n = 1.5                                                     # samples per pixel at 4:2:0
    idct_bytes, colour_bytes = H * W * (2 * n + n), H * W * (n + 3)
    t_r, t_a = timed(recon), timed(augment)
    total = B * (idct_bytes + colour_bytes)
    print("reconstruct B = %d at %d x %d 4:2:0 (pixels equal Pillow's): %.3f ms per call (median of 20, device events)" % (B, H, W, t_r))
    print("  bytes per image from the shapes: idct launch %.2f MB (coefficients in, planes out), colour launch %.2f MB "
          "(planes in, RGB out), both %.2f MB" % (idct_bytes / 1e6, colour_bytes / 1e6, (idct_bytes + colour_bytes) / 1e6))
    print("  %.2f TB/s over both launches = %.0f %% of the 6.3 TB/s achievable HBM rate (8 TB/s peak)" % (total / t_r / 1e9, total / t_r / 1e9 / 6.3 * 100))
    print("dspn_augment_batch_u8 of the same batch to (%d, 3, %d, %d), no label maps: %.3f ms per call" % (B, H // 2, W // 2, t_a))


def _write_records(root, n):
    from PIL import Image
    from dspnet_amd.dataset import recordio
    os.makedirs(os.path.join(root, "cityscapes", "SegmentationClass"), exist_ok=True)
    rec = recordio.MXIndexedRecordIO(os.path.join(root, "train.idx"), os.path.join(root, "train.rec"), "w")
    g = np.random.Generator(np.random.PCG64(7))
    lines = []
    for i in range(n):
        rows = np.full((10, 6), -1.0)
        for k in range(4):
            x0, y0 = g.uniform(0, .8), g.uniform(0, .8)
            rows[k] = [g.integers(0, 8), x0, y0, x0 + g.uniform(.05, .2), y0 + g.uniform(.05, .2), g.uniform(0, 1)]
        label = np.array([2, 6] + rows.reshape(-1).tolist(), np.float32)
        rec.write_idx(i, recordio.pack(recordio.IRHeader(0, label, i, 0), jpeg_bytes(picture(3000 + i), 92)))
        seg = np.repeat(np.repeat(g.integers(0, 19, (H // 64, W // 64)).astype(np.uint8), 64, 0), 64, 1)   # large regions
        Image.fromarray(seg).save(os.path.join(root, "cityscapes", "SegmentationClass", "city_%06d_gtFine_labelTrainIds.png" % i))
        lines.append("%d\tJPEGImages/city_%06d_leftImg8bit.jpg\n" % (i, i))
    rec.close()
    with open(os.path.join(root, "train.lst"), "w") as f:
        f.writelines(lines)
    return os.path.join(root, "train.rec")


def iterator(args):
    import torch
    from dspnet_amd.dataset import iterator as it
    dev = torch.device("cuda", 0)
    B, n = 32, args.records
    path = _write_records(args.workdir, n)
    print("MultiTaskRecordIter, B = %d, data shape (3, 512, 1024), %d records of %d x %d JPEG (quality 92, 4:2:0) + label PNG, "
          "%d timed batches after the constructor's warm-up batch, window closed by a device synchronise" % (B, n, H, W, args.batches))
    for threads in (8, 16):
        rates = {False: [], True: []}
        for rep in range(2):
            for dj_on in (False, True):                         # alternated
                itr = it.MultiTaskRecordIter(path, B, (3, 512, 1024), device=dev, decode_threads=threads, device_jpeg=dj_on)
                torch.cuda.synchronize(dev)
                done, t0 = 0, time.perf_counter()
                while done < args.batches:
                    if not itr.iter_next():
                        itr.reset()
                    itr.next()
                    done += 1
                torch.cuda.synchronize(dev)
                rates[dj_on].append(done / (time.perf_counter() - t0))
                fb = itr.jpeg_fallbacks
                itr._drop_ahead()
                del itr
        off, on = np.mean(rates[False]), np.mean(rates[True])
        print("  decode_threads %2d: device_jpeg off %.2f batches/s (%.0f images/s; runs %s), on %.2f batches/s (%.0f images/s; runs %s), "
              "ratio %.2f, fallbacks %d" % (threads, off, off * B, ["%.2f" % r for r in rates[False]], on, on * B,
                                           ["%.2f" % r for r in rates[True]], on / off, fb))


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
        a.workdir = tempfile.mkdtemp(prefix="jpeg_measure_")
    {"host": host, "device": device, "iterator": iterator}[a.what](a)
