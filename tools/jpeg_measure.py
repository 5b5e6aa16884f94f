"""Measurements of the device JPEG decode (include/dspn_jpeg.h), written to profiles/jpeg_device_decode.txt by hand from
this script's output.  Everything is generated from seeds.

    python tools/jpeg_measure.py host                      # 1: entropy pass against Pillow's full decode, per image
    python tools/jpeg_measure.py device                    # 2: reconstruction of B = 32 at 1024 x 2048, device events
    python tools/jpeg_measure.py iterator --workdir DIR    # 3: MultiTaskRecordIter batches/s, device_jpeg off and on
    python tools/jpeg_measure.py entropy --workdir DIR     # profiles/jpeg_device_entropy.txt: the entropy pass on the device

`host` needs no GPU; `device`, `iterator` and `entropy` fail without one."""
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


def jpeg_bytes(arr, quality, restart_interval=0):
    """restart_interval > 0: Pillow's restart_marker_blocks, the bytes jpeg_encode.encode_batch(restart_interval=) writes"""
    from PIL import Image
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": restart_interval} if restart_interval else {}
    Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=2, **kw)
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


def _write_records(root, n, restart_interval=0, distinct=None):
    """distinct: the number of different pictures the records cycle through (None: every record its own)"""
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
        rec.write_idx(i, recordio.pack(recordio.IRHeader(0, label, i, 0), jpeg_bytes(picture(3000 + i % (distinct or n)), 92, restart_interval)))
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


def entropy(args):
    """the device entropy pass against the 16-thread host entropy pass: B = 32 streams of 1024 x 2048 4:2:0 at quality 92
    and 75, at the restart intervals of --intervals (MCUs; one MCU row of these images is 128)"""
    import torch
    from dspnet_amd.dataset import iterator as it
    from dspnet_amd.dataset import jpeg as dj
    dev = torch.device("cuda", 0)
    B = 32
    intervals = [int(v) for v in args.intervals.split(",")]
    refused = [v for v in intervals if v > dj.DEVICE_MAX_INTERVAL]
    if refused:                                                 # the rows at 128 and 512 of the profile were taken with the constant at 512
        print("intervals %s are above DSPN_JPEG_DEVICE_MAX_INTERVAL = %d: such streams stay on the host pass, left out" %
              (refused, dj.DEVICE_MAX_INTERVAL))
        intervals = [v for v in intervals if v <= dj.DEVICE_MAX_INTERVAL]
    pictures = [picture(2000 + i) for i in range(8)]
    print("device entropy pass, B = %d streams (8 distinct) of %d x %d 4:2:0; host yardstick: dspn_jpeg_entropy_decode of the same "
          "batch on a pool of 16 threads (%d CPUs visible)" % (B, H, W, os.cpu_count()))
    for quality in (92, 75):
        plain = [jpeg_bytes(p, quality) for p in pictures]
        for interval in intervals:
            streams = [jpeg_bytes(p, quality, interval) for p in pictures]
            growth = sum(map(len, streams)) / sum(map(len, plain)) - 1
            payloads = [streams[b % 8] for b in range(B)]
            infos = [dj.probe_info(s)[1] for s in payloads]
            sizes = [H * W * 3] * B
            batch = dj.CodedBatch(infos, np.cumsum([0] + sizes[:-1]), True)
            t0 = time.perf_counter()
            assert all(index(p) for p, index in zip(payloads, batch.indexers()))
            t_index = (time.perf_counter() - t0) / B
            batch.answered([True] * B)
            assert batch.device_entropy == B and batch.host_count == 0
            pool = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
            batch.upload(torch.empty(1, dtype=torch.int16), dev)
            keep = batch.launch(pool)
            torch.cuda.synchronize(dev)
            batch.check()
            assert (pool[:sizes[0]].view(H, W, 3).cpu().numpy() == pillow_decode(payloads[0])).all(), "pixels differ from Pillow's"
            desc_dev, scan_dev, status = keep[1], keep[2], keep[3]
            a, b = B * dj.SAMPLE.itemsize, B * (dj.SAMPLE.itemsize + dj.SCAN.itemsize)
            coef_dev = keep[0]

            def launch():
                dj.entropy_decode_device(scan_dev, desc_dev[:a], desc_dev[a:b], desc_dev[b:].view(torch.int32), coef_dev, status)

            for _ in range(3):
                launch()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(11)]
            ev[0].record()
            for k in range(10):
                launch(); ev[k + 1].record()
            torch.cuda.synchronize(dev)
            t_dev = np.median([ev[k].elapsed_time(ev[k + 1]) for k in range(10)])
            # the host pass of the same batch, 16 threads, the parent commit's code path
            bufs = [np.empty(int(i["coef_count"]), np.int16) for i in infos]
            with ThreadPoolExecutor(16) as tp:
                walls = []
                for _ in range(4):
                    t0 = time.perf_counter()
                    assert not any(tp.map(lambda k: dj.entropy_decode(payloads[k], infos[k], bufs[k]), range(B)))
                    walls.append(time.perf_counter() - t0)
            up_dev = batch.scan_bytes + desc_dev.numel()
            up_host = 2 * sum(int(i["coef_count"]) for i in infos) + a
            print("  quality %d, interval %3d MCUs: %5d segments/image, file +%.2f %% (mean %.0f KB); device entropy launch %.3f ms per batch "
                  "(median of 10, device events), host pass on 16 threads %.1f ms per batch (best of 4; runs %s), scan index %.3f ms/image on "
                  "one thread; upload %.2f MB per batch against %.2f MB of coefficients" %
                  (quality, interval, int(batch.scans[0]["segments"]), 100 * growth, np.mean([len(s) for s in streams]) / 1e3, t_dev,
                   min(walls) * 1e3, ["%.1f" % (w * 1e3) for w in walls], t_index * 1e3, up_dev / 1e6, up_host / 1e6))
            del keep, pool
    n = args.records
    print("MultiTaskRecordIter, B = %d, data shape (3, 512, 1024), device_jpeg=True, %d records per file (16 distinct pictures, quality 92), %d timed batches, "
          "device_entropy off and on alternated, two runs each" % (B, n, args.batches))
    for interval in intervals:
        path = _write_records(os.path.join(args.workdir, "ri%d" % interval), n, interval, distinct=16)
        for threads in (8, 16):
            rates = {False: [], True: []}
            for run in range(2):
                for on in (False, True):
                    itr = it.MultiTaskRecordIter(path, B, (3, 512, 1024), device=dev, decode_threads=threads, device_jpeg=True,
                                                 device_entropy=on)
                    torch.cuda.synchronize(dev)
                    done, t0 = 0, time.perf_counter()
                    while done < args.batches:
                        if not itr.iter_next():
                            itr.reset()
                        itr.next()
                        done += 1
                    torch.cuda.synchronize(dev)
                    rates[on].append(done / (time.perf_counter() - t0))
                    counted = itr.jpeg_device_entropy
                    itr._drop_ahead()
                    del itr
            off, on_ = np.mean(rates[False]), np.mean(rates[True])
            print("  interval %3d, decode_threads %2d: device_entropy off %.2f batches/s (runs %s), on %.2f batches/s (runs %s), ratio %.2f, "
                  "%d records through the device pass in the last run" % (interval, threads, off, ["%.2f" % r for r in rates[False]], on_,
                                                                         ["%.2f" % r for r in rates[True]], on_ / off, counted))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["host", "device", "iterator", "entropy"])
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--records", type=int, default=128)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--intervals", default="8,16,32", help="entropy: restart intervals in MCUs")
    a = ap.parse_args()
    if a.what in ("iterator", "entropy") and not a.workdir:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix="jpeg_measure_")
    {"host": host, "device": device, "iterator": iterator, "entropy": entropy}[a.what](a)
