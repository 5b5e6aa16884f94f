"""Measurements of the device JPEG encode (include/dspn_jpeg_encode.h), written into DESIGN.md by hand from this script's
output.  Everything is generated from seeds; it fails without a GPU.

    python tools/jpeg_encode_measure.py [--images 16] [--threads 8] [--quality 95]

Per run: the two device launches alone (device events), encode_batch end to end (host clock around a call that ends with
the files in hand), and Pillow encoding the same images on the same host with the same number of threads, the two
alternated; the first file is compared with Pillow's before anything is timed.  Then the entropy pass on the device
(device_entropy=True): its files asserted equal, its two calls alone by device events, and encode_batch end to end with the
switch off and on, alternated."""
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


def pillow_file(arr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from dspnet_amd import _lib
    from dspnet_amd.dataset import jpeg_encode as je
    dev = torch.device("cuda", 0)
    host = [picture(4000 + i) for i in range(a.images)]
    images = [torch.from_numpy(x).to(dev) for x in host]
    files = je.encode_batch(images, quality=a.quality, threads=a.threads)
    assert files[0] == pillow_file(host[0], a.quality) and files[-1] == pillow_file(host[-1], a.quality), "files differ from Pillow's"
    cpu = "?"
    with open("/proc/cpuinfo") as f:
        for line in f:
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    print("%d images of %d x %d RGB, quality %d, 4:2:0, mean file %.0f KB (equal to Pillow's); %d threads; host CPU: %s (%d visible)"
          % (a.images, H, W, a.quality, np.mean([len(f) for f in files]) / 1e3, a.threads, cpu, os.cpu_count()))

    # 1: the two launches alone
    tables = je.quant_tables(a.quality)
    samples = np.zeros(a.images, je.SAMPLE)
    co = 0
    for k in range(a.images):
        co += je.fill_sample(samples[k], W, H, 3, (2, 2), tables, co, k * H * W * 3)
    pool = torch.cat([im.reshape(-1) for im in images])
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    coefs = torch.empty(co, dtype=torch.int16, device=dev)
    ws = torch.empty(co, dtype=torch.uint8, device=dev)
    cmap = (je._c.c_int * 3)(0, 1, 2)
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = _lib.lib()

    def launches():
        _lib.check(lib.dspn_jpeg_encode_blocks_batch_u8(pool.data_ptr(), pool.numel(), cmap, desc.data_ptr(), a.images, coefs.data_ptr(),
                                                        co, ws.data_ptr(), ws.numel(), st))

    for _ in range(3):
        launches()
    reps = 20
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for k in range(reps):
        launches(); ev[k + 1].record()
    torch.cuda.synchronize(dev)
    t_dev = float(np.median([ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]))
    n = 1.5
    moved = a.images * H * W * (3 + n + n + 2 * n)
    print("device launches alone: %.3f ms per call (median of %d, device events), %.1f us per image; %.1f MB per image from the "
          "shapes (pixels in, planes out and in, coefficients out) = %.2f TB/s" % (t_dev, reps, t_dev * 1e3 / a.images, moved / a.images / 1e6,
                                                                                    moved / t_dev / 1e9))

    # 2, 3: end to end against Pillow, alternated
    def ours():
        return je.encode_batch(images, quality=a.quality, threads=a.threads)

    def pillow():
        with ThreadPoolExecutor(a.threads) as tp:
            return list(tp.map(lambda x: pillow_file(x, a.quality), host))

    ours(); pillow()
    t = {"ours": [], "pillow": []}
    for _ in range(a.reps):
        for name, fn in (("ours", ours), ("pillow", pillow)):
            t0 = time.perf_counter(); fn(); t[name].append(time.perf_counter() - t0)
    o, p = np.median(t["ours"]) * 1e3, np.median(t["pillow"]) * 1e3
    print("encode_batch end to end (device tensors in, files out): %.1f ms per batch, %.2f ms per image (median of %d; runs %s)"
          % (o, o / a.images, a.reps, ["%.1f" % (x * 1e3) for x in t["ours"]]))
    print("Pillow, %d threads, host arrays in, files out: %.1f ms per batch, %.2f ms per image (runs %s); ratio Pillow / encode_batch %.2f"
          % (a.threads, p, p / a.images, ["%.1f" % (x * 1e3) for x in t["pillow"]], p / o))
    # where the end-to-end time goes: the entropy pass alone, from coefficients already on the host
    hostc = coefs.cpu().numpy()
    with ThreadPoolExecutor(a.threads) as tp:
        t0 = time.perf_counter(); list(tp.map(lambda s: je.entropy_encode(hostc, s), samples)); t_ent = time.perf_counter() - t0
    t0 = time.perf_counter(); je.entropy_encode(hostc, samples[0]); t_one = time.perf_counter() - t0
    print("entropy pass alone: %.1f ms per batch on %d threads, %.2f ms for one image on one thread" % (t_ent * 1e3, a.threads, t_one * 1e3))

    # 4: the entropy pass on the device (device_entropy=True): the same files, the launches alone, end to end off / on alternated
    assert je.encode_batch(images, quality=a.quality, threads=a.threads, device_entropy=True) == files, "device entropy: files differ"
    intervals = torch.zeros(a.images, dtype=torch.int32, device=dev)
    sizes, status, ews = je.entropy_scan_batch(coefs, desc, intervals)
    total = int(sizes.sum().item())
    assert not status.any().item() and total == sum(len(f) - len(je.headers(s)) - 2 for f, s in zip(files, samples))
    offsets = (torch.cumsum(sizes, 0) - sizes).contiguous()
    scans = torch.empty(total, dtype=torch.uint8, device=dev)
    ews_bytes = lib.dspn_jpeg_entropy_encode_workspace_bytes(co, a.images)

    def scan_call():
        _lib.check(lib.dspn_jpeg_entropy_encode_scan_batch(coefs.data_ptr(), co, desc.data_ptr(), intervals.data_ptr(), a.images,
                                                           sizes.data_ptr(), status.data_ptr(), ews.data_ptr(), ews_bytes, st))

    def write_call():
        _lib.check(lib.dspn_jpeg_entropy_encode_write_batch(co, a.images, offsets.data_ptr(), scans.data_ptr(), total, ews.data_ptr(),
                                                            ews_bytes, st))

    t_calls = {}
    for name, fn in (("scan", scan_call), ("write", write_call)):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for k in range(reps):
            fn(); ev[k + 1].record()
        torch.cuda.synchronize(dev)
        t_calls[name] = float(np.median([ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]))
    print("device entropy pass alone: scan call (10 launches) %.3f ms, write call (1 launch) %.3f ms per batch (medians of %d, device "
          "events); %.1f MB of coefficients read twice, %.2f MB of scans out; workspace %.0f MB"
          % (t_calls["scan"], t_calls["write"], reps, co * 2 / 1e6, total / 1e6, ews_bytes / 1e6))

    def device():
        return je.encode_batch(images, quality=a.quality, threads=a.threads, device_entropy=True)

    ours(); device()
    t = {"host": [], "device": []}
    for _ in range(a.reps):
        for name, fn in (("host", ours), ("device", device)):
            t0 = time.perf_counter(); fn(); t[name].append(time.perf_counter() - t0)
    hh, dd = np.median(t["host"]) * 1e3, np.median(t["device"]) * 1e3
    print("encode_batch end to end, host entropy pass on %d threads: %.1f ms per batch (median of %d; runs %s)"
          % (a.threads, hh, a.reps, ["%.1f" % (x * 1e3) for x in t["host"]]))
    print("encode_batch end to end, device_entropy=True: %.1f ms per batch (runs %s); ratio host / device %.2f"
          % (dd, ["%.1f" % (x * 1e3) for x in t["device"]], hh / dd))


if __name__ == "__main__":
    main()
