"""Measurements of the colour jitter (include/dspn_colour_jitter.h), written into DESIGN.md by hand from this script's
output.  Everything is generated from seeds.

    python tools/colour_jitter_measure.py device                     # 1: one call over B = 32 at 1024 x 2048 x 3, device events
    python tools/colour_jitter_measure.py iterator --workdir DIR     # 2: MultiTaskRecordIter batches/s, jitter off and on

Both fail without a GPU.  The record file of `iterator` is the one of tools/jpeg_measure.py."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

H, W = 1024, 2048
HBM_COPY_RATE = 6.29e12                                         # bytes/s, the measured float4 copy rate of the part


def device(args):
    import torch
    import ref_colour_jitter as ref
    from bench import GpuSensors
    from dspnet_amd.dataset import colour_jitter as cj
    dev = torch.device("cuda", 0)
    sensors = GpuSensors(0)
    B, per = 32, H * W * 3
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    source = torch.randint(0, 256, (B * per,), dtype=torch.uint8, device=dev, generator=gen)
    pool, other = source.clone(), torch.empty_like(source)
    offsets, sizes = [b * per for b in range(B)], [(H, W)] * B
    train = cj.ColorJitter(random_hue_prob=.5, random_saturation_prob=.5, random_illumination_prob=.5, random_contrast_prob=.5)
    rows = {"shifts and gain, every image": [(7, -13, 21, 1300)] * B,
            "shifts alone, every image": [(7, -13, 21, 1024)] * B,
            "gain alone, every image": [(0, 0, 0, 1300)] * B,
            "drawn with all four probabilities 0.5": cj.draw(train, B, np.random.RandomState(3))}

    def timed(fn, reps=50):
        """every call starts from the source pixels (copied in outside the timed pair of events), as in the pipeline, where
        the decode has just written the pool: jittering the same bytes over and over would drive them to one colour"""
        for _ in range(5):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        clocks = []
        for a, b in ev:
            pool.copy_(source)
            a.record(); fn(); b.record()
            clocks.append(sensors.read())
        torch.cuda.synchronize(dev)
        ts = [a.elapsed_time(b) for a, b in ev]
        return np.median(ts), min(ts), max(ts), GpuSensors.summarise(clocks).get("sclk_mhz", {}).get("median", "unread")

    moved = 2 * B * per
    print("dspn_colour_jitter_batch_u8, B = %d at %d x %d x 3: %.1f MB read and %.1f MB written per call; device events around "
          "each call after 5 warm-up calls, 50 calls.  Byte floor at the part's measured copy rate (%.2f TB/s): %.3f ms -- the "
          "pool fits the Infinity Cache, so repeated calls can run above that rate" % (B, H, W, B * per / 1e6, B * per / 1e6,
                                                                                        HBM_COPY_RATE / 1e12, moved / HBM_COPY_RATE * 1e3))
    med, lo, hi, clock = timed(lambda: other.copy_(pool))
    print("  %-40s: %.3f ms per call (median; min %.3f, max %.3f), %.2f TB/s; sclk %s MHz" %
          ("device copy of the pool (same bytes moved)", med, lo, hi, moved / med / 1e9, clock))
    for name, params in rows.items():
        desc = torch.from_numpy(cj.describe(params, offsets, sizes).view(np.uint8).reshape(-1)).to(dev)
        pool.copy_(source)
        cj.launch(pool, desc)
        torch.cuda.synchronize(dev)
        k = B - 1                                               # one strip of the last image against the restatement
        got = pool[k * per:k * per + 64 * W * 3].view(64, W, 3).cpu().numpy()
        want = ref.jitter(source[k * per:k * per + 64 * W * 3].view(64, W, 3).cpu().numpy(), *params[k])
        assert np.array_equal(got, want), "the launch differs from the restatement"
        active = sum(1 for p in params if tuple(int(v) for v in p) != cj.IDENTITY)
        med, lo, hi, clock = timed(lambda: cj.launch(pool, desc))
        print("  %-40s: %.3f ms per call (median; min %.3f, max %.3f), %d of %d images touched, %.2f TB/s over their bytes, "
              "%.1f ps per pixel; sclk %s MHz" % (name, med, lo, hi, active, B, 2 * active * per / med / 1e9,
                                                  med * 1e9 / max(active * H * W, 1), clock))


def iterator(args):
    import torch
    from jpeg_measure import _write_records
    from dspnet_amd.dataset import colour_jitter as cj
    from dspnet_amd.dataset import iterator as it
    dev = torch.device("cuda", 0)
    B, n = 32, args.records
    path = _write_records(args.workdir, n)
    train = cj.ColorJitter(random_hue_prob=.5, random_saturation_prob=.5, random_illumination_prob=.5, random_contrast_prob=.5)
    print("MultiTaskRecordIter, B = %d, data shape (3, 512, 1024), %d records of %d x %d JPEG (quality 92, 4:2:0) + label PNG, "
          "device_jpeg and device_png on, %d timed batches after the constructor's warm-up batch, window closed by a device "
          "synchronise; jitter: all four probabilities 0.5" % (B, n, H, W, args.batches))
    for threads in (8, 16):
        rates = {False: [], True: []}
        for rep in range(3):
            for on in (False, True):                            # alternated
                itr = it.MultiTaskRecordIter(path, B, (3, 512, 1024), device=dev, decode_threads=threads, device_jpeg=True,
                                             device_png=True, color_jitter=train if on else None, jitter_seed=1)
                torch.cuda.synchronize(dev)
                done, t0 = 0, time.perf_counter()
                while done < args.batches:
                    if not itr.iter_next():
                        itr.reset()
                    itr.next()
                    done += 1
                torch.cuda.synchronize(dev)
                rates[on].append(done / (time.perf_counter() - t0))
                itr._drop_ahead()
                del itr
        off, on = np.mean(rates[False]), np.mean(rates[True])
        print("  decode_threads %2d: jitter off %.2f batches/s (runs %s), on %.2f batches/s (runs %s), ratio %.3f" %
              (threads, off, ["%.2f" % r for r in rates[False]], on, ["%.2f" % r for r in rates[True]], on / off))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["device", "iterator"])
    ap.add_argument("--records", type=int, default=128)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if a.what == "iterator" and not a.workdir:
        import tempfile
        a.workdir = tempfile.mkdtemp(prefix="colour_jitter_measure_")
    {"device": device, "iterator": iterator}[a.what](a)
