"""Times dspn_det_augment_batch_u8 (include/dspn_det_augment.h) per interpolation method for B = 32 sources of
1024 x 2048 resized to 512 x 512, by the device-event timing tools/jpeg_measure.py uses for dspn_augment_batch_u8 (median
of 20 calls after 3 warm-up calls), beside the floor the bytes of the call set: source bytes read once plus float planes
written once, over the 6.3 TB/s achievable HBM rate.  Needs a GPU.

    python tools/det_augment_measure.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SRC_H, SRC_W, H, W = 32, 1024, 2048, 512, 512
HBM = 6.3e12
NAMES = ("linear", "cubic", "area", "nearest", "lanczos4")


def main():
    import torch
    from bench import GpuSensors
    from dspnet_amd.dataset import det_iterator as di
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    dev = torch.device("cuda", 0)
    sensors = GpuSensors(0)
    per = SRC_H * SRC_W * 3
    pool = torch.randint(0, 256, (B * per,), dtype=torch.uint8, device=dev)
    data = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    mean = (123.68, 116.779, 103.939)

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        clocks = []
        for k in range(reps):
            fn(); ev[k + 1].record()
            clocks.append(sensors.read())
        torch.cuda.synchronize(dev)
        return np.median([ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]), clocks

    floor_bytes = B * per + data.numel() * 4
    print("dspn_det_augment_batch_u8, B = %d, %d x %d -> %d x %d, device events, median of 20 calls" % (B, SRC_H, SRC_W, H, W))
    print("bytes from the shapes: %.1f MB sources + %.1f MB planes = %.1f MB; at %.1f TB/s: %.1f us"
          % (B * per / 1e6, data.numel() * 4 / 1e6, floor_bytes / 1e6, HBM / 1e12, floor_bytes / HBM * 1e6))
    cases = [(NAMES[m], m, (0, 0, SRC_W, SRC_H)) for m in di.METHODS]
    cases.append(("area, zoom-out x 2 (canvas 2048 x 4096)", di.AREA, (-SRC_W // 2, -SRC_H // 2, 2 * SRC_W, 2 * SRC_H)))
    for name, method, window in cases:
        plans = [{"src_w": SRC_W, "src_h": SRC_H, "img_offset": b * per, "window": window, "method": method, "mirror": b & 1}
                 for b in range(B)]
        samples, tables = di.pack_batch(plans, H, W)
        desc = torch.from_numpy(samples.view(np.uint8).reshape(-1)).to(dev)
        tab = torch.from_numpy(tables).to(dev)
        t, clocks = timed(lambda: di.augment_on_device(pool, desc, tab, H, W, mean, out=data))
        clock = GpuSensors.summarise(clocks).get("sclk_mhz", {}).get("median", "unread")
        print("  %-42s %d x %d taps  %.3f ms per call  (x %.1f of the floor; sclk %s MHz)"
              % (name, samples["ky"][0], samples["kx"][0], t, t * 1e-3 / (floor_bytes / HBM), clock))


if __name__ == "__main__":
    main()
