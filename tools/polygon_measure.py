"""Measurement of the Cityscapes label-map preparation (dataset/cityscapes_labels.py) against the same work through Pillow
on the host, written to DESIGN.md by hand from this script's output.  Everything is generated from seeds.

    python tools/polygon_measure.py --images 16 --repeats 5 --workdir DIR

Both sides read the same `*_gtFine_polygons.json` files (synthetic 2048 x 1024 street scenes, about 100 polygons each,
tests/ref_polygon.py's street_scene) and write the same four PNG files per image.  Host side: what the preparation scripts
do -- parse, one ImageDraw.polygon per object and encoding, Image.save.  Device side: write_label_images.  Wall clock
around whole passes with the device idle before and after (torch.cuda.synchronize); the first pass of each side is a
warm-up and is not counted; the median and the spread of the others are printed, and the device side is also split into
its host table building, the two kernels (device events) and the PNG write."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W = 1024, 2048
LABELS = ["sky", "building", "vegetation", "road", "sidewalk", "pole", "car", "person", "truck", "rider", "bicycle",
          "cargroup", "traffic sign", "bus"]


def write_scenes(workdir, n):
    import ref_polygon as rp
    paths = []
    for i in range(n):
        g = np.random.default_rng(500 + i)
        objects = [{"label": LABELS[int(g.integers(0, len(LABELS)))] if k > 3 else LABELS[k],
                    "polygon": [list(p) for p in xy]} for k, xy in enumerate(rp.street_scene(1000 + i, H, W))]
        path = os.path.join(workdir, "scene_%06d_000019_gtFine_polygons.json" % i)
        with open(path, "w") as f:
            json.dump({"imgHeight": H, "imgWidth": W, "objects": objects}, f)
        paths.append(path)
    return paths


def pillow_pass(paths, out_dir):
    from PIL import Image, ImageDraw
    from dspnet_amd.dataset import cityscapes_labels as cl
    for path in paths:
        drawn = cl.drawn_objects(cl.load_annotation(path))
        for c, (kind, background) in enumerate(zip(cl.KINDS, (0, 255, 0, 255))):
            im = Image.new("L" if c < 2 else "I", (W, H), background)
            draw = ImageDraw.Draw(im)
            for xy, values in drawn:
                draw.polygon(xy, fill=values[c])
            if c >= 2:
                im = Image.fromarray(np.asarray(im).astype(np.uint16))
            im.save(cl.output_path(path, kind, out_dir))


def device_split(paths):
    """one pass taken apart: seconds of host tables, kernels (device events) and everything else up to the maps"""
    import torch
    from dspnet_amd import functional as fn
    from dspnet_amd.dataset import cityscapes_labels as cl
    t0 = time.perf_counter()
    anns = [cl.load_annotation(p) for p in paths]
    polygons, images, orders = [], [], []
    for b, ann in enumerate(anns):
        for order, (xy, _) in enumerate(cl.drawn_objects(ann), 1):
            polygons.append(xy); images.append(b); orders.append(order)
    t1 = time.perf_counter()
    tables = cl.polygon_tables(polygons, images, orders, H, W, fn.polygon_wave_entries())
    t2 = time.perf_counter()
    dev = [torch.from_numpy(t).cuda() for t in tables[:3]]
    table = torch.zeros(len(polygons) + len(paths), 4, dtype=torch.int32, device="cuda")
    offs = torch.zeros(len(paths), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    owner = fn.polygon_rasterize(dev[0], dev[1], dev[2], tables[3], len(paths), H, W)
    b.record()
    fn.polygon_resolve(owner, table, offs)
    c.record()
    torch.cuda.synchronize()
    return {"parse_s": t1 - t0, "tables_s": t2 - t1, "jobs": int(tables[2].shape[0]), "edges": int(tables[0].shape[0]),
            "rasterize_ms": a.elapsed_time(b), "resolve_ms": b.elapsed_time(c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workdir", default=None)
    args = ap.parse_args()
    import torch
    from dspnet_amd.dataset import cityscapes_labels as cl
    assert torch.cuda.is_available(), "polygon_measure needs a GPU"
    with tempfile.TemporaryDirectory(dir=args.workdir) as tmp:
        paths = write_scenes(tmp, args.images)
        out_host, out_dev = os.path.join(tmp, "host"), os.path.join(tmp, "device")
        os.makedirs(out_host); os.makedirs(out_dev)
        times = {"pillow": [], "device": []}
        for r in range(args.repeats + 1):
            t = time.perf_counter()
            pillow_pass(paths, out_host)
            host_s = time.perf_counter() - t
            torch.cuda.synchronize()
            t = time.perf_counter()
            cl.write_label_images(paths, out_dir=out_dev)
            torch.cuda.synchronize()
            dev_s = time.perf_counter() - t
            if r:
                times["pillow"].append(host_s / args.images * 1e3)
                times["device"].append(dev_s / args.images * 1e3)
        same = 0
        from PIL import Image
        for p in paths:
            for kind in cl.KINDS:
                x = np.asarray(Image.open(cl.output_path(p, kind, out_host)))
                y = np.asarray(Image.open(cl.output_path(p, kind, out_dev)))
                same += int(np.array_equal(x, y))
        result = {"images": args.images, "repeats": args.repeats, "files_equal": same, "files": 4 * len(paths),
                  "split_first_8": device_split(paths[:8])}
        for k, v in times.items():
            result[k + "_ms_per_image"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(json.dumps(result))


if __name__ == "__main__":
    main()
