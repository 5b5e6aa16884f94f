"""Generates tests/golden/cityscapes_label_maps.npz and tests/golden/polygon_street_scene.npz.

cityscapes_label_maps.npz: what the REFERENCE's own preparation functions -- createLabelImage of
data/cityscapes/Scripts/preparation/json2labelImg.py and createInstanceImage of json2instanceImg.py, imported unmodified
from the reference checkout at generation time -- paint for the synthetic polygon files under
tests/golden/cityscapes_polygons/, for the encodings "ids" and "trainIds"; and the <size> / <bndbox> numbers of
dataset/cs_json2xml.py.  That script is Python 2 and does its work in main() while writing a file, so its arithmetic
(lines 38 and 65-75) is restated below with Python 2's `/` and round() spelled out.

polygon_street_scene.npz: the polygons of tests/ref_polygon.py's street_scene(20261020) and the owner map that
PIL.ImageDraw.polygon paints for them into a mode "I" image, polygon k with fill k + 1.

Run with:  python tests/golden/make_cityscapes_label_maps_golden.py [path of the reference checkout, default /root/reference]

`PIL.PILLOW_VERSION` -- the alias of `PIL.__version__` that Pillow < 7 exported and both scripts import to check that
PIL is Pillow -- is restored before the import; nothing else about Pillow is touched."""
import glob
import json
import math
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

PIL.PILLOW_VERSION = PIL.__version__
sys.path.insert(0, os.path.join(REFERENCE, "data", "cityscapes", "Scripts", "preparation"))
import json2labelImg as j2l            # noqa: E402  (the reference's scripts)
import json2instanceImg as j2i         # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import ref_polygon                     # noqa: E402


def py2_round(v):
    a = math.floor(abs(v))
    if abs(v) - a >= 0.5:
        a += 1
    return math.copysign(a, v)


def py2_half(v):
    return int(py2_round(v // 2 if isinstance(v, int) else v / 2))


def boxes(parsed):
    ncols, nrows = py2_half(parsed["imgWidth"]), py2_half(parsed["imgHeight"])
    rows = []
    for label in parsed["objects"]:
        xminval, xmaxval, yminval, ymaxval = ncols, 0, nrows, 0
        for p in label["polygon"]:
            x, y = py2_half(p[0]), py2_half(p[1])
            xminval, xmaxval, yminval, ymaxval = min(xminval, x), max(xmaxval, x), min(yminval, y), max(ymaxval, y)
        rows.append((xminval, yminval, xmaxval, ymaxval))
    return np.asarray([ncols, nrows], np.int64), np.asarray(rows, np.int64).reshape(-1, 4)


def main():
    out = {}
    files = sorted(glob.glob(os.path.join(HERE, "cityscapes_polygons", "*_gtFine_polygons.json")))
    for k, path in enumerate(files):
        ann = j2l.Annotation()
        ann.fromJsonFile(path)
        out["file_%d" % k] = np.array(os.path.basename(path))
        out["labelIds_%d" % k] = np.array(j2l.createLabelImage(ann, "ids")).astype(np.uint8)
        out["labelTrainIds_%d" % k] = np.array(j2l.createLabelImage(ann, "trainIds")).astype(np.uint8)
        out["instanceIds_%d" % k] = np.array(j2i.createInstanceImage(ann, "ids")).astype(np.int32)
        out["instanceTrainIds_%d" % k] = np.array(j2i.createInstanceImage(ann, "trainIds")).astype(np.int32)
        with open(path) as f:
            out["size_%d" % k], out["boxes_%d" % k] = boxes(json.load(f))
        print(os.path.basename(path), out["labelIds_%d" % k].shape, "instance ids", np.unique(out["instanceIds_%d" % k]).tolist())
    out["count"] = np.int64(len(files))
    out["pillow_version"] = np.array(PIL.__version__)
    dst = os.path.join(HERE, "cityscapes_label_maps.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")

    H, W = 1024, 2048
    polys = ref_polygon.street_scene(20261020, H, W)
    im = Image.new("I", (W, H), 0)
    draw = ImageDraw.Draw(im)
    for k, xy in enumerate(polys):
        draw.polygon(xy, fill=k + 1)
    dst = os.path.join(HERE, "polygon_street_scene.npz")
    np.savez_compressed(dst, points=np.concatenate([np.asarray(p, np.int32) for p in polys]),
                        counts=np.asarray([len(p) for p in polys], np.int32), owner=np.array(im).astype(np.uint8 if len(polys) < 256 else np.int32),
                        pillow_version=np.array(PIL.__version__))
    print("wrote", dst, len(polys), "polygons,", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
