"""The annotation rules of the Cityscapes preparation scripts and cs_json2xml.py's boxes (dataset/cityscapes_labels.py)
against tests/golden/cityscapes_label_maps.npz, recorded from the reference's own createLabelImage / createInstanceImage
(tests/golden/make_cityscapes_label_maps_golden.py).  The maps are painted here with the host restatement of the fill
rule; the device paints them in tests/test_cityscapes_labels_gpu.py."""
import glob
import json
import os

import numpy as np
import pytest

import ref_polygon as rp
from dspnet_amd.dataset import cityscapes_labels as cl

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "cityscapes_polygons", "*_gtFine_polygons.json")))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "cityscapes_label_maps.npz"))
    assert int(g["count"]) == len(FILES) == 3
    assert [str(g["file_%d" % k]) for k in range(len(FILES))] == [os.path.basename(f) for f in FILES]
    return g


def host_maps(ann):
    H, W = ann["imgHeight"], ann["imgWidth"]
    drawn = cl.drawn_objects(ann)
    out = {}
    for c, (kind, background) in enumerate(zip(cl.KINDS, (0, 255, 0, 255))):
        out[kind] = rp.paint(H, W, [(xy, v[c]) for xy, v in drawn], background=background)
    return out


@pytest.mark.parametrize("k", range(3))
def test_rules_reproduce_the_reference_maps(golden, k):
    maps = host_maps(cl.load_annotation(FILES[k]))
    for kind in cl.KINDS:
        assert np.array_equal(maps[kind], golden["%s_%d" % (kind, k)].astype(np.int32)), (FILES[k], kind)


@pytest.mark.parametrize("k", range(3))
def test_polygon_boxes(golden, k):
    got = cl.polygon_boxes(FILES[k])
    assert [got["width"], got["height"]] == golden["size_%d" % k].tolist()
    assert [list(b[1:]) for b in got["boxes"]] == golden["boxes_%d" % k].tolist()
    with open(FILES[k]) as f:
        d = json.load(f)
    assert [b[0] for b in got["boxes"]] == [o["label"] for o in d["objects"]]
    assert cl.polygon_boxes(d) == got


def test_polygon_boxes_arithmetic():
    d = {"imgWidth": 2047, "imgHeight": 1025, "objects": [
        {"label": "car", "polygon": [[3, 5], [7, 9], [-3, 1]]},                 # Python 2: 3 / 2 == 1, -3 / 2 == -2
        {"label": "car", "polygon": [[3.0, 5.0], [7.0, 2.5], [-3.0, 1.0]]},     # round(1.5) == 2, round(-1.5) == -2, round(1.25) == 1
        {"label": "sky", "polygon": []},
        {"label": "sky", "polygon": [[5000, 4000]]},                             # extents start from the size and from 0
    ]}
    got = cl.polygon_boxes(d)
    assert (got["width"], got["height"]) == (1023, 512)
    assert got["boxes"] == [("car", -2, 0, 3, 4), ("car", -2, 1, 4, 3), ("sky", 1023, 512, 0, 0), ("sky", 1023, 512, 2500, 2000)]


def test_load_annotation_truncates_and_reads_deleted():
    ann = cl.load_annotation({"imgWidth": "48", "imgHeight": 32.0, "objects": [
        {"label": "car", "polygon": [[1.9, -0.9], [5.5, 6.99]], "deleted": 1},
        {"label": "road", "polygon": [[1, 2]]}]})
    assert ann == {"imgWidth": 48, "imgHeight": 32, "objects": [
        {"label": "car", "polygon": [(1, 0), (5, 6)], "deleted": True},
        {"label": "road", "polygon": [(1, 2)], "deleted": False}]}
    assert cl.load_annotation(ann) == ann


def _ann(*labels, deleted=()):
    tri = [(1, 1), (9, 2), (4, 8)]
    return {"imgWidth": 12, "imgHeight": 10,
            "objects": [{"label": l, "polygon": tri, "deleted": i in deleted} for i, l in enumerate(labels)]}


def test_instance_numbering_groups_and_skips():
    drawn = cl.drawn_objects(_ann("car", "person", "car", "cargroup", "car", "license plate", "road", "polegroup",
                                  "caravan", "trailergroup", "car", deleted=(2,)))
    assert [v for _, v in drawn] == [
        (26, 13, 26000, 13000), (24, 11, 24000, 11000), (26, 13, 26, 13), (26, 13, 26001, 13001), (7, 0, 7, 0),
        (18, 255, 18, 255), (29, 255, 29000, 255000), (30, 255, 30, 255), (26, 13, 26002, 13002)]


def test_unknown_label_is_named():
    with pytest.raises(ValueError, match="'spaceship'"):
        cl.drawn_objects(_ann("car", "spaceship"))
    with pytest.raises(ValueError, match="'spaceship'"):
        cl.drawn_objects(_ann("spaceshipgroup"))
    assert cl.drawn_objects(_ann("spaceship", deleted=(0,))) == []


def test_output_names():
    p = "/data/gtFine/train/aachen/aachen_000000_000019_gtFine_polygons.json"
    assert cl.output_path(p, "labelTrainIds") == "/data/gtFine/train/aachen/aachen_000000_000019_gtFine_labelTrainIds.png"
    assert cl.output_path(p, "instanceIds", "/out") == "/out/aachen_000000_000019_gtFine_instanceIds.png"
