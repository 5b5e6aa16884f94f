"""label_maps / write_label_images on the device against tests/golden/cityscapes_label_maps.npz, recorded from the
reference's createLabelImage / createInstanceImage.  The files are read back with the project's own PNG decode."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "cityscapes_polygons", "*_gtFine_polygons.json")))
KINDS = ("labelIds", "labelTrainIds", "instanceIds", "instanceTrainIds")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "cityscapes_label_maps.npz"))
    assert [str(g["file_%d" % k]) for k in range(int(g["count"]))] == [os.path.basename(f) for f in FILES]
    return g


def test_label_maps_batch_and_single(gpu_device, golden):
    import torch
    from dspnet_amd.dataset import cityscapes_labels as cl
    both = cl.label_maps(FILES[:2], gpu_device)                   # two files of one size in one call
    third = cl.label_maps([cl.load_annotation(FILES[2])], gpu_device)
    for kind in KINDS:
        dtype = torch.uint8 if kind.startswith("label") else torch.int32
        assert both[kind].dtype == third[kind].dtype == dtype and both[kind].shape == (2, 32, 48)
        for k, got in ((0, both[kind][0]), (1, both[kind][1]), (2, third[kind][0])):
            assert np.array_equal(got.cpu().numpy(), golden["%s_%d" % (kind, k)]), (kind, k)
    with pytest.raises(ValueError, match="one size"):
        cl.label_maps(FILES, gpu_device)


def test_written_files_decode_to_the_golden_maps(gpu_device, golden, tmp_path):
    from dspnet_amd.dataset import cityscapes_labels as cl
    from dspnet_amd.dataset import png
    paths = cl.write_label_images(FILES[:2], out_dir=str(tmp_path), device=gpu_device)
    paths += cl.write_label_images(FILES[2:], out_dir=str(tmp_path), kinds=KINDS[:3], device=gpu_device)
    want_names = [os.path.basename(f).replace("_polygons.json", "_%s.png" % kind)
                  for k, f in enumerate(FILES) for kind in (KINDS if k < 2 else KINDS[:3])]
    assert [os.path.basename(p) for p in paths] == want_names and sorted(os.listdir(tmp_path)) == sorted(want_names)
    payloads = []
    for p in paths:
        with open(p, "rb") as f:
            payloads.append(f.read())
    decoded = png.decode_batch(payloads, gpu_device)
    for p, image in zip(paths, decoded):
        stem, kind = os.path.basename(p)[:-4].rsplit("_", 1)
        k = [os.path.basename(f) for f in FILES].index(stem + "_polygons.json")
        a = image.cpu().numpy()
        assert a.dtype == (np.uint8 if kind.startswith("label") else np.uint16), (p, a.dtype)
        assert np.array_equal(a.astype(np.int32), golden["%s_%d" % (kind, k)].astype(np.int32)), p


def test_instance_train_ids_beyond_16_bits_raise(gpu_device, golden, tmp_path):
    """a caravan / trailer that is no group has trainId 255, so its instanceTrainId is 255000 + n: no 16-bit file"""
    from dspnet_amd.dataset import cityscapes_labels as cl
    assert golden["instanceTrainIds_2"].max() > 65535
    with pytest.raises(ValueError, match="16-bit"):
        cl.write_label_images(FILES[2:], out_dir=str(tmp_path), kinds=("instanceTrainIds",), device=gpu_device)
    assert os.listdir(tmp_path) == []
