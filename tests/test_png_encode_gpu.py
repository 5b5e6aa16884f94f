"""PNG encode on the device (include/dspn_png_encode.h) against Pillow: the filtered stream of every case of
tests/ref_png_encode.py, alone and as one mixed batch, equals the inflated IDAT data of Pillow's file for the same pixels byte
for byte; the finished files open in Pillow and in this project's decoder with the same pixels, hold exactly IHDR, IDAT, IEND
with good CRCs, and are no larger than Pillow's beyond the bound DESIGN.md section 4 states; evaluate_net(device_png=True)
writes the files of the default path.  Pillow's streams and the device's files are computed once per module."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_png  # noqa: E402
import ref_png_encode as ref  # noqa: E402

from dspnet_amd import _lib  # noqa: E402
from dspnet_amd.dataset import png  # noqa: E402
from dspnet_amd.dataset import png_encode as pe  # noqa: E402

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")

CASES = ref.cases()
NAMES = [n for n, _ in CASES]
MODES = {1: "L", 2: "I;16", 3: "RGB"}
# File size against Pillow's for the same pixels.  The filtered bytes are equal and both sides run zlib at level 6 with
# Z_FILTERED; Pillow feeds deflate through its own output buffer, which moves a few block boundaries.  Measured on an MI355X
# host (profiles/png_device_encode.txt): 0.9917 to 1.0013 over this case list, 0.9707 to 1.0017 over 32 labelId maps of
# 1024 x 2048, 1.0017 to 1.0018 over 32 mosaics of 2048 x 4096 x 3.  The bound is that worst case, 1.0018, plus 0.005 for
# zlib builds that differ between machines, and 16 bytes for files of a few dozen bytes, where one byte is over a percent.
SIZE_RATIO_BOUND = 1.0018 + 0.005
SIZE_SLACK_BYTES = 16


def bpp_of(a):
    return 3 if a.ndim == 3 else a.itemsize


@pytest.fixture(scope="module")
def pillow_files():
    return {n: ref.pillow_file(a) for n, a in CASES}


@pytest.fixture(scope="module")
def pillow_streams(pillow_files):
    return {n: ref.idat(f) for n, f in pillow_files.items()}


@pytest.fixture(scope="module")
def device_images(gpu_device):
    return {n: torch.from_numpy(a).to(gpu_device) for n, a in CASES}


@pytest.fixture(scope="module")
def device_files(device_images):
    """the whole case list as one mixed batch"""
    return dict(zip(NAMES, pe.encode_batch([device_images[n] for n in NAMES])))


def test_pillow_takes_every_filter_over_the_case_list(pillow_streams):
    taken = {t for n, a in CASES for t in ref.filter_types(pillow_streams[n], a)}
    assert taken == {0, 1, 2, 4}
    for name, ft in ref.TIE_TYPES.items():
        assert ref.filter_types(pillow_streams[name], dict(CASES)[name])[1] == ft


@pytest.mark.parametrize("name", NAMES)
def test_filter_bytes_equal_pillow(name, device_images, pillow_streams):
    (got,) = pe.filter_batch([device_images[name]])            # a batch of one
    a = dict(CASES)[name]
    assert len(got) == pe.filtered_bytes(a.shape[1], a.shape[0], bpp_of(a)) == len(pillow_streams[name])
    assert ref.filter_types(got, a) == ref.filter_types(pillow_streams[name], a)
    assert got == pillow_streams[name]


def test_filter_bytes_of_one_mixed_batch(device_images, pillow_streams):
    """every image starts where the one before it ended: all four output alignments, formats side by side"""
    got = pe.filter_batch([device_images[n] for n in NAMES])
    assert len(got) == len(NAMES)
    for name, stream in zip(NAMES, got):
        assert stream == pillow_streams[name], name
    back = pe.filter_batch([device_images[n] for n in reversed(NAMES)])       # other offsets, the same bytes
    assert back == got[::-1]


def test_host_inputs_views_and_a_side_stream(gpu_device, device_images, pillow_streams):
    names = ["rb65_L", "rb66_I16", "rb69_RGB"]
    arrays = [dict(CASES)[n] for n in names]
    want = [pillow_streams[n] for n in names]
    assert pe.filter_batch(arrays) == want                                    # numpy arrays are uploaded
    assert pe.filter_batch([torch.from_numpy(a) for a in arrays]) == want     # host tensors too
    wide = torch.from_numpy(np.concatenate([arrays[0], arrays[0]], 1)).to(gpu_device)
    assert pe.filter_batch([wide[:, :arrays[0].shape[1]]]) == want[:1]        # a view that is not contiguous
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        assert pe.filter_batch([device_images[n] for n in names]) == want
    with pytest.raises(_lib.DspnError, match=r"float32 \(2, 2\)"):
        pe.encode_batch([device_images["rb65_L"], torch.zeros(2, 2, device=gpu_device)])


def test_files_open_in_pillow_and_in_the_device_decoder(gpu_device, device_files):
    for name, a in CASES:
        im = Image.open(io.BytesIO(device_files[name]))
        assert im.mode == MODES[bpp_of(a)] and im.size == (a.shape[1], a.shape[0]), name
        np.testing.assert_array_equal(np.asarray(im), a, err_msg=name)
    grey = [(n, a) for n, a in CASES if a.ndim == 2]
    decoded = png.decode_batch([device_files[n] for n, _ in grey], gpu_device)
    for (name, a), t in zip(grey, decoded):
        assert t.dtype == (torch.uint16 if a.dtype == np.uint16 else torch.uint8)
        np.testing.assert_array_equal(t.cpu().numpy(), a, err_msg=name)


def test_files_parse_strictly(device_files, pillow_streams):
    for name, a in CASES:
        payload = device_files[name]
        parts = list(ref_png.chunks(payload))
        kinds = [k for k, _ in parts]
        assert payload[:8] == png.SIGNATURE
        assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and len(kinds) >= 3 and set(kinds[1:-1]) == {b"IDAT"}, name
        assert b"".join([payload[:8]] + [ref_png.chunk(k, d) for k, d in parts]) == payload, name       # every CRC, no byte between
        info = png.probe(payload)                               # checks the CRCs of its own accord
        depth, colour = pe.FORMATS[bpp_of(a)]
        assert (info["width"], info["height"], info["bit_depth"], info["colour_type"], info["interlace"]) == \
            (a.shape[1], a.shape[0], depth, colour, 0), name
        assert ref.idat(payload) == pillow_streams[name], name


def test_file_sizes_stay_at_pillows(device_files, pillow_files):
    worst = 0.0
    for name in NAMES:
        mine, theirs = len(device_files[name]), len(pillow_files[name])
        print("size %-18s %8d %8d %.4f" % (name, mine, theirs, mine / theirs))
        worst = max(worst, mine / theirs)
        assert mine <= theirs * SIZE_RATIO_BOUND + SIZE_SLACK_BYTES, name
    print("worst ratio %.4f" % worst)


def test_compress_level_and_thread_count_change_no_pixel(device_images, device_files):
    names = ["noise_RGB", "dramp_L", "arange_I16"]
    batch = [device_images[n] for n in names]
    assert pe.encode_batch(batch, threads=1) == [device_files[n] for n in names]
    fast = pe.encode_batch(batch, compress_level=1, threads=3)
    for name, payload in zip(names, fast):
        assert ref.idat(payload) == ref.idat(device_files[name])


def test_batch_of_one_and_the_empty_batch(device_images, device_files, monkeypatch):
    assert pe.encode_batch([device_images["rb257_L"]]) == [device_files["rb257_L"]]

    def no_launch(*a, **k):
        raise AssertionError("an empty batch launches nothing")
    monkeypatch.setattr(pe, "filter_into", no_launch)
    assert pe.encode_batch([]) == [] and pe.filter_batch([]) == []


def test_save_pngs_and_save_maps(gpu_device, device_images, tmp_path):
    from dspnet_amd.dataset import distance_labels
    from dspnet_amd.detect import render
    names = ["rb255_RGB", "rb63_L", "noise_I16_odd"]
    paths = [str(tmp_path / (n + ".png")) for n in names]
    render.save_pngs(paths, [device_images[n] for n in names])
    for n, p in zip(names, paths):
        np.testing.assert_array_equal(np.asarray(Image.open(p)), dict(CASES)[n])
    with pytest.raises(_lib.DspnError, match="2 paths for 3 images"):
        render.save_pngs(paths[:2], [device_images[n] for n in names])
    maps = torch.stack([device_images["arange_I16"], device_images["arange_I16"].flip(0)])
    paths = [str(tmp_path / ("disparity%d.png" % i)) for i in range(2)]
    distance_labels.save_maps(paths, maps)
    for p, m in zip(paths, maps):
        im = Image.open(p)
        assert im.mode == "I;16"
        np.testing.assert_array_equal(np.asarray(im), m.cpu().numpy())
    with pytest.raises(ValueError, match="uint16"):
        distance_labels.save_maps(paths[:1], [device_images["rb63_L"]])


def test_evaluate_net_device_png_writes_the_default_paths_files(gpu_device, tmp_path):
    from dspnet_amd import synthetic
    from dspnet_amd.evaluate.multi_eval import evaluate_net
    from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
    S, B, full = 128, 2, (64, 96)
    classes = ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
    net = get_multi_symbol_train("resnet-50", S, num_classes=8, batch_size=B, device=gpu_device)
    gen = synthetic.rng(233)
    batches = [{"data": torch.from_numpy(synthetic.images(B, S, S, gen)).to(gpu_device),
                "label_det": torch.from_numpy(synthetic.det_labels(B, gen=gen, height=S, width=S)).to(gpu_device),
                "label_seg": torch.from_numpy(synthetic.seg_labels(B, S, S, gen=gen)).to(gpu_device)} for _ in range(2)]
    batches[0]["fnames"] = ["/data/SegmentationClass/aachen_000000_000019_gtFine_labelTrainIds.png",
                            "/data/SegmentationClass/aachen_000001_000019_gtFine_labelTrainIds.png"]
    seg = ["s%d" % i for i in range(19)]
    host_dir, dev_dir = tmp_path / "host", tmp_path / "device"
    base = evaluate_net(net, batches, classes, seg, full_res=full, results_dir=str(host_dir))
    out = evaluate_net(net, batches, classes, seg, full_res=full, results_dir=str(dev_dir), device_png=True)
    assert set(out) == set(base)
    for k in base:
        if k != "class_maps":
            np.testing.assert_equal(out[k], base[k], err_msg=k)                  # identical; NaN equals NaN here
    for a, b in zip(base["class_maps"], out["class_maps"]):
        assert torch.equal(a, b)
    assert sorted(os.listdir(str(dev_dir))) == sorted(os.listdir(str(host_dir))) == ["output", "results"]
    for sub, mode, shape in (("results", "L", full), ("output", "RGB", (2 * S, 2 * S, 3))):
        names = sorted(os.listdir(str(host_dir / sub)))
        assert len(names) == 2 * B and sorted(os.listdir(str(dev_dir / sub))) == names
        for name in names:
            want, got = Image.open(str(host_dir / sub / name)), Image.open(str(dev_dir / sub / name))
            assert got.mode == want.mode == mode and np.asarray(got).shape == tuple(shape)
            np.testing.assert_array_equal(np.asarray(got), np.asarray(want))
            with open(str(host_dir / sub / name), "rb") as f, open(str(dev_dir / sub / name), "rb") as g:
                assert ref.idat(g.read()) == ref.idat(f.read())                  # the same filtered stream, too
