"""The deflate of the PNG encode on the device (dspn_png_deflate_batch) against the host encoder that runs the same rule text:
every stream of tests/png_deflate_cases.py, alone and as one batch in both orders, equals deflate_host's byte for byte and
inflates to its input; nothing beyond the reported sizes is written.  encode_batch(device_deflate=True) writes strict files with
the pixels and the filtered stream of the default path, which itself still writes the bytes it wrote before; save_pngs and
evaluate_net pass the keyword through.  The host streams are computed once per module."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
Image = pytest.importorskip("PIL.Image")
import png_deflate_cases as pc  # noqa: E402
import ref_png  # noqa: E402
import ref_png_encode as ref  # noqa: E402

from dspnet_amd import _lib  # noqa: E402
from dspnet_amd.dataset import png  # noqa: E402
from dspnet_amd.dataset import png_encode as pe  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = pc.cases()
NAMES = [n for n, _ in CASES]
IMAGES = ref.cases()
MODES = {1: "L", 2: "I;16", 3: "RGB"}


@pytest.fixture(scope="module")
def host_streams():
    return {n: pe.deflate_host(d) for n, d in CASES}


@pytest.fixture(scope="module")
def device_streams(gpu_device):
    return {n: torch.frombuffer(bytearray(d), dtype=torch.uint8).to(gpu_device) for n, d in CASES}


@pytest.fixture(scope="module")
def device_images(gpu_device):
    return {n: torch.from_numpy(a).to(gpu_device) for n, a in IMAGES}


@pytest.fixture(scope="module")
def deflated_files(device_images):
    """the image case list as one mixed batch through the device deflate"""
    return dict(zip([n for n, _ in IMAGES], pe.encode_batch([device_images[n] for n, _ in IMAGES], device_deflate=True)))


@pytest.mark.parametrize("name", NAMES)
def test_one_stream_equals_the_host_encoder(name, device_streams, host_streams):
    (got,) = pe.deflate_batch([device_streams[name]])
    assert got == host_streams[name]
    assert pc.inflate_strictly(got) == dict(CASES)[name]


def test_one_batch_in_both_orders(device_streams, host_streams):
    """streams lie back to back in the output: the two orders put their starts at every alignment"""
    got = pe.deflate_batch([device_streams[n] for n in NAMES])
    assert len(got) == len(NAMES)
    for name, z in zip(NAMES, got):
        assert z == host_streams[name], name
    back = pe.deflate_batch([device_streams[n] for n in reversed(NAMES)])
    assert back == got[::-1]
    starts = np.cumsum([0] + [len(z) for z in got[:-1]]), np.cumsum([0] + [len(z) for z in back[:-1]])
    assert {int(s) % 4 for s in starts[0]} | {int(s) % 4 for s in starts[1]} == {0, 1, 2, 3}


def test_host_inputs_are_uploaded(host_streams):
    names = ["runs_257_to_263", "block_plus_1", "fibonacci"]
    d = dict(CASES)
    want = [host_streams[n] for n in names]
    assert pe.deflate_batch([d[n] for n in names]) == want                                         # bytes
    assert pe.deflate_batch([np.frombuffer(d[n], np.uint8) for n in names]) == want                 # arrays
    assert pe.deflate_batch([]) == []
    with pytest.raises(_lib.DspnError, match="stream 1: .*at least one byte"):
        pe.deflate_batch([b"\x01", b""])


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_nothing_beyond_the_streams_is_written(lead, gpu_device, device_streams, host_streams):
    """the C entry point with pools at every alignment: the bytes in front of `out`, behind the last stream and in a guard band
    behind the pool keep their pattern; an input pool with the spans out of order and bytes between them"""
    names = ["zeros_noise_zeros", "one_byte", "runs_257_to_263", "block_plus_1", "png_rb65_L"]
    d = dict(CASES)
    gap, guard = 5, 64
    spans, parts, at = [], [], lead
    for n in reversed(names):                                   # the pool holds them in the other order
        parts += [torch.full((at - sum(p.numel() for p in parts),), 0xA5, dtype=torch.uint8, device=gpu_device), device_streams[n]]
        spans.insert(0, (at, len(d[n])))
        at += len(d[n]) + gap
    pool = torch.cat(parts)
    bound = sum(pe.deflate_bound(len(d[n])) for n in names)
    whole = torch.full((lead + bound + guard,), 0x5A, dtype=torch.uint8, device=gpu_device)
    out = whole[lead:lead + bound]
    result = torch.zeros(2 * len(names), dtype=torch.int64, device=gpu_device)
    ws = pe.deflate_into(spans, pool, out, result)
    torch.cuda.synchronize(gpu_device)
    del ws
    placed = result.cpu().numpy().reshape(-1, 2)
    host = whole.cpu().numpy()
    at = 0
    for n, (o, size) in zip(names, placed):
        assert o == at and host[lead + o:lead + o + size].tobytes() == host_streams[n], n
        at += size
    assert (host[:lead] == 0x5A).all() and (host[lead + at:] == 0x5A).all()


def test_files_of_the_device_deflate(gpu_device, device_images, deflated_files):
    for name, a in IMAGES:
        payload = deflated_files[name]
        bpp = 3 if a.ndim == 3 else a.itemsize
        im = Image.open(io.BytesIO(payload))
        assert im.mode == MODES[bpp] and im.size == (a.shape[1], a.shape[0]), name
        np.testing.assert_array_equal(np.asarray(im), a, err_msg=name)
        parts = list(ref_png.chunks(payload))
        assert payload[:8] == png.SIGNATURE and [k for k, _ in parts] == [b"IHDR", b"IDAT", b"IEND"], name
        assert b"".join([payload[:8]] + [ref_png.chunk(k, d) for k, d in parts]) == payload, name       # every CRC, no byte between
    filtered = pe.filter_batch([device_images[n] for n, _ in IMAGES])
    for (name, _), stream in zip(IMAGES, filtered):
        idat = dict(ref_png.chunks(deflated_files[name]))[b"IDAT"]
        assert zlib.decompress(idat) == stream, name
        assert idat == pe.deflate_host(stream), name
    grey = [(n, a) for n, a in IMAGES if a.ndim == 2]
    decoded = png.decode_batch([deflated_files[n] for n, _ in grey], gpu_device)
    for (name, a), t in zip(grey, decoded):
        np.testing.assert_array_equal(t.cpu().numpy(), a, err_msg=name)
    colour = [(n, a) for n, a in IMAGES if a.ndim == 3]
    decoded = png.decode_rgb_batch([deflated_files[n] for n, _ in colour], gpu_device)
    for (name, a), t in zip(colour, decoded):
        np.testing.assert_array_equal(t.cpu().numpy().reshape(a.shape), a, err_msg=name)


def test_default_path_writes_the_bytes_it_wrote(device_images, deflated_files):
    names = [n for n, _ in IMAGES]
    batch = [device_images[n] for n in names]
    filtered = pe.filter_batch(batch)
    want = [pe.assemble(f, a.shape[1], a.shape[0], 3 if a.ndim == 3 else a.itemsize) for f, (_, a) in zip(filtered, IMAGES)]
    assert pe.encode_batch(batch) == want
    assert pe.encode_batch(batch, device_deflate=False, threads=1) == want
    some = ["noise_RGB", "dramp_L", "arange_I16"]
    assert pe.encode_batch([device_images[n] for n in some], device_deflate=True, threads=1, compress_level=1) == [deflated_files[n] for n in some]
    assert pe.encode_batch([], device_deflate=True) == []


def test_save_pngs_and_save_maps_pass_the_keyword(gpu_device, device_images, deflated_files, tmp_path):
    from dspnet_amd.dataset import distance_labels
    from dspnet_amd.detect import render
    names = ["rb255_RGB", "rb63_L", "noise_I16_odd"]
    plain = [str(tmp_path / (n + ".png")) for n in names]
    deflated = [str(tmp_path / (n + "_device.png")) for n in names]
    render.save_pngs(plain, [device_images[n] for n in names])
    render.save_pngs(deflated, [device_images[n] for n in names], device_deflate=True)
    for n, p, q in zip(names, plain, deflated):
        np.testing.assert_array_equal(np.asarray(Image.open(q)), np.asarray(Image.open(p)))
        with open(q, "rb") as f:
            assert f.read() == deflated_files[n]
    maps = torch.stack([device_images["arange_I16"], device_images["arange_I16"].flip(0)])
    paths = [str(tmp_path / ("disparity%d.png" % i)) for i in range(2)]
    distance_labels.save_maps(paths, maps, device_deflate=True)
    for p, m in zip(paths, maps):
        im = Image.open(p)
        assert im.mode == "I;16"
        np.testing.assert_array_equal(np.asarray(im), m.cpu().numpy())
    with open(paths[0], "rb") as f:
        assert f.read() == deflated_files["arange_I16"]


def test_evaluate_net_device_deflate_writes_the_same_pixels(gpu_device, tmp_path):
    """the setup of tests/test_png_encode_gpu.py's evaluation test"""
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
    with pytest.raises(ValueError, match="device_deflate=True needs device_png=True"):
        evaluate_net(net, batches, classes, seg, full_res=full, results_dir=str(tmp_path / "none"), device_deflate=True)
    base_dir, dev_dir = tmp_path / "filtered", tmp_path / "deflated"
    base = evaluate_net(net, batches, classes, seg, full_res=full, results_dir=str(base_dir), device_png=True)
    out = evaluate_net(net, batches, classes, seg, full_res=full, results_dir=str(dev_dir), device_png=True, device_deflate=True)
    assert set(out) == set(base)
    for k in base:
        if k != "class_maps":
            np.testing.assert_equal(out[k], base[k], err_msg=k)                  # identical; NaN equals NaN here
    for a, b in zip(base["class_maps"], out["class_maps"]):
        assert torch.equal(a, b)
    assert sorted(os.listdir(str(dev_dir))) == sorted(os.listdir(str(base_dir))) == ["output", "results"]
    for sub, mode in (("results", "L"), ("output", "RGB")):
        names = sorted(os.listdir(str(base_dir / sub)))
        assert len(names) == 2 * B and sorted(os.listdir(str(dev_dir / sub))) == names
        for name in names:
            want, got = Image.open(str(base_dir / sub / name)), Image.open(str(dev_dir / sub / name))
            assert got.mode == want.mode == mode
            np.testing.assert_array_equal(np.asarray(got), np.asarray(want))
            with open(str(base_dir / sub / name), "rb") as f, open(str(dev_dir / sub / name), "rb") as g:
                theirs, mine = f.read(), g.read()
            assert ref.idat(mine) == ref.idat(theirs)                            # the same filtered stream
            assert dict(ref_png.chunks(mine))[b"IDAT"] == pe.deflate_host(ref.idat(theirs))
