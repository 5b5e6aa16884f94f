"""Device half of the JPEG decode (dspn_jpeg_reconstruct_batch_u8) and the iterator switch device_jpeg=True: the pixels equal
Pillow's byte for byte over the matrix of tests/jpeg_cases.py, nothing is written outside a sample's output, and the
iterator yields the same batches either way."""
import io
import os

import numpy as np
import pytest

import jpeg_cases as jc
from dspnet_amd import _lib
from dspnet_amd.dataset import iterator as it
from dspnet_amd.dataset import jpeg as dj
from dspnet_amd.dataset import recordio


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(3))
def test_decode_batch_equals_pillow(gpu_device, part):
    """three batched calls, each a third of the matrix dealt round-robin: every call mixes all sizes, the three chroma
    layouts, greyscale and restart streams, so many img_offsets (odd ones included) meet in one launch"""
    import torch
    names = [c[0] for c in jc.CASES][part::3]
    assert len(names) > 90
    if part == 0:
        assert "16x16-ss2-rstblocks1" in [c[0] for c in jc.CASES]
    payloads = [jc.stream(n) for n in names]
    got = dj.decode_batch(payloads, gpu_device)
    assert len(got) == len(names)
    for name, data, g in zip(names, payloads, got):
        want = torch.from_numpy(jc.pillow_pixels(data).copy())
        assert g.dtype == torch.uint8 and tuple(g.shape) == tuple(want.shape), name
        assert torch.equal(g.cpu(), want), name


@pytest.mark.gpu
def test_restart_interval_one(gpu_device):
    import torch
    data = jc.stream("16x16-ss2-rstblocks1")
    assert dj.probe(data)["restart_interval"] == 1 and dj.probe(data)["hsamp"][0] == 2 and dj.probe(data)["vsamp"][0] == 2
    (got,) = dj.decode_batch([data], gpu_device)
    assert torch.equal(got.cpu(), torch.from_numpy(jc.pillow_pixels(data).copy()))


@pytest.mark.gpu
def test_decode_batch_names_the_reason(gpu_device):
    progressive = jc.encode(jc.image(1, 24, 24, "smooth"), progressive=True)
    with pytest.raises(ValueError, match="progressive"):
        dj.decode_batch([jc.stream("8x8-ss0-q90-std-smooth"), progressive], gpu_device)


def _low_level_batch(names, skip, dev, guard=64, spoil=None):
    """one dspn_jpeg_reconstruct_batch_u8 call with `guard` bytes of 0xA5 around every sample's output -> (pool, regions)"""
    return jc.low_level_batch([jc.stream(n) for n in names], skip, dev, guard, spoil)


@pytest.mark.gpu
def test_guard_bytes_and_skip(gpu_device):
    names = ["17x33-ss2-q90-std-noise", "1x1-ss2-q90-std-smooth", "37x53-ss1-q100-opt-noise", "50x31-grey-q90-noise",
             "64x200-ss0-q30-std-smooth", "50x31-ss2-q90-opt-smooth", "16x16-ss2-rstblocks1"]
    skip = {2}
    pool, regions = _low_level_batch(names, skip, gpu_device)
    covered = np.zeros(pool.size, bool)
    for k, (name, (at, n)) in enumerate(zip(names, regions)):
        covered[at:at + n] = True
        if k in skip:
            assert (pool[at:at + n] == 0xA5).all(), "a skipped sample's region was written"
        else:
            np.testing.assert_array_equal(pool[at:at + n], jc.pillow_pixels(jc.stream(name)).reshape(-1), err_msg=name)
    assert (pool[~covered] == 0xA5).all() and (~covered).sum() == 2 * 64 * len(names)


@pytest.mark.gpu
def test_untrustworthy_descriptors_write_nothing(gpu_device):
    """offsets and grids that would index outside the coefficient pool, a component plane or the output pool: the
    sample is left alone (like skip), its neighbours are decoded"""
    names = ["17x33-ss2-q90-std-noise", "37x53-ss1-q90-std-noise", "50x31-ss0-q90-std-noise", "16x16-ss2-q90-std-noise",
             "8x8-grey-q90-noise", "64x200-ss2-q90-std-smooth"]

    def spoil(s):
        s[0]["coef_offset"][2] = 1 << 40                        # past the coefficient pool
        s[1]["blocks_w"][1] = 1                                 # a chroma grid narrower than the image needs
        s[2]["img_offset"] = (1 << 31) + 5                      # past the output pool
        s[3]["hsamp"] = 3                                       # not a supported layout
        s[4]["coef_offset"][0] = -64

    pool, regions = _low_level_batch(names, set(), gpu_device, spoil=spoil)
    for k, (name, (at, n)) in enumerate(zip(names, regions)):
        if k < 5:
            assert (pool[at:at + n] == 0xA5).all(), name
        else:
            np.testing.assert_array_equal(pool[at:at + n], jc.pillow_pixels(jc.stream(name)).reshape(-1), err_msg=name)
    assert (pool[:64] == 0xA5).all() and (pool[-64:] == 0xA5).all()


@pytest.mark.gpu
def test_reconstruct_argument_checks(gpu_device):
    import torch
    lib = _lib.lib()
    t = torch.zeros(1024, dtype=torch.uint8, device=gpu_device)
    p = t.data_ptr()
    assert lib.dspn_jpeg_reconstruct_workspace_bytes(640) >= 640 and lib.dspn_jpeg_reconstruct_workspace_bytes(0) == 0
    assert lib.dspn_jpeg_reconstruct_batch_u8(p, 64, p, 0, p, 64, p, 64, None) == -1            # B
    assert lib.dspn_jpeg_reconstruct_batch_u8(p, 64, p, 2000, p, 64, p, 64, None) == -1
    assert lib.dspn_jpeg_reconstruct_batch_u8(p, 65, p, 1, p, 64, p, 65, None) == -1            # whole blocks
    assert lib.dspn_jpeg_reconstruct_batch_u8(p, 128, p, 1, p, 64, p, 64, None) == -2 and b"workspace" in lib.dspn_last_error()
    assert lib.dspn_jpeg_reconstruct_batch_u8(p + 2, 64, p, 1, p, 64, p, 64, None) == -1 and b"aligned" in lib.dspn_last_error()


SIZES = [(96, 160)] * 4 + [(128, 192)] * 4                     # per record: every staging pool grows once after its first use


def _write_dataset(root, n, g, progressive=(2,), sizes=SIZES, boxes=(0, 1, 3, 5, 2, 4, 1, 6)):
    """as tests/test_record_iter.py::_write_dataset, with the records of `progressive` re-encoded progressive, record 5
    greyscale and a size per record"""
    from PIL import Image
    os.makedirs(os.path.join(root, "cityscapes", "SegmentationClass"), exist_ok=True)
    rec = recordio.MXIndexedRecordIO(os.path.join(root, "train.idx"), os.path.join(root, "train.rec"), "w")
    lines = []
    for i in range(n):
        hw = sizes[i]
        yy, xx = np.mgrid[:hw[0], :hw[1]]
        chans = [127 + 100 * np.sin(xx / g.uniform(5, 15) + g.uniform(0, 3)) * np.cos(yy / g.uniform(5, 15)) for _ in range(3)]
        img = np.clip(np.stack(chans, -1) + g.normal(0, 6, hw + (3,)), 0, 255).astype(np.uint8)
        rows = np.full((10, 6), -1.0)
        for k in range(boxes[i % len(boxes)]):
            x0, y0 = g.uniform(0, .8), g.uniform(0, .8)
            rows[k] = [g.integers(0, 8), x0, y0, x0 + g.uniform(.01, .3), y0 + g.uniform(.01, .3), g.uniform(0, 1)]
        label = np.array([2, 6] + rows.reshape(-1).tolist(), np.float32)
        header = recordio.IRHeader(0, label, i, 0)
        if i in progressive or i == 5:
            buf = io.BytesIO()
            picture = img[:, :, 1] if i == 5 else img[:, :, ::-1]
            Image.fromarray(picture.copy()).save(buf, format="JPEG", quality=92, progressive=i in progressive)
            rec.write_idx(i, recordio.pack(header, buf.getvalue()))
        else:
            rec.write_idx(i, recordio.pack_img(header, img, quality=92))
        seg = g.integers(0, 19, hw).astype(np.uint8)
        seg[g.random(hw) < .1] = 255
        seg[:4, :4] = 40
        Image.fromarray(seg).save(os.path.join(root, "cityscapes", "SegmentationClass", "city_%06d_gtFine_labelTrainIds.png" % i))
        lines.append("%d\tJPEGImages/city_%06d_leftImg8bit.jpg\n" % (i, i))
    rec.close()
    with open(os.path.join(root, "train.lst"), "w") as f:
        f.writelines(lines)
    return os.path.join(root, "train.rec")


@pytest.fixture(scope="module")
def record_file(tmp_path_factory):
    return _write_dataset(str(tmp_path_factory.mktemp("jpeg_records")), 8, np.random.Generator(np.random.PCG64(17)))


@pytest.fixture(scope="module")
def progressive_record_file(tmp_path_factory):
    """all eight records progressive: no batch has anything for the device"""
    return _write_dataset(str(tmp_path_factory.mktemp("jpeg_records_progressive")), 8,
                          np.random.Generator(np.random.PCG64(18)), progressive=range(8))


def _same_batches(gpu_device, record_file, enable_aug, prefetch, fallbacks):
    import torch
    kw = dict(enable_aug=enable_aug, prefetch=prefetch, device=gpu_device)
    a = it.MultiTaskRecordIter(record_file, 4, (3, 64, 128), **kw)
    b = it.MultiTaskRecordIter(record_file, 4, (3, 64, 128), device_jpeg=True, **kw)
    assert a.device_jpeg is False and a.jpeg_fallbacks == 0 and b.jpeg_fallbacks == 0
    seen = 0
    for epoch in range(2):
        while a.iter_next():
            (ba, fa), (bb, fb) = a.next(), b.next()
            assert fa == fb
            assert torch.equal(ba.data[0], bb.data[0])
            assert torch.equal(ba.label[0], bb.label[0]) and torch.equal(ba.label[1], bb.label[1])
            seen += 4
        assert not b.iter_next()
        a.reset(); b.reset()
    assert seen == 16
    assert b.jpeg_fallbacks == fallbacks and a.jpeg_fallbacks == 0


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("enable_aug", [True, False])
def test_iterator_device_jpeg_yields_the_same_batches(gpu_device, record_file, enable_aug, prefetch):
    _same_batches(gpu_device, record_file, enable_aug, prefetch, fallbacks=2)    # the progressive record, once per epoch


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [True, False])
def test_iterator_device_jpeg_all_fallback_batches(gpu_device, progressive_record_file, prefetch):
    """the pixels go up directly and nothing JPEG-related is uploaded or launched: 8 fallbacks per epoch"""
    _same_batches(gpu_device, progressive_record_file, True, prefetch, fallbacks=16)


def test_device_jpeg_refuses_the_decoded_cache(tmp_path):
    """the refusal comes before any file is opened or any device touched"""
    with pytest.raises(ValueError, match="cache_decoded"):
        it.MultiTaskRecordIter(str(tmp_path / "none.rec"), 4, (3, 64, 128), device_jpeg=True, cache_decoded=True)
