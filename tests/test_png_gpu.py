"""Device half of the PNG decode (dspn_png_unfilter_batch) and the iterator switch device_png=True: the samples equal Pillow's
byte for byte at the sizes where the kernel changes path (wave and band boundaries, dword fetch and store edges, both byte
widths, every filter type), nothing is written outside an image's output, and the iterator yields the same batches either
way."""
import io
import os

import numpy as np
import pytest

import ref_png as rp
from dspnet_amd import _lib
from dspnet_amd.dataset import iterator as it
from dspnet_amd.dataset import png as dp
from dspnet_amd.dataset import recordio

HEIGHTS = (1, 2, 63, 64, 65, 129)
WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257)
KINDS = (0, 1, 2, 3, 4, "mix")
_cache = {}


def cases():
    """[(name, payload, Pillow's samples)], built once: every width x byte width x filter kind with the heights dealt round,
    every height x byte width x filter kind with the widths dealt round, and heights past the 1024 rows one workgroup covers
    at a time (the band hand-over: once and twice), random bytes throughout; one palette stream"""
    if "cases" in _cache:
        return _cache["cases"]
    g = np.random.Generator(np.random.PCG64(77))
    shapes, k = [], 0
    for w in WIDTHS:
        for bpp in (1, 2):
            for kind in KINDS:
                shapes.append((HEIGHTS[k % len(HEIGHTS)], w, bpp, kind)); k += 1
    for h in HEIGHTS:
        for bpp in (1, 2):
            for kind in KINDS:
                shapes.append((h, WIDTHS[k % len(WIDTHS)], bpp, kind)); k += 5
    shapes += [(1030, 5, 1, "mix"), (1030, 5, 2, "mix"), (1030, 5, 1, 4), (1030, 5, 2, 3), (1025, 1, 1, 2), (1024, 3, 2, 4),
               (2050, 3, 1, "mix"), (2050, 2, 2, "mix")]
    out = []
    for h, w, bpp, kind in shapes:
        data = rp.write(rp.random_image(g, h, w, bpp), rp.filters_for(g, h, kind), idat_chunks=1 + len(out) % 3)
        out.append(("%dx%d-b%d-%s" % (h, w, bpp, kind), data, rp.pillow(data)))
    data = rp.write(g.integers(0, 256, (66, 18), dtype=np.uint8), rp.filters_for(g, 66, "mix"), palette=True)
    out.append(("66x18-palette-mix", data, rp.pillow(data)))
    _cache["cases"] = out
    return out


def _low_level_batch(picked, skip, dev, guard=61, spoil=None):
    """one dspn_png_unfilter_batch call with `guard` bytes of 0xA5 around every image's output (and as many unused bytes
    between the images' raw rows, so raw and output offsets take every alignment) -> (pool, [(offset, bytes)])"""
    import torch
    infos = [dp.probe(data) for _, data, _ in picked]
    samples = np.zeros(len(picked), dp.SAMPLE)
    raw = np.full(sum(i["raw_bytes"] + guard for i in infos) + guard, 0x5A, np.uint8)
    ro, oo, regions = 0, 0, []
    for k, ((name, data, _), info) in enumerate(zip(picked, infos)):
        ro += guard
        oo += guard
        assert info["supported"] and dp.inflate_into(data, info, raw[ro:ro + info["raw_bytes"]]) == 0, name
        dp.fill_sample(samples[k], info, ro, oo, skip=int(k in skip))
        n = info["height"] * info["row_bytes"]
        regions.append((oo, n))
        ro += info["raw_bytes"]
        oo += n
    oo += guard
    if spoil:
        spoil(samples)
    pool = torch.full((oo,), 0xA5, dtype=torch.uint8, device=dev)
    desc = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
    dp.unfilter(torch.from_numpy(raw).to(dev), desc, pool)
    torch.cuda.synchronize(dev)
    return pool.cpu().numpy(), regions


def _samples(pool, at, n, want):
    got = np.frombuffer(pool[at:at + n].tobytes(), "<u2" if want.dtype == np.uint16 else np.uint8)
    return got.reshape(want.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(3))
def test_unfilter_equals_pillow(gpu_device, part):
    """three batched calls, each a third of the matrix dealt round-robin, so every call mixes sizes, byte widths and filter
    types; 16-bit outputs are compared as uint16 values (the byte order), the guards around every output are intact"""
    picked = cases()[part::3]
    assert len(picked) > 70
    pool, regions = _low_level_batch(picked, set(), gpu_device)
    covered = np.zeros(pool.size, bool)
    for (name, _, want), (at, n) in zip(picked, regions):
        covered[at:at + n] = True
        np.testing.assert_array_equal(_samples(pool, at, n, want), want, err_msg=name)
    assert (pool[~covered] == 0xA5).all() and (~covered).sum() == 61 * (len(picked) + 1)


@pytest.mark.gpu
def test_guard_bytes_and_skip(gpu_device):
    picked = [c for c in cases() if c[0] in ("1030x5-b1-mix", "1030x5-b2-mix", "66x18-palette-mix")] + cases()[:9]
    assert len(picked) == 12
    skip = {1, 5}
    pool, regions = _low_level_batch(picked, skip, gpu_device, guard=64)
    covered = np.zeros(pool.size, bool)
    for k, ((name, _, want), (at, n)) in enumerate(zip(picked, regions)):
        covered[at:at + n] = True
        if k in skip:
            assert (pool[at:at + n] == 0xA5).all(), "a skipped image's region was written"
        else:
            np.testing.assert_array_equal(_samples(pool, at, n, want), want, err_msg=name)
    assert (pool[~covered] == 0xA5).all() and (pool[:64] == 0xA5).all() and (pool[-64:] == 0xA5).all()


@pytest.mark.gpu
def test_untrustworthy_descriptors_write_nothing(gpu_device):
    """offsets and sizes that would index outside the raw pool or the output pool: the image is left alone (like skip), its
    neighbours are decoded, the call succeeds"""
    picked = [c for c in cases() if c[0].startswith(("64x", "65x", "129x"))][:8]
    assert len(picked) == 8

    def spoil(s):
        s[0]["raw_offset"] = -1
        s[1]["out_offset"] = -8
        s[2]["out_offset"] = (1 << 40) + 3                      # past the output pool
        s[3]["raw_offset"] = (1 << 31) + 1                      # past the raw pool
        s[4]["width"] = s[4]["height"] = 0x7fffffff             # height * (row_bytes + 1) overflows 63 bits
        s[4]["bytes_per_pixel"] = 2
        s[5]["bytes_per_pixel"] = 3
        s[6]["height"] = 1 << 20                                # rows past both pools

    pool, regions = _low_level_batch(picked, set(), gpu_device, spoil=spoil)
    covered = np.zeros(pool.size, bool)
    for k, ((name, _, want), (at, n)) in enumerate(zip(picked, regions)):
        covered[at:at + n] = True
        if k < 7:
            assert (pool[at:at + n] == 0xA5).all(), name
        else:
            np.testing.assert_array_equal(_samples(pool, at, n, want), want, err_msg=name)
    assert (pool[~covered] == 0xA5).all()


@pytest.mark.gpu
def test_unfilter_argument_checks(gpu_device):
    import torch
    lib = _lib.lib()
    t = torch.full((1024,), 0xA5, dtype=torch.uint8, device=gpu_device)
    p = t.data_ptr()
    call = lib.dspn_png_unfilter_batch
    assert call(None, 64, p, 1, p, 64, None) == -1 and b"null" in lib.dspn_last_error()
    assert call(p, 64, None, 1, p, 64, None) == -1 and b"null" in lib.dspn_last_error()
    assert call(p, 64, p, 1, None, 64, None) == -1 and b"null" in lib.dspn_last_error()
    assert call(p, 64, p, -1, p, 64, None) == -1 and b"negative" in lib.dspn_last_error()
    assert call(p, -64, p, 1, p, 64, None) == -1 and b"negative" in lib.dspn_last_error()
    assert call(p, 64, p, 1, p, -64, None) == -1 and b"negative" in lib.dspn_last_error()
    assert call(p, 64, p + 4, 1, p, 64, None) == -1 and b"aligned" in lib.dspn_last_error()
    assert call(None, 0, None, 0, None, 0, None) == 0           # an empty batch is a no-op
    torch.cuda.synchronize(gpu_device)
    assert (t.cpu() == 0xA5).all()


@pytest.mark.gpu
def test_decode_batch_equals_pillow(gpu_device):
    import torch
    picked = cases()[5::7]
    assert {c[2].dtype for c in picked} == {np.dtype(np.uint8), np.dtype(np.uint16)}
    got = dp.decode_batch([c[1] for c in picked], gpu_device)
    assert len(got) == len(picked) and dp.decode_batch([], gpu_device) == []
    for (name, _, want), g in zip(picked, got):
        assert g.dtype == (torch.uint16 if want.dtype == np.uint16 else torch.uint8) and tuple(g.shape) == want.shape, name
        np.testing.assert_array_equal(g.cpu().numpy(), want, err_msg=name)


@pytest.mark.gpu
def test_decode_batch_names_the_reason(gpu_device):
    good = cases()[0][1]
    with pytest.raises(ValueError, match="stream 1 .*interlace"):
        dp.decode_batch([good, rp.write_interlaced(np.zeros((9, 9), np.uint8))], gpu_device)
    with pytest.raises(_lib.DspnError, match="stream 1"):
        dp.decode_batch([good, good[:-12]], gpu_device)


SIZES = [(96, 160)] * 4 + [(128, 192)] * 4                     # per record: every staging pool grows once after its first use


def _write_dataset(root, n, g, interlaced=(3,), sizes=SIZES, boxes=(0, 1, 3, 5, 2, 4, 1, 6)):
    """as tests/test_jpeg_gpu.py::_write_dataset (record 2 progressive, record 5 greyscale, a size per record), the label
    maps from the filter-choosing writer: random filter types, the records of `interlaced` interlaced, of the others
    record 1 as a palette stream and record 6 as RGB"""
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
        if i in (2, 5):
            buf = io.BytesIO()
            if i == 2:
                Image.fromarray(img[:, :, ::-1].copy()).save(buf, format="JPEG", quality=92, progressive=True)
            else:
                Image.fromarray(img[:, :, 1].copy()).save(buf, format="JPEG", quality=92)
            rec.write_idx(i, recordio.pack(header, buf.getvalue()))
        else:
            rec.write_idx(i, recordio.pack_img(header, img, quality=92))
        seg = g.integers(0, 19, hw).astype(np.uint8)
        seg[g.random(hw) < .1] = 255
        seg[:4, :4] = 40
        filters = rp.filters_for(g, hw[0], "mix")
        if i in interlaced:
            data = rp.write_interlaced(seg)
        elif i == 6:
            data = rp.write_rgb(np.stack([seg, seg, seg], -1), filters)
        else:
            data = rp.write(seg, filters, palette=(i == 1))
        with open(os.path.join(root, "cityscapes", "SegmentationClass", "city_%06d_gtFine_labelTrainIds.png" % i), "wb") as f:
            f.write(data)
        lines.append("%d\tJPEGImages/city_%06d_leftImg8bit.jpg\n" % (i, i))
    rec.close()
    with open(os.path.join(root, "train.lst"), "w") as f:
        f.writelines(lines)
    return os.path.join(root, "train.rec")


@pytest.fixture(scope="module")
def record_file(tmp_path_factory):
    return _write_dataset(str(tmp_path_factory.mktemp("png_records")), 8, np.random.Generator(np.random.PCG64(19)))


@pytest.fixture(scope="module")
def interlaced_record_file(tmp_path_factory):
    """all eight label maps interlaced: no batch has anything for the device"""
    return _write_dataset(str(tmp_path_factory.mktemp("png_records_interlaced")), 8,
                          np.random.Generator(np.random.PCG64(20)), interlaced=range(8))


def _same_batches(gpu_device, record_file, enable_aug, prefetch, device_jpeg, fallbacks):
    import torch
    kw = dict(enable_aug=enable_aug, prefetch=prefetch, device=gpu_device, device_jpeg=device_jpeg)
    a = it.MultiTaskRecordIter(record_file, 4, (3, 64, 128), **kw)
    b = it.MultiTaskRecordIter(record_file, 4, (3, 64, 128), device_png=True, **kw)
    assert a.device_png is False and a.png_fallbacks == 0 and b.device_png is True and b.png_fallbacks == 0
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
    assert b.png_fallbacks == fallbacks and a.png_fallbacks == 0
    assert b.jpeg_fallbacks == a.jpeg_fallbacks == (2 if device_jpeg else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("enable_aug,prefetch,device_jpeg", [(True, True, False), (True, False, False), (False, True, False),
                                                             (False, False, False), (True, True, True)])
def test_iterator_device_png_yields_the_same_batches(gpu_device, record_file, enable_aug, prefetch, device_jpeg):
    # the interlaced and the RGB label map, once per epoch
    _same_batches(gpu_device, record_file, enable_aug, prefetch, device_jpeg, fallbacks=4)


@pytest.mark.gpu
@pytest.mark.parametrize("prefetch", [True, False])
def test_iterator_device_png_all_fallback_batches(gpu_device, interlaced_record_file, prefetch):
    """the label bytes go up directly and nothing PNG-related is uploaded or launched: 8 fallbacks per epoch"""
    _same_batches(gpu_device, interlaced_record_file, True, prefetch, False, fallbacks=16)
