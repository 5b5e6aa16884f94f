"""Device half of the JPEG encode (dspn_jpeg_encode_blocks_batch_u8) and its callers: the quantised coefficients equal those
of Pillow's stream for the same pixels (read with tests/ref_jpeg.py), the files equal Pillow's byte for byte, nothing is
written outside a valid sample's blocks, and record files written through the device equal those written with pack_img."""
import io
import os

import numpy as np
import pytest

import jpeg_encode_cases as ec
from dspnet_amd import _lib
from dspnet_amd.dataset import iterator as it
from dspnet_amd.dataset import jpeg_encode as je
from dspnet_amd.dataset import recordio

# the low-level harness lives next to the cases (tests/test_pipeline_edges_gpu.py shares it)
GUARD, _reference_blocks, _low_level_batch, _regions, _check_batch = (ec.GUARD, ec.reference_blocks, ec.low_level_batch, ec.regions,
                                                                      ec.check_batch)


@pytest.mark.gpu
def test_coefficients_equal_pillows_in_one_mixed_batch(gpu_device):
    """all 112 cases (7 sizes x 4:2:0 / 4:2:2 / 4:4:4 / grey x quality 95 / 30 x noise / smooth) in one call: every offset
    differs, colour and grey samples and all three chroma layouts meet in each launch"""
    cases = ec.CASES
    assert len(cases) == 112
    coefs, samples, ws = _low_level_batch(cases, gpu_device)
    _check_batch(cases, coefs, samples, ws)


@pytest.mark.gpu
def test_more_rows_than_one_workgroup_pass_and_odd_row_counts(gpu_device):
    """a plane wider than the 1024 samples one workgroup covers per unit, and the heights at which padding rows before the
    2 x 2 average instead of after it would change bits (H even, H mod 16 in 1..8)"""
    import torch
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(77))
    shapes = [(10, 1100, 3), (18, 2100, 3), (22, 40, 3), (6, 1032, 1)]
    imgs = [g.integers(0, 256, s if s[2] == 3 else s[:2]).astype(np.uint8) for s in shapes]
    for ss, pillow_ss in (("4:2:0", 2), ("4:2:2", 1)):
        got = je.encode_batch([torch.from_numpy(a).to(gpu_device) for a in imgs], quality=90, subsampling=ss)
        for a, f in zip(imgs, got):
            buf = io.BytesIO()
            kw = {"subsampling": pillow_ss} if a.ndim == 3 else {}
            Image.fromarray(a).save(buf, format="JPEG", quality=90, **kw)
            assert f == buf.getvalue(), (a.shape, ss)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ec.LAYOUTS)
def test_encode_batch_equals_pillows_files(gpu_device, layout):
    import torch
    cases = [c for c in ec.CASES if c[2] == layout]
    for q in ec.QUALITIES:
        sub = [c for c in cases if c[3] == q]
        images = [torch.from_numpy(ec.pixels(c).copy()).to(gpu_device) for c in sub]
        got = je.encode_batch(images, quality=q, subsampling="4:2:0" if layout == "grey" else layout)
        assert len(got) == len(sub) == 14
        for c, f in zip(sub, got):
            assert f == ec.pillow_file(c), ec.name(c)


@pytest.mark.gpu
def test_pack_img_batch_equals_pack_img(gpu_device):
    import torch
    cases = [c for c in ec.CASES if c[2] == "4:2:0" and c[3] == 95]
    bgr = [np.ascontiguousarray(ec.pixels(c)[:, :, ::-1]) for c in cases]
    headers = [recordio.IRHeader(0, np.arange(k + 2, dtype=np.float32), k, 0) for k in range(len(cases))]
    headers[0] = recordio.IRHeader(0, 3.0, 0, 0)
    got = recordio.pack_img_batch(headers, [torch.from_numpy(a).to(gpu_device) for a in bgr], quality=95)
    assert got == [recordio.pack_img(h, a, quality=95) for h, a in zip(headers, bgr)]
    # non-contiguous views of a larger tensor are taken as they are
    big = torch.from_numpy(bgr[-1]).to(gpu_device)
    (view,) = recordio.pack_img_batch(headers[:1], [big[3:40, 5:150]], quality=60)
    assert view == recordio.pack_img(headers[0], bgr[-1][3:40, 5:150], quality=60)


@pytest.mark.gpu
def test_guard_bytes_and_skip(gpu_device):
    cases = [(21, 37, "4:2:0", 95, "noise"), (1, 1, "4:2:0", 95, "smooth"), (24, 40, "4:2:2", 30, "noise"),
             (9, 15, "grey", 95, "noise"), (64, 200, "4:4:4", 30, "smooth"), (24, 40, "4:2:0", 95, "smooth")]
    coefs, samples, ws = _low_level_batch(cases, gpu_device, skip={2})
    _check_batch(cases, coefs, samples, ws, untouched={2})


@pytest.mark.gpu
def test_untrustworthy_descriptors_write_nothing(gpu_device):
    """offsets, sizes and grids that would index outside the image pool, the coefficient pool or a component plane, or
    that contradict each other: the sample is left alone (like skip), its neighbours are encoded"""
    cases = [(21, 37, "4:2:0", 95, "noise"), (24, 40, "4:2:2", 95, "noise"), (16, 16, "4:4:4", 95, "noise"),
             (9, 15, "4:2:0", 95, "noise"), (8, 8, "grey", 95, "noise"), (16, 16, "4:2:0", 30, "noise"),
             (24, 40, "4:2:0", 30, "smooth"), (64, 200, "4:2:0", 95, "smooth")]
    regions = {}

    def spoil(s):
        for k in range(len(cases)):
            regions[k] = _regions(s, k)
        s[0]["coef_offset"][2] = 1 << 40                        # past the coefficient pool
        s[1]["blocks_w"][1] = 1                                 # a chroma grid narrower than the image needs
        s[2]["img_offset"] = (1 << 31) + 5                      # past the image pool
        s[3]["hsamp"] = 3                                       # not a supported layout
        s[4]["coef_offset"][0] = -64
        s[5]["width"] = 60000                                   # pixels the pool does not hold, grids that contradict the size
        s[6]["blocks_h"][0] += 1                                # a luma grid taller than the real one

    coefs, samples, ws = _low_level_batch(cases, gpu_device, spoil=spoil)
    for k, case in enumerate(cases):
        for c, (at, n) in enumerate(regions[k]):
            if k < 7:
                assert (coefs[at:at + n] == -23131).all(), ec.name(case)
                assert (ws[GUARD + at:GUARD + at + n] == 0xA5).all(), ec.name(case)
            else:
                np.testing.assert_array_equal(coefs[at:at + n], _reference_blocks(case)[c].reshape(-1), err_msg=ec.name(case))
    assert (coefs[:GUARD // 2] == -23131).all() and (coefs[-GUARD // 2:] == -23131).all()
    assert (ws[:GUARD] == 0xA5).all() and (ws[-GUARD:] == 0xA5).all()


@pytest.mark.gpu
def test_encode_blocks_argument_checks(gpu_device):
    import torch
    lib = _lib.lib()
    t = torch.zeros(1024, dtype=torch.uint8, device=gpu_device)
    p = t.data_ptr()
    rgb, bad = (je._c.c_int * 3)(0, 1, 2), (je._c.c_int * 3)(0, 1, 1)
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, rgb, p, 0, p, 64, p, 64, None) == -1            # B
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, rgb, p, 2000, p, 64, p, 64, None) == -1
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, rgb, p, 1, p, 65, p, 65, None) == -1            # whole blocks
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, bad, p, 1, p, 64, p, 64, None) == -1 and b"permutation" in lib.dspn_last_error()
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, None, p, 1, p, 64, p, 64, None) == -1 and b"null" in lib.dspn_last_error()
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, rgb, p, 1, p, 128, p, 64, None) == -2 and b"workspace" in lib.dspn_last_error()
    assert lib.dspn_jpeg_encode_blocks_batch_u8(p, 64, rgb, p, 1, p + 2, 64, p, 64, None) == -1 and b"aligned" in lib.dspn_last_error()
    with pytest.raises(ValueError, match="subsampling"):
        je.encode_batch([t.view(32, 32)], subsampling="4:1:1")
    with pytest.raises(ValueError, match="uint8"):
        je.encode_batch([t.view(32, 32).float()])
    with pytest.raises(ValueError, match="uint8"):
        je.encode_batch([t.view(32, 32).cpu()])
    assert je.encode_batch([]) == []


@pytest.mark.gpu
def test_a_call_on_another_stream_gives_the_same_bytes(gpu_device):
    import torch
    cases = [c for c in ec.CASES if c[3] == 30 and c[4] == "noise" and c[2] != "grey"][:9]
    side = torch.cuda.Stream(gpu_device)
    coefs, samples, ws = _low_level_batch(cases, gpu_device, stream=side)
    _check_batch(cases, coefs, samples, ws)
    sub = [c for c in cases if c[2] == "4:2:2"]
    images = [torch.from_numpy(ec.pixels(c).copy()).to(gpu_device) for c in sub]
    torch.cuda.synchronize(gpu_device)
    with torch.cuda.stream(side):
        got = je.encode_batch(images, quality=30, subsampling="4:2:2")
    assert got == [ec.pillow_file(c) for c in sub]


@pytest.mark.gpu
def test_save_jpeg_writes_pillows_file(gpu_device, tmp_path):
    import torch
    from PIL import Image
    from dspnet_amd.detect import render
    case = (21, 37, "4:2:0", 95, "smooth")
    want = ec.pillow_file(case)
    render.save_jpeg(str(tmp_path / "a.jpg"), torch.from_numpy(ec.pixels(case).copy()).to(gpu_device))
    assert (tmp_path / "a.jpg").read_bytes() == want
    grey = ec.pixels((9, 15, "grey", 30, "noise"))
    render.save_jpeg(str(tmp_path / "g.jpg"), grey, quality=30)             # a host array is uploaded first
    assert (tmp_path / "g.jpg").read_bytes() == ec.pillow_file((9, 15, "grey", 30, "noise"))
    assert Image.open(str(tmp_path / "a.jpg")).size == (37, 21)
    with pytest.raises(_lib.DspnError, match="uint8"):
        render.save_jpeg(str(tmp_path / "b.jpg"), torch.zeros(4, 4, 3, device=gpu_device))


def _write_sources(root, n, g, hw=(96, 160)):
    """image files, their .lst, label-map PNGs and a record pair written by hand with pack_img -> (prefix of the list, by-hand .rec)"""
    from PIL import Image
    os.makedirs(os.path.join(root, "JPEGImages"), exist_ok=True)
    os.makedirs(os.path.join(root, "cityscapes", "SegmentationClass"), exist_ok=True)
    hand = recordio.MXIndexedRecordIO(os.path.join(root, "hand.idx"), os.path.join(root, "hand.rec"), "w")
    lines = []
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    for i in range(n):
        chans = [127 + 100 * np.sin(xx / g.uniform(5, 15) + g.uniform(0, 3)) * np.cos(yy / g.uniform(5, 15)) for _ in range(3)]
        img = np.clip(np.stack(chans, -1) + g.normal(0, 6, hw + (3,)), 0, 255).astype(np.uint8)
        rel = "JPEGImages/city_%06d_leftImg8bit.%s" % (i, "png" if i == 3 else "jpg")
        kw = dict(format="PNG") if i == 3 else dict(format="JPEG", quality=97, subsampling=(2, 0, 1, 2)[i % 4], progressive=(i == 2))
        Image.fromarray(img).save(os.path.join(root, rel), **kw)
        rows = np.full((10, 6), -1.0)
        for k in range(i % 4):
            x0, y0 = g.uniform(0, .8), g.uniform(0, .8)
            rows[k] = [g.integers(0, 8), x0, y0, x0 + g.uniform(.01, .3), y0 + g.uniform(.01, .3), g.uniform(0, 1)]
        label = np.array([2, 6] + rows.reshape(-1).tolist(), np.float32)
        lines.append("%d\t%s\t%s\n" % (i, "\t".join("%f" % v for v in label), rel))
        label = np.array([float("%f" % v) for v in label], np.float32)                 # what the list's text carries
        with open(os.path.join(root, rel), "rb") as f:
            decoded = recordio.imdecode(f.read())                                       # BGR, as cv2.imread gives it
        hand.write_idx(i, recordio.pack_img(recordio.IRHeader(0, label, i, 0), decoded, quality=92))
        seg = g.integers(0, 19, hw).astype(np.uint8)
        segfile = rel.replace("leftImg8bit.jpg", "gtFine_labelTrainIds.png").replace("JPEGImages", "SegmentationClass")   # the iterator's rule
        Image.fromarray(seg).save(os.path.join(root, "cityscapes", segfile), format="PNG")
    hand.close()
    with open(os.path.join(root, "train.lst"), "w") as f:
        f.writelines(lines)
    return os.path.join(root, "train"), os.path.join(root, "hand.rec")


@pytest.mark.gpu
def test_write_records_equals_pack_img_in_a_loop(gpu_device, tmp_path):
    """8 sources (4:2:0, 4:4:4, 4:2:2 and progressive JPEGs, one PNG) in batches of 3: the .rec and .idx equal the ones
    written with pack_img record by record, and the iterator yields the same batches from either pair"""
    import torch
    from dspnet_amd.dataset import im2rec
    root = str(tmp_path)
    prefix, hand = _write_sources(root, 8, np.random.Generator(np.random.PCG64(23)))
    assert im2rec.write_records(prefix, root, quality=92, batch=3, device=gpu_device) == 8
    with open(prefix + ".rec", "rb") as a, open(hand, "rb") as b:
        assert a.read() == b.read()
    with open(prefix + ".idx") as a, open(hand[:-4] + ".idx") as b:
        assert a.read() == b.read()
    with open(os.path.join(root, "hand.lst"), "w") as f, open(prefix + ".lst") as src:
        f.write(src.read())
    kw = dict(enable_aug=False, prefetch=False, device=gpu_device, device_jpeg=True)
    a = it.MultiTaskRecordIter(prefix + ".rec", 4, (3, 64, 128), **kw)
    b = it.MultiTaskRecordIter(hand, 4, (3, 64, 128), **kw)
    seen = 0
    while a.iter_next():
        assert b.iter_next()
        (ba, fa), (bb, fb) = a.next(), b.next()
        assert fa == fb
        assert torch.equal(ba.data[0], bb.data[0])
        assert torch.equal(ba.label[0], bb.label[0]) and torch.equal(ba.label[1], bb.label[1])
        seen += 4
    assert seen == 8 and a.jpeg_fallbacks == 0
