"""dspn_det_augment_batch_u8 and DetIter on the GPU: every comparison is torch.equal against the numpy restatement of
include/dspn_det_augment.h (tests/ref_det_augment.py)."""
import numpy as np
import pytest
import torch

import ref_det_augment as ref
from dspnet_amd import _lib
from dspnet_amd.dataset import det_iterator as di
from dspnet_amd.dataset import rand_sampler as rs

pytestmark = pytest.mark.gpu

MEAN = (123.68, 116.779, 103.939)


def _launch(dev, pool, samples, tables, H, W, mean=MEAN):
    pool_dev = torch.from_numpy(pool).to(dev)
    desc_dev = torch.from_numpy(samples.view(np.uint8).reshape(-1)).to(dev)
    tab_dev = torch.from_numpy(tables).to(dev)
    out = di.augment_on_device(pool_dev, desc_dev, tab_dev, H, W, mean)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def sources():
    gen = np.random.RandomState(21)
    return [gen.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (64, 48), (5, 7))]


# (source, window x0 y0 w h or None, mirror)
MIXED = [
    (0, None, False),                       # whole image; 37 x 53 -> both axes shrink
    (0, None, True),
    (1, (5, 10, 30, 50), False),            # crop mode; x grows, y shrinks: the area switch
    (1, (2, 3, 44, 20), True),              # crop mode; x shrinks, y grows
    (2, None, False),                       # 5 x 7: both axes grow
    (2, (-3, -2, 13, 9), True),             # padding mode, negative origins, both grow
    (0, (-20, -30, 100, 90), False),        # padding mode, both shrink
    (0, (-20, -30, 100, 90), True),
    (1, (17, 3, 1, 40), True),              # a 1-pixel-wide window
    (1, (0, 20, 48, 1), False),             # ... and a 1-pixel-high one
]


@pytest.mark.parametrize("H,W", [(32, 40), (33, 41)])
@pytest.mark.parametrize("method", di.METHODS)
def test_mixed_batch_equals_restatement(gpu_device, sources, method, H, W):
    images = [sources[k] for k, _, _ in MIXED]
    pool, samples, tables, want = ref.augment_images(images, [w for _, w, _ in MIXED], [method] * len(MIXED),
                                                     [m for _, _, m in MIXED], H, W, MEAN)
    if method == di.AREA:                                       # both rules of the area method are in the batch
        assert samples["kx"][0] == 3 and samples["kx"][2] == 2 and samples["ky"][2] == 2 and samples["ky"][6] == 4
    got = _launch(gpu_device, pool, samples, tables, H, W)
    assert torch.equal(got, torch.from_numpy(want))


def test_mixed_methods_in_one_batch(gpu_device, sources):
    """the method is per sample: the five of them, mirrored and not, in one launch"""
    cases = [(k % 3, MIXED[k][1], bool(k & 1), di.METHODS[k % 5]) for k in range(10)]
    pool, samples, tables, want = ref.augment_images([sources[c[0]] for c in cases], [c[1] for c in cases],
                                                     [c[3] for c in cases], [c[2] for c in cases], 33, 41, (0., 1., 2.))
    assert set(samples["kx"]) >= {1, 2, 4, 8}
    assert torch.equal(_launch(gpu_device, pool, samples, tables, 33, 41, (0., 1., 2.)), torch.from_numpy(want))


@pytest.mark.parametrize("method", di.METHODS)
def test_rows_wider_than_a_workgroup(gpu_device, sources, method):
    """W = 300 is one full strip of 256 pixels and one of 44: the staged x tables of the second strip start at column 256
    (at column 0 of the table under the mirror)"""
    H, W = 3, 300
    cases = [(0, None, False), (0, None, True), (1, (-100, -10, 700, 90), True), (2, None, True)]
    pool, samples, tables, want = ref.augment_images([sources[k] for k, _, _ in cases], [w for _, w, _ in cases],
                                                     [method] * 4, [m for _, _, m in cases], H, W, MEAN)
    assert torch.equal(_launch(gpu_device, pool, samples, tables, H, W), torch.from_numpy(want))


def test_area_with_64_taps(gpu_device, monkeypatch):
    img = np.random.RandomState(22).randint(0, 256, (640, 640, 3)).astype(np.uint8)
    pool, samples, tables, want = ref.augment_images([img, img], [None, None], [di.AREA] * 2, [False, True], 10, 10, MEAN)
    assert samples["kx"][0] == 64 and samples["ky"][0] == 64
    block = img.astype(np.float64).reshape(10, 64, 10, 64, 3).mean(axis=(1, 3)).transpose(2, 0, 1)
    assert np.abs(want[0] + np.asarray(MEAN)[:, None, None] - block).max() <= 0.5 + 1e-4       # the restatement is a box average
    assert torch.equal(_launch(gpu_device, pool, samples, tables, 10, 10), torch.from_numpy(want))
    # one tap more is refused while the batch is planned: nothing is uploaded, nothing is launched
    monkeypatch.setattr(di, "_entry", lambda: pytest.fail("a launch was attempted"))
    big = np.zeros((650, 650, 3), np.uint8)
    with pytest.raises(_lib.DspnError, match="65 taps"):
        ref.augment_images([big], [None], [di.AREA], [False], 10, 10, MEAN)


# ---- DetIter end to end ---------------------------------------------------------------------------------------------
def _samplers():
    crop = dict(min_scale=.3, max_scale=1., min_aspect_ratio=.5, max_aspect_ratio=2., max_trials=25)
    return [rs.RandCropper(min_overlap=o, **crop) for o in (.1, .3, .5, .7, .9)] + \
           [rs.RandPadder(min_scale=1., max_scale=4., min_aspect_ratio=.5, max_aspect_ratio=2., min_gt_scale=.05)]


@pytest.fixture(scope="module")
def jpeg_list(gpu_device, tmp_path_factory):
    """eight small JPEGs written by the device encoder, and their list in the format Imdb.save_imglist writes"""
    from dspnet_amd.dataset import jpeg_encode
    root = tmp_path_factory.mktemp("det_jpegs")
    gen = np.random.RandomState(23)
    images = []
    for k in range(8):
        h, w = 40 + 7 * k, 96 - 5 * k
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(xx * 3 + yy * 2 + 40 * k) % 256, (xx * yy // 7 + 90) % 256, (255 - xx - yy) % 256], axis=2)
        images.append(np.clip(smooth + gen.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8))
    files = jpeg_encode.encode_batch([torch.from_numpy(im).to(gpu_device) for im in images], quality=90)
    lines = []
    for k, data in enumerate(files):
        with open(str(root / ("im%d.jpg" % k)), "wb") as f:
            f.write(data)
        lab = np.array([[k % 8, .10, .15, .55, .70], [(k + 3) % 8, .45, .30, .92, .88], [(k + 5) % 8, .30, .05, .62, .40]][:2 + k % 2])
        lines.append("\t".join([str(k), "2", "5"] + ["{0:.4f}".format(x) for x in lab.ravel()] + ["im%d.jpg" % k]) + "\n")
    with open(str(root / "all.lst"), "w") as f:
        f.writelines(lines)
    with open(str(root / "four.lst"), "w") as f:
        f.writelines(lines[:4])
    return str(root)


def _two_epochs(it):
    out = []
    for _ in range(2):
        while it.iter_next():
            b = it.next()
            out.append((b.data[0].cpu().clone(), b.label[0].cpu().clone(), b.pad, b.index, list(it.batch_indices)))
        it.reset()
    return out


@pytest.mark.parametrize("device_jpeg", [False, True])
def test_det_iter_equals_the_host_path(gpu_device, jpeg_list, monkeypatch, device_jpeg):
    """Pillow decode, the samplers and the restatement on the host against DetIter on the device, from the same seed"""
    import os
    db = di.ListImdb(os.path.join(jpeg_list, "all.lst"), jpeg_list)
    kwargs = dict(mean_pixels=list(MEAN), rand_mirror=True, shuffle=True, rand_seed=233)
    it = di.DetIter(db, 4, (3, 33, 41), rand_samplers=_samplers(), device=gpu_device, device_jpeg=device_jpeg, **kwargs)
    got = _two_epochs(it)
    torch.cuda.synchronize()
    if device_jpeg:
        assert it.jpeg_fallbacks == 0                           # every file went through the device decode
    monkeypatch.setattr(di.DetIter, "_device_batch", ref.device_batch_on_host)
    want = _two_epochs(di.DetIter(db, 4, (3, 33, 41), rand_samplers=_samplers(), device="cpu", **kwargs))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g[2:] == w[2:]
        assert g[1].dtype == torch.float32 and tuple(g[1].shape) == (4, 3, 5) and torch.equal(g[1], w[1])
        assert tuple(g[0].shape) == (4, 3, 33, 41) and torch.equal(g[0], w[0])
    # the augmentation was at work: some sample was cropped or padded to another label than the database's
    assert any(not np.array_equal(g[1][k].numpy(), db.label_from_index(g[4][k]).astype(np.float32))
               for g in got for k in range(4))


def test_det_iter_mixed_fallback_batch(gpu_device, tmp_path):
    """two baseline JPEGs beside a progressive one and a PNG: coefficients go up for two samples of every batch and
    Pillow's pixels for the other two, and the batches equal those with the device decode off"""
    from PIL import Image
    gen = np.random.RandomState(24)
    lines = []
    for k, (h, w, name, kw) in enumerate([(40, 96, "a.jpg", {}), (47, 91, "b.jpg", {}), (45, 80, "c.jpg", {"progressive": True}),
                                          (38, 51, "d.png", {})]):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(xx * 3 + yy * 2 + 40 * k) % 256, (xx * yy // 7 + 90) % 256, (255 - xx - yy) % 256], axis=2)
        Image.fromarray(np.clip(smooth + gen.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)).save(str(tmp_path / name), **kw)
        lab = np.array([[k, .10, .15, .55, .70], [k + 3, .45, .30, .92, .88]])
        lines.append("\t".join([str(k), "2", "5"] + ["{0:.4f}".format(x) for x in lab.ravel()] + [name]) + "\n")
    with open(str(tmp_path / "mixed.lst"), "w") as f:
        f.writelines(lines)
    db = di.ListImdb(str(tmp_path / "mixed.lst"), str(tmp_path))
    kwargs = dict(mean_pixels=list(MEAN), rand_samplers=_samplers(), rand_mirror=True, shuffle=True, rand_seed=233,
                  device=gpu_device)
    on = di.DetIter(db, 4, (3, 33, 41), device_jpeg=True, **kwargs)
    got = _two_epochs(on)
    off = di.DetIter(db, 4, (3, 33, 41), device_jpeg=False, **kwargs)
    want = _two_epochs(off)
    torch.cuda.synchronize()
    assert on.jpeg_fallbacks == 4 and off.jpeg_fallbacks == 0   # the progressive file and the PNG, once per epoch
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g[2:] == w[2:]
        assert torch.equal(g[1], w[1]) and torch.equal(g[0], w[0])


def test_fit_consumes_the_fit_view(gpu_device, jpeg_list):
    """two steps of train.solver.fit on the detection-only graph of tests/test_graph_gpu.py::test_single_task_graphs_train
    (resnet-50 at 256, batch 2), fed by DetIter.fit_view()"""
    import os
    from dspnet_amd.symbol.multitask_symbol_factory import get_det_symbol_train
    from dspnet_amd.train.solver import MultiTaskSolver, fit
    db = di.ListImdb(os.path.join(jpeg_list, "four.lst"), jpeg_list, label_width=6, pad_rows=200)
    it = di.DetIter(db, 2, (3, 256, 256), mean_pixels=list(MEAN), rand_samplers=_samplers(), rand_mirror=True, shuffle=True,
                    rand_seed=233, device=gpu_device, device_jpeg=True)
    net = get_det_symbol_train("resnet-50", 256, num_classes=8, batch_size=2, device=gpu_device, seed=11)
    steps = []
    history = fit(MultiTaskSolver(net), it.fit_view(), num_epoch=1, batch_end_callback=lambda p: steps.append(p.nbatch))
    torch.cuda.synchronize()
    assert steps == [1, 2] and len(history) == 1
    assert np.isfinite(history[0]["CrossEntropy"]) and np.isfinite(history[0]["SmoothL1"])    # no segmentation task to score
