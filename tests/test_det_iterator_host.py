"""Host side of the detection iterator (no GPU): the samplers against the reference's recorded output, the window and tap
table planning, the numpy restatement of the launch against torch's CPU interpolation, and DetIter's bookkeeping with the
device call replaced by the restatement."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import ref_det_augment as ref
from dspnet_amd import _lib
from dspnet_amd.dataset import det_iterator as di
from dspnet_amd.dataset import rand_sampler as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = {di.LINEAR: "linear", di.CUBIC: "cubic", di.AREA: "area", di.NEAREST: "nearest", di.LANCZOS4: "lanczos4"}


def _generator():
    spec = importlib.util.spec_from_file_location("make_rand_sampler_golden", os.path.join(GOLDEN, "make_rand_sampler_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


# ---- 1. samplers ----------------------------------------------------------------------------------------------------
def test_samplers_equal_the_reference_bit_for_bit():
    gen = _generator()
    doc = np.load(os.path.join(GOLDEN, "rand_sampler.npz"))
    assert sorted(set(k.split("/")[0] for k in doc.files)) == sorted(gen.CASES)
    for name, case in gen.CASES.items():
        got = gen.run_case(rs, case, rng=np.random.RandomState(case[3]))
        for key in ("counts", "boxes", "labels", "pos"):
            want = doc[name + "/" + key]
            assert got[key].dtype == want.dtype and np.array_equal(got[key], want), (name, key)
        if name != "pad_none":
            assert (got["counts"] > 0).any() and (got["counts"] == 0).any(), name
    assert (doc["crop_x3/counts"] > 1).any()                    # later samples drawn against the already cropped label
    # rng=None is the global stream, as in the reference
    got = gen.run_case(rs, gen.CASES["crop_05"])
    assert np.array_equal(got["boxes"], doc["crop_05/boxes"]) and np.array_equal(got["pos"], doc["crop_05/pos"])
    # a label without a valid row: the padder draws and gives up (pad_none above), the cropper raises like the reference
    with pytest.raises(ValueError):
        gen.run_case(rs, gen.RAISES, rng=np.random.RandomState(gen.RAISES[3]))


def test_samplers_carry_a_sixth_column_through():
    gen = _generator()
    for name in ("crop_03", "crop_x3", "pad"):
        cls, kwargs, label, seed = gen.CASES[name]
        five = gen.run_case(rs, (cls, kwargs, label, seed), rng=np.random.RandomState(seed))
        dist = np.where(label[:, :1] > -1, 10.0 + np.arange(label.shape[0])[:, None] * 1.5, -1.0)
        six = gen.run_case(rs, (cls, kwargs, np.hstack([label, dist]), seed), rng=np.random.RandomState(seed))
        assert np.array_equal(six["counts"], five["counts"]) and np.array_equal(six["boxes"], five["boxes"])
        assert np.array_equal(six["pos"], five["pos"]) and six["labels"].shape[2] == 6
        assert np.array_equal(six["labels"][:, :, :5], five["labels"])
        valid = six["labels"][:, :, 0] > -1
        assert valid.any() and (six["labels"][:, :, 5][~valid] == -1).all()
        # every surviving row keeps the distance of the row it came from: classes are distinct in these labels
        by_class = {label[r, 0]: dist[r, 0] for r in range(label.shape[0]) if label[r, 0] > -1}
        assert len(by_class) == (label[:, 0] > -1).sum()
        want = np.vectorize(by_class.get)(six["labels"][:, :, 0][valid])
        assert np.array_equal(six["labels"][:, :, 5][valid], want)


def test_sampler_constructors_assert_like_the_reference():
    for bad in (dict(min_scale=.5, max_scale=.4), dict(min_scale=0.), dict(max_scale=1.5), dict(min_aspect_ratio=1.5),
                dict(max_aspect_ratio=.5), dict(min_overlap=1.5), dict(max_trials=0), dict(max_sample=-1)):
        with pytest.raises(AssertionError):
            rs.RandCropper(**bad)
    for bad in (dict(min_scale=.5), dict(min_scale=2., max_scale=1.), dict(min_gt_scale=2.), dict(max_aspect_ratio=.5)):
        with pytest.raises(AssertionError):
            rs.RandPadder(**bad)
    c, p = rs.RandCropper(), rs.RandPadder()
    assert (c.max_trials, c.max_sample, c.min_overlap, c.config) == (50, 1, 0., {"gt_constraint": "center"})
    assert (p.max_trials, p.max_sample, p.min_gt_scale) == (50, 1, .01)


# ---- 2. crop_window -------------------------------------------------------------------------------------------------
def test_crop_window():
    assert di.crop_window((.1, .2, .6, .9), 100, 50) == (10, 10, 50, 35, False)
    assert di.crop_window((.109, .219, .601, .999), 100, 50) == (10, 10, 50, 39, False)        # int() truncates
    # negative origins truncate toward zero: int(-.259 * 100) == -25, not -26
    assert di.crop_window((-.259, -.119, 1.301, 1.5), 100, 50) == (-25, -5, 155, 80, True)
    # the edges of the crop / pad decision
    assert di.crop_window((0., 0., 1., 1.), 100, 50) == (0, 0, 100, 50, False)                # xmin == 0, xmax == width
    assert di.crop_window((.5, 0., 1., 1.), 100, 50) == (50, 0, 50, 50, False)                # xmax == width
    assert di.crop_window((0., 0., 1.01, 1.), 100, 50) == (0, 0, 101, 50, True)               # one column past it
    assert di.crop_window((-.001, 0., 1., 1.), 1000, 50) == (-1, 0, 1001, 50, True)
    assert di.crop_window((-.0001, 0., 1., 1.), 1000, 50) == (0, 0, 1000, 50, False)          # truncates to the image
    # a window that neither lies inside the image nor contains it: the reference's slice assignment fails
    for box in ((.2, -.1, 1.3, 1.2), (-.2, .1, 1.2, 1.3), (-.2, -.2, .9, 1.2), (-.2, -.2, 1.2, .9)):
        with pytest.raises(ValueError):
            di.crop_window(box, 100, 50)
    with pytest.raises(ValueError):
        di.crop_window((.5, .5, .504, .9), 100, 50)                                         # empty window


# ---- 3. resize_taps -------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 5, 7, 13, 16, 31, 32, 64)


def _flags(method):
    return (True, False) if method == di.AREA else (None,)


def test_every_tap_row_sums_to_2048():
    for method in di.METHODS:
        for n_src in SIZES:
            for n_dst in SIZES:
                for flag in _flags(method):
                    if flag and n_src < n_dst:
                        continue
                    first, coef = di.resize_taps(n_src, n_dst, method, flag)
                    assert first.dtype == np.int32 and coef.dtype == np.int16
                    assert first.shape == (n_dst,) and coef.shape[0] == n_dst and 1 <= coef.shape[1] <= 64
                    assert (coef.astype(np.int64).sum(axis=1) == 2048).all(), (NAMES[method], n_src, n_dst, flag)
                    # a tap with weight reads inside the canvas or next to its edge (the clamp replicates)
                    assert (first > -8).all() and (first < n_src).all()
    assert di.resize_taps(32, 16, di.AREA)[1].shape[1] == 2 and (di.resize_taps(32, 16, di.AREA)[1] == 1024).all()
    assert di.resize_taps(16, 32, di.NEAREST)[1].shape[1] == 1


def test_equal_sizes_give_unit_taps():
    for method in di.METHODS:
        for n in (1, 2, 7, 32):
            for flag in _flags(method):
                first, coef = di.resize_taps(n, n, method, flag)
                for d in range(n):
                    idx = np.clip(first[d] + np.arange(coef.shape[1]), 0, n - 1)
                    weight = np.bincount(idx, weights=coef[d], minlength=n)
                    assert weight[d] == 2048 and np.count_nonzero(coef[d]) == 1, (NAMES[method], n, d)


def test_more_than_64_taps_is_refused():
    assert di.resize_taps(640, 10, di.AREA, True)[1].shape == (10, 64)
    assert (di.resize_taps(640, 10, di.AREA, True)[1] == 32).all()
    with pytest.raises(_lib.DspnError, match="65 taps"):
        di.resize_taps(650, 10, di.AREA, True)
    plan = {"src_w": 650, "src_h": 20, "img_offset": 0, "window": (0, 0, 650, 20), "method": di.AREA, "mirror": False}
    with pytest.raises(_lib.DspnError):
        di.pack_batch([plan], 10, 10)
    assert di.resize_taps(650, 10, di.AREA, False)[1].shape == (10, 2)      # the two-tap rule has no such limit
    assert di.resize_taps(650, 10, di.LANCZOS4)[1].shape == (10, 8)


def test_area_switches_rule_when_one_axis_grows():
    # both axes shrink: the box average on both
    (fx, cx), (fy, cy) = di.sample_taps(40, 30, 20, 10, di.AREA)
    assert cx.shape[1] == 2 and (cx == 1024).all() and cy.shape[1] == 3 and np.array_equal(fy, np.arange(10) * 3)
    # the y axis grows: BOTH axes use the two-tap rule, also the shrinking x axis
    (fx2, cx2), (fy2, cy2) = di.sample_taps(40, 30, 20, 45, di.AREA)
    assert cx2.shape[1] == 2 and cy2.shape[1] == 2
    want = di.resize_taps(40, 20, di.AREA, False)
    assert np.array_equal(fx2, want[0]) and np.array_equal(cx2, want[1])
    # i = floor(d s), t = (d + 1) - (i + 1) / s: at s = 2 every t is 1/2
    assert np.array_equal(fx2, np.arange(20) * 2) and (cx2 == 1024).all()
    # a fractional shrink keeps partial covers, each at least 1e-3 of a pixel
    first, coef = di.resize_taps(7, 3, di.AREA, True)
    assert coef.shape[1] == 3 and np.array_equal(first, [0, 2, 4])
    assert np.array_equal(coef[0], [877, 878, 293])             # 3/7, 3/7, 1/7 of 2048 round to 2049: the first largest gives one up


def test_lanczos_taps_are_symmetric():
    # t and 1 - t mirror the eight taps: output d of 3 -> 8 sits at f = 3 d / 8 - 5 / 16, so d and 7 - d are such a pair
    first, coef = di.resize_taps(3, 8, di.LANCZOS4)
    c = di.resize_coefficients(3, 8, di.LANCZOS4, False)[1]
    for d in range(8):
        assert np.allclose(c[d], c[7 - d][::-1], rtol=0, atol=1e-15)
        assert np.abs(coef[d].astype(int) - coef[7 - d][::-1]).max() <= 1      # up to where the residual went
    assert np.allclose(c.sum(axis=1), 1) and (c[:, 3] + c[:, 4] > .8).all()


# ---- 4. the restatement against torch on the CPU --------------------------------------------------------------------
def _whole_image_case(h, w, H, W, method, seed):
    img = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    _, _, _, got = ref.augment_images([img], [None], [method], [False], H, W, (0., 0., 0.))
    box = w >= W and h >= H
    fx, cx = di.resize_coefficients(w, W, method, box)
    fy, cy = di.resize_coefficients(h, H, method, box)
    qx, qy = di.resize_taps(w, W, method, box)[1].astype(np.float64), di.resize_taps(h, H, method, box)[1].astype(np.float64)
    # coefficient quantisation plus the final rounding, from the tables themselves
    err = np.abs(qy[:, :, None, None] * qx[None, None, :, :] / 2.0 ** 22 - cy[:, :, None, None] * cx[None, None, :, :])
    bound = 255 * err.sum(axis=(1, 3)) + 0.5 + 1e-3
    x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    return got[0].astype(np.float64), x, bound


@pytest.mark.parametrize("h,w,H,W", [(37, 53, 32, 40), (5, 7, 33, 41), (64, 48, 32, 40), (32, 40, 32, 40), (16, 20, 32, 40),
                                     (64, 80, 32, 40), (1, 9, 4, 3)])
def test_restatement_matches_torch_interpolate(h, w, H, W):
    for method, mode in ((di.LINEAR, "bilinear"), (di.CUBIC, "bicubic")):
        got, x, bound = _whole_image_case(h, w, H, W, method, 3)
        want = torch.nn.functional.interpolate(x, size=(H, W), mode=mode, align_corners=False)[0].numpy()
        want = np.clip(want, 0, 255)                            # the launch saturates to uint8 before the mean
        diff = np.abs(got - want)
        print(mode, (h, w), (H, W), "max diff %.4f, smallest margin %.4f" % (diff.max(), (bound[None] - diff).min()))
        assert (diff <= bound[None]).all(), (mode, diff.max(), bound.max())
        assert bound.max() < 2.0                                # the bound itself stays a rounding bound


@pytest.mark.parametrize("h,w,H,W", [(37, 53, 32, 40), (5, 7, 33, 41), (64, 48, 32, 40), (32, 40, 32, 40), (16, 20, 32, 40),
                                     (64, 80, 32, 40)])
def test_restatement_matches_torch_nearest(h, w, H, W):
    got, x, _ = _whole_image_case(h, w, H, W, di.NEAREST, 4)
    want = torch.nn.functional.interpolate(x, size=(H, W), mode="nearest")[0].numpy()
    assert (got == want).all()


@pytest.mark.parametrize("h,w,H,W", [(64, 80, 32, 40), (96, 40, 32, 40), (33, 123, 33, 41), (640, 640, 10, 10)])
def test_restatement_matches_avg_pool_for_area(h, w, H, W):
    got, x, bound = _whole_image_case(h, w, H, W, di.AREA, 5)
    want = torch.nn.functional.avg_pool2d(x, (h // H, w // W))[0].numpy()
    diff = np.abs(got - want)
    print("area", (h, w), (H, W), "max diff %.4f" % diff.max())
    assert (diff <= bound[None]).all() and bound.max() < 1.0


def test_restatement_window_fill_and_mirror():
    img = np.random.RandomState(6).randint(0, 256, (6, 8, 3)).astype(np.uint8)
    mean = (1.5, 2.25, 3.)
    # nearest at the canvas size is a copy: the padding shows the fill, the mirror flips the columns
    _, s, t, got = ref.augment_images([img, img, img], [(-2, -1, 12, 9), (-2, -1, 12, 9), (3, 2, 4, 3)], [di.NEAREST] * 3,
                                      [False, True, False], 9, 12, mean)
    can = np.full((9, 12, 3), 128, np.uint8)
    can[1:7, 2:10] = img
    want = can.astype(np.float64).transpose(2, 0, 1) - np.asarray(mean)[:, None, None]
    assert np.array_equal(got[0], want.astype(np.float32)) and np.array_equal(got[1], want[:, :, ::-1].astype(np.float32))
    assert s["xtab"][0] == s["xtab"][1] and s["ytab"][0] == s["ytab"][1]       # equal tables are shared
    crop = np.repeat(np.repeat(img[2:5, 3:7], 3, axis=0), 3, axis=1)
    assert np.array_equal(got[2], (crop.astype(np.float64).transpose(2, 0, 1) - np.asarray(mean)[:, None, None]).astype(np.float32))


# ---- 5. DetIter bookkeeping, the device call replaced by the restatement -------------------------------------------
class _Imdb(object):
    def __init__(self, paths, labels):
        self.paths, self.labels, self.num_images = paths, labels, len(paths)

    def image_path_from_index(self, i):
        return self.paths[i]

    def label_from_index(self, i):
        return self.labels[i]


class _FixedSampler(rs.RandSampler):
    """returns the crops it was given and records that it was asked"""

    def __init__(self, log, tag, crops):
        super(_FixedSampler, self).__init__(1, 1)
        self.log, self.tag, self.crops = log, tag, crops

    def sample(self, label):
        self.log.append(self.tag)
        return [(box, lab.copy()) for box, lab in self.crops]


@pytest.fixture()
def imdb(tmp_path):
    from PIL import Image
    gen = np.random.RandomState(9)
    paths, labels = [], []
    for k in range(5):
        h, w = 20 + 3 * k, 31 - 2 * k
        Image.fromarray(gen.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(str(tmp_path / ("im%d.png" % k)))
        lab = -np.ones((3, 5))
        lab[0] = [k, .1, .2, .5, .7]
        if k % 2:
            lab[1] = [k + 1, .3, .1, .9, .6]
        paths.append(str(tmp_path / ("im%d.png" % k)))
        labels.append(lab)
    return _Imdb(paths, labels)


@pytest.fixture()
def host_launch(monkeypatch):
    """DetIter._device_batch by the restatement; -> the list of everything it was handed"""
    seen = []

    def device_batch(self, prep):
        seen.append(prep)
        return ref.device_batch_on_host(self, prep)
    monkeypatch.setattr(di.DetIter, "_device_batch", device_batch)
    return seen


def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_det_iter_draw_order(imdb, host_launch, monkeypatch):
    log = []
    real = np.random.uniform
    monkeypatch.setattr(np.random, "uniform", lambda *a, **k: (log.append("uniform"), real(*a, **k))[1])
    lab = -np.ones((3, 5))
    lab[0] = [7, .2, .2, .6, .6]
    none, some = _FixedSampler(log, "s0", []), _FixedSampler(log, "s1", [((.25, .25, .75, .75), lab)])
    # no crop: samplers in list order, no pick draw, the interpolation draw, the mirror draw
    it = di.DetIter(imdb, 2, (3, 8, 10), rand_samplers=[none, _FixedSampler(log, "s0b", [])], rand_mirror=True, device="cpu")
    assert log == ["s0", "s0b", "uniform", "uniform"] * 2
    # a crop exists: the pick draw comes between the samplers and the interpolation draw
    del log[:]
    it = di.DetIter(imdb, 2, (3, 8, 10), rand_samplers=[none, some], rand_mirror=True, device="cpu")
    assert log == ["s0", "s1", "uniform", "uniform", "uniform"] * 2
    assert tuple(host_launch[-1]["samples"]["canvas_w"]) == (int(.75 * 31) - int(.25 * 31), int(.75 * 29) - int(.25 * 29))
    assert (it._label[:, 0, 0] == 7).all()                      # the label is the crop's
    # no mirror: no mirror draw; not training: no sampler is asked, the interpolation draw still happens, always linear
    del log[:]
    di.DetIter(imdb, 2, (3, 8, 10), rand_samplers=[none, some], rand_mirror=False, device="cpu")
    assert log == ["s0", "s1", "uniform", "uniform"] * 2
    del log[:]
    it = di.DetIter(imdb, 2, (3, 8, 10), rand_samplers=[none, some], rand_mirror=True, is_train=False, device="cpu")
    assert log == ["uniform"] * 2 and (host_launch[-1]["samples"]["kx"] == 2).all()
    assert not host_launch[-1]["samples"]["mirror"].any()


def test_det_iter_seed_and_constructor_batch(imdb, host_launch):
    np.random.seed(5)
    probe = np.random.uniform(0, 1, 4)
    # the constructor builds one batch: two interpolation draws are gone before the first next()
    it = di.DetIter(imdb, 2, 8, rand_seed=5, device="cpu")
    assert len(host_launch) == 1 and np.random.uniform(0, 1) == probe[2]
    # rand_seed=0 does not seed: the stream goes on from where it is
    np.random.seed(5)
    di.DetIter(imdb, 2, 8, rand_seed=0, device="cpu")
    np.random.seed(5)
    np.random.uniform(0, 1)
    di.DetIter(imdb, 2, 8, rand_seed=0, device="cpu")
    assert np.random.uniform(0, 1) == probe[3]
    # the methods the draws pick are the reference's list order
    np.random.seed(5)
    it = di.DetIter(imdb, 2, 8, device="cpu")
    taps = {di.LINEAR: 2, di.CUBIC: 4, di.NEAREST: 1, di.LANCZOS4: 8}
    for k in range(2):
        method = int(probe[k] * 5)
        s = host_launch[-1]["samples"][k]
        if method in taps:
            assert s["kx"] == taps[method] and s["ky"] == taps[method]
    assert it.provide_data == [("data", (2, 3, 8, 8))] and it.provide_label == [("label", (2, 3, 5))]


def test_det_iter_epoch_padding_and_indices(imdb, host_launch):
    np.random.seed(1)
    it = di.DetIter(imdb, 2, (3, 8, 10), shuffle=True, device="cpu")
    view, seen = it.fit_view(), []
    for epoch in range(2):
        got = []
        while view.iter_next():
            pad, index = it.getpad(), it.getindex()
            batch, indices = view.next()
            assert (batch.pad, batch.index) == (pad, index) and batch.label[1] is None and len(batch.label) == 2
            assert tuple(batch.data[0].shape) == (2, 3, 8, 10) and tuple(batch.label[0].shape) == (2, 3, 5)
            got.append((indices, batch.pad, batch.index))
        seen.append(got)
        order = list(it._index)
        if epoch == 0:
            assert order == [0, 1, 2, 3, 4]                     # no shuffle until reset()
        # five images at batch 2: the third batch holds the last image and pads from the middle, (4 + 1 + 5 // 2) % 5 = 2
        assert [g[0] for g in got] == [order[0:2], order[2:4], [order[4], order[2]]]
        assert [g[1:] for g in got] == [(0, 0), (0, 1), (1, 2)]
        with pytest.raises(StopIteration):
            it.next()
        view.reset()
    assert sorted(it._index) == [0, 1, 2, 3, 4] and list(it._index) != [0, 1, 2, 3, 4]


def test_det_iter_not_training(imdb, host_launch):
    it = di.DetIter(imdb, 2, (3, 8, 10), mean_pixels=[1, 2, 3], is_train=False, rand_mirror=True,
                    rand_samplers=[rs.RandCropper(min_scale=.3, max_trials=25)], device="cpu")
    assert it.provide_label == []
    batches = [it.next() for _ in range(3)]
    assert batches[0].label == [None]
    last = batches[-1]
    assert last.pad == 1 and host_launch[-1]["count"] == 1
    assert not last.data[0][1].any()                            # the slot past the end stays a zero image
    img = _pixels(imdb.paths[4])
    _, _, _, want = ref.augment_images([img], [None], [di.LINEAR], [False], 8, 10, (1., 2., 3.))
    assert np.array_equal(last.data[0][0].numpy(), want[0])


def test_det_iter_mirror_flips_valid_rows_only(imdb, host_launch):
    for seed in range(40):                                      # a seed whose first two mirror draws differ
        np.random.seed(seed)
        draws = np.random.uniform(0, 1, 4)
        if (draws[1] > .5) != (draws[3] > .5):
            break
    np.random.seed(seed)
    it = di.DetIter(imdb, 2, (3, 8, 10), rand_mirror=True, device="cpu")
    flags = [draws[1] > .5, draws[3] > .5]
    assert list(host_launch[-1]["samples"]["mirror"]) == [int(f) for f in flags]
    for k in range(2):
        want = imdb.labels[k].copy()
        if flags[k]:
            valid = want[:, 0] > -1
            x0 = want[valid, 1].copy()
            want[valid, 1] = 1.0 - want[valid, 3]
            want[valid, 3] = 1.0 - x0
        assert np.array_equal(it._label[k].numpy(), want.astype(np.float32))
        assert (it._label[k].numpy()[imdb.labels[k][:, 0] < 0] == -1).all()
        img = _pixels(imdb.paths[k])
        method = int(draws[2 * k] * 5)
        _, _, _, data = ref.augment_images([img], [None], [method], [flags[k]], 8, 10, (128., 128., 128.))
        assert np.array_equal(it._data[k].numpy(), data[0])
    assert np.array_equal(imdb.labels[0][0], [0, .1, .2, .5, .7])    # the database's labels are not written to


def test_list_imdb_round_trip(tmp_path):
    labels = [np.array([[1, .1, .2, .3, .4], [2, .5, .5, .75, .875]]), np.array([[0, .25, .125, .5, .625]]),
              np.array([[3, .0, .0, 1., 1.], [4, .2, .2, .4, .4], [5, .6, .6, .8, .8]])]
    paths = ["a/x.jpg", "b.jpg", "c d.jpg"]
    with open(str(tmp_path / "t.lst"), "w") as f:              # Imdb.save_imglist (dataset/imdb.py:81-82)
        for k, (lab, path) in enumerate(zip(labels, paths)):
            f.write("\t".join([str(k), str(2), str(lab.shape[1])] + ["{0:.4f}".format(x) for x in lab.ravel()] + [path]) + "\n")
    db = di.ListImdb(str(tmp_path / "t.lst"), "/data")
    assert db.num_images == 3 and db.image_path_from_index(2) == "/data/c d.jpg"
    for k, lab in enumerate(labels):
        got = db.label_from_index(k)
        assert got.shape == (3, 5) and got.dtype == np.float64
        assert np.array_equal(got[:lab.shape[0]], lab) and (got[lab.shape[0]:] == -1).all()
    six = di.ListImdb(str(tmp_path / "t.lst"), "/data", label_width=6, pad_rows=4)
    got = six.label_from_index(1)
    assert got.shape == (4, 6) and np.array_equal(got[0], [0, .25, .125, .5, .625, 0.]) and (got[1:] == -1).all()
    with pytest.raises(ValueError):
        di.ListImdb(str(tmp_path / "t.lst"), "/data", pad_rows=2)
    with pytest.raises(ValueError):
        di.ListImdb(str(tmp_path / "t.lst"), "/data", label_width=7)


def test_entry_checks_arguments_before_any_hip_call():
    import ctypes
    lib = _lib.lib()
    mean = (ctypes.c_double * 3)(0, 0, 0)
    assert lib.dspn_det_augment_batch_u8(None, 256, 256, 1, 8, 8, mean, 256, None) == -1
    assert b"null argument" in lib.dspn_last_error()
    assert lib.dspn_det_augment_batch_u8(256, 256, 256, 0, 8, 8, mean, 256, None) == -1 and b"bad shape" in lib.dspn_last_error()
    assert lib.dspn_det_augment_batch_u8(256, 256, 256, 1, 8, 0, mean, 256, None) == -1
    assert lib.dspn_det_augment_batch_u8(256, 256, 256, 1, 70000, 8, mean, 256, None) == -1
