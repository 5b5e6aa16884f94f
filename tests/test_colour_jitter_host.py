"""Colour jitter without a GPU: the two restatements of include/dspn_colour_jitter.h against each other and against the
real-valued HLS model (Python's colorsys), the parameter draws, the configuration and the descriptor layout."""
import colorsys
import os
import re

import numpy as np
import pytest

import ref_colour_jitter as ref
from dspnet_amd.dataset import colour_jitter as cj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge_colours():
    out = [(v, v, v) for v in (0, 1, 127, 128, 254, 255)]                                  # greys
    out += [(200, 55, 100), (55, 200, 100), (100, 55, 200), (255, 0, 77), (0, 77, 255)]    # sm == 255
    out += [(200, 56, 100), (56, 200, 100), (100, 56, 200), (255, 1, 77), (1, 77, 255)]    # sm == 256
    out += [(90, 90, 10), (90, 10, 90), (10, 90, 90), (255, 255, 0), (0, 255, 255), (255, 0, 255)]   # tied maxima
    out += [(a + da, a + db, a + dc) for a in (0, 100, 127, 254) for da, db, dc in
            ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1))]            # d == 1
    out += [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 0, 1), (255, 1, 0), (254, 0, 255)]
    return out


@pytest.fixture(scope="module")
def colours():
    gen = np.random.RandomState(31)
    return np.concatenate([np.asarray(_edge_colours()), gen.randint(0, 256, (4000, 3))]).astype(np.int64)


def _hls_grid():
    hs = [0, 1, 29, 30, 31, 59, 60, 61, 89, 90, 91, 119, 120, 121, 149, 150, 179, 180]
    ls = [0, 1, 64, 127, 128, 129, 200, 254, 255]
    ss = [0, 1, 2, 100, 128, 254, 255]
    return np.asarray([(h, l, s) for h in hs for l in ls for s in ss], np.int64)


def test_numpy_restatement_equals_the_exact_rationals(colours):
    H, L, S = ref.forward(colours)
    for k, c in enumerate(colours):
        assert (H[k], L[k], S[k]) == ref.forward_exact(*(int(v) for v in c)), c
    assert H.min() >= 0 and H.max() <= 179 and S.max() <= 255 and L.max() <= 255
    grid = _hls_grid()
    rgb = ref.inverse(grid[:, 0], grid[:, 1], grid[:, 2])
    assert rgb.min() >= 0 and rgb.max() <= 255
    for k, (h, l, s) in enumerate(grid):
        assert tuple(rgb[k]) == ref.inverse_exact(int(h), int(l), int(s)), (h, l, s)
    gen = np.random.RandomState(32)
    for k in range(600):
        p = (gen.randint(-180, 181), gen.randint(-255, 256), gen.randint(-255, 256), gen.randint(0, 4097))
        if k % 5 == 0:
            p = (0, 0, 0, p[3])                                  # the skip of the round trip
        if k % 7 == 0:
            p = p[:3] + (1024,)
        c = colours[k]
        assert tuple(ref.jitter(c, *p)) == ref.jitter_exact(c, *p), (c, p)


def test_identity_parameters_change_nothing_but_the_round_trip_would(colours):
    assert np.array_equal(ref.jitter(colours, 0, 0, 0, 1024), colours)
    H, L, S = ref.forward(colours)
    assert not np.array_equal(ref.inverse(H, L, S), colours)       # why the header skips it


def test_forward_is_within_half_a_level_and_one_degree_of_colorsys(colours):
    H, L, S = ref.forward(colours)
    for k, (r, g, b) in enumerate(colours):
        h, l, s = colorsys.rgb_to_hls(r / 255., g / 255., b / 255.)
        assert abs(L[k] - 255 * l) <= 0.5 + 1e-9, (r, g, b)
        assert abs(S[k] - 255 * s) <= 0.5 + 1e-9, (r, g, b)
        if r == g == b:
            assert H[k] == 0 and S[k] == 0
            continue
        diff = abs(2 * H[k] - 360 * h) % 360
        assert min(diff, 360 - diff) <= 1 + 1e-9, (r, g, b)


def test_inverse_is_within_half_a_level_of_colorsys():
    grid = _hls_grid()
    assert (grid[:, 0] == 180).any() and (grid[:, 2] == 0).any()
    rgb = ref.inverse(grid[:, 0], grid[:, 1], grid[:, 2])
    for k, (h, l, s) in enumerate(grid):
        want = colorsys.hls_to_rgb(h / 180., l / 255., s / 255.)
        assert max(abs(rgb[k][c] - 255 * want[c]) for c in range(3)) <= 0.5 + 1e-9, (h, l, s)


# ---- draw -----------------------------------------------------------------------------------------------------------
class Recorder(object):
    """a RandomState that writes down what was asked of it"""

    def __init__(self, seed):
        self._rs, self.calls = np.random.RandomState(seed), []

    def uniform(self, lo, hi):
        self.calls.append(("uniform", lo, hi))
        return self._rs.uniform(lo, hi)

    def randint(self, lo, hi):
        self.calls.append(("randint", lo, hi))
        return self._rs.randint(lo, hi)


TRAIN = cj.ColorJitter(random_hue_prob=0.5, random_saturation_prob=0.5, random_illumination_prob=0.5, random_contrast_prob=0.5)


def test_defaults_are_the_reference_s():
    want = [("random_hue_prob", 0.0), ("max_random_hue", 18), ("random_saturation_prob", 0.0), ("max_random_saturation", 32),
            ("random_illumination_prob", 0.0), ("max_random_illumination", 32), ("random_contrast_prob", 0.0),
            ("max_random_contrast", 0.5)]
    assert list(cj.ColorJitter._fields) == [k for k, _ in want]
    assert list(cj.ColorJitter()) == [v for _, v in want]
    assert cj.config(None) is None and cj.config(cj.ColorJitter()) is None and cj.config(dict(want)) is None
    assert cj.config(dict(want, random_hue_prob=0.5)) == cj.ColorJitter(random_hue_prob=0.5)
    with pytest.raises(ValueError):
        cj.config(cj.ColorJitter(random_hue_prob=0.5, max_random_hue=181))
    with pytest.raises(TypeError):
        cj.config(3)


def test_draw_is_a_function_of_the_seed():
    a = cj.draw(TRAIN, 64, np.random.RandomState(5))
    b = cj.draw(TRAIN, 64, np.random.RandomState(5))
    c = cj.draw(TRAIN, 64, np.random.RandomState(6))
    assert a.dtype == np.int32 and a.shape == (64, 4) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(cj.draw(TRAIN._asdict(), 64, np.random.RandomState(5)), a)
    assert np.abs(a[:, 0]).max() <= 18 and np.abs(a[:, 1]).max() <= 32 and np.abs(a[:, 2]).max() <= 32
    assert a[:, 3].min() >= 512 and a[:, 3].max() <= 1536
    for col in range(3):                                            # each component applied to some images, left off others
        assert (a[:, col] != 0).any() and (a[:, col] == 0).any()
    assert (a[:, 3] != 1024).any() and (a[:, 3] == 1024).any()


def test_draw_order_is_hue_saturation_illumination_contrast():
    cfg = cj.ColorJitter(0.5, 10, 0.5, 20, 0.5, 30, 0.5, 0.25)
    rec, twin = Recorder(7), np.random.RandomState(7)
    got = cj.draw(cfg, 40, rec)
    calls = iter(rec.calls)
    for row in got:
        want = [0, 0, 0, 1024]
        for col, m in ((0, 10), (2, 20), (1, 30)):                  # dh, then ds, then dl
            assert next(calls) == ("uniform", 0, 1)
            if twin.uniform(0, 1) < 0.5:
                assert next(calls) == ("randint", -m, m + 1)
                want[col] = twin.randint(-m, m + 1)
        assert next(calls) == ("uniform", 0, 1)
        if twin.uniform(0, 1) < 0.5:
            assert next(calls) == ("uniform", -0.25, 0.25)
            want[3] = int(np.rint((1 + twin.uniform(-0.25, 0.25)) * 1024))
        assert list(row) == want
    assert next(calls, None) is None


def test_probability_zero_draws_nothing():
    rec = Recorder(8)
    assert np.array_equal(cj.draw(cj.ColorJitter(), 9, rec), np.tile([0, 0, 0, 1024], (9, 1))) and rec.calls == []
    rec = Recorder(8)
    got = cj.draw(cj.ColorJitter(random_illumination_prob=1.0), 9, rec)
    assert [c[0] for c in rec.calls] == ["uniform", "randint"] * 9 and all(c[1:] == (-32, 33) for c in rec.calls[1::2])
    assert (got[:, [0, 2]] == 0).all() and (got[:, 3] == 1024).all()
    rec = Recorder(8)
    got = cj.draw(cj.ColorJitter(random_contrast_prob=1.0), 9, rec)
    assert [c[0] for c in rec.calls] == ["uniform", "uniform"] * 9 and (got[:, :3] == 0).all()


# ---- descriptors ----------------------------------------------------------------------------------------------------
def test_descriptor_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "dspn_colour_jitter.h")).read()
    assert cj.SAMPLE.itemsize == int(re.search(r"#define DSPN_JITTER_SAMPLE_BYTES (\d+)", text).group(1))
    assert cj.SAMPLE.itemsize % 8 == 0
    body = re.search(r"typedef struct dspn_jitter_sample \{(.*?)\} dspn_jitter_sample;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("long long", "").replace("int", "").split(",")]
    assert names == list(cj.SAMPLE.names)
    s = cj.describe([[1, -2, 3, 900], [0, 0, 0, 1024]], [7, 1 << 33], [(5, 6), (1, 2)])
    assert s["img_offset"].tolist() == [7, 1 << 33] and s["height"].tolist() == [5, 1] and s["width"].tolist() == [6, 2]
    assert [s[k].tolist() for k in ("dh", "dl", "ds", "gain")] == [[1, 0], [-2, 0], [3, 0], [900, 1024]]
    with pytest.raises(ValueError):
        cj.describe([[0, 0, 0, 1024]], [0, 1], [(1, 1)])


# ---- DetIter's host phase -------------------------------------------------------------------------------------------
class _Imdb(object):
    def __init__(self, paths, labels):
        self._paths, self._labels, self.num_images = paths, labels, len(paths)

    def image_path_from_index(self, index):
        return self._paths[index]

    def label_from_index(self, index):
        return self._labels[index]


def test_det_iter_draws_from_a_stream_of_its_own(tmp_path, monkeypatch):
    """the host phase hands the device phase one parameter row per sample, batch after batch out of RandomState(jitter_seed),
    and leaves the global stream where it is without the feature"""
    import ref_det_augment
    from PIL import Image
    from dspnet_amd.dataset import det_iterator as di
    from dspnet_amd.dataset import rand_sampler
    gen = np.random.RandomState(9)
    paths = []
    for k in range(4):
        Image.fromarray(gen.randint(0, 256, (20 + 3 * k, 31 - 2 * k, 3)).astype(np.uint8)).save(str(tmp_path / ("im%d.png" % k)))
        paths.append(str(tmp_path / ("im%d.png" % k)))
    db = _Imdb(paths, [np.array([[k, .1, .2, .5, .7], [-1] * 5]) for k in range(4)])
    seen = []

    def device_batch(self, prep):
        seen.append(prep["jitter"])
        return ref_det_augment.device_batch_on_host(self, prep)
    monkeypatch.setattr(di.DetIter, "_device_batch", device_batch)

    def run(**kw):
        del seen[:]
        it = di.DetIter(db, 2, (3, 8, 10), rand_samplers=[rand_sampler.RandCropper(min_scale=.3, max_trials=25)], rand_mirror=True,
                        shuffle=True, rand_seed=7, device="cpu", **kw)
        while it.iter_next():
            it.next()
        return list(seen), np.random.get_state()

    off, state_off = run()
    on, state_on = run(color_jitter=TRAIN, jitter_seed=3)
    evl, _ = run(color_jitter=TRAIN, jitter_seed=3, is_train=False)
    zero, state_zero = run(color_jitter=cj.ColorJitter(), jitter_seed=3)
    assert off == [None] * 3 and evl == [None] * 3 and zero == [None] * 3
    twin = np.random.RandomState(3)
    assert len(on) == 3 and all(np.array_equal(rows, cj.draw(TRAIN, 2, twin)) for rows in on)
    for other in (state_on, state_zero):
        assert state_off[0] == other[0] and np.array_equal(state_off[1], other[1]) and state_off[2:] == other[2:]


def test_apply_with_identity_rows_touches_nothing(monkeypatch):
    """no descriptor is built, nothing is uploaded, nothing is launched: a tensor that is not even on a device passes"""
    import torch
    monkeypatch.setattr(cj, "launch", lambda *a, **k: pytest.fail("a launch was attempted"))
    monkeypatch.setattr(cj, "describe", lambda *a, **k: pytest.fail("descriptors were built"))
    pool = torch.zeros(12, dtype=torch.uint8)
    assert cj.apply(pool, [[0, 0, 0, 1024]] * 2, [0, 6], [(1, 2), (2, 1)]) == ()
    assert cj.apply(pool, np.zeros((0, 4), np.int32), [], []) == ()
