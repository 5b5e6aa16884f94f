"""tests/ref_polygon.py == the installed Pillow, pixel for pixel: ImageDraw.polygon(xy, fill=v) without outline, modes L
and I.  No case is skipped or tolerated.  The host tables of the device rasteriser (dataset/cityscapes_labels.py) are
held to the same pictures through the kernel's arithmetic replayed on the host (ref_polygon.owner_from_tables)."""
import itertools

import numpy as np
import pytest
from PIL import Image, ImageDraw

import ref_polygon as rp


def pillow(W, H, xy, value=7, mode="L"):
    im = Image.new(mode, (W, H), 0)
    ImageDraw.Draw(im).polygon(xy, fill=value)
    return np.array(im)


def same(W, H, xy, value=7, mode="L"):
    want = pillow(W, H, xy, value, mode)
    got = rp.fill_polygon(np.zeros((H, W), want.dtype), xy, value)
    assert np.array_equal(got, want), (W, H, xy, np.argwhere(got != want)[:8].tolist())


HAND = rp.HAND_CASES


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    W = 80 if name.startswith("comb") else 16
    for mode, value in (("L", 200), ("I", 70000)):
        same(W, 13, HAND[name], value, mode)


def test_one_point_is_refused_as_by_pillow():
    with pytest.raises(TypeError):
        pillow(8, 8, [(3, 3)])
    with pytest.raises(TypeError):
        rp.fill_polygon(np.zeros((8, 8), np.uint8), [(3, 3)], 1)


def test_flat_coordinate_list():
    want = pillow(16, 13, [2, 2, 12, 3, 6, 11])
    assert np.array_equal(rp.fill_polygon(np.zeros((13, 16), np.uint8), [2, 2, 12, 3, 6, 11], 7), want)


def test_every_lattice_triangle():
    """every ordered triangle on a 6 x 6 lattice, stretched and shifted so that some vertices fall outside the 8 x 8 image"""
    lattice = [(x - 1 + (x > 3) * 3, y - 1 + (y > 2) * 3) for x in range(6) for y in range(6)]
    bad = []
    for tri in itertools.permutations(lattice, 3):
        want = pillow(8, 8, list(tri))
        if not np.array_equal(rp.fill_polygon(np.zeros((8, 8), np.uint8), list(tri), 7), want):
            bad.append(tri)
    assert not bad, (len(bad), bad[:5])


def random_corpus(seed, count, max_side=40, max_vertices=12):
    rng = np.random.default_rng(seed)
    for t in range(count):
        W, H = int(rng.integers(4, max_side)), int(rng.integers(4, max_side))
        lo = -6 if t % 3 == 0 else 0
        n = int(rng.integers(3, max_vertices + 1))
        yield W, H, [(int(rng.integers(lo, W - lo)), int(rng.integers(lo, H - lo))) for _ in range(n)]


def test_random_corpus():
    bad = []
    for W, H, xy in random_corpus(20261020, 3200):
        if not np.array_equal(rp.fill_polygon(np.zeros((H, W), np.uint8), xy, 7), pillow(W, H, xy)):
            bad.append((W, H, xy))
    assert not bad, (len(bad), bad[:3])


def test_small_dense_corpus():
    """tiny images, few vertices: shared vertices, retraced edges and touching corners are the common case here"""
    bad = []
    for W, H, xy in random_corpus(7, 6000, max_side=11, max_vertices=6):
        if not np.array_equal(rp.fill_polygon(np.zeros((H, W), np.uint8), xy, 7), pillow(W, H, xy)):
            bad.append((W, H, xy))
    assert not bad, (len(bad), bad[:3])


def test_street_scene_golden_is_what_pillow_paints():
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "polygon_street_scene.npz"))
    polys = rp.street_scene(20261020)
    assert np.array_equal(np.concatenate([np.asarray(p, np.int32) for p in polys]), g["points"])
    im = Image.new("I", (2048, 1024), 0)
    for k, xy in enumerate(polys):
        ImageDraw.Draw(im).polygon(xy, fill=k + 1)
    assert np.array_equal(np.array(im), g["owner"].astype(np.int32))


def test_host_tables_replay_to_the_restatement():
    """polygon_tables + the kernel's arithmetic on the host == painting the polygons one after the other; a capacity of
    4 entries sends many rows down the spill route's offsets, which must not overlap and must be large enough"""
    from dspnet_amd.dataset import cityscapes_labels as cl
    rng = np.random.default_rng(3)
    cases = [[HAND[k] for k in sorted(HAND) if k != "float_vertices"]]
    for t in range(150):
        W, H = int(rng.integers(4, 40)), int(rng.integers(4, 40))
        lo = -6 if t % 3 == 0 else 0
        cases.append([[(int(rng.integers(lo, W - lo)), int(rng.integers(lo, H - lo))) for _ in range(int(rng.integers(2, 13)))]
                      for _ in range(int(rng.integers(1, 4)))])
    for polys in cases:
        H, W = 24, 36
        e, p, j, scratch = cl.polygon_tables(polys, [0] * len(polys), list(range(1, len(polys) + 1)), H, W, 4)
        want = rp.paint(H, W, [(xy, k + 1) for k, xy in enumerate(polys)])
        assert np.array_equal(rp.owner_from_tables(e, p, j, 1, H, W)[0], want), polys
        spill = j[j[:, 3] > 4]
        if len(spill):
            ends = spill[:, 4] + 2 * spill[:, 3]
            assert (spill[1:, 4] >= ends[:-1]).all() and ends.max() <= scratch
