"""The polygon rasteriser on the device (include/dspn_polygon.h) == tests/ref_polygon.py, which tests/test_polygon_host.py
holds equal to Pillow: owner map and the four looked-up outputs, every comparison an equality.  Nothing here needs
Pillow; the one picture taken from Pillow is the recorded street scene under tests/golden/."""
import itertools
import os

import numpy as np
import pytest

import ref_polygon as rp

pytestmark = pytest.mark.gpu

HAND = {k: rp.int_points(v) for k, v in rp.HAND_CASES.items()}


def _values(order):
    """the table row of the polygon painted `order`-th: distinct in every column, beyond 255 in the int32 ones"""
    return ((order * 7) % 256, (order * 13 + 5) % 256, order * 1000 + 3, order * 77 + 70000)


BACKGROUND = (0, 255, 0, 255)


def run(images, H, W, device, want_spill=None):
    """images: per image its polygons in painter's order -> the device's owner map, after checking it and the four
    outputs against the restatement"""
    import torch
    from dspnet_amd import functional as fn
    from dspnet_amd.dataset import cityscapes_labels as cl
    polygons, index, orders, table, offsets = [], [], [], [], []
    for b, polys in enumerate(images):
        offsets.append(len(table))
        table.append(BACKGROUND)
        for k, xy in enumerate(polys, 1):
            polygons.append(xy)
            index.append(b)
            orders.append(k)
            table.append(_values(k))
    spill = torch.zeros(1, dtype=torch.int32, device=device)
    owner = cl.rasterize(polygons, index, orders, len(images), H, W, device, spill_count=spill)
    outs = fn.polygon_resolve(owner, torch.tensor(table, dtype=torch.int32, device=device),
                              torch.tensor(offsets, dtype=torch.int32, device=device))
    got = owner.cpu().numpy()
    want = np.stack([rp.paint(H, W, [(xy, k) for k, xy in enumerate(polys, 1)]) for polys in images])
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    rows = np.asarray(table, np.int64)
    for c, (out, dtype) in enumerate(zip(outs, (np.uint8, np.uint8, np.int32, np.int32))):
        a = out.cpu().numpy()
        expect = np.stack([rows[offsets[b] + want[b], c] for b in range(len(images))]).astype(dtype)
        assert a.dtype == dtype and np.array_equal(a, expect), c
    if want_spill is not None:
        assert int(spill.item()) == want_spill
    return got


@pytest.mark.parametrize("W", [1, 63, 64, 65, 150])
def test_hand_cases_one_per_image(gpu_device, W):
    names = sorted(HAND)
    run([[HAND[n]] for n in names], 13, W, gpu_device)


def test_hand_cases_shifted_across_the_chunk_boundary(gpu_device):
    """the same shapes moved so that their spans straddle x = 64 and x = 128 of a 150-wide image"""
    run([[[(x + dx, y) for x, y in HAND[n]]] for n in sorted(HAND) for dx in (57, 121)], 13, 150, gpu_device)


def test_batch_of_none_one_and_many(gpu_device):
    rng = np.random.default_rng(5)
    many = [[(int(rng.integers(-5, 75)), int(rng.integers(-5, 45))) for _ in range(int(rng.integers(2, 10)))]
            for _ in range(40)]
    got = run([[], [HAND["bow_tie"]], many], 40, 70, gpu_device)
    assert not got[0].any()


def test_painters_order_all_six(gpu_device):
    a = [(2, 2), (30, 4), (20, 28)]
    b = [(10, 1), (38, 12), (6, 24)]
    c = [(1, 14), (36, 9), (33, 30), (12, 31)]
    got = run([list(p) for p in itertools.permutations([a, b, c])], 33, 41, gpu_device)
    assert len({g.tobytes() for g in got}) == 6


def test_more_polygons_than_a_byte_and_the_largest_order(gpu_device):
    """the order key is the whole int32: nothing is packed beside it, so no polygon count is special.  300 polygons in
    one image pass 255 (where an 8-bit key would wrap), and the orders 2^31 - 2 and 2^31 - 1 still compare"""
    import torch
    from dspnet_amd.dataset import cityscapes_labels as cl
    rng = np.random.default_rng(6)
    polys = []
    for _ in range(300):
        x, y = int(rng.integers(0, 60)), int(rng.integers(0, 44))
        polys.append([(x, y), (x + int(rng.integers(1, 9)), y + int(rng.integers(0, 4))), (x + int(rng.integers(0, 5)), y + int(rng.integers(1, 9)))])
    got = run([polys], 48, 64, gpu_device)
    assert got.max() > 255
    tri, quad = [(1, 1), (14, 3), (5, 12)], [(3, 0), (12, 0), (12, 9), (3, 9)]
    top = 2 ** 31 - 1
    for orders in ((top - 1, top), (top, top - 1)):
        owner = cl.rasterize([tri, quad], [0, 0], list(orders), 1, 14, 16, gpu_device).cpu().numpy()[0]
        want = np.maximum(rp.paint(14, 16, [(tri, orders[0])]), rp.paint(14, 16, [(quad, orders[1])]))
        assert np.array_equal(owner, want)


def _comb_tables(teeth, H, W, capacity):
    from dspnet_amd.dataset import cityscapes_labels as cl
    xy = rp.comb(teeth)
    return xy, cl.polygon_tables([xy], [0], [1], H, W, capacity)


def test_both_routes_through_the_c_abi(gpu_device):
    """the entries of a row on either side of what one wave keeps in LDS.  A comb of t teeth has 4 t + 2 entries on the
    row where its teeth end; the job's entry bound is then raised to exactly the capacity (still the LDS route) and to
    one more (the spill route), and the device's own count of spilled jobs is read back."""
    import torch
    from dspnet_amd import functional as fn
    cap = fn.polygon_wave_entries()
    H = 12
    for teeth, spills in ((cap // 4 - 1, False), (cap // 4, True)):
        W = 2 * teeth + 6
        xy, (edges, polys, jobs, scratch) = _comb_tables(teeth, H, W, cap)
        assert jobs[:, 3].max() == 4 * teeth + 2 and (jobs[:, 3].max() > cap) == spills
        run([[xy]], H, W, gpu_device, want_spill=int((jobs[:, 3] > cap).sum()))
    # the same comb below the capacity, its bounds moved to the two sides of it by hand
    teeth = cap // 4 - 1
    W = 2 * teeth + 6
    xy, (edges, polys, jobs, _) = _comb_tables(teeth, H, W, cap)
    want = rp.paint(H, W, [(xy, 1)])
    dev = [torch.from_numpy(t).to(gpu_device) for t in (edges, polys)]
    for bound, spilled in ((cap, 0), (cap + 1, 1)):
        j = jobs.copy()
        widest = int(np.argmax(j[:, 3]))
        j[widest, 3], j[widest, 4] = bound, 0
        count = torch.zeros(1, dtype=torch.int32, device=gpu_device)
        owner = fn.polygon_rasterize(dev[0], dev[1], torch.from_numpy(j).to(gpu_device), 2 * (cap + 1), 1, H, W,
                                     spill_count=count)
        assert np.array_equal(owner.cpu().numpy()[0], want)
        assert int(count.item()) == spilled


def test_spill_route_on_every_row(gpu_device):
    """every job forced down the spill route (bounds above the capacity, offsets laid out here): same picture"""
    import torch
    from dspnet_amd import functional as fn
    from dspnet_amd.dataset import cityscapes_labels as cl
    cap = fn.polygon_wave_entries()
    names = [n for n in sorted(HAND)]
    H, W = 13, 80
    edges, polys, jobs, _ = cl.polygon_tables([HAND[n] for n in names], list(range(len(names))), [1] * len(names), H, W, cap)
    jobs = jobs.copy()
    jobs[:, 3] = cap + 1 + np.arange(len(jobs)) % 3
    jobs[:, 4] = np.cumsum(2 * jobs[:, 3]) - 2 * jobs[:, 3]
    count = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    owner = fn.polygon_rasterize(*[torch.from_numpy(t).to(gpu_device) for t in (edges, polys, jobs)],
                                 int((2 * jobs[:, 3]).sum()), len(names), H, W, spill_count=count)
    want = np.stack([rp.paint(H, W, [(HAND[n], 1)]) for n in names])
    assert np.array_equal(owner.cpu().numpy(), want)
    assert int(count.item()) == len(jobs)


@pytest.mark.parametrize("H", [1, 5, 9])
def test_rows_clipped_at_top_and_bottom(gpu_device, H):
    polys = [[(3, -7), (20, -2), (14, 15), (1, 11)], [(8, 2), (25, 3), (17, 30)], [(0, -3), (30, -3), (30, H + 3), (0, H + 3)],
             [(5, H), (9, H - 1), (12, H)], [(5, H - 1), (9, H - 2), (12, H - 1)], [(2, 0), (6, 0), (4, -5)]]
    run([[p] for p in polys] + [polys], H, 31, gpu_device)


def test_street_scene_against_pillows_recording(gpu_device):
    from dspnet_amd.dataset import cityscapes_labels as cl
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "polygon_street_scene.npz"))
    cuts = np.cumsum(g["counts"])[:-1]
    polys = [[(int(x), int(y)) for x, y in p] for p in np.split(g["points"], cuts)]
    owner = cl.rasterize(polys, [0] * len(polys), list(range(1, len(polys) + 1)), 1, 1024, 2048, gpu_device)
    got = owner.cpu().numpy()[0]
    want = g["owner"].astype(np.int32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
