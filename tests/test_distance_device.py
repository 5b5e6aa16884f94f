"""Box-median selection (include/dspn_distance.h): what can be checked without a GPU -- the slice helper the kernel's
box table is written in, the argument checks of the C entries, and the host arithmetic of the distance labels."""
import ctypes

import numpy as np
import pytest

from dspnet_amd import _lib
from dspnet_amd import functional as fn


@pytest.mark.parametrize("size", [1, 2, 5, 8])
def test_slice_bounds_is_numpy_slicing(size):
    axis = np.arange(size)
    for start in range(-size - 2, size + 3):
        for stop in range(-size - 2, size + 3):
            lo, hi = fn.slice_bounds(start, stop, size)
            want = axis[start:stop]
            assert 0 <= lo <= hi <= size, (start, stop, lo, hi)
            assert hi - lo == want.size, (start, stop, lo, hi)
            np.testing.assert_array_equal(axis[lo:hi], want)
    assert fn.slice_bounds(3, 10 ** 12, size) == (min(3, size), size)      # far beyond the size: clipped


def test_rank_select_rejects_bad_arguments_without_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks first

    for call in (lib.dspn_box_rank_select_f32, lib.dspn_box_rank_select_u16):
        assert call(p, 1, 8, 8, p, -1, None, p, p, None) == -1 and b"K < 0" in lib.dspn_last_error()
        assert call(p, 1, 0, 8, p, 1, None, p, p, None) == -1 and b"> 0" in lib.dspn_last_error()
        assert call(p, 1, 8, -3, p, 1, None, p, p, None) == -1 and b"> 0" in lib.dspn_last_error()
        assert call(p, 0, 8, 8, p, 1, None, p, p, None) == -1
        assert call(p, 1, 1 << 16, 1 << 15, p, 1, None, p, p, None) == -1 and b"2^31" in lib.dspn_last_error()
        assert call(None, 1, 8, 8, p, 1, None, p, p, None) == -1 and b"null pointer" in lib.dspn_last_error()
        assert call(p, 1, 8, 8, None, 1, None, p, p, None) == -1 and b"null pointer" in lib.dspn_last_error()
        assert call(p, 1, 8, 8, p, 1, None, None, p, None) == -1
        assert call(p, 1, 8, 8, p, 1, None, p, None, None) == -1
        assert call(None, 1, 8, 8, None, 0, None, None, None, None) == 0        # K == 0: nothing to do, no HIP call


def test_distance_boxes_rejects_bad_arguments_without_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)

    def boxes(det=p, B=2, N=10, hh=8, ww=8, mode=0, max_boxes=4, out=p, src=p, count=p, ws=p, ws_bytes=1 << 10):
        return lib.dspn_distance_boxes_f32(det, B, N, hh, ww, 0.1, mode, max_boxes, out, src, count, ws, ws_bytes, None)

    assert boxes(hh=0) == -1 and b"hh and ww" in lib.dspn_last_error()
    assert boxes(ww=-1) == -1 and b"hh and ww" in lib.dspn_last_error()
    assert boxes(mode=2) == -1 and b"mode is 0" in lib.dspn_last_error()
    assert boxes(mode=-1) == -1 and b"mode is 0" in lib.dspn_last_error()
    assert boxes(B=-1) == -1 and b"negative" in lib.dspn_last_error()
    assert boxes(N=-1) == -1 and boxes(max_boxes=-1) == -1
    assert boxes(B=1 << 16, N=1 << 15) == -1 and b"2^31" in lib.dspn_last_error()
    assert boxes(count=None) == -1 and b"null count" in lib.dspn_last_error()
    assert boxes(det=None) == -1 and b"null pointer" in lib.dspn_last_error()
    assert boxes(out=None) == -1 and boxes(src=None) == -1
    assert boxes(ws=None) == -2 and b"workspace too small" in lib.dspn_last_error()
    assert boxes(ws_bytes=7) == -2 and b"workspace too small" in lib.dspn_last_error()


def test_workspace_query_is_pure():
    lib = _lib.lib()
    assert lib.dspn_distance_boxes_workspace_bytes(32) == 32 * 4
    assert lib.dspn_distance_boxes_workspace_bytes(1) == 4
    assert lib.dspn_distance_boxes_workspace_bytes(0) == 0 and lib.dspn_distance_boxes_workspace_bytes(-5) == 0


def test_wrappers_reject_what_the_kernel_does_not_take():
    import torch
    with pytest.raises(AssertionError):
        fn.box_rank_select(torch.zeros(1, 4, 4, dtype=torch.float64), torch.zeros(1, 5, dtype=torch.int32))
    with pytest.raises(AssertionError):
        fn.box_rank_select(torch.zeros(1, 4, 4), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(AssertionError):
        fn.distance_boxes(torch.zeros(1, 4, 6), 8, 8, 0.1, 0, 4)
    with pytest.raises(_lib.DspnError, match="max_boxes = 4"):
        fn.check_box_count(5, 4)
    fn.check_box_count(4, 4)


def test_label_arithmetic_hand_cases():
    from dspnet_amd.dataset import distance_labels as dl
    # the 50 m case of test_distance_metric_hand_case: 2200 * 75 / (3300 + 1e-3) = 49.99998...
    assert dl.distance_from_median(np.float32(3300.0)) == 50
    # 2200 * 75 / 100.001 = 1649.98 m: beyond 1000 -> 200; so is a box of zeros (1.65e8 m)
    assert dl.distance_from_median(100.0) == 200 and dl.distance_from_median(0.0) == 200
    assert dl.distance_from_median(2200. * 75. / 1000. - 1e-3 + 1e-6) == 1000      # just inside the rule
    # halves go away from zero (Python 2's round), where Python 3's round() goes to even
    q = 165000. / 64.5 - 1e-3
    assert 2200. * 75. / (q + 1e-3) == 64.5 and round(64.5) == 64
    assert dl.distance_from_median(q) == 65
    assert [dl.round_half_away(v) for v in (0.5, 1.5, 2.5, 2.4999999, -0.5, -2.5, 3.0, 0.49999999999999994)] == \
        [1, 2, 3, 2, -1, -3, 3, 0]


def test_label_boxes_follow_the_script():
    from dspnet_amd.dataset import distance_labels as dl
    hh, ww = 100, 200
    boxes = [[40, 20, 80, 40], [-5, -7, 10, 10], [30, 5, 30, 9], [150, 50, 400, 300], [10, 10, 5, 20], [10, 10, 20, -10],
             [250, 0, 260, 10]]
    got = dl.resolve_boxes(boxes, hh, ww)
    disp = np.arange(hh * ww).reshape(hh, ww)
    for (xmin, ymin, xmax, ymax), (x0, x1, y0, y1) in zip(boxes, got.tolist()):
        xmin, ymin = max(0, xmin), max(0, ymin)
        if xmin == xmax:
            xmax = xmin + 1
        np.testing.assert_array_equal(disp[y0:y1, x0:x1].ravel(), disp[ymin:ymax, xmin:xmax].ravel())
    assert got[2].tolist() == [30, 31, 5, 9] and got[3].tolist() == [150, 200, 50, 100]
    assert got[4, 0] == got[4, 1] and got[6, 0] == got[6, 1]                 # empty regions
    assert got[5].tolist() == [10, 20, 10, 90]                                # a negative stop counts from the end
    with pytest.raises(ValueError, match="box 1 covers no pixel"):
        dl.box_distances(np.zeros((hh, ww), np.float32), [[1, 1, 5, 5], [10, 10, 5, 20]], device="cpu")
