"""Writes tests/golden/rand_sampler.npz: what the reference's samplers (tools/rand_sampler.py) return for fixed seeds.

    python tests/golden/make_rand_sampler_golden.py [path of the reference's rand_sampler.py]

The reference module is imported by path and run unchanged under Python 3; numpy 2 removed the `np.lib.pad` alias it
calls, so `np.lib.pad = np.pad` is put back first (the same function).  None of the module's text is here.

Per case the fixture holds, for CALLS calls of `sample(label)` after `np.random.seed(seed)` (every call gets a fresh copy of
the case's label): the number of samples of each call, all crop boxes, all output labels, and the position of the MT19937
stream after each call (the index into the key block and a CRC of the block).  CASES is read by
tests/test_det_iterator_host.py, which replays them on dspnet_amd.dataset.rand_sampler."""
import importlib.util
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CALLS = 60

# class, x0, y0, x1, y1; -1 rows below
LABEL_A = np.array([[1, .10, .15, .45, .60], [3, .55, .30, .90, .85], [0, .40, .05, .62, .28],
                    [-1, -1, -1, -1, -1], [-1, -1, -1, -1, -1]], np.float64)
LABEL_BIG = np.array([[2, .08, .10, .93, .90], [5, .42, .44, .58, .57], [-1, -1, -1, -1, -1]], np.float64)
LABEL_SMALL = np.array([[4, .30, .30, .42, .38], [6, .05, .50, .95, .97], [-1, -1, -1, -1, -1]], np.float64)
# boxes along the border: a crop that touches one without holding its centre is refused, so even min_overlap .1 fails
LABEL_RING = np.array([[1, .0, .0, .5, .12], [2, .5, .0, 1, .12], [3, .0, .88, .5, 1], [0, .5, .88, 1, 1],
                       [4, .0, .12, .1, .88], [5, .9, .12, 1, .88]], np.float64)
LABEL_NONE = -np.ones((3, 5), np.float64)

_CROP = dict(min_scale=.3, max_scale=1., min_aspect_ratio=.5, max_aspect_ratio=2., max_trials=25)
# name -> (class name, constructor arguments, label, seed); the five croppers are config/config.py:39-44
CASES = {
    "crop_01": ("RandCropper", dict(_CROP, min_overlap=.1), LABEL_RING, 233),
    "crop_03": ("RandCropper", dict(_CROP, min_overlap=.3), LABEL_A, 233),
    "crop_05": ("RandCropper", dict(_CROP, min_overlap=.5), LABEL_A, 233),
    "crop_07": ("RandCropper", dict(_CROP, min_overlap=.7), LABEL_A, 233),
    "crop_09": ("RandCropper", dict(_CROP, min_overlap=.9), LABEL_BIG, 233),
    "pad": ("RandPadder", dict(min_scale=1., max_scale=4., min_aspect_ratio=.5, max_aspect_ratio=2., min_gt_scale=.05,
                               max_trials=25, max_sample=2), LABEL_SMALL, 233),
    "crop_x3": ("RandCropper", dict(_CROP, min_overlap=.3, max_sample=3), LABEL_A, 7),
    "pad_none": ("RandPadder", dict(min_scale=1., max_scale=4., min_aspect_ratio=.5, max_aspect_ratio=2.,
                                    min_gt_scale=.05, max_trials=25, max_sample=2), LABEL_NONE, 11),
}
# the cropper takes the maximum of an empty IoU vector on a label without a valid row: the reference raises ValueError
RAISES = ("RandCropper", dict(_CROP, min_overlap=.1), LABEL_NONE, 11)


def stream_position(state):
    """(index into the key block, CRC of the block) of an MT19937 state tuple"""
    return int(state[2]), zlib.crc32(np.ascontiguousarray(state[1]).tobytes())


def run_case(module, case, rng=None):
    """CALLS calls of the sampler of `module` -> dict of arrays.  rng=None: the global stream, seeded here (the reference
    knows no other); otherwise the RandomState the sampler is given."""
    cls, kwargs, label, seed = case
    if rng is None:
        np.random.seed(seed)
        sampler = getattr(module, cls)(**kwargs)
        state = np.random.get_state
    else:
        sampler = getattr(module, cls)(rng=rng, **kwargs)
        state = rng.get_state
    counts, boxes, labels, pos = [], [], [], []
    for _ in range(CALLS):
        got = sampler.sample(label.copy())
        counts.append(len(got))
        for box, lab in got:
            boxes.append(np.asarray(box, np.float64))
            labels.append(np.asarray(lab, np.float64))
        pos.append(stream_position(state()))
    return {"counts": np.asarray(counts, np.int64),
            "boxes": np.asarray(boxes, np.float64).reshape(-1, 4),
            "labels": np.asarray(labels, np.float64).reshape((len(labels),) + label.shape),
            "pos": np.asarray(pos, np.int64)}


def main(argv):
    path = argv[1] if len(argv) > 1 else "/root/reference/tools/rand_sampler.py"
    if not hasattr(np.lib, "pad"):
        np.lib.pad = np.pad
    spec = importlib.util.spec_from_file_location("reference_rand_sampler", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, case in CASES.items():
        got = run_case(ref, case)
        print("%-9s accepted %3d samples in %d calls, %d calls without one" %
              (name, got["counts"].sum(), CALLS, (got["counts"] == 0).sum()))
        if name != "pad_none":
            assert (got["counts"] > 0).any() and (got["counts"] == 0).any(), name + ": accepts and rejects at least once"
        else:
            assert not got["counts"].any()
        for k, v in got.items():
            out[name + "/" + k] = v
    assert (out["crop_x3/counts"] > 1).any(), "the reassigned-label path is exercised"
    try:
        run_case(ref, RAISES)
    except ValueError:
        pass
    else:
        raise AssertionError("the reference's cropper is expected to raise on a label without a valid row")
    np.savez_compressed(os.path.join(HERE, "rand_sampler.npz"), **out)


if __name__ == "__main__":
    main(sys.argv)
