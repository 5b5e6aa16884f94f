"""GPU parity of MultiBoxDetection with the CPU oracle on every sort, select, grouping and NMS route of the operator.

The cases are mbx_cases.DET_EDGE_CASES; tests/test_mbx_cases_host.py shows (without a GPU) that each still meets the
condition it was built for and that together they reach every route of dspn_multibox_detection_f32.

Bar: no tolerance.  NaNs must sit at the same positions, every other value must have the same BITS (-0 is not +0).  Each case
runs twice, on a caller-owned workspace filled with 0x00 and with 0xFF: whatever the kernels read, they must have written
(the suppression-mask words the scan is said never to read, the keys behind the valid rows, stale class ids)."""
import numpy as np
import pytest
import torch

import mbx_cases as mc
from dspnet_amd import operator as op
from oracle import multibox as om

pytestmark = pytest.mark.gpu


def assert_same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32
    gn, en = np.isnan(got), np.isnan(exp)
    assert (gn == en).all(), f"{what}: NaN positions differ at {np.argwhere(gn != en)[:8].tolist()}"
    diff = (got.view(np.uint32) != exp.view(np.uint32)) & ~en
    if diff.any():
        where = np.argwhere(diff)
        first = tuple(where[0])
        raise AssertionError(f"{what}: {len(where)} values differ ({len(np.unique(where[:, :2], axis=0))} rows); first at "
                             f"{first}: got {got[first]!r} expected {exp[first]!r}; rows {where[:6].tolist()}")


def run_detection_edges(anc, prob, loc, expected=None, **kw):
    """the operator on a workspace of zeros and on one of 0xFF bytes, both against the oracle"""
    if expected is None:
        expected = om.multibox_detection(prob, loc, anc, **kw)
    B, A = prob.shape[0], anc.shape[1]
    a, p, l = (torch.tensor(x, device="cuda") for x in (anc, prob, loc))
    nbytes = op.detection_workspace_bytes(B, A)
    for fill in (0x00, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        got = op.MultiBoxDetection(p, l, a, workspace=ws, **kw).cpu().numpy()
        assert_same_bits(got, expected, f"workspace filled with {fill:#04x}")
    return expected


@pytest.mark.parametrize("cid", list(mc.DET_EDGE_CASES))
def test_detection_edge_case(gpu_device, cid):
    name, kw = mc.DET_EDGE_CASES[cid]
    anc, prob, loc = mc.det_inputs(name)
    run_detection_edges(anc, prob, loc, expected=mc.det_expected(cid), **kw)


def test_helper_sees_a_sign_of_zero_and_a_moved_nan():
    """(no GPU needed, but it guards the bar of this file) the comparison is on bits"""
    a = np.array([[0.0, np.nan, 1.0]], np.float32)
    assert_same_bits(a, a.copy(), "same")
    with pytest.raises(AssertionError, match="values differ"):
        assert_same_bits(np.array([[-0.0, np.nan, 1.0]], np.float32), a, "zero")
    with pytest.raises(AssertionError, match="NaN positions"):
        assert_same_bits(np.array([[0.0, 1.0, np.nan]], np.float32), a, "nan")
