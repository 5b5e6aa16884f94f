"""GPU parity of MultiBoxDetection and MultiBoxTarget with the CPU oracle on every route of the two operators.

The cases are mbx_cases.DET_EDGE_CASES; tests/test_mbx_cases_host.py shows (without a GPU) that each still meets the
condition it was built for and that together they reach every route of dspn_multibox_detection_f32.  The same holds for
mbx_cases.TGT_EDGE_CASES and dspn_multibox_target_f32 (test_target_edge_case).

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


def target_codes(ws, batch):
    """the per-sample deferred codes a MultiBoxTarget call left at the head of its workspace"""
    torch.cuda.synchronize()
    return ws[:4 * batch].cpu().numpy().view(np.int32).tolist()


@pytest.mark.parametrize("cid", list(mc.TGT_EDGE_CASES))
def test_target_edge_case(gpu_device, cid):
    """MultiBoxTarget on every case of mbx_cases.TGT_EDGE_CASES, on a caller-owned workspace of 0x00 and of 0xFF bytes.
    cls_target, loc_mask and columns 0, 1, 4 of loc_target: equal NaN positions, equal bits elsewhere.  Columns 2 and 3: the
    one float the double-precision logarithm rounds to (mbx_cases.log_bracket; the bracket of every entry of the case is
    asserted to hold a single float first), which must also lie within one float of glibc's logf.  The deferred error codes
    against the oracle's return code."""
    anc, lab, pred, kw = mc.tgt_inputs(cid)
    (lt_e, lm_e, ct_e), rc, matched, _ = mc.tgt_expected(cid)
    variances = kw.get("variances", (0.1, 0.1, 0.2, 0.2))
    assert mc.ambiguous_log_brackets(anc, lab, matched, variances) == 0
    B, L, A = lab.shape[0], lab.shape[1], anc.shape[1]
    routes = mc.tgt_case_routes(cid)
    codes_e = [2 if r.bad_terminator else 3 if r.exit == "short" else 0 for r in routes]
    assert rc == -max(codes_e)
    a, l, p = (torch.tensor(x, device="cuda") for x in (anc, lab, pred))
    nbytes = op.target_workspace_bytes(B, A, L)
    exact = [0, 1, 4]
    for fill in (0x00, 0xFF):
        what = f"workspace filled with {fill:#04x}"
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        lt, lm, ct = (t.cpu().numpy() for t in op.MultiBoxTarget(a, l, p, workspace=ws, **kw))
        assert_same_bits(ct, ct_e, what + ": cls_target")
        assert_same_bits(lm, lm_e, what + ": loc_mask")
        assert_same_bits(lt.reshape(B, A, 5)[..., exact], lt_e.reshape(B, A, 5)[..., exact], what + ": loc_target dx dy dist")
        mc.assert_log_columns(lt, anc, lab, matched, variances)
        assert target_codes(ws, B) == codes_e, what


def test_helper_sees_a_sign_of_zero_and_a_moved_nan():
    """(no GPU needed, but it guards the bar of this file) the comparison is on bits"""
    a = np.array([[0.0, np.nan, 1.0]], np.float32)
    assert_same_bits(a, a.copy(), "same")
    with pytest.raises(AssertionError, match="values differ"):
        assert_same_bits(np.array([[-0.0, np.nan, 1.0]], np.float32), a, "zero")
    with pytest.raises(AssertionError, match="NaN positions"):
        assert_same_bits(np.array([[0.0, 1.0, np.nan]], np.float32), a, "nan")
