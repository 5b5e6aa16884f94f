"""Writes wgrad_host_verdicts.json: return value and full dspn_last_error() text of calls that the host path of the weight
gradient refuses before any launch -- dspn_conv2d_wgrad_bn_f32 / _bf16, dspn_conv2d_wgrad_slabs_f32 / _bf16 and
dspn_conv2d_wgrad_f32 -- competing reasons in their order.  SELF-GENERATED: run against the library whose decisions are to be
pinned (no GPU needed, DSPN_* knobs unset; DSPN_LIB names another build); tests/test_cabi.py replays it row by row.  The
pointers only stand for "given": every row is refused before anything is launched, which main() asserts, and the test replays
the rows only where no GPU is visible.  (Split counts and workspace sizes: conv_plan_queries.json.)

new_refusals(): calls with Cout, R, S, stride or dil of 0.  They are NOT generated from a library: the library the fixture was
first written from divided by Cout * R * S * Cin on them.  The test asserts them directly (-1, "bad geometry")."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

F16X2, UNSCALED_OK, DY_PLANES, X_PLANES = 3, 0x100, 0x200, 0x400      # include/dspn_nn.h DSPN_MATH_*

# the arguments of a call that every entry takes: (1, 8, 8, 64) x (1, 8, 8, 64), 3 x 3, stride 1, pad 1, fp32 math, a workspace
# of dspn_conv2d_wgrad_workspace_bytes.  Pointers: 1 = given, 0 = NULL.  Ho / Wo None: H / W; out (dw of _bn and _f32, slabs of
# _slabs) and out_bytes (workspace_bytes / slabs_bytes; None: what the query says)
BASE = dict(x=1, in_scale=0, in_shift=0, in_relu=0, dy=1, out=1, N=1, H=8, W=8, Cin=64, Cout=64, ldy=64, R=3, S=3, stride=1, pad=1,
            dil=1, Ho=None, Wo=None, accumulate=0, math=0, x_absmax=0, dy_absmax=0, workspace=1, out_bytes=None)
ONE_SLAB = 4 * 64 * 3 * 3 * 64                          # of BASE
BLOCKS = dict(x_absmax=1, dy_absmax=1)
BATCH_2GIB = dict(N=8192, H=64, W=64)                   # x of 8 GiB (4 GiB as bfloat16) in images of 1 MiB
IMAGE_2GIB = {"f32": dict(H=8192, W=8192, Cin=8, Ho=8, Wo=8), "bf16": dict(H=8192, W=8192, Cin=16, Ho=8, Wo=8)}      # one image of x
DY_IMAGE_2GIB = {"f32": dict(Ho=8192, Wo=8192, Cout=8, ldy=8), "bf16": dict(Ho=8192, Wo=8192, Cout=16, ldy=16)}      # ... of dy
ENTRIES = ("bn_f32", "bn_bf16", "slabs_f32", "slabs_bf16")


def refused_cases():
    """(entry, overrides of BASE) of every refused call"""
    rows = []
    for e in ENTRIES:
        rows += [(e, {k: 0}) for k in ("N", "H", "W", "Cin", "Ho", "Wo", "ldy")]      # geometry zeros
        rows += [(e, kw) for kw in (
            dict(in_scale=1), dict(in_shift=1),                                       # the affine pair
            dict(math=4), dict(math=-1),
            dict(x=0), dict(dy=0), dict(x=0, dy=0),                                   # null pointers
            dict(Cin=66), dict(ldy=66), dict(Cin=68, out_bytes=16), dict(ldy=68, out_bytes=16),      # kEPC: 4 floats, 8 bfloat16 (the float build takes 68)
            dict(out_bytes=ONE_SLAB - 1), dict(out_bytes=0),                          # less than one slab
            # ... of a call whose plan wants 16.  (With ONE_SLAB and more that call is TAKEN: the plan makes do with the slabs there
            # are, so "fewer slabs than the plan wants" has no row and no text.)
            dict(N=32, out_bytes=ONE_SLAB - 4),
            IMAGE_2GIB[e.rsplit("_", 1)[1]], DY_IMAGE_2GIB[e.rsplit("_", 1)[1]],
            # two reasons compete
            dict(N=0, math=4), dict(Ho=0, in_scale=1), dict(in_scale=1, math=4), dict(math=4, x=0), dict(x=0, Cin=66),
            dict(Cin=66, out_bytes=16), dict(x=0, out_bytes=16), dict(BATCH_2GIB, x=0), dict(BATCH_2GIB, Cin=66),
            dict(BATCH_2GIB, out_bytes=16), dict(BATCH_2GIB, math=4), dict(IMAGE_2GIB[e.rsplit("_", 1)[1]], out_bytes=16),
            # the two-piece math: the float build wants both magnitude blocks or DSPN_MATH_UNSCALED_OK (the short workspace shows how
            # far a call gets that is otherwise taken)
            # (the bfloat16 build takes the mode as its own bf16 math)
            dict(math=F16X2, out_bytes=16), dict(math=F16X2, x_absmax=1, out_bytes=16), dict(math=F16X2, dy_absmax=1, out_bytes=16),
            dict(math=F16X2 | UNSCALED_OK, out_bytes=16), dict(math=F16X2 | UNSCALED_OK, x_absmax=1, out_bytes=16),
            dict(BLOCKS, math=F16X2, out_bytes=16), dict(math=F16X2, x=0), dict(math=4 | UNSCALED_OK),
        )]
        # the plane flags: the float build's two-piece math only, whole 32-channel blocks, the block the planes were cut by
        for flag in (DY_PLANES, X_PLANES):
            rows += [(e, dict(BLOCKS, math=m | flag)) for m in (0, 1, 2, 4)]
            rows += [(e, dict(BLOCKS, math=m | flag, out_bytes=16)) for m in (1, F16X2)]      # (what the bfloat16 entries say to the flag)
        rows += [(e, kw) for kw in (
            dict(BLOCKS, math=F16X2 | DY_PLANES, ldy=128, out_bytes=16), dict(BLOCKS, math=F16X2 | DY_PLANES, Cout=48, ldy=48, out_bytes=16),
            dict(math=F16X2 | DY_PLANES, x_absmax=1), dict(math=F16X2 | DY_PLANES | UNSCALED_OK, x_absmax=1),
            dict(BLOCKS, math=F16X2 | X_PLANES, Cin=48, out_bytes=16), dict(math=F16X2 | X_PLANES, dy_absmax=1),
            dict(math=F16X2 | X_PLANES | UNSCALED_OK, dy_absmax=1), dict(BLOCKS, math=F16X2 | X_PLANES, in_scale=1, in_shift=1),
            dict(BLOCKS, math=F16X2 | X_PLANES, in_scale=1),      # (the affine pair comes first)
            dict(BLOCKS, math=F16X2 | DY_PLANES | X_PLANES, Cout=48, ldy=48, Cin=48),      # both flags wrong: dy's text
            dict(BLOCKS, math=F16X2 | DY_PLANES | X_PLANES, out_bytes=16), dict(BLOCKS, math=F16X2 | DY_PLANES | X_PLANES, N=0),
        )]
    # a batch of 2 GiB or more: the _bn entries run it in chunks, the _slabs entries refuse it
    rows += [("slabs_f32", dict(BATCH_2GIB)), ("slabs_bf16", dict(BATCH_2GIB)), ("slabs_f32", dict(BATCH_2GIB, math=F16X2))]
    rows += [("slabs_f32", dict(out=0)), ("slabs_bf16", dict(out=0)), ("slabs_f32", dict(out=0, out_bytes=0)),
             ("bn_f32", dict(workspace=0)), ("bn_bf16", dict(workspace=0)), ("bn_f32", dict(workspace=0, out=0)),
             ("bn_f32", dict(workspace=0, out_bytes=0))]
    # dspn_conv2d_wgrad_f32 goes through the _bn entry: fp32 math, no affine, no blocks
    rows += [("f32", kw) for kw in (
        dict(N=0), dict(ldy=0), dict(x=0), dict(dy=0), dict(workspace=0), dict(Cin=66), dict(ldy=66), dict(out_bytes=ONE_SLAB - 1),
        IMAGE_2GIB["f32"], dict(N=0, x=0), dict(Cin=66, out_bytes=16))]
    return [(e, dict(kw)) for e, kw in rows]


def new_refusals():
    """(entry, overrides of BASE): geometry that the fixture's first library did not check"""
    zeros = (dict(Cout=0), dict(R=0), dict(S=0), dict(R=0, S=0), dict(stride=0), dict(dil=0), dict(Cout=0, math=4), dict(R=0, x=0))
    return [(e, dict(kw)) for e in ENTRIES + ("f32",) for kw in zeros if not (e == "f32" and "math" in kw)]


def refused_call(lib, entry, overrides):
    """-> [return value, dspn_last_error() text] of one raw call of dspn_conv2d_wgrad_<entry>"""
    a = dict(BASE)
    a.update(overrides)
    p = lambda given: ctypes.c_void_p(256) if given else None  # noqa: E731   (never dereferenced on the host)
    Ho = a["H"] if a["Ho"] is None else a["Ho"]
    Wo = a["W"] if a["Wo"] is None else a["Wo"]
    nbytes = a["out_bytes"]
    if nbytes is None:
        nbytes = lib.dspn_conv2d_wgrad_workspace_bytes(a["N"], Ho, Wo, a["Cin"], a["Cout"], a["R"], a["S"])
    geom = [a["N"], a["H"], a["W"], a["Cin"], a["Cout"], a["ldy"], a["R"], a["S"], a["stride"], a["pad"], a["pad"], a["dil"], Ho, Wo]
    affine = [p(a["in_scale"]), p(a["in_shift"]), a["in_relu"]]
    math = [a["math"], p(a["x_absmax"]), p(a["dy_absmax"])]
    if entry == "f32":
        assert not set(overrides) & {"in_scale", "in_shift", "in_relu", "math", "x_absmax", "dy_absmax"}, overrides
        rc = lib.dspn_conv2d_wgrad_f32(p(a["x"]), p(a["dy"]), p(a["out"]), *geom, a["accumulate"], p(a["workspace"]), nbytes, None)
    elif entry.startswith("slabs_"):
        rc = getattr(lib, "dspn_conv2d_wgrad_" + entry)(p(a["x"]), *affine, p(a["dy"]), p(a["out"]), nbytes, *geom, *math, None)
    else:
        rc = getattr(lib, "dspn_conv2d_wgrad_" + entry)(p(a["x"]), *affine, p(a["dy"]), p(a["out"]), *geom, a["accumulate"], *math,
                                                        p(a["workspace"]), nbytes, None)
    return [rc, lib.dspn_last_error().decode()]


def main():
    assert not [k for k in os.environ if k.startswith("DSPN_") and k != "DSPN_LIB"], "unset the DSPN_* knobs"
    import torch
    assert not torch.cuda.is_available(), "the refused calls carry stand-in pointers: write the fixture where no GPU is visible"
    from dspnet_amd import _lib
    lib = _lib.lib()
    refused = []
    for entry, kw in refused_cases():
        rc, text = refused_call(lib, entry, kw)
        assert rc in (-1, -2), ("not refused by the host path (DSPN_ERR_ARG / DSPN_ERR_WORKSPACE)", entry, kw, rc, text)
        refused.append({"entry": entry, "args": kw, "results": [rc, text]})
    with open(os.path.join(HERE, "wgrad_host_verdicts.json"), "w") as f:
        f.write("{\"refused\": [\n")
        f.write(",\n".join("  " + json.dumps(r) for r in refused))
        f.write("\n ],\n \"new_refusals\": [\n")
        f.write(",\n".join("  " + json.dumps({"entry": e, "args": kw}) for e, kw in new_refusals()))
        f.write("\n]}\n")
    print(len(refused), "refused rows,", len(new_refusals()), "new refusals")


if __name__ == "__main__":
    main()
