"""Writes dgrad_host_verdicts.json: what the host path of the data gradient decides before any launch -- (a) the verdicts of
the two route queries (dspn_conv2d_dgrad_bn_sadd_route_f32, dspn_conv2d_dgrad_bn_recompute_route_f32) under every launch
setting, with the dspn_last_error() text where the verdict is 0; (b) return value and text of calls the variant entries
(_sadd, _sums, _apply, their bfloat16 twins, and dspn_conv2d_dgrad_bn_f32) refuse.  SELF-GENERATED: run against the library
whose decisions are to be pinned (no GPU needed, DSPN_* knobs unset; DSPN_LIB names another build); tests/test_cabi.py
replays it row by row.  The pointers of (b) only stand for "given": every row is refused before anything is launched, which
main() asserts, and the test replays (b) only where no GPU is visible."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

WIDE_TILES, TILE_SPANNING = (0, 1, 3, 4), (0, 1)        # dspn_conv_set_wide_tiles / dspn_conv_set_tile_spanning; defaults 0 / 1
F16X2, UNSCALED_OK, DY_PLANES = 3, 0x100, 0x200         # include/dspn_nn.h DSPN_MATH_*

# (N, H, W, Cin, ldy)
ROUTE_SHAPES = [
    (128, 16, 16, 128, 64), (64, 16, 16, 256, 96), (128, 16, 20, 128, 64),
    (128, 16, 18, 128, 64),                             # W % 4 != 0
    (129, 15, 17, 128, 64),                             # M % 128 != 0
    (2, 8, 8, 128, 1024),                               # split-K
    (128, 16, 16, 128, 32),                             # one k-step
    (128, 16, 16, 130, 64), (0, 16, 16, 128, 64), (128, 16, 16, 128, 0), (128, 16, 16, 128, 48),      # degenerate
    (32, 128, 128, 256, 64), (32, 64, 64, 512, 128), (32, 32, 32, 1024, 256), (32, 16, 16, 2048, 512),    # headline bench, conv1 calls
]
SPLIT_K = dict(N=2, H=8, W=8, Cin=128, ldy=1024)
M_ODD = dict(N=129, H=15, W=17, Cin=128, ldy=64)
TWO_GIB = dict(N=8192, H=16, W=16, Cin=128, ldy=256)


def route_cases():
    return [(wide, xt, planes) + s for wide in WIDE_TILES for xt in TILE_SPANNING for planes in (0, 1) for s in ROUTE_SHAPES]


def route_query(lib, case):
    """[addend verdict, text or None, recompute verdict, text or None] (the text is stale after a 1)"""
    wide, xt, planes, *shape = case
    out = []
    try:
        assert lib.dspn_conv_set_wide_tiles(wide) == 0 and lib.dspn_conv_set_tile_spanning(xt) == 0
        for fn in (lib.dspn_conv2d_dgrad_bn_sadd_route_f32, lib.dspn_conv2d_dgrad_bn_recompute_route_f32):
            v = fn(*shape, planes)
            out += [v, None if v else lib.dspn_last_error().decode()]
    finally:
        lib.dspn_conv_set_wide_tiles(0)
        lib.dspn_conv_set_tile_spanning(1)
    return out


# the arguments of a call that every variant entry takes at the default settings: (128, 16, 16, 128) <- (128, 16, 16, 64), dy as
# piece planes.  Pointers: 1 = given, 0 = NULL.
BASE = dict(dy=1, wt=0, wt_planes=1, dx=1, N=128, H=16, W=16, Cin=128, ldy=64, R=1, S=1, stride=1, pad=0, dil=1, Ho=None, Wo=None,
            dx_ldc=None, accumulate=0, bn_x=1, bn_scale=1, bn_shift=1, bn_mean=1, bn_rstd=1, bn_relu=1, bn_sums=1, bn_sums_short=0,
            bn_dy_absmax=0, math=F16X2 | DY_PLANES, dy_absmax=1, w_absmax=1, workspace=0, workspace_bytes=0,
            addend=1, addend_h=None, addend_w=None, dx_absmax=1, bn_workspace=1, bn_workspace_short=0)


def refused_cases():
    """(entry, overrides of BASE) of every refused call"""
    rows = []
    for e in ("sadd", "sums", "apply"):
        rows += [(e + "_f32", kw) for kw in (
            dict(math=0, dy_absmax=0, w_absmax=0), dict(math=1, dy_absmax=0, w_absmax=0), dict(math=2),     # fp32, bf16, three-piece math
            dict(math=F16X2),                           # a float dy
            dict(dx_ldc=160),                           # a strided dx
            dict(stride=2, Ho=8, Wo=8),                 # stride 2
            SPLIT_K, M_ODD, TWO_GIB,
            # two reasons compete
            dict(math=0, dy_absmax=0, w_absmax=0, dx_ldc=160), dict(SPLIT_K, math=F16X2), dict(M_ODD, math=F16X2),
            dict(R=3, S=3, pad=1, dx_ldc=160), dict(TWO_GIB, Cin=130), dict(math=F16X2, dy_absmax=0, w_absmax=0, dx_ldc=160),
            dict(math=F16X2 | DY_PLANES, ldy=48), dict(SPLIT_K, math=2), dict(N=0, dx_ldc=160),
        )]
        rows += [(e + "_bf16", kw) for kw in (dict(math=1, dy_absmax=0, w_absmax=0, wt=1, wt_planes=0), dict(), dict(dx_ldc=160),
                                              dict(SPLIT_K, math=1, wt=1, wt_planes=0))]
    # a 3 x 3, pad 1 (the strided addend itself goes with any stride-1 geometry: those calls are taken, so they have no row)
    rows += [(e + "_f32", kw) for e in ("sums", "apply") for kw in (dict(R=3, S=3, pad=1), dict(R=3, S=3, pad=1, wt=1),
                                                                   dict(pad=1, Ho=18, Wo=18), dict(pad=1))]
    rows += [("sadd_f32", kw) for kw in (
        dict(accumulate=1), dict(addend_h=7), dict(addend_w=9), dict(addend=0), dict(addend_h=0), dict(bn_sums=0),
        dict(N=128, H=16, W=18), dict(N=128, H=16, W=4),      # W % 4 != 0, W < 8
        dict(accumulate=1, addend=0), dict(accumulate=1, dx_ldc=160), dict(bn_sums=0, math=F16X2), dict(SPLIT_K, bn_sums=0),
        dict(SPLIT_K, bn_sums=0, workspace=1, workspace_bytes=1 << 30),      # (without sums and with a workspace the call would be split)
        dict(addend_h=7, W=18))]
    rows += [("sums_f32", kw) for kw in (
        dict(dx=1), dict(accumulate=1), dict(bn_dy_absmax=1), dict(bn_sums=0), dict(bn_sums=0, accumulate=1), dict(Cin=130),
        dict(bn_sums_short=1), dict(bn_x=0))]
    rows += [("apply_f32", kw) for kw in (
        dict(bn_workspace=0), dict(bn_workspace_short=1), dict(dx=0), dict(bn_x=0), dict(bn_scale=0), dict(bn_workspace_short=1, math=0),
        dict(Cin=130, bn_workspace_short=1), dict(accumulate=1, math=F16X2))]
    # the shared refusals of dspn_conv2d_dgrad_bn_f32
    rows += [("bn_f32", kw) for kw in (
        dict(N=0), dict(ldy=0), dict(H=0), dict(Cin=0), dict(R=0), dict(ldy=6), dict(stride=3), dict(stride=2, dil=2, Ho=8, Wo=8),      # bad geometry
        dict(math=0 | DY_PLANES), dict(math=2 | DY_PLANES), dict(math=F16X2 | DY_PLANES, dy_absmax=0), dict(math=4), dict(math=-1),
        dict(math=F16X2, dy_absmax=0), dict(math=F16X2, w_absmax=0),      # missing magnitude blocks
        dict(bn_x=0), dict(bn_mean=0), dict(bn_rstd=0), dict(bn_scale=0), dict(bn_shift=0),      # missing BatchNorm operands
        dict(bn_sums_short=1), dict(dx_ldc=160), dict(Cin=130, math=F16X2), dict(TWO_GIB),
        dict(dy=0), dict(dx=0), dict(wt=0, wt_planes=0), dict(wt=1, wt_planes=0),      # null pointers; split math without weight planes
        dict(N=0, math=4), dict(math=4 | DY_PLANES), dict(bn_x=0, dx_ldc=160), dict(dy=0, bn_sums_short=1),
        dict(math=F16X2 | UNSCALED_OK, dy_absmax=0, w_absmax=0, wt=1, wt_planes=0),
        dict(math=F16X2 | UNSCALED_OK | DY_PLANES, dy_absmax=0, w_absmax=0))]
    return [(e, dict(kw)) for e, kw in rows]


def refused_call(lib, entry, overrides):
    """-> [return value, dspn_last_error() text] of one raw call of dspn_conv2d_dgrad_<entry>"""
    name, tensors = entry.rsplit("_", 1)
    a = dict(BASE, dx=0 if name == "sums" else 1)      # (the sums pass stores no dx)
    a.update(overrides)
    p = lambda given: ctypes.c_void_p(256) if given else None  # noqa: E731   (never dereferenced on the host)
    Ho = a["H"] if a["Ho"] is None else a["Ho"]
    Wo = a["W"] if a["Wo"] is None else a["Wo"]
    args = [p(a["dy"]), p(a["wt"]), p(a["wt_planes"]), p(a["dx"]), a["N"], a["H"], a["W"], a["Cin"], a["ldy"], a["R"],
            a["S"], a["stride"], a["pad"], a["pad"], a["dil"], Ho, Wo, a["Cin"] if a["dx_ldc"] is None else a["dx_ldc"], a["accumulate"],
            p(a["bn_x"]), p(a["bn_scale"]), p(a["bn_shift"])]
    math = [a["math"], p(a["dy_absmax"]), p(a["w_absmax"])]
    if name == "apply":
        args += [a["bn_relu"], p(a["dx_absmax"])] + math + [p(a["bn_workspace"]), 4 * (3 * a["Cin"] - a["bn_workspace_short"]), None]
    else:
        tiles = lib.dspn_conv2d_dgrad_bn_tiles(a["N"], a["H"], a["W"], a["Cin"], a["stride"])
        args += [p(a["bn_mean"]), p(a["bn_rstd"]), a["bn_relu"], p(a["bn_sums"]),
                 4 * max(0, 2 * tiles * a["Cin"] - a["bn_sums_short"]) if a["bn_sums"] else 0, p(a["bn_dy_absmax"])]
        args += math + [p(a["workspace"]), a["workspace_bytes"]]
        if name == "sadd":
            args += [p(a["addend"]), (a["H"] + 1) // 2 if a["addend_h"] is None else a["addend_h"],
                     (a["W"] + 1) // 2 if a["addend_w"] is None else a["addend_w"]]
        args.append(None)
    fn = getattr(lib, "dspn_conv2d_dgrad_bn_%s" % tensors if name == "bn" else "dspn_conv2d_dgrad_bn_%s_%s" % (name, tensors))
    rc = fn(*args)
    return [rc, lib.dspn_last_error().decode()]


def main():
    assert not [k for k in os.environ if k.startswith("DSPN_") and k != "DSPN_LIB"], "unset the DSPN_* knobs"
    import torch
    assert not torch.cuda.is_available(), "the refused calls carry stand-in pointers: write the fixture where no GPU is visible"
    from dspnet_amd import _lib
    lib = _lib.lib()
    routes = [{"args": list(c), "results": route_query(lib, c)} for c in route_cases()]
    refused = []
    for entry, kw in refused_cases():
        rc, text = refused_call(lib, entry, kw)
        assert rc in (-1, -2), ("not refused by the host path (DSPN_ERR_ARG / DSPN_ERR_WORKSPACE)", entry, kw, rc, text)
        refused.append({"entry": entry, "args": kw, "results": [rc, text]})
    with open(os.path.join(HERE, "dgrad_host_verdicts.json"), "w") as f:
        f.write("{\"route_args\": %s,\n \"routes\": [\n" % json.dumps(["wide_tiles", "tile_spanning", "dy_planes", "N", "H", "W", "Cin", "ldy"]))
        f.write(",\n".join("  " + json.dumps(r) for r in routes))
        f.write("\n ],\n \"refused\": [\n")
        f.write(",\n".join("  " + json.dumps(r) for r in refused))
        f.write("\n]}\n")
    print(len(routes), "route rows,", len(refused), "refused rows")


if __name__ == "__main__":
    main()
