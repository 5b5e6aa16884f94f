"""Writes conv_plan_queries.json: arguments and results of the five pure plan queries of the convolution library
(dspn_conv2d_stats_layout, _dgrad_bn_tiles, _wgrad_splits, _wgrad_workspace_bytes, _split_workspace_bytes) for the layer
shapes of the graphs this project builds, plus edge cases.  SELF-GENERATED: run against the library whose sizing is to be
pinned (no GPU needed, DSPN_* knobs unset); tests/test_cabi.py asserts equality row by row."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def out_size(h, k, stride, pad, dil=1):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def resnet50(size=512):
    """(H, W, Cin, Cout, k, stride, pad, dil) of every convolution of the bottleneck resnet-50 trunk"""
    rows = [(size, size, 4, 64, 7, 2, 3, 1)]
    h = out_size(out_size(size, 7, 2, 3), 3, 2, 1)
    cin = 64
    for stage, (nf, units) in enumerate(zip((256, 512, 1024, 2048), (3, 4, 6, 3))):
        q = nf // 4
        for u in range(units):
            s = 2 if (stage > 0 and u == 0) else 1
            rows.append((h, h, cin, q, 1, 1, 0, 1))
            if u == 0:
                rows.append((h, h, cin, nf, 1, s, 0, 1))
            rows.append((h, h, q, q, 3, s, 1, 1))
            h = out_size(h, 3, s, 1)
            rows.append((h, h, q, nf, 1, 1, 0, 1))
            cin = nf
    return rows


def vgg16_reduced(size=512):
    rows, h, cin = [], size, 4
    for block, (nf, n) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3))):
        for _ in range(n):
            rows.append((h, h, cin, nf, 3, 1, 1, 1))
            cin = nf
        if block < 4:
            h = -(-h // 2) if block == 2 else h // 2
    rows.append((h, h, 512, 1024, 3, 1, 6, 6))
    rows.append((h, h, 1024, 1024, 1, 1, 0, 1))
    return rows


def ssd(maps, extras, anchors, num_classes=8):
    """extra layers (1x1 + strided 3x3) behind the last map, then loc / cls heads on every map, direct and tap-expanded"""
    rows = []
    h, c = maps[-1]
    maps = list(maps)
    for nf, s, p in extras:
        mid = max(128, nf // 2)
        rows.append((h, h, c, mid, 1, 1, 0, 1))
        rows.append((h, h, mid, nf, 3, s, p, 1))
        h, c = out_size(h, 3, s, p), nf
        maps.append((h, c))
    for (h, c), na in zip(maps, anchors):
        for cout in (na * 5, na * (num_classes + 1)):
            rows.append((h, h, c, (cout + 3) // 4 * 4, 3, 1, 1, 1))
            rows.append((h, h, c, cout * 9, 1, 1, 0, 1))
    return rows


def edge_cases():
    rows = [(1, 16, 16, 64, cout, k, 1, k // 2, 1) for cout in (19, 32, 33, 64, 65, 171, 256) for k in (1, 3)]
    for m in (1, 63, 64, 65, 128 * 256 - 1, 128 * 256, 128 * 256 + 1):
        for cout in (32, 64, 256):
            rows.append((1, 1, m, 64, cout, 1, 1, 0, 1))
    rows += [(2, 15, 17, 64, 128, 3, 2, 1, 1), (1, 7, 7, 128, 128, 1, 2, 0, 1), (3, 33, 31, 32, 64, 3, 2, 1, 1)]
    rows += [(n, 1, 1, 256, 128, 3, 1, 1, 1) for n in (1, 8)]
    return rows


def cases():
    r50_ssd = ssd([(64, 512), (32, 1024), (16, 2048)], [(512, 2, 1), (256, 2, 1), (256, 2, 1), (128, 2, 1)], (4, 4, 6, 6, 6, 4, 4))
    vgg_ssd = ssd([(64, 512), (32, 1024)], [(512, 2, 1), (256, 2, 1), (256, 2, 1), (256, 2, 1), (256, 1, 1)], (4, 6, 6, 6, 6, 4, 4))
    out = []
    for n in (1, 8, 32):
        out += [(n,) + r for r in resnet50() + r50_ssd]
    for n in (1, 16):
        out += [(n,) + r for r in vgg16_reduced() + vgg_ssd]
    out += edge_cases()
    return sorted(set(out))


def query(lib, case):
    n, h, w, cin, cout, k, stride, pad, dil = case
    ho, wo = out_size(h, k, stride, pad, dil), out_size(w, k, stride, pad, dil)
    tile_rows = ctypes.c_int(0)
    tiles = lib.dspn_conv2d_stats_layout(n * ho * wo, cout, ctypes.byref(tile_rows))
    return {
        "stats_layout": [tiles, tile_rows.value],
        "dgrad_bn_tiles": lib.dspn_conv2d_dgrad_bn_tiles(n, h, w, cin, stride),
        "wgrad_splits": lib.dspn_conv2d_wgrad_splits(n, ho, wo, cin, cout, k, k, stride),
        "wgrad_workspace_bytes": lib.dspn_conv2d_wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k),
        "split_workspace_bytes": [lib.dspn_conv2d_split_workspace_bytes(n * ho * wo, cout),
                                  lib.dspn_conv2d_split_workspace_bytes(n * h * w, cin)],
    }


def main():
    assert not [k for k in os.environ if k.startswith("DSPN_") and k != "DSPN_LIB"], "unset the DSPN_* knobs"
    from dspnet_amd import _lib
    lib = _lib.lib()
    rows = [{"args": list(c), "results": query(lib, c)} for c in cases()]
    doc = {"args": ["N", "H", "W", "Cin", "Cout", "k", "stride", "pad", "dil"], "rows": rows}
    with open(os.path.join(HERE, "conv_plan_queries.json"), "w") as f:
        f.write("{\"args\": %s,\n \"rows\": [\n" % json.dumps(doc["args"]))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main()
