"""Training with fixed BatchNorm statistics, the parts that need no GPU: the C ABI (header, exports, refusals before any HIP
call), the flag word functional.bn_backward_from_sums forms in every phase, Graph.set_global_stats and the training builders
on CPU-device graphs."""
import ctypes
import os
import re

import pytest
import torch

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from test_cabi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
NEW_SYMBOLS = ("dspn_bn_backward_ex_f32", "dspn_bn_backward_ex_bf16", "dspn_bn_backward_maxpool_ex_f32")
# the BatchNorms the reference's module flag `use_global_stats` reaches (its symbol/multitask_symbol_builder.py:275-315)
DECODER_BATCHNORMS = ["res3_reduced_bn", "res3_reduced2_bn", "res4_reduced_bn", "res4_reduced2_bn", "res5_reduced_bn",
                      "score2_pool4_bn", "score2_pool2_bn", "score2_pool1_bn", "score3_conv_bn"]


def test_header_declares_and_library_exports_the_mode():
    text = open(os.path.join(ROOT, "include", "dspn_nn.h")).read()
    m = re.search(r"^#define DSPN_BN_SUMS_FIXED_STATS (\d+)$", text, flags=re.M)
    assert m and int(m.group(1)) == 16 == fn.BN_SUMS_FIXED_STATS
    assert fn.BN_SUMS_FIXED_STATS & (fn.BN_SUMS_PLANES | fn.BN_SUMS_FINALIZE_ONLY | fn.BN_SUMS_APPLY_ONLY | fn.BN_SUMS_PARKED) == 0
    decl, lib = declared_symbols(), _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in decl and hasattr(lib, name) and name in _lib.SIGNATURES, name
        plain = _lib.SIGNATURES[name.replace("_ex_", "_")]
        assert _lib.SIGNATURES[name] == (plain[0], plain[1] + [ctypes.c_int]), "the plain arguments plus a trailing int"


def test_refusals_before_any_hip_call():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)        # never dereferenced: every call below fails its checks first

    def bwd(f, fixed, C=8):
        return f(p, p, p, p, p, p, None, p, None, p, 512, C, 1, 0, None, p, 1 << 20, None, fixed)

    def pool(fixed, C=8):
        return lib.dspn_bn_backward_maxpool_ex_f32(p, p, p, p, p, 1, 8, 8, C, 3, 2, 1, 4, 4, p, p, None, p, None, p, 1, None, p,
                                                   1 << 20, None, fixed)

    def sums(f, flags, C=8):
        return f(p, p, p, p, p, p, None, p, 4, p, None, p, 512, C, 1, 0, None, None, None, None, flags, p, 1 << 20, None)
    for f in (lib.dspn_bn_backward_ex_f32, lib.dspn_bn_backward_ex_bf16):
        for bad in (2, -1, 16):
            assert bwd(f, bad) == -1 and b"fixed_stats must be 0 or 1" in lib.dspn_last_error()
        for ok in (0, 1):
            assert bwd(f, ok, C=6) == -1 and b"positive multiple of 4" in lib.dspn_last_error()
    for bad in (2, -1):
        assert pool(bad) == -1 and b"fixed_stats must be 0 or 1" in lib.dspn_last_error()
    assert pool(1, C=6) == -1 and b"bad geometry" in lib.dspn_last_error()
    for f in (lib.dspn_bn_backward_from_sums_f32, lib.dspn_bn_backward_from_sums_bf16):
        for word in (16 | 2 | 4, 16 | 8, 16 | 8 | 4, 32, 16 | 32):
            assert sums(f, word) == -1 and b"flag word" in lib.dspn_last_error(), word
        for word in (16, 16 | 2, 16 | 4, 16 | 2 | 8):      # accepted words get as far as the next check
            assert sums(f, word, C=6) == -1 and b"positive multiple of 4" in lib.dspn_last_error(), word
    # dx == NULL is the finalize alone, with or without the mode
    f = lib.dspn_bn_backward_from_sums_f32
    for word, text in ((16, b"finalize-only"), (16 | 2 | 8, b"finalize-only"), (16 | 2, b"positive multiple of 4")):
        rc = f(p, p, p, p, p, p, None, p, 4, None, None, p, 512, 6, 1, 0, None, None, None, None, word, p, 1 << 20, None)
        assert rc == -1 and text in lib.dspn_last_error(), word


def test_from_sums_sets_the_flag_bit_in_every_phase(monkeypatch):
    words = []

    def entry(*args):
        words.append(args[20])
        return 0
    monkeypatch.setattr(fn, "_f", lambda name, t: entry if name == "dspn_bn_backward_from_sums" else None)
    monkeypatch.setattr(fn, "stream", lambda: 0)          # (nothing is launched)
    C, tiles = 8, 2
    x, dy = torch.zeros(1, 1, 4, C), torch.zeros(1, 1, 4, C)
    v = torch.zeros(C)
    tab, ws = torch.zeros(tiles, 2, C), torch.zeros(12 * C + 64, dtype=torch.uint8)
    for fixed in (False, True):
        bit = fn.BN_SUMS_FIXED_STATS if fixed else 0
        kw = dict(dx=torch.zeros_like(x), dgamma=v, dbeta=v, workspace=ws, fixed_stats=fixed)
        args = (x, v, v, dy, v, v, v, tab, tiles)
        del words[:]
        fn.bn_backward_from_sums(*args, **kw)
        fn.bn_backward_from_sums(*args, phase=1, **kw)
        fn.bn_backward_from_sums(*args, phase=1, park=True, **kw)
        fn.bn_backward_from_sums(*args, phase=2, **kw)
        fn.bn_backward_from_sums(*args, **dict(kw, dx=fn.NO_OUTPUT))
        assert words == [bit, bit | 2, bit | 2 | 8, bit | 4, bit | 2], (fixed, words)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stub_prior(monkeypatch):
    """MultiBoxPrior, the one operator a graph BUILD calls, stubbed (as tests/test_graph_wiring.py does): no kernel runs"""
    from dspnet_amd import operator as op

    def fake_prior(data, sizes, ratios, **kw):
        H, W = data if isinstance(data, tuple) else data.shape[-2:]
        return torch.zeros(1, H * W * (len(sizes) + len(ratios) - 1), 4)
    monkeypatch.setattr(op, "MultiBoxPrior", fake_prior)


def _build(builder, **kw):
    from dspnet_amd.symbol import multitask_symbol_factory as F
    return getattr(F, builder)("resnet-50", 128, num_classes=8, batch_size=1, device=CPU, **kw)


def _fixed(net):
    return [n for n, node in net.g.bn_nodes.items() if node.use_global_stats]


@pytest.mark.parametrize("builder", ["get_multi_symbol_train", "get_det_symbol_train", "get_seg_symbol_train"])
def test_training_builders_take_a_pattern(stub_prior, builder):
    from dspnet_amd.symbol.multitask_symbol_builder import DECODER_GLOBAL_STATS_PATTERN, EVERY_BATCHNORM_PATTERN
    plain = _build(builder)
    assert _fixed(plain) == [] and len(plain.g.bn_nodes) >= 50
    every = _build(builder, global_stats_pattern=EVERY_BATCHNORM_PATTERN)
    assert _fixed(every) == list(every.g.bn_nodes) == list(plain.g.bn_nodes)
    # (the keyword of the test builders stays refused on a training builder -- tests/test_bn_moving_cabi.py -- and says where to go)
    with pytest.raises(ValueError, match="global_stats_pattern"):
        _build(builder, use_global_stats=True)
    some = _build(builder, global_stats_pattern=r"stage1_unit[12]_bn")
    assert _fixed(some) == [n for n in plain.g.bn_nodes if n.startswith(("stage1_unit1_bn", "stage1_unit2_bn"))] and len(_fixed(some)) == 6
    with pytest.raises(ValueError, match="matches no BatchNorm"):
        _build(builder, global_stats_pattern=r"no_such_layer")
    with pytest.raises(ValueError, match="matches no BatchNorm"):
        _build(builder, global_stats_pattern=r"unit1_bn1")           # re.match: anchored at the start of the name
    # the reference's own configuration: the decoder's BatchNorms, exactly -- on the graphs that have a decoder
    if builder == "get_det_symbol_train":
        with pytest.raises(ValueError, match="matches no BatchNorm"):
            _build(builder, global_stats_pattern=DECODER_GLOBAL_STATS_PATTERN)
    else:
        dec = _build(builder, global_stats_pattern=DECODER_GLOBAL_STATS_PATTERN)
        assert sorted(_fixed(dec)) == sorted(DECODER_BATCHNORMS)
        both = _build(builder, global_stats_pattern=DECODER_GLOBAL_STATS_PATTERN, freeze_pattern=r"^(bn_data|conv0|bn0|stage1_)")
        assert sorted(_fixed(both)) == sorted(DECODER_BATCHNORMS) and len(both.fixed_param_names) > 0


def test_test_builders_are_unchanged(stub_prior):
    from dspnet_amd.symbol import multitask_symbol_factory as F
    for glob in (False, True):
        net = F.get_multi_symbol("resnet-50", 128, num_classes=8, batch_size=1, device=CPU, use_global_stats=glob)
        assert all(node.use_global_stats == glob for node in net.g.bn_nodes.values())


def test_graph_set_global_stats():
    from dspnet_amd import engine as E
    g = E.Graph(CPU)
    x = g.tensor((1, 8, 8, 8), "data", requires_grad=False, dtype=torch.float32)
    a = g.add(E.BatchNorm(g, x, "first_bn")).out
    b = g.add(E.BatchNorm(g, a, "second_bn", fix_gamma=True)).out
    g.add(E.BatchNorm(g, b, "third_bn"))
    nodes = g.bn_nodes
    assert list(nodes) == ["first_bn", "second_bn", "third_bn"] and not any(n.use_global_stats for n in nodes.values())
    assert g.set_global_stats(["third_bn"]) == ["third_bn"] and nodes["third_bn"].use_global_stats
    assert g.set_global_stats(r"fi") == ["first_bn"]
    for bad in (r"bn", r"fourth", ["first_bn", "fourth_bn"]):
        with pytest.raises(ValueError):
            g.set_global_stats(bad)
    assert [n.use_global_stats for n in nodes.values()] == [True, False, True]
    # the mode decides the finalize's block: fixed statistics win over tracking
    g.bn_track = True
    assert nodes["first_bn"]._moving()._obj.mode == fn.BN_GLOBAL and nodes["second_bn"]._moving()._obj.mode == fn.BN_TRACK
    g.bn_track = False
    assert nodes["second_bn"]._moving() is None
    g.finalize(0)
    with pytest.raises(RuntimeError, match="before finalize"):
        g.set_global_stats(["first_bn"])
