"""The training monitor without a GPU: the validated table builder of the statistics pass (functional.tensor_stats_table), the
mx.mon.Monitor semantics of train.monitor.Monitor against a stubbed statistics function, its names on a graph built on the
CPU device, and the argument checks of include/dspn_monitor.h (no kernel runs here: tests/test_monitor_gpu.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from dspnet_amd import operator as op
from dspnet_amd.symbol import multitask_symbol_factory as F
from dspnet_amd.symbol.multitask_symbol_builder import known_argument_names
from dspnet_amd.train import monitor as M

CPU = torch.device("cpu")


# ------------------------------------------------------------------ the table builder
def test_table_builder_rejects_bad_rows():
    buf = torch.zeros(64)
    p = buf.data_ptr()
    ok = (p, torch.float32, 2, 3, 4)
    fn.tensor_stats_table([ok], CPU)
    for bad, text in [((p, torch.float32, 2, 5, 4), "C <= ld"),            # ld < C
                      ((p, torch.float32, 0, 3, 4), "rows >= 1"),          # rows < 1
                      ((p, torch.float32, -1, 3, 4), "rows >= 1"),
                      ((p, torch.float32, 2, 0, 4), "1 <= C"),
                      ((p, torch.float16, 2, 3, 4), "dtype"),              # unknown dtypes
                      ((p, torch.int32, 2, 3, 4), "dtype"),
                      ((p, "f32", 2, 3, 4), "dtype"),
                      ((0, torch.float32, 2, 3, 4), "null"),               # null base
                      ((p + 2, torch.float32, 2, 3, 4), "aligned"),        # a float at an odd 2-byte address
                      ((p + 1, torch.bfloat16, 2, 3, 4), "aligned")]:
        with pytest.raises(ValueError, match=text):
            fn.tensor_stats_table([ok, bad], CPU)
    with pytest.raises(ValueError, match="at least one row"):
        fn.tensor_stats_table([], CPU)
    fn.tensor_stats_table([(p + 2, torch.bfloat16, 2, 3, 4), (p + 4, torch.float32, 1, 7, 7)], CPU)


def test_table_builder_chunk_prefix_matches_numpy():
    L = fn.tensor_stats_chunk_elems()
    rng = np.random.default_rng(5)
    buf = torch.zeros(64)
    shapes = [(1, 1, 1), (1, L - 1, L - 1), (1, L, L), (1, L + 1, L + 1), (1, 3 * L + 5, 3 * L + 5), (7, 3, 4), (5, 19, 20),
              (5, 19, 24), (2 * L // 19 + 3, 19, 20), (L, 3, 4)]
    shapes += [(int(r), int(c), int(c + e)) for r, c, e in zip(rng.integers(1, 3000, 200), rng.integers(1, 70, 200),
                                                               rng.integers(0, 9, 200))]
    entries = [(buf.data_ptr() + 4 * (i % 3), torch.bfloat16 if i % 4 == 0 else torch.float32, r, c, ld)
               for i, (r, c, ld) in enumerate(shapes)]
    dev, n_rows, n_chunks = fn.tensor_stats_table(entries, CPU)
    tab = dev.numpy().view(np.dtype(fn.STATS_ROW_FIELDS))
    assert tab.dtype.itemsize == 40 and n_rows == len(shapes) == len(tab)
    elems = np.array([r * c for r, c, _ in shapes], np.int64)
    chunks = -(-elems // L)
    assert np.array_equal(tab["first_chunk"], np.concatenate([[0], np.cumsum(chunks)[:-1]]))
    assert n_chunks == int(chunks.sum())
    assert np.array_equal(tab["rows"], [s[0] for s in shapes]) and np.array_equal(tab["C"], [s[1] for s in shapes])
    assert np.array_equal(tab["ld"], [s[2] for s in shapes]) and np.array_equal(tab["base"], [e[0] for e in entries])
    assert np.array_equal(tab["dtype"], [1 if e[1] == torch.bfloat16 else 0 for e in entries]) and not tab["reserved"].any()


def test_entry_of_a_tensor():
    t = torch.zeros(2, 5, 5, 20)
    assert fn.tensor_stats_entry(t) == (t.data_ptr(), torch.float32, 1, 1000, 1000)
    assert fn.tensor_stats_entry(t, 20) == (t.data_ptr(), torch.float32, 1, 1000, 1000)
    assert fn.tensor_stats_entry(t, 19) == (t.data_ptr(), torch.float32, 50, 19, 20)


# ------------------------------------------------------------------ C ABI
def test_cabi_argument_checks_without_gpu():
    lib = _lib.lib()
    L = lib.dspn_tensor_stats_chunk_elems()
    assert L > 0 and L % 16 == 0 and L == fn.tensor_stats_chunk_elems()
    ws = lib.dspn_tensor_stats_workspace_bytes
    assert ws(3, 10) == ws(3, 10) == 10 * 48 and ws(300, 10000) == 10000 * 48      # pure: one partial per chunk
    assert ws(0, 10) == 0 and ws(3, 0) == 0 and ws(-1, -1) == 0
    assert np.dtype(fn.STATS_OUT_FIELDS).itemsize == 48 and np.dtype(fn.STATS_ROW_FIELDS).itemsize == 40
    p = ctypes.c_void_p(256)        # never dereferenced: every call below fails its checks first
    call = lib.dspn_tensor_stats
    assert call(None, 1, 1, p, p, 48, None) == -1 and b"null pointer" in lib.dspn_last_error()
    assert call(p, 1, 1, None, p, 48, None) == -1 and b"null pointer" in lib.dspn_last_error()
    assert call(p, 1, 1, p, None, 48, None) == -1 and b"workspace" in lib.dspn_last_error()
    assert call(p, 0, 1, p, p, 48, None) == -1 and b"n_rows" in lib.dspn_last_error()
    assert call(p, -3, 1, p, p, 48, None) == -1 and b"n_rows" in lib.dspn_last_error()
    assert call(p, 2, 1, p, p, 96, None) == -1 and b"n_chunks" in lib.dspn_last_error()
    assert call(p, 2, 5, p, p, 5 * 48 - 1, None) == -1 and b"workspace too small" in lib.dspn_last_error()


# ------------------------------------------------------------------ Monitor semantics (statistics function stubbed)
@pytest.fixture(scope="module")
def net():
    real = op.MultiBoxPrior

    def fake_prior(data, sizes, ratios, **kw):       # the one operator a graph BUILD calls (tests/test_graph_wiring.py)
        H, W = data if isinstance(data, tuple) else data.shape[-2:]
        return torch.zeros(1, H * W * (len(sizes) + len(ratios) - 1), 4)
    op.MultiBoxPrior = fake_prior
    try:
        return F.get_multi_symbol_train("resnet-50", 128, num_classes=8, batch_size=1, device=CPU)
    finally:
        op.MultiBoxPrior = real


class StubStats:
    """stands in for functional.tensor_stats: row i of a table gets sumsq = (i + 1) * n_i (so rms = sqrt(i + 1)), and the
    launches are counted"""

    def __init__(self):
        self.calls = []

    def __call__(self, table, out=None, workspace=None):
        dev, n_rows, n_chunks = table
        tab = dev.numpy().view(np.dtype(fn.STATS_ROW_FIELDS))
        rec = np.zeros(n_rows, dtype=fn.STATS_OUT_FIELDS)
        rec["sumsq"] = (np.arange(n_rows) + 1) * (tab["rows"] * tab["C"])
        self.calls.append(n_rows)
        return rec


def run_step(mon):
    mon.tic()
    mon.after_forward(); mon.after_backward(); mon.after_update()
    return mon.toc()


def test_interval_arming_and_toc_outside_an_armed_batch(net):
    mon = M.Monitor(3, pattern="^conv0").install(net)
    mon.stats = stub = StubStats()
    assert mon.toc() == [] and not mon.armed
    got = [run_step(mon) for _ in range(7)]
    assert [bool(r) for r in got] == [True, False, False, True, False, False, True]      # batches 1, 4, 7 (mx.mon.Monitor.tic)
    assert [r[0][0] for r in got if r] == [1, 4, 7]
    assert len(stub.calls) == 3 * 2                            # activations + parameters per armed batch, no gradient table
    assert mon.toc() == []
    with pytest.raises(ValueError):
        M.Monitor(0)


def test_pattern_sort_and_values(net):
    mon = M.Monitor(1, pattern="^stage1.*_weight$", sort=True).install(net)
    mon.stats = StubStats()
    res = run_step(mon)
    names = [k for _, k, _ in res]
    want = sorted(p.name for p in net.g.param_order if p.name.startswith("stage1") and p.name.endswith("_weight"))
    assert names == want and len(names) > 5
    order = mon.names("parameters")
    for n, k, v in res:
        assert n == 1 and v.endswith("\t") and float(v) == pytest.approx(math.sqrt(order.index(k) + 1), rel=1e-15)
    unsorted = M.Monitor(1, pattern="^stage1.*_weight$").install(net)
    unsorted.stats = StubStats()
    assert [k for _, k, _ in run_step(unsorted)] == order != names        # table (graph) order unless sort=True
    assert set(mon.raw()) == set(names) and mon.raw()[names[0]]["n"] == net.g.params[names[0]].size
    # stat_func receives the record, not the tensor
    custom = M.Monitor(1, stat_func=lambda rec: int(rec["n"]), pattern="^conv0_weight$").install(net)
    custom.stats = StubStats()
    assert run_step(custom) == [(1, "conv0_weight", "%d\t" % (64 * 7 * 7 * 3))]      # 3 logical input channels of the padded 4


def test_default_statistic_on_non_finite_records():
    rec = np.zeros(1, dtype=M.RECORD_FIELDS)[0]
    rec["n"], rec["sumsq"] = 4, 16.0
    assert M.rms(rec) == 2.0
    rec["n_posinf"] = 1
    assert M.rms(rec) == float("inf")
    rec["n_neginf"], rec["n_posinf"] = 2, 0
    assert M.rms(rec) == float("inf")
    rec["n_nan"] = 1
    assert math.isnan(M.rms(rec))


def test_alias_fan_out_and_skipped_virtual_tensors(net):
    g = net.g
    mon = M.Monitor(1).install(net)
    mon.stats = StubStats()
    virtual = {k for k, t in g.tensors.items() if t.data is None}
    assert virtual and set(mon.skipped) == virtual and all("virtual" in why for why in mon.skipped.values())
    aliases = {k: t.alias_of.name for k, t in g.tensors.items() if t.alias_of is not None and t.data is not None}
    assert aliases
    rows = mon.passes["activations"].names
    for alias, src in aliases.items():
        (row,) = [r for r in rows if alias in r]
        assert src in row                                      # one row, both names
    raw = (run_step(mon), mon.raw())[1]
    for alias, src in aliases.items():
        assert raw[alias] == raw[src]
    assert set(mon.names("activations")) == set(g.tensors) - virtual
    assert len(rows) == len(set(g.tensors) - virtual) - len(aliases)
    assert not set(mon.names()) & virtual


def test_parameter_and_aux_names_are_the_reference_symbols(net):
    g = net.g
    mon = M.Monitor(1, grads=True).install(net)
    inputs = {"data", "label_det", "seg_out_label"}
    moving = {name + s for name, _, _ in g.bn_names for s in ("_moving_mean", "_moving_var")}
    assert set(mon.names("parameters")) == (known_argument_names(g) - inputs) | moving
    assert set(mon.names("gradients")) == {p.name + "_grad" for p in g.param_order}
    assert len(mon.names()) == len(set(mon.names()))
    # the rows of a parameter and of its gradient are the same range of the two arenas
    tab = {k: mon.passes[k].table[0].numpy().view(np.dtype(fn.STATS_ROW_FIELDS)) for k in ("parameters", "gradients")}
    for which, arena in (("parameters", g.arena), ("gradients", g.grad_arena)):
        names = [r[0] for r in mon.passes[which].names]
        for p in g.param_order:
            row = tab[which][names.index(p.name + ("_grad" if which == "gradients" else ""))]
            assert row["base"] == arena.data_ptr() + 4 * p.offset
            assert (row["rows"] - 1) * row["ld"] + row["C"] <= p.size
    assert M.Monitor(1, pattern="^stage1").install(net).passes["gradients"].table is None       # grads=False: no table
