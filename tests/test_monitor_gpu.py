"""The statistics pass of the training monitor on the GPU (include/dspn_monitor.h, dspnet_amd/csrc/monitor.hip) against numpy
float64 on host copies -- at the edges of its chunk length, of its 16-byte loads and of its element types -- and the monitor
at graph level: what it reports, that a monitored iteration leaves the bits of an unmonitored one, fit(check_finite=...).

Tolerances (L = chunk length, n <= 10^6 elements): absmax and the three counts are exact.  sumsq: every float32 square is
exact in double and a sum of n non-negative terms carries at most (n - 1) * 2^-53 ~ 1.2e-10 relative, so 1e-9.  sum:
n * 2^-53 * sum|x| absolute."""
import collections
import math

import numpy as np
import pytest
import torch

from dspnet_amd import _lib
from dspnet_amd import functional as fn
from dspnet_amd import synthetic
from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
from dspnet_amd.train import monitor as M
from dspnet_amd.train.solver import MultiTaskSolver, fit

pytestmark = pytest.mark.gpu

L = fn.tensor_stats_chunk_elems()
OUT = np.dtype(fn.STATS_OUT_FIELDS)
FIELDS = ("sumsq", "sum", "absmax", "n_nan", "n_posinf", "n_neginf")


# ------------------------------------------------------------------ kernel level
def _values(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "denormal":
        x = (rng.integers(1, 1 << 22, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
        assert (np.abs(x) < np.finfo(np.float32).tiny).all() and (x != 0).all()
        return x
    if kind == "huge":                                        # the float32 square overflows, the double must not
        return (np.float32(3e38) * rng.choice(np.array([-1, 1], np.float32), n)).astype(np.float32)
    if kind == "nonfinite":                                   # NaN at the first and the last logical element, infinities elsewhere
        x = rng.standard_normal(n).astype(np.float32)
        x[0] = x[-1] = np.nan
        if n > 8:
            x[n // 3], x[n // 2], x[n // 2 + 1] = np.inf, -np.inf, -np.inf
        if n > 2 * L:
            x[L - 1], x[L], x[2 * L + 3] = np.inf, np.nan, -np.inf
        return x
    raise KeyError(kind)


# name -> (dtype, rows, C, ld, offset of the base in elements, values)
SPECS = collections.OrderedDict()
for _n in (1, 3, 4, 255, 256, 257, L - 1, L, L + 1, 3 * L + 5):
    SPECS["flat_%d" % _n] = ("f32", 1, _n, _n, 0, "normal")
SPECS["pad_7x3_4"] = ("f32", 7, 3, 4, 0, "normal")
SPECS["pad_5x19_20"] = ("f32", 5, 19, 20, 0, "normal")
SPECS["pad_bf16_5x19_24"] = ("bf16", 5, 19, 24, 0, "normal")
SPECS["pad_big_19_20"] = ("f32", 2 * L // 19 + 7, 19, 20, 0, "normal")          # rows * C > 2L: a chunk boundary falls mid-row
SPECS["pad_big_3_4"] = ("f32", L, 3, 4, 0, "normal")
SPECS["pad_big_bf16_19_24"] = ("bf16", 2 * L // 19 + 7, 19, 24, 0, "normal")
SPECS["pad_big_nonfinite"] = ("f32", 2 * L // 19 + 7, 19, 20, 0, "nonfinite")
SPECS["pad_unaligned_pitch_5x19_21"] = ("f32", 5, 19, 21, 0, "normal")          # a pitch that is no multiple of 16 bytes
SPECS["off1_flat_257"] = ("f32", 1, 257, 257, 1, "normal")                       # a base that is 4-byte aligned only
SPECS["off1_flat_3L5"] = ("f32", 1, 3 * L + 5, 3 * L + 5, 1, "nonfinite")
SPECS["off1_pad_5x19_20"] = ("f32", 5, 19, 20, 1, "normal")
SPECS["off1_pad_big"] = ("f32", 2 * L // 19 + 7, 19, 20, 1, "normal")
SPECS["off3_flat_2"] = ("f32", 1, 2, 2, 3, "normal")                             # shorter than its head
for _n in (1, 7, 8, 9, L + 1):
    SPECS["bf16_flat_%d" % _n] = ("bf16", 1, _n, _n, 0, "normal")
SPECS["bf16_off1_flat"] = ("bf16", 1, L + 9, L + 9, 1, "normal")                 # 2-byte aligned only
SPECS["bf16_off3_nonfinite"] = ("bf16", 1, 2 * L + 11, 2 * L + 11, 3, "nonfinite")
SPECS["zeros"] = ("f32", 1, L + 1, L + 1, 0, "zeros")
SPECS["denormals"] = ("f32", 1, 1000, 1000, 0, "denormal")
SPECS["huge"] = ("f32", 1, 1000, 1000, 0, "huge")
SPECS["nonfinite_flat"] = ("f32", 1, 3 * L + 5, 3 * L + 5, 0, "nonfinite")
SPECS["nonfinite_small"] = ("f32", 1, 2, 2, 0, "nonfinite")                      # nothing finite at all
SMALL = 300 - len(SPECS)                                                         # ... and many rows of 1 - 8 elements


class Case:
    def __init__(self, name, spec, dev, rng):
        dtype, rows, C, ld, off, kind = spec
        self.name, self.n = name, rows * C
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        logical = torch.from_numpy(_values(kind, rows * C, rng)).to(tdt)          # (bf16: rounded here, the checker reads the rounded values)
        even = (torch.arange(rows)[:, None] + torch.arange(ld)[None, :]) % 2 == 0
        phys = torch.where(even, float("nan"), 1e30).to(tdt)                      # the pad lanes: NaN and 1e30, never zero
        phys[:, :C] = logical.view(rows, C)
        flat = phys.reshape(-1)[:(rows - 1) * ld + C]                             # nothing behind the last logical element is allocated for
        buf = torch.full((off + flat.numel(),), float("nan"), dtype=tdt)
        buf[off:] = flat
        self.buf = buf.to(dev)                                                    # torch allocations are 256-byte aligned
        assert self.buf.data_ptr() % 16 == 0
        self.entry = (self.buf.data_ptr() + off * buf.element_size(), tdt, rows, C, ld)
        self.x = logical.to(torch.float64).numpy()

    def expected(self):
        x = self.x
        fin = np.isfinite(x)
        f = x[fin]
        return dict(sumsq=math.fsum(f * f), sum=math.fsum(f), abs_sum=math.fsum(np.abs(f)),       # (f * f is exact in double)
                    absmax=np.float32(np.max(np.abs(f))) if f.size else np.float32(0),
                    n_nan=int(np.isnan(x).sum()), n_posinf=int((x == np.inf).sum()), n_neginf=int((x == -np.inf).sum()))


def run_table(entries, dev, **kw):
    table = fn.tensor_stats_table(entries, dev)
    return fn.stats_records(fn.tensor_stats(table, **kw), len(entries)).copy()


@pytest.fixture(scope="module")
def world(gpu_device):
    """every case, its record measured ALONE (a 1-row table each), and the 300-row table over all of them"""
    rng = np.random.default_rng(20240607)
    cases = collections.OrderedDict((k, Case(k, v, gpu_device, rng)) for k, v in SPECS.items())
    small = torch.from_numpy(rng.standard_normal(SMALL * 9 + 8).astype(np.float32))
    small_dev = small.to(gpu_device)
    for i in range(SMALL):
        c = Case.__new__(Case)
        c.name, c.n = "small_%d" % i, 1 + i % 8
        c.buf = small_dev
        c.entry = (small_dev.data_ptr() + 4 * (9 * i + i % 4), torch.float32, 1, c.n, c.n)
        c.x = small[9 * i + i % 4:9 * i + i % 4 + c.n].to(torch.float64).numpy()
        cases[c.name] = c
    assert len(cases) == 300
    alone = {k: run_table([c.entry], gpu_device)[0] for k, c in cases.items()}
    entries = [c.entry for c in cases.values()]
    together = run_table(entries, gpu_device)
    torch.cuda.synchronize()
    return cases, alone, together, entries


@pytest.mark.parametrize("name", list(SPECS) + ["small_0", "small_7", "small_%d" % (SMALL - 1)])
def test_record_matches_numpy_float64(world, name):
    cases, alone, _, _ = world
    c, rec = cases[name], alone[name]
    exp = c.expected()
    print(name, {k: rec[k] for k in FIELDS}, exp)
    assert rec["absmax"] == exp["absmax"] and rec["absmax"].dtype == np.float32
    assert (int(rec["n_nan"]), int(rec["n_posinf"]), int(rec["n_neginf"])) == (exp["n_nan"], exp["n_posinf"], exp["n_neginf"])
    assert abs(rec["sumsq"] - exp["sumsq"]) <= 1e-9 * exp["sumsq"]
    assert abs(rec["sum"] - exp["sum"]) <= c.n * 2.0 ** -53 * exp["abs_sum"]
    assert rec["reserved"] == 0


def test_pad_lanes_hold_nan_and_1e30_and_are_skipped(world):
    cases, alone, _, _ = world
    for name in ("pad_7x3_4", "pad_5x19_20", "pad_bf16_5x19_24", "pad_big_19_20", "pad_big_3_4", "off1_pad_big"):
        c = cases[name]
        whole = c.buf.float().cpu().numpy()
        assert np.isnan(whole).any() and (whole > 1e29).any()
        assert alone[name]["n_nan"] == 0 and alone[name]["absmax"] < 10


def test_second_run_and_the_300_row_table_give_the_same_bits(world, gpu_device):
    cases, alone, together, entries = world
    assert len(together) == 300
    for i, (k, c) in enumerate(cases.items()):
        assert together[i].tobytes() == alone[k].tobytes(), k             # alone == inside the table, bit for bit
    again = run_table(entries, gpu_device)
    assert again.tobytes() == together.tobytes()                          # run to run
    rev = run_table(entries[::-1], gpu_device)                            # ... and wherever the row sits in the table
    assert rev[::-1].tobytes() == together.tobytes()


def test_non_default_stream_with_caller_owned_buffers(world, gpu_device):
    cases, _, together, entries = world
    table = fn.tensor_stats_table(entries, gpu_device)
    out = torch.full((300 * OUT.itemsize + 64,), 0xAB, dtype=torch.uint8, device=gpu_device)
    ws = torch.empty(_lib.lib().dspn_tensor_stats_workspace_bytes(table[1], table[2]), dtype=torch.uint8, device=gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        got = fn.tensor_stats(table, out=out, workspace=ws)
    side.synchronize()
    assert got is out and fn.stats_records(out, 300).tobytes() == together.tobytes()
    assert bool((out[300 * OUT.itemsize:] == 0xAB).all())                 # nothing written behind the records
    short = torch.empty(ws.numel() - 1, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(_lib.DspnError, match="workspace too small"):
        fn.tensor_stats(table, out=out, workspace=short)


# ------------------------------------------------------------------ graph level
def make(seed=233, batch=2, size=128, **solver_kw):
    """the smallest multi-task training graph of tests/test_graph_gpu.py: resnet-50, batch 2, 128 x 128"""
    dev = torch.device("cuda", 0)
    net = get_multi_symbol_train("resnet-50", (3, size, size), num_classes=8, batch_size=batch, device=dev, seed=1)
    gen = synthetic.rng(seed)
    batch_t = (torch.from_numpy(synthetic.images(batch, size, size, gen)).to(dev),
               torch.from_numpy(synthetic.det_labels(batch, gen=gen, height=size, width=size)).to(dev),
               torch.from_numpy(synthetic.seg_labels(batch, size, size, gen=gen)).to(dev))
    solver = MultiTaskSolver(net, **solver_kw)
    solver.set_batch(*batch_t)
    return net, solver, batch_t


def state(net):
    g = net.g
    aux = [b for n in g.bn_nodes.values() for b in (n.moving_mean, n.moving_var)]
    return [g.arena, g.grad_arena, g.mom_arena] + aux


def assert_same_state(a, b):
    for i, (x, y) in enumerate(zip(state(a), state(b))):
        assert torch.equal(x, y), ("arena", "grad_arena", "mom_arena")[i] if i < 3 else "aux state %d" % (i - 3)


def rms64(x):
    x = x.double()
    return float(torch.sqrt((x * x).sum() / x.numel()))


def logical_param(p, arena):
    v = arena[p.offset:p.offset + p.size].view(p.shape)
    if p.kind == "conv":
        return v[..., :p.logical[1]]
    return v[:p.logical[0]] if (p.kind == "vec" and p.logical is not None) else v


def test_everything_is_reported_and_matches_torch_float64(gpu_device):
    net, solver, _ = make()
    g = net.g
    solver.step()                                  # (so that momenta and moving statistics are not at their start values)
    mon = M.Monitor(1, grads=True).install(net)
    solver.monitor = mon
    snap = {}
    hooks = {k: getattr(mon, k) for k in ("after_forward", "after_backward", "after_update")}

    def after_forward():
        hooks["after_forward"]()
        snap["act"] = {k: (t.data if t.channels is None else t.data[..., :t.channels]).clone() for k, t in g.tensors.items()
                       if t.data is not None}

    def after_backward():
        hooks["after_backward"]()
        snap["grad"] = g.grad_arena.clone()

    def after_update():
        hooks["after_update"]()
        snap["par"] = g.arena.clone()
        snap["aux"] = {name + s: getattr(g.bn_nodes[name], s[1:])[:ch].clone() for name, ch, _ in g.bn_names
                       for s in ("_moving_mean", "_moving_var")}

    mon.after_forward, mon.after_backward, mon.after_update = after_forward, after_backward, after_update
    mon.tic()
    solver.step()
    res = mon.toc()
    want = {k: rms64(v) for k, v in snap["act"].items()}
    want.update(snap_aux := {k: rms64(v) for k, v in snap["aux"].items()})
    for p in g.param_order:
        want[p.name] = rms64(logical_param(p, snap["par"]))
        want[p.name + "_grad"] = rms64(logical_param(p, snap["grad"]))
    want.update({name + "_gamma": 1.0 for name, _, fix in g.bn_names if fix})
    got = {k: float(v) for _, k, v in res}
    assert len(got) == len(res) and all(n == 1 for n, _, _ in res)
    assert set(got) == set(want)                   # every parameter, aux state, parameter gradient and materialised tensor
    assert set(mon.skipped) == {k for k, t in g.tensors.items() if t.data is None} and mon.skipped
    worst = max((abs(got[k] - want[k]) / want[k] if want[k] else abs(got[k]), k) for k in want if np.isfinite(want[k]))
    print("largest relative deviation of the default statistic:", worst, "over", len(want), "names")
    for k in want:
        assert np.isfinite(want[k]) and abs(got[k] - want[k]) <= 1e-9 * want[k], (k, got[k], want[k])
    assert sum(v > 0 for k, v in got.items() if k.endswith("_grad")) > 100 and len(snap_aux) == 2 * len(g.bn_names)
    raw = mon.raw()
    assert raw["data_nhwc"]["n"] == 2 * 128 * 128 * 3 and raw["conv0_weight"]["n"] == 64 * 7 * 7 * 3


def test_monitored_steps_leave_the_bits_of_unmonitored_steps(gpu_device):
    """Eager and replayed steps agree bit for bit on this graph (tests/test_graph_gpu.py asserts it for the parameters, this test
    for gradients, momenta and aux states too), so the rule is full equality: three steps with the monitor armed on every
    one == three plain steps, and a recorded step around one armed (eager) iteration == the same number of plain steps"""
    net_a, solver_a, _ = make()
    net_b, solver_b, _ = make()
    solver_b.monitor = mon = M.Monitor(1, grads=True).install(net_b)
    for _ in range(3):
        solver_a.step()
        mon.tic()
        solver_b.step()
        assert len(mon.toc()) > 500
    torch.cuda.synchronize()
    assert_same_state(net_a, net_b)
    for _ in range(2):
        solver_a.step()                            # a: 5 eager steps in all
    net_c, solver_c, _ = make()
    net_d, solver_d, _ = make()
    assert solver_c.capture(warmup=2) and solver_d.capture(warmup=2)
    solver_c.monitor = mon = M.Monitor(2, grads=True).install(net_c)
    mon.tic(); mon.toc()                           # (uses up the armed batch 0: the next armed one is the second step below)
    armed = []
    for _ in range(3):
        mon.tic()
        armed.append(mon.armed)
        solver_c.step()
        solver_d.step()
        armed.append(len(mon.toc()) > 500)
    assert armed == [False, False, True, True, False, False]
    assert solver_c._graph is not None and solver_c._replays == 2 and solver_d._replays == 3      # the recording was kept
    torch.cuda.synchronize()
    assert_same_state(net_d, net_c)                # replay, ARMED EAGER, replay == three replays
    assert_same_state(net_a, net_c)                # ... == five eager steps


def test_pattern_reports_only_matching_names(gpu_device):
    net, solver, _ = make()
    solver.monitor = mon = M.Monitor(1, pattern="^stage1.*_weight$", grads=True).install(net)
    mon.tic()
    solver.step()
    res = mon.toc_print()
    names = [k for _, k, _ in res]
    want = [p.name for p in net.g.param_order if p.name.startswith("stage1") and p.name.endswith("_weight")]
    assert names == want and len(names) > 5
    assert all(np.isfinite(float(v)) and float(v) > 0 for _, _, v in res) and mon.toc() == []


Batch = collections.namedtuple("Batch", "data label")


class OneBatch:
    """an iterator of `steps` copies of one batch, in the form fit() reads"""

    def __init__(self, batch, steps):
        self.batch, self.steps, self.i = batch, steps, 0

    def reset(self):
        self.i = 0

    def iter_next(self):
        return self.i < self.steps

    def next(self):
        self.i += 1
        return Batch([self.batch[0]], [self.batch[1], self.batch[2]]), None


class CountingLib:
    """the ctypes handle with a count per entry point"""

    def __init__(self, real):
        self._real, self.counts = real, collections.Counter()

    def __getattr__(self, name):
        f = getattr(self._real, name)

        def call(*a):
            self.counts[name] += 1
            return f(*a)
        return call


def test_check_finite(gpu_device, monkeypatch):
    net, solver, batch = make()
    fit(solver, OneBatch(batch, 1), num_epoch=1)                      # (first-use work of the step and of the metrics)
    counts = {}
    for every in (0, 1):
        proxy = CountingLib(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", proxy)
        # clean weights: nothing is raised.  (4 steps: one period of the range guard, whose launches differ from step to step)
        hist = fit(solver, OneBatch(batch, 4), num_epoch=1, check_finite=every)
        monkeypatch.undo()
        assert hist[0]["nbatch"] == 4
        counts[every] = proxy.counts
    extra = {"dspn_tensor_stats": 4, "dspn_tensor_stats_workspace_bytes": 1, "dspn_tensor_stats_chunk_elems": 1}
    assert not any(k.startswith("dspn_tensor_stats") for k in counts[0])              # 0: no launch (and no read)
    assert counts[1] - counts[0] == collections.Counter(extra) and not counts[0] - counts[1]      # every other call: unchanged
    g = net.g
    w = next(p for p in g.param_order if p.kind == "conv")
    g.arena[w.offset + 5] = float("nan")
    with pytest.raises(_lib.DspnError, match="check_finite") as e:
        fit(solver, OneBatch(batch, 3), num_epoch=1, check_finite=1)
    print(e.value)
    assert w.name in str(e.value) and "NaN" in str(e.value)
