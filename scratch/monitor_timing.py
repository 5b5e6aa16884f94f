"""profiles/monitor_timing.txt: the training monitor's three table launches at the bench shape (resnet-50 multi-task,
512 x 512, batch 32, pattern '.*', grads=True) between HIP events, beside the bandwidth sgd_kernel reaches in the same
process and the wall time of a Python loop of per-tensor torch norms over the same tensors.
    python scratch/monitor_timing.py            (profiler off)
    rocprofv3 --kernel-trace --stats --output-format csv -- python scratch/monitor_timing.py --profile     (two armed steps only)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dspnet_amd import functional as fn  # noqa: E402
from dspnet_amd import synthetic  # noqa: E402
from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train  # noqa: E402
from dspnet_amd.train import monitor as M  # noqa: E402
from dspnet_amd.train.solver import MultiTaskSolver  # noqa: E402

B, S = int(os.environ.get("MON_BATCH", 32)), int(os.environ.get("MON_SIZE", 512))
PROFILE_ONLY = "--profile" in sys.argv
dev = torch.device("cuda", 0)


def say(s):
    print(s, flush=True)


net = get_multi_symbol_train("resnet-50", (3, S, S), num_classes=8, batch_size=B, device=dev, seed=0)
gen = synthetic.rng(0)
solver = MultiTaskSolver(net)
solver.set_batch(torch.from_numpy(synthetic.images(B, S, S, gen)).to(dev),
                 torch.from_numpy(synthetic.det_labels(B, gen=gen, height=S, width=S)).to(dev),
                 torch.from_numpy(synthetic.seg_labels(B, S, S, gen=gen)).to(dev))
g = net.g
mon = M.Monitor(1, grads=True).install(net)
solver.monitor = mon
for _ in range(2):
    mon.tic(); solver.step(); res = mon.toc()
torch.cuda.synchronize()
say("resnet-50 multi-task, %dx%d, batch %d, pattern='.*', grads=True: %d names (%d skipped as virtual)"
    % (S, S, B, len(res), len(mon.skipped)))
if PROFILE_ONLY:
    sys.exit(0)


def timed(f, reps=10):
    f(); torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2], ts[0], ts[-1]


mon.activated = True
say("launch        rows   chunks        bytes   median ms (min .. max of 10)    GB/s")
total_ms = 0.0
for which in M.PASSES:
    ps = mon.passes[which]
    nbytes = mon.bytes_read(which)
    med, lo, hi = timed(lambda: mon._launch(which))
    total_ms += med
    say("%-12s %5d %8d %12d   %8.3f (%.3f .. %.3f)   %8.1f" % (which, ps.table[1], ps.table[2], nbytes, med, lo, hi, nbytes / med / 1e6))
mon.activated = False
say("three launches together: %.3f ms of device time (HIP events, median of 10 each)" % total_ms)
# stage 2 alone is not separable by events inside the call; the largest activation row gives its length
big = max(ps_rows * C for _, _, ps_rows, C, _ in mon.passes["activations"].entries)
say("largest activation row: %d elements = %d chunks of %d" % (big, -(-big // fn.tensor_stats_chunk_elems()), fn.tensor_stats_chunk_elems()))

# the project's HBM-roof kernel in the same session: sgd_kernel reads w, grad, mom and writes w, mom: 5 x 4 bytes per element
n = g.arena.numel()
w, gr, mo = g.arena.clone(), g.grad_arena.clone(), g.mom_arena.clone()
med, lo, hi = timed(lambda: fn.sgd_momentum(w, gr, mo, 0.0, 0.9, 0.0, 1.0))
say("sgd_kernel over the %d-float arena: %.3f ms (%.3f .. %.3f) = %.1f GB/s at 20 bytes per element" % (n, med, lo, hi, 20.0 * n / med / 1e6))
# ... and over a stream of the activations' size, so that the comparison is not one of 100 MB against gigabytes
na = min(mon.bytes_read("activations") // 4 // 3, 1 << 29)
a3 = [torch.zeros(na, device=dev) for _ in range(3)]
med, lo, hi = timed(lambda: fn.sgd_momentum(a3[0], a3[1], a3[2], 0.0, 0.9, 0.0, 1.0))
say("sgd_kernel over 3 x %d floats: %.3f ms (%.3f .. %.3f) = %.1f GB/s at 20 bytes per element" % (na, med, lo, hi, 20.0 * na / med / 1e6))
del a3

# the parent commit's only alternative: a Python loop of per-tensor torch norms over the same tensor set, with its synchronisations
tensors = [(t.data if t.channels is None else t.data[..., :t.channels]) for t in g.tensors.values() if t.data is not None]
tensors += [p.grad for p in g.param_order] + [p.data for p in g.param_order]
tensors += [b for nd in g.bn_nodes.values() for b in (nd.moving_mean, nd.moving_var)]


def loop():
    return [float(t.float().norm().item()) / (t.numel() ** 0.5) for t in tensors]


loop(); torch.cuda.synchronize()
ts = []
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter(); loop(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
say("python loop of .float().norm().item() over the same %d tensors: %.1f ms wall (runs: %s)" % (len(tensors), sorted(ts)[1], ", ".join("%.1f" % t for t in ts)))
ts = []
for _ in range(3):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    mon.activated = True
    for which in M.PASSES:
        mon._launch(which)
    out = mon._read()
    ts.append((time.perf_counter() - t0) * 1e3)
    mon.activated = False
say("monitor: three launches + read-out of %d records on the host: %.2f ms wall (runs: %s)" % (len(out), sorted(ts)[1], ", ".join("%.2f" % t for t in ts)))
# the cost inside a step: armed step (eager + 3 launches + toc) against an eager step
solver.monitor = None
def plain():
    solver.step(); torch.cuda.synchronize()
def armed():
    mon.tic(); solver.step(); mon.toc()
plain(); t0 = time.perf_counter(); [plain() for _ in range(5)]; tp = (time.perf_counter() - t0) / 5 * 1e3
solver.monitor = mon
armed(); t0 = time.perf_counter(); [armed() for _ in range(5)]; ta = (time.perf_counter() - t0) / 5 * 1e3
say("eager step %.1f ms; armed step with toc() %.1f ms (wall, mean of 5)" % (tp, ta))
