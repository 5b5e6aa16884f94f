"""mx.mon.Monitor for this build: train/train_multitask.py:93-94, :156-159, :249, :317 hands
`mx.mon.Monitor(iter_monitor, pattern=monitor_pattern)` to Module.fit, which prints norm(x) / sqrt(x.size) of every
operator output, argument and aux state whose name matches the pattern, every `iter_monitor` batches.

Here the statistics of all monitored tensors of a kind come from ONE batched pass over a descriptor table
(functional.tensor_stats, include/dspn_monitor.h): sum of squares, sum and largest magnitude of the finite elements and
the numbers of NaN / +Inf / -Inf, accumulated in double and bit-reproducible.  Three tables, built once in install():

    activations   after forward                                       <tensor> as Graph.tensors keys them
    gradients     after backward and the all-reduce's finish()        <param>_grad (grads=True; rows of the gradient arena)
    parameters    after the update, with the aux states               <param>, <bn>_gamma, <bn>_moving_mean, <bn>_moving_var

-- the order Module.fit gives them: tic, forward_backward, update, toc.  MultiTaskSolver calls the three hooks of an
armed iteration (after_forward / after_backward / after_update); nothing waits until toc() reads the records.

Activation gradients are not offered: they alias, accumulate in place and may hold piece planes.  A tensor reached under
two names (a BlockGrad alias) is measured once and reported under both.  A virtual tensor (a deferred BatchNorm output
that is never materialised) cannot be read: it is listed in `skipped` with the reason.  The `_gamma` of a fix_gamma
BatchNorm, which MXNet lists and sets to 1 and this build does not materialise, is reported from a buffer of ones.
Padded lanes (channels 3 -> 4, 19 -> 20, bf16 to multiples of 8, in activations and in convolution weights) are not
part of a tensor: n is the logical element count, as the reference's x.size."""
import logging
import math
import re

import numpy as np
import torch

from .. import functional as fn

# the host record of one tensor: include/dspn_monitor.h dspn_stats_out + n, the number of (logical) elements
RECORD_FIELDS = [("sumsq", "<f8"), ("sum", "<f8"), ("absmax", "<f4"), ("n_nan", "<u8"), ("n_posinf", "<u8"),
                 ("n_neginf", "<u8"), ("n", "<i8")]
PASSES = ("activations", "gradients", "parameters")


def rms(rec):
    """the default statistic, norm(x) / sqrt(x.size), with MXNet's result for non-finite data: NaN when the tensor holds
    one, inf when it holds infinities only"""
    if rec["n_nan"] > 0:
        return float("nan")
    if rec["n_posinf"] + rec["n_neginf"] > 0:
        return float("inf")
    return math.sqrt(float(rec["sumsq"]) / float(rec["n"]))


def nonfinite(rec):
    return int(rec["n_nan"]) + int(rec["n_posinf"]) + int(rec["n_neginf"])


def param_entry(p, arena):
    """the statistics row of a parameter inside `arena` (the parameter, gradient or momentum arena): its LOGICAL elements --
    a convolution weight [Cout, kh, kw, Cin_phys] counts the first Cin of every row, a per-channel vector its first
    `channels` entries"""
    base = arena.data_ptr() + 4 * p.offset
    if p.kind == "conv" and p.logical is not None and p.logical[1] < p.shape[3]:
        return (base, torch.float32, p.shape[0] * p.shape[1] * p.shape[2], p.logical[1], p.shape[3])
    n = int(p.logical[0]) if (p.kind == "vec" and p.logical is not None) else p.size
    return (base, torch.float32, 1, n, n)


def tensor_entry(t):
    """the statistics row of a materialised activation, or the reason it has none"""
    if t.data is None:
        return None, "virtual: a deferred BatchNorm output, applied inside the convolutions that read it and never materialised"
    if t.data.dtype not in (torch.float32, torch.bfloat16):
        return None, "dtype %s (float32 and bfloat16 are read)" % t.data.dtype
    if not t.data.is_contiguous() or t.data.numel() == 0:
        return None, "not a contiguous, non-empty buffer"
    return fn.tensor_stats_entry(t.data, t.channels), None


class _Pass:
    """one table launch: rows (one per distinct buffer), the names each row is reported under, its element count"""

    def __init__(self):
        self.entries, self.names, self.index = [], [], {}
        self.table = self.out = self.ws = None
        self.result = None

    def add(self, name, entry):
        key = (entry[0], entry[1]) + tuple(entry[2:])
        if key in self.index:
            self.names[self.index[key]].append(name)
            return
        self.index[key] = len(self.entries)
        self.entries.append(entry)
        self.names.append([name])

    def counts(self):
        return np.array([rows * C for _, _, rows, C, _ in self.entries], np.int64)


class Monitor:
    """Monitor(interval, stat_func=None, pattern='.*', sort=False, grads=False): the interface of mx.mon.Monitor.
    stat_func receives the tensor's record (numpy record with the fields of RECORD_FIELDS), not the tensor, and returns a
    number; the default is rms.  grads=True adds '<param>_grad'.  install(net) -- a MultiTaskNet or its Graph -- builds
    the tables; tic() arms every interval-th batch; toc() -> [(nbatch, name, value string)]; toc_print() logs them;
    raw() -> {name: record} of the last read-out.  skipped: {name: reason} of matching tensors that cannot be read.
    stats: the function that runs one table (functional.tensor_stats)."""

    def __init__(self, interval, stat_func=None, pattern=".*", sort=False, grads=False):
        if int(interval) < 1:
            raise ValueError("Monitor: interval must be >= 1, got %r" % (interval,))
        self.interval, self.stat_func, self.sort, self.grads = int(interval), stat_func or rms, bool(sort), bool(grads)
        self.re_prog = re.compile(pattern)
        self.step, self.activated = 0, False
        self.net = self.g = None
        self.passes, self.skipped = {}, {}
        self.stats = fn.tensor_stats
        self._raw = {}
        self._keep = []            # buffers the tables point into that nothing else holds (the ones of fix_gamma)

    # -- construction -----------------------------------------------------------
    def install(self, net):
        g = getattr(net, "g", net)
        self.net, self.g = net, g
        self.passes = {k: _Pass() for k in PASSES}
        self.skipped, self._keep = {}, []
        match = self.re_prog.match
        act, grad, par = (self.passes[k] for k in PASSES)
        for name, t in g.tensors.items():
            if not match(name):
                continue
            entry, why = tensor_entry(t)
            if entry is None:
                self.skipped[name] = why
            else:
                act.add(name, entry)
        for p in g.param_order:
            if match(p.name):
                par.add(p.name, param_entry(p, g.arena))
            if self.grads and match(p.name + "_grad"):
                grad.add(p.name + "_grad", param_entry(p, g.grad_arena))
        ones = None
        for name, channels, fix_gamma in g.bn_names:
            node = g.bn_nodes[name]
            if fix_gamma and match(name + "_gamma"):
                if ones is None or ones.numel() < channels:
                    ones = torch.ones(max(channels, 2048), dtype=torch.float32, device=g.device)
                    self._keep.append(ones)
                par.add(name + "_gamma", (ones.data_ptr(), torch.float32, 1, channels, channels))
            for suffix, buf in (("_moving_mean", node.moving_mean), ("_moving_var", node.moving_var)):
                if match(name + suffix):
                    par.add(name + suffix, (buf.data_ptr(), torch.float32, 1, channels, channels))
        for ps in self.passes.values():
            if ps.entries:
                ps.table = fn.tensor_stats_table(ps.entries, g.device)
        return self

    def names(self, which=None):
        """every name that is reported (of one pass: 'activations' | 'gradients' | 'parameters'), in table order"""
        return [n for k in ((which,) if which else PASSES) for row in self.passes[k].names for n in row]

    def bytes_read(self, which):
        """bytes of logical elements one launch of the pass reads"""
        return int(sum(rows * C * (2 if dt == torch.bfloat16 else 4) for _, dt, rows, C, _ in self.passes[which].entries))

    # -- the iteration ------------------------------------------------------------
    @property
    def armed(self):
        return self.activated

    def tic(self):
        """start collecting for this batch when it is an interval-th one (call before the step)"""
        if self.step % self.interval == 0:
            for ps in self.passes.values():
                ps.result = None
            self.activated = True
        self.step += 1

    def _launch(self, which):
        ps = self.passes.get(which)
        if not self.activated or ps is None or ps.table is None:
            return
        if ps.out is None and self.stats is fn.tensor_stats:
            # caller-owned buffers per pass: a record stays until toc() reads it, whatever runs in between
            dev, n_rows, n_chunks = ps.table
            ps.out = torch.zeros(n_rows * np.dtype(fn.STATS_OUT_FIELDS).itemsize, dtype=torch.uint8, device=dev.device)
            ps.ws = torch.empty(max(1, fn.L().dspn_tensor_stats_workspace_bytes(n_rows, n_chunks)), dtype=torch.uint8,
                                device=dev.device)
        ps.result = self.stats(ps.table, out=ps.out, workspace=ps.ws)

    def after_forward(self):
        """activations.  What a side stream still writes (the detection branch, MultiBoxDetection) is joined first: a
        matter of stream order, not of values"""
        if not self.activated or self.passes["activations"].table is None:
            return
        if self.g.device.type == "cuda":
            self.g.join_side()
            det = getattr(self.net, "det", None)
            if det is not None:
                det.join()
        self._launch("activations")

    def after_backward(self):
        self._launch("gradients")

    def after_update(self):
        self._launch("parameters")

    def _read(self):
        out = {}
        for ps in self.passes.values():
            if ps.result is None:
                continue
            res = ps.result
            rec = fn.stats_records(res, len(ps.entries)) if isinstance(res, torch.Tensor) else np.asarray(res)
            full = np.zeros(len(ps.entries), dtype=RECORD_FIELDS)
            for k, _ in RECORD_FIELDS[:-1]:
                full[k] = rec[k]
            full["n"] = ps.counts()
            for i, names in enumerate(ps.names):
                for name in names:
                    out[name] = full[i]
            ps.result = None
        return out

    def toc(self):
        """end collecting: [(nbatch, name, value string)] of this batch, [] when it was not armed"""
        if not self.activated:
            return []
        self.activated = False
        self._raw = self._read()
        names = sorted(self._raw) if self.sort else list(self._raw)
        return [(self.step, name, str(self.stat_func(self._raw[name])) + "\t") for name in names]

    def toc_print(self):
        res = self.toc()
        for n, k, v in res:
            logging.info("Batch: {:7d} {:30s} {:s}".format(n, k, v))
        return res

    def raw(self):
        """{name: record} of the last read-out (toc / toc_print)"""
        return self._raw


class FiniteCheck:
    """fit(check_finite=N): every N-th step one statistics pass over the rows of the gradient arena and the loss outputs,
    launched behind the step; read() -- at the metric read-out, which synchronises anyway -- raises DspnError naming up
    to eight tensors that hold a NaN or an infinity, with their counts."""

    LOSS_TENSORS = ("cls_prob", "loc_loss", "seg_prob_nhwc")

    def __init__(self, net, every):
        g = getattr(net, "g", net)
        self.every, self.count = int(every), 0
        ps = self.ps = _Pass()
        for p in g.param_order:
            ps.add(p.name + "_grad", param_entry(p, g.grad_arena))
        for name in self.LOSS_TENSORS:
            t = g.tensors.get(name)
            entry = tensor_entry(t)[0] if t is not None else None
            if entry is not None:
                ps.add(name, entry)
        ps.table = fn.tensor_stats_table(ps.entries, g.device)
        dev, n_rows, n_chunks = ps.table
        ps.out = torch.zeros(n_rows * np.dtype(fn.STATS_OUT_FIELDS).itemsize, dtype=torch.uint8, device=dev.device)
        ps.ws = torch.empty(max(1, fn.L().dspn_tensor_stats_workspace_bytes(n_rows, n_chunks)), dtype=torch.uint8, device=dev.device)

    def launch(self):
        self.count += 1
        if self.count % self.every == 0:
            self.ps.result = fn.tensor_stats(self.ps.table, out=self.ps.out, workspace=self.ps.ws)

    def read(self):
        if self.ps.result is None:
            return
        rec = fn.stats_records(self.ps.result, len(self.ps.entries))
        self.ps.result = None
        bad = [(names, r) for names, r in zip(self.ps.names, rec) if nonfinite(r)]
        if bad:
            from .._lib import DspnError
            raise DspnError("check_finite: step %d left non-finite values in %d tensor(s): " % (self.count, len(bad)) + "; ".join(
                "%s (%d NaN, %d +Inf, %d -Inf)" % ("/".join(names), r["n_nan"], r["n_posinf"], r["n_neginf"])
                for names, r in bad[:8]) + (" ..." if len(bad) > 8 else ""))
