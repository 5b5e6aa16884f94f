"""Static-graph executor for the DSPNet hot path.

MXNet binds a Symbol to an executor and calls forward()/backward()
(multi_solver.py:250-290).  This is the counterpart: a list of nodes with
statically shaped NHWC buffers, run in order for forward and in reverse for
backward.  Every node launches the HIP kernels of include/dspn_nn.h on torch's
current stream; nothing here computes with torch ops.

Gradient buffers: the first producer of a tensor's gradient in a backward pass
writes it, later ones accumulate (kernels take an `accumulate` flag).  A
residual add hands its output-gradient buffer to its inputs by aliasing, so
the gradient of a whole ResNet stage lives in one buffer that each unit
accumulates into (stream order makes this safe: every reader of the old value
was enqueued before the accumulating kernel).

All parameters live in one flat fp32 arena (with matching gradient and momentum
arenas) so the optimizer is one kernel and data-parallel reduction works on a
few large contiguous buckets.
"""
import math
import os
import re

import numpy as np
import torch

from . import backward_route as R, functional as fn, graph_plan
from .magnitudes import Magnitudes


# Test switch: with FUSE_BATCHNORM = False every BatchNorm runs its own statistics / apply / backward kernels and
# convolutions never read raw pre-BN tensors (the graph is then built from the plain kernels only).
FUSE_BATCHNORM = True
# Test switch: False builds score3_conv in the direct form (BilinearConcat + tap-expanded Conv) instead of
# BilinearConcatConv.
COMMUTE_RESIZE_CONV = True
# A/B switch (bf16 tensors): BatchNorm outputs read by multi-tap convolutions are materialised instead of being applied in
# the loaders ("auto" BatchNorms: inceptionv3 towers; the residual units set theirs in symbol/resnet.py)
MATERIALISE_MULTITAP_INPUT_BF16 = os.environ.get("DSPN_MAT3X3", "1") != "0"


_SHARED_STREAMS = {}


def shared_stream(device, kind, priority=0):
    """ONE stream per (device, purpose) for the whole process -- the step stream of the solvers, the side streams of the
    detection branch / MultiBoxTarget / MultiBoxDetection.  Round 4, measured: with a fresh set of streams per graph, the
    SECOND graph of a process ran its convolutions 25 % slower (fp32 MFMA mode: 57.5 -> 79.0 ms per step, conv kernel time 52.9
    -> 65.9 ms): HIP multiplexes streams onto a few hardware queues, and a main stream that lands on the queue of a side
    stream waits behind its long one-workgroup-per-sample kernels.  Graphs of one process run one at a time; sharing the
    streams keeps the mapping of the first graph."""
    key = (str(device), kind)
    ent = _SHARED_STREAMS.get(key)
    if ent is None:
        ent = _SHARED_STREAMS[key] = (torch.cuda.Stream(device=device, priority=priority), priority)
    assert ent[1] == priority, "shared stream %r of %s was created with priority %d, asked for %d" % (kind, device, ent[1], priority)
    return ent[0]


def join_forked_streams(device):
    """A graph recording abandoned half way (an exception): the current, capturing stream waits for every shared stream the
    recording forked and has not joined again, so that the recording can end (it cannot while a forked stream is unjoined)."""
    cur = torch.cuda.current_stream(device)
    for (dev, _), (s, _) in _SHARED_STREAMS.items():
        if dev != str(device) or s == cur:
            continue
        with torch.cuda.stream(s):
            forked = torch.cuda.is_current_stream_capturing()
        if forked:
            cur.wait_stream(s)


# Round 6: weight gradients on a stream of their own (WGRAD_SIDE below).  A weight gradient READS its layer's output gradient;
# the only writers of that buffer later in the same backward pass are ACCUMULATIONS through an alias (the residual stream:
# conv3's output gradient is handed to the unit's input, whose first BatchNorm adds its own gradient in place).  Every
# accumulating writer gets its target from Tensor.grad_target() / give_grad(): they make the current stream wait for the
# weight gradient that still reads the buffer.
class WgradSide:
    """What the weight gradients beside the chain carry from one call to the next, for ONE graph (Graph.wg)."""

    def __init__(self, device):
        self.device = device
        self.stream = None        # the second stream, taken on first use (Graph.wgrad_beside)
        self.events, self.used = [], 0      # event pool; how many of them this pass has handed out
        self.last = None          # event behind the last work given to the stream in this pass
        self.reads = {}           # data_ptr of an output-gradient buffer -> event behind the weight gradient that reads it

    def event(self):
        if self.used == len(self.events):
            self.events.append(torch.cuda.Event())
        self.used += 1
        return self.events[self.used - 1]

    def before_write(self, buf):
        if self.reads and buf is not None:
            ev = self.reads.pop(buf.data_ptr(), None)
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)

    def reset(self):
        """forget the pass (joined, or abandoned: nothing is waited for)"""
        self.last, self.used = None, 0
        self.reads.clear()


class Tensor:
    """An activation: NHWC (or any) device buffer + its gradient slot.  dtype: the graph's activation storage type
    (functional.ACT_DTYPE: float32, or bfloat16 for the `*_bf16` kernels) unless given -- graph inputs, loss inputs
    and graph outputs are float32 in both.  Made by Graph.tensor only."""

    def __init__(self, g, shape, name, requires_grad=True, data=None, virtual=False, dtype=None):
        self.name = name
        self.shape = tuple(int(s) for s in shape)
        self.requires_grad = requires_grad
        self.device = device = g.device
        self._wg = g.wg
        self.dtype = data.dtype if data is not None else (dtype or fn.ACT_DTYPE)
        # virtual: never materialised (a BatchNorm output that only convolutions consume: they apply the affine in
        # their tile loaders, see BatchNorm(defer_apply=True)); .data stays None so any other consumer fails loudly
        self.affine_src = None
        self.producer = None       # the Conv node that writes this tensor (it can emit BatchNorm tile statistics)
        self.bn_node = None        # the BatchNorm node that writes (or, deferred, describes) this tensor
        # "f16x2" math: index of a magnitude block that BOUNDS |values| once the producer has run in this step (a materialised
        # BatchNorm takes it while it writes the tensor; pooled / aliased tensors inherit their source's -- a bound that is too
        # large by less than 2^17 costs the two-piece math nothing), and the tensor whose values this one shares (BlockGrad)
        self.am_slot = None
        self.alias_of = None
        self.grad_planes = False   # this backward pass: .grad holds fp16 piece planes, not floats (BatchNorm.dx_planes)
        self.sc_compact = None     # this backward pass: the projection shortcut's share of .grad, compact (Conv._data_gradient)
        self.channels = None       # logical channel count when the last axis is padded (19 -> 20, 3 -> 4)
        self.data = None if virtual else (data if data is not None else fn.zeros(*self.shape, device=device, dtype=self.dtype))
        self.grad = None
        self._own_grad = None
        self._gw = False  # gradient written in the current backward pass

    def own_grad(self):
        if self._own_grad is None:
            self._own_grad = (torch.zeros_like(self.data) if self.data is not None
                              else fn.zeros(*self.shape, device=self.device, dtype=self.dtype))
        return self._own_grad

    def grad_target(self):
        """(buffer, accumulate) for a kernel that produces this tensor's gradient"""
        if not self._gw:
            self.grad = self.own_grad()
            self._gw = True
            return self.grad, False
        self._wg.before_write(self.grad)
        return self.grad, True

    def give_grad(self, buf):
        """hand over a finished gradient buffer (alias if first, else accumulate)"""
        if not self._gw:
            self.grad = buf
            self._gw = True
        else:
            self._wg.before_write(self.grad)
            fn.add(self.grad, buf, out=self.grad)


class Param:
    def __init__(self, name, shape, init, wd_mult=1.0):
        self.name, self.shape, self.init, self.wd_mult = name, tuple(shape), init, wd_mult
        # frozen (Graph.set_freeze: MXNet's fixed_param_names): no gradient is computed for it where that can be skipped,
        # the optimizer never writes it or its momentum, the all-reduce never carries it.  lr_mult: the symbol's __lr_mult__
        # (2.0 on the multibox head biases), honoured by MultiTaskSolver(optimizer_rules="module")
        self.fixed, self.lr_mult = False, 1.0
        self.data = self.grad = None
        self.offset = 0
        # shape of the same parameter in the reference's checkpoint: (Cout, Cin, kh, kw) for a Convolution weight,
        # (in, out, kh, kw) for a Deconvolution weight, (C,) otherwise -- without the channel padding of `shape`
        self.logical = None
        self.kind = "vec"          # "conv" | "deconv" | "vec"

    @property
    def size(self):
        return int(np.prod(self.shape))


class Wiring:
    """What a node writes and reads, recorded ONCE (Graph.add) and read by everything that plans from the graph's structure:
    the freeze rule, the passes of graph_plan, the solver's bucket owners.  A node is wired completely in its constructor."""

    def __init__(self, outputs):
        self.outputs = outputs     # the engine Tensors the node's constructor made, in creation order
        self.reads = []            # (attribute name, Tensor) of every other Tensor it holds: the name is the role (x, x_raw, residual ...)
        self.params = []           # the Params it holds

    def record(self, node):
        made = {id(t) for t in self.outputs}
        for k, v in vars(node).items():
            for t in (v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else (v,)):
                if isinstance(t, Tensor) and id(t) not in made:
                    self.reads.append((k, t))
                elif isinstance(t, Param):
                    self.params.append(t)


class Node:
    """Every node's constructor takes the graph first.  The tensors it creates are its outputs (Wiring.outputs):
    __init_subclass__ brackets the outermost constructor with the graph's tensor count."""

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        init = cls.__dict__.get("__init__")
        if init is None:
            return

        def wrapped(self, g, *args, __init=init, **kwargs):
            if "wiring" in self.__dict__:          # (a subclass constructor calling its parent's)
                return __init(self, g, *args, **kwargs)
            start = len(g.all_tensors)
            self.wiring = None
            __init(self, g, *args, **kwargs)
            self.wiring = Wiring(g.all_tensors[start:])
        wrapped.__wrapped__ = init
        cls.__init__ = wrapped

    def forward(self):
        raise NotImplementedError

    def backward(self):
        pass


class Graph:
    def __init__(self, device):
        self.device = device
        self.nodes = []
        self.params = {}
        self.param_order = []
        self.bn_names = []         # (name, channels, fix_gamma) of every BatchNorm, for checkpoint files
        self.bn_nodes = {}         # name -> BatchNorm (moving statistics: get_aux / set_aux)
        # moving statistics of the BatchNorms built into this graph (set by the builders before the first BatchNorm):
        # bn_momentum (the reference's 0.9) and bn_global (every BatchNorm normalises with its moving statistics: inference)
        self.bn_momentum, self.bn_global = 0.9, False
        # True only while the solver runs the forward of a step that updates the parameters: the moving statistics then
        # advance once (MultiTaskSolver._train_forward); a bare forward() leaves them as they are
        self.bn_track = False
        self.tensors = {}
        self.all_tensors = []
        self.pre_forward = []      # callables run at the top of forward() (joins of side-stream work)
        # round 6: weight gradients may run on a stream of their own (WGRAD_SIDE).  A solver with a gradient all-reduce clears it:
        # every bucket release would make the step's stream wait for that stream, and no N > 1 run has measured the mix
        self.wgrad_side_allowed = True
        self.wg = WgradSide(device)
        self._bn_chain = None      # batchnorm_chain(), once the graph is complete
        # round 4: nodes [first, last] whose FORWARD runs on a second stream beside the nodes behind them (the detection
        # branch -- small SSD layers, heads, packing, target matching: tens of launches of 1 - 32 workgroups -- beside the
        # segmentation decoder); the first reader of their results calls join_side().  (first, last, stream, ready, done)
        self.side_segment = None
        self.side_pending = False
        # ... and the BACKWARD of some of those nodes beside the decoder's (set_side_backward): only nodes whose gradients
        # stay inside the branch; every main-stream node of the branch waits for what the side stream has been given so far
        self.side_bwd = None
        self.on_branch_stream = False      # True while backward_node runs a node of the branch on the side stream
        self.side_fwd_events, self.side_fwd_waits = {}, {}   # graph_plan.side_sync
        self.side_plan = None      # what the builder asked for (any device) and what graph_plan.side_sync made of it
        self.slab_tables = {}      # key -> (conv nodes, device table) of deferred split-K slab reductions
        # the compact data gradient of a projection shortcut between its two calls (graph_plan.shortcut_compaction): ONE flat
        # buffer sized for the largest pair -- a pair's two calls are neighbours on the step's stream, so only one is live
        self.sc_compact_buf = None
        self.bn1_recompute_calls = 0   # apply passes run inside a recomputed data gradient so far (BatchNorm._apply)
        self.wt_table = None       # descriptor table of every Conv's (weight, transposed weight) pair
        self.wt_batched = False    # True while backward() runs after one batched transpose launch
        self.arena = self.grad_arena = self.mom_arena = None
        self.half_operands = False  # bf16 convolution operands: refreshed from the float masters at the top of forward()
        # math of the float-tensor convolutions of THIS graph (include/dspn_nn.h DSPN_MATH_*), fixed when the graph is
        # created: a later functional.set_conv_math() does not change what an existing graph computes
        self.math = fn.get_conv_math()
        self.wp_table = None       # split math: descriptor table of every piece-plane weight operand (one launch per step)
        # "f16x2" math: the ledger of the step's operand magnitudes (magnitudes.py); nodes hold slot indices
        self.mag = Magnitudes(self.math)
        # round 5: the range GUARD of the "f16x2" math.  Per magnitude slot the smallest non-zero per-channel magnitude travels
        # beside the largest (the ledger's minima); a convolution one of whose operands spanned more than
        # 2^GUARD_BITS in the PREVIOUS pass runs all three of its calls in the three-piece bf16 math this step (guard_fb on the
        # node; the span of a trained net's channels moves over many steps, not within one).  DSPN_RANGE_GUARD=0 switches it off.
        self.guard = dict(enabled=os.environ.get("DSPN_RANGE_GUARD", "1") != "0", have_stats=False, risk=frozenset(),
                          calls=0, calls_total=0, at_risk_slots=0)
        # frozen parameters (set_freeze, before the first node is built): names and / or a regex matched with re.match
        self.fixed_names, self.freeze_re, self.freezing = frozenset(), None, False
        # the derived operands of FROZEN weights (transposes, bf16 copies, piece planes; magnitudes and per-row minima in the
        # ledger) have tables of their own, run once and again only after set_params / load_params (frozen_stale)
        self.wt_frozen = self.wp_frozen = None
        self.frozen_stale = False

    def set_freeze(self, fixed_param_names=None, freeze_pattern=None):
        """Freeze parameters of the nodes built from now on: every name in fixed_param_names and every name freeze_pattern
        matches (re.match, as train_multitask.py applies --freeze).  Then a node's outputs need a gradient only if one of
        its inputs does or it owns a parameter that is not frozen (MXNet's rule); without freezing nothing changes."""
        assert not self.nodes, "set_freeze() before the graph is built"
        self.fixed_names = frozenset(fixed_param_names or ())
        self.freeze_re = re.compile(freeze_pattern) if freeze_pattern else None
        self.freezing = bool(self.fixed_names) or self.freeze_re is not None

    def is_fixed(self, name):
        return name in self.fixed_names or (self.freeze_re is not None and self.freeze_re.match(name) is not None)

    @property
    def fixed_param_names(self):
        """the frozen parameters this graph materialises, sorted"""
        return sorted(p.name for p in self.param_order if p.fixed)

    # -- construction ---------------------------------------------------------
    def tensor(self, shape, name, requires_grad=True, data=None, virtual=False, dtype=None):
        t = Tensor(self, shape, name, requires_grad, data=data, virtual=virtual, dtype=dtype)
        assert name not in self.tensors, "duplicate tensor name " + name
        self.tensors[name] = t
        self.all_tensors.append(t)
        return t

    def param(self, name, shape, init):
        assert name not in self.params, name
        p = Param(name, shape, init)
        p.fixed = self.freezing and self.is_fixed(name)
        self.params[name] = p
        self.param_order.append(p)
        return p

    def add(self, node):
        """Records the node's wiring; while freezing, applies MXNet's gradient rule: its outputs need a gradient only if an input
        does or it owns a parameter that is not frozen.  Only ever switches a gradient off: a node nothing behind asks a
        gradient of never runs its backward (Tensor._gw stays False), so a frozen prefix leaves backward altogether."""
        self.nodes.append(node)
        w = node.wiring
        w.record(node)
        if self.freezing and all(p.fixed for p in w.params) and not any(t.requires_grad for _, t in w.reads):
            for t in w.outputs:
                t.requires_grad = False
        return node

    @property
    def scalars(self):
        """the magnitude arena of the "f16x2" math; None in the other math modes and on CPU graphs"""
        return self.mag.arena

    def range_report(self):
        """"f16x2" math, after a step (one device -> host copy): (tensors seen, tensors whose channel magnitudes span more than
        2^16, largest span in bits) over the convolution inputs whose BatchNorm finalize saw per-channel extremes.  The
        two-piece math keeps fp32 relative accuracy for elements within 2^17 of their tensor's largest magnitude; channels
        further below keep an absolute error of 2^-39 of that magnitude (include/dspn_nn.h)."""
        return self.mag.range_report()

    GUARD_BITS = 16
    GUARD_PERIOD = 4

    def slot_spans(self):
        """the ledger's spans (largest, smallest non-zero per-channel magnitude per slot) as numpy arrays (synchronises);
        nan / inf where a slot has no per-channel information"""
        both = self.mag.spans_device().cpu().numpy()
        return both[0], both[1]

    def _update_guard(self, blocking=False):
        """Called at the top of forward(), before the magnitude arena is zeroed: which convolutions run their calls of THIS
        pass in the three-piece math.  The spans of the pass issued last are copied to pinned host memory behind it (no
        synchronisation); the decisions are taken from the copy made one pass EARLIER, which has long arrived -- the host
        runs ahead of the device and must not wait for it, and taking a fixed lag (not "whatever has arrived") keeps a run
        reproducible.  blocking=True (MultiTaskSolver's calibration pass, tests): decide from the pass issued last.
        A forward() that is being RECORDED into a HIP graph cannot look at the device: it keeps the decisions it is recorded
        with and takes the weights' minima every step; MultiTaskSolver polls guard_poll() between replays instead."""
        gd = self.guard
        gd["calls"] = 0
        capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if capturing:
            gd["wmin_now"] = True      # (the recorded launch sequence is the same every step: the minima are part of it)
            return
        gd["count"] = gd.get("count", 0) + 1
        # the weights' per-channel minima cost a launch over every weight: taken in the pass BEFORE one whose spans are read
        gd["wmin_now"] = blocking or gd["count"] % self.GUARD_PERIOD == self.GUARD_PERIOD - 1 or not gd["have_stats"]
        if not gd["enabled"] or self.scalars is None or not gd["have_stats"]:
            return
        if not blocking and gd["count"] % self.GUARD_PERIOD != 0:
            return                     # spans move over many steps: looked at every GUARD_PERIOD-th pass (0.7 % of the step -> 0.2 %)
        both = self._guard_fetch(blocking)
        if both is not None:
            self._guard_decide(both)

    def _guard_fetch(self, blocking):
        """the (largest, smallest) magnitudes per slot of the pass issued last: read now (blocking), or -- without waiting for
        the device -- the copy requested one call EARLIER (None while there is none)"""
        gd = self.guard
        if blocking:
            gd["queue"] = []
            return self.mag.spans_device().cpu().numpy()
        pool = gd.setdefault("pinned", [torch.empty((2, self.mag.slots), dtype=torch.float32, pin_memory=True)
                                        for _ in range(3)])       # (at most two copies are in flight)
        host = pool[gd.get("pin_i", 0) % 3]
        gd["pin_i"] = gd.get("pin_i", 0) + 1
        host.copy_(self.mag.spans_device(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        gd.setdefault("queue", []).append((host, ev))
        if len(gd["queue"]) < 2:
            return None
        host, ev = gd["queue"].pop(0)
        ev.synchronize()
        return host.numpy()

    def _guard_decide(self, both):
        """-> True when the set of convolutions on the fallback changed"""
        gd = self.guard
        mx, mn = both[0], both[1]
        ok = np.isfinite(mn) & (mn > 0) & (mx > 0)
        wide = np.zeros(mx.shape, bool)
        wide[ok] = np.log2(mx[ok] / mn[ok]) > self.GUARD_BITS
        gd["at_risk_slots"] = int(wide.sum())
        risk = set()
        if wide.any():
            for n in self.nodes:
                if isinstance(n, Conv) and n.am_x is not None and not n.tap_expand:
                    if wide[n.am_x] or wide[n.am_w] or wide[n.am_dy]:
                        risk.add(id(n))
        if risk == gd["risk"]:
            return False
        gd["risk"] = frozenset(risk)
        for n in self.nodes:
            if isinstance(n, Conv):
                n.guard_fb = id(n) in risk
        return True

    def guard_poll(self, blocking=False):
        """The guard of a RECORDED step (MultiTaskSolver.capture; advisor r5): called between two replays, on the stream they
        run on.  Copies the spans of the replayed pass out behind it and decides from the copy of the previous poll
        (blocking=True: from this pass).  -> True when the set of convolutions on the fallback changed: the recorded launch
        sequence no longer is the step, the caller drops the graph and records a new one."""
        gd = self.guard
        if not gd["enabled"] or self.scalars is None or not gd["have_stats"]:
            return False
        both = self._guard_fetch(blocking)
        return both is not None and self._guard_decide(both)

    def guard_report(self):
        """(convolutions on the fallback this pass, fallback kernel calls this pass, slots whose span exceeded 2^GUARD_BITS last pass)"""
        return len(self.guard["risk"]), self.guard["calls"], self.guard["at_risk_slots"]

    def guard_count_call(self):
        """a convolution call of this pass ran on the guard's fallback"""
        self.guard["calls"] += 1
        self.guard["calls_total"] += 1

    def finalize(self, seed=0):
        """allocate the flat parameter / gradient / momentum arenas and initialise"""
        graph_plan.plan(self)
        self._wt_pairs_nodes = [n for n in self.nodes if isinstance(n, Conv) and (n.wt is not None or n.wh is not None)]
        off = 0
        for p in self.param_order:
            p.offset = off
            off += (p.size + 3) // 4 * 4
        self.arena = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.grad_arena = torch.zeros_like(self.arena)
        self.mom_arena = torch.zeros_like(self.arena)
        rng = np.random.Generator(np.random.PCG64(seed))
        host = np.zeros(off, np.float32)
        for p in self.param_order:
            host[p.offset:p.offset + p.size] = np.asarray(p.init(rng, p.shape), np.float32).reshape(-1)
        self.arena.copy_(torch.from_numpy(host))
        for p in self.param_order:
            p.data = self.arena[p.offset:p.offset + p.size].view(p.shape)
            p.grad = self.grad_arena[p.offset:p.offset + p.size].view(p.shape)
        if self._wt_pairs_nodes and self.device.type == "cuda":
            # bf16 operands: every Conv has a bf16 copy wh of its float master (forward operand); a Conv whose input
            # needs no gradient still gets a (scratch) transposed operand so that one table row serves it
            for n in self._wt_pairs_nodes:
                if n.wt is None:
                    n.wt = fn.zeros(n.w.shape[3], n.w.shape[1], n.w.shape[2], n.out.shape[3], device=self.device,
                                    dtype=n.wh.dtype)
            # split math: a data gradient that contracts over whole 32-channel blocks reads piece planes, not the float
            # transpose (Conv.__init__ allocated them); only the other layers stay in the transpose table
            pairs = [n for n in self._wt_pairs_nodes if n.wtp is None or n.wh is not None]
            for frozen in (False, True):
                rows = [(n.w.data, n.wt, n.wh) for n in pairs if n.w.fixed == frozen]
                if rows:
                    tab = fn.weight_transpose_table(rows, self.device)
                    setattr(self, "wt_frozen" if frozen else "wt_table", tab)
                    self.half_operands = tab[3]
        if self.device.type == "cuda":
            wnodes = [n for n in self.nodes if getattr(n, "am_w", None) is not None and getattr(n, "w", None) is not None]
            self.mag.allocate(self.device, wnodes, minima=self.guard["enabled"])
            convs = [n for n in self.nodes if isinstance(n, Conv) and (n.wp is not None or n.wtp is not None)]
            for frozen in (False, True):
                planes = [(n.w.data, n.wp, n.wtp) + ((self.mag.block(n.am_w),) if self.math == "f16x2" else ())
                          for n in convs if n.w.fixed == frozen]
                if planes:
                    setattr(self, "wp_frozen" if frozen else "wp_table", fn.weight_planes_table(planes, self.device))
            self.frozen_stale = any(t is not None for t in (self.wt_frozen, self.wp_frozen, self.mag.am_frozen))
        if self.device.type == "cuda":
            # every Conv keeps the split-K partial sums of its weight gradient in a buffer of its own, so that the
            # slab sums of many layers run as one launch (flush_slabs) instead of one small kernel per layer
            for n in self.nodes:
                if isinstance(n, Conv):
                    n.alloc_slabs()
        return self

    def flush_slabs(self, key="all", convs=None, beside=False):
        """sum the pending split-K slabs of `convs` (default: every Conv) into their weight gradients, one launch.
        beside (the weight gradients run on a stream of their own, WGRAD_SIDE): the sum goes to THAT stream, behind the weight
        gradients it reads and behind what the current stream has issued; the current stream does not wait (join_side_backward
        does, at the end of the pass)"""
        nodes, table = self._slab_table(key, convs if convs is not None else self.nodes)
        wg = self.wg
        beside = beside and wg.last is not None
        if not beside:
            self.wgrad_beside_join()      # (before a bucket's gradients leave: its weight gradients on the second stream have finished)
        if not nodes:
            return
        ran = [n for n in nodes if n.slabs_fresh]
        if ran:
            # (some convolution had no output gradient in this pass: reduce only the ones that ran, from a table of their own)
            args = table if len(ran) == len(nodes) else self._slab_table(frozenset(map(id, ran)), ran)[1]
            if beside:
                main, side = torch.cuda.current_stream(self.device), wg.stream
                ev = wg.event()
                ev.record(main)
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    fn.slab_reduce_batch(*args)
                    done = wg.event()
                    done.record(side)
                wg.last = done
            else:
                fn.slab_reduce_batch(*args)
        for n in nodes:
            n.slabs_fresh = False

    def _slab_table(self, key, convs):
        """(conv nodes with slabs among `convs`, device table of their slab sums), built once per key"""
        if key not in self.slab_tables:
            nodes = [n for n in convs if isinstance(n, Conv) and n.slabs is not None]
            table = fn.slab_reduce_table([(n.slabs, n.w.grad, False) for n in nodes], self.device) if nodes else None
            self.slab_tables[key] = (nodes, table)
        return self.slab_tables[key]

    def load_params(self, values):
        """values: name -> numpy array in the param's (device-layout) shape"""
        self.frozen_stale = self.frozen_stale or any(self.params[k].fixed for k in values)
        for k, v in values.items():
            self.params[k].data.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)).view(self.params[k].shape))

    def _node_tensors(self, n):
        """every engine Tensor a node holds (its wiring record), each with the tensors whose buffers it reads through: the raw
        input of a deferred BatchNorm (affine_src) and the source of a BlockGrad alias"""
        seen, out = set(), []

        def take(t):
            while t is not None and id(t) not in seen:
                seen.add(id(t))
                out.append(t)
                if t.affine_src is not None:
                    take(t.affine_src[0])
                t = t.alias_of

        for t in [t for _, t in n.wiring.reads] + n.wiring.outputs:
            take(t)
        return out

    # -- execution ------------------------------------------------------------
    def forward(self):
        self.wt_batched = False        # the weights may have changed since the last batched transpose
        if self.half_operands:         # bf16 copies (forward) and transposes (data gradient) of every weight, one launch
            fn.weight_transpose_batch(*self.wt_table)
            self.wt_batched = True
        if self.mag.active:            # "f16x2" math: every operand magnitude of the step starts from zero; the weights' now
            self._update_guard(blocking=self.guard.pop("decide_now", False))
            self.mag.begin_step(minima=self.guard.get("wmin_now", True))     # (frozen weights' slots: refresh_frozen)
        self.refresh_frozen()
        if self.wp_table is not None:  # split math: the piece planes of every weight (forward and data-gradient operands;
            fn.weight_planes_batch(*self.wp_table)     # "f16x2": cut relative to the magnitudes just taken)
        for f in self.pre_forward:
            f()
        seg = self.side_segment
        if seg is None:
            for n in self.nodes:
                n.forward()
            self.guard["have_stats"] = True
            return
        first, last, side, ready, done = seg
        self.join_side()
        for i, n in enumerate(self.nodes):
            if i < first or i > last:
                for src in self.side_fwd_waits.get(i, ()):     # (a tensor written inside the segment: graph_plan.side_sync)
                    torch.cuda.current_stream(self.device).wait_event(self.side_fwd_events[src])
                n.forward()
                continue
            if i == first:       # the branch reads what the main stream has produced so far
                ready.record(torch.cuda.current_stream(self.device))
                side.wait_event(ready)
            with torch.cuda.stream(side), fn.workspace_lane(1):
                n.forward()
                if i in self.side_fwd_events:
                    self.side_fwd_events[i].record(side)
                if i == last:
                    done.record(side)
                    self.side_pending = True
        self.guard["have_stats"] = True       # (forward-only use -- the Detector -- is guarded by the spans of inputs and weights)

    def refresh_frozen(self):
        """the derived operands of the frozen weights -- bf16 copies and transposes, magnitudes, per-row minima, piece planes
        (cut by those magnitudes) -- formed when they are stale: after finalize() and after set_params / load_params"""
        if not self.frozen_stale:
            return
        self.frozen_stale = False
        if self.wt_frozen is not None:
            fn.weight_transpose_batch(*self.wt_frozen)
        self.mag.refresh_frozen()
        if self.wp_frozen is not None:
            fn.weight_planes_batch(*self.wp_frozen)

    def set_side_segment(self, first, last):
        """nodes [first, last] run their forward on the branch stream.  On a CPU graph only the plan is kept (side_plan):
        tests/test_side_plan.py checks what graph_plan.side_sync derives from it for every preset without a GPU."""
        assert 0 <= first <= last < len(self.nodes)
        self.side_plan = dict(first=first, last=last, bwd=None)
        if self.device.type == "cuda":
            self.side_segment = (first, last, shared_stream(self.device, "branch", -1), torch.cuda.Event(), torch.cuda.Event())

    def set_side_backward(self, side_nodes, lo, hi, fork_after):
        """side_nodes: indices (within [lo, hi]) whose backward runs on the side stream; it starts behind the backward of
        node `fork_after` (the last producer of the branch's incoming gradients), not behind whatever the main stream was
        given after it"""
        assert self.side_plan is not None and all(lo <= i <= hi for i in side_nodes) and fork_after > hi
        self.side_plan["bwd"] = dict(side=frozenset(side_nodes), lo=lo, hi=hi, fork_after=fork_after)
        if self.side_segment is not None:
            self.side_bwd = dict(side=frozenset(side_nodes), lo=lo, hi=hi, fork_after=fork_after, fork_ev=torch.cuda.Event(),
                                 prog_ev=torch.cuda.Event(), forked=False, dirty=False, active=True)

    def backward_node(self, idx):
        """backward of node idx on the stream it belongs to (the main stream unless set_side_backward says otherwise)"""
        sb, n = self.side_bwd, self.nodes[idx]
        if sb is None or not sb["active"]:
            n.backward()
            return
        if idx in sb["side"]:
            side = self.side_segment[2]
            if not sb["forked"]:
                side.wait_event(sb["fork_ev"])
                sb["forked"] = True
            with torch.cuda.stream(side), fn.workspace_lane(1):
                self.on_branch_stream = True
                try:
                    n.backward()
                finally:
                    self.on_branch_stream = False
                sb["prog_ev"].record(side)
            sb["dirty"] = True
            return
        if sb["dirty"] and idx <= sb["hi"]:      # a main-stream node of (or below) the branch: behind everything given to the side stream
            torch.cuda.current_stream(self.device).wait_event(sb["prog_ev"])
            sb["dirty"] = False
        n.backward()
        if idx == sb["fork_after"]:
            sb["fork_ev"].record(torch.cuda.current_stream(self.device))

    # -- round 6 (WGRAD_SIDE): every weight gradient of the step's stream on a second stream, off the data-gradient chain
    def batchnorm_chain(self):
        """True for a graph whose backward pass is mostly the chain data gradient -> BatchNorm finalize -> apply (more than half
        of its convolutions gather a BatchNorm's backward sums): there a weight gradient beside the chain fills gaps (resnet-50);
        without BatchNorm the chain is as MFMA-bound as the weight gradients and sharing the chip costs (vgg16_reduced)"""
        if self._bn_chain is None:
            convs = [n for n in self.nodes if isinstance(n, Conv)]
            self._bn_chain = 2 * sum(1 for n in convs if n.bn_bwd_node is not None) > len(convs)
        return self._bn_chain

    def wgrad_beside(self, conv, dy, planes, xa, dya):
        """-> False, nothing launched, for a node of the branch stream or a tap-expanded one (backward_route.conv_route asks for
        neither)"""
        main = torch.cuda.current_stream(self.device)
        if main == shared_stream(self.device, "branch", -1) or conv.tap_expand:
            return False
        wg = self.wg
        if wg.stream is None:
            # the stream MultiBoxTarget uses in the forward pass, idle during backward.  (On the detection branch's stream, behind
            # that branch's own backward: +0.9 % instead of +1.9 %; a fifth stream of its own: the same +1.9 %; stream priorities
            # make no measurable difference: profiles/r06_stream_priority_ab.txt.)
            wg.stream = shared_stream(self.device, "target")
        ready, done = wg.event(), wg.event()
        ready.record(main)
        wg.stream.wait_event(ready)
        with torch.cuda.stream(wg.stream), fn.workspace_lane(2):
            conv._weight_gradient(dy, planes, xa, dya)
            done.record(wg.stream)
        wg.reads[dy.data_ptr()] = done
        wg.last = done
        return True

    def wgrad_beside_join(self, final=False):
        wg = self.wg
        if wg.last is not None:
            torch.cuda.current_stream(self.device).wait_event(wg.last)
            wg.last = None
        if final:
            wg.reset()

    def join_side_backward(self):
        self.wgrad_beside_join(final=True)
        sb = self.side_bwd
        if sb is not None and sb["dirty"]:
            torch.cuda.current_stream(self.device).wait_event(sb["prog_ev"])
            sb["dirty"] = False

    def side_backward_busy(self, idx):
        """True while gradients of the branch may still be in flight on the side stream (the solver holds its slab reductions)"""
        sb = self.side_bwd
        return sb is not None and sb["active"] and sb["dirty"] and idx >= sb["lo"]

    def join_side(self):
        """order the current stream behind the side segment's forward (idempotent; called by the first reader of its results)"""
        if self.side_pending:
            torch.cuda.current_stream(self.device).wait_event(self.side_segment[4])
            self.side_pending = False

    def begin_backward(self):
        """reset the gradient bookkeeping; all data-gradient operands (transposed weights) in one launch"""
        for t in self.all_tensors:
            t._gw = False
            t.grad = None
            t.grad_planes = False
            t.sc_compact = None
        if self.side_bwd is not None:
            assert not self.side_bwd["dirty"], "the previous backward pass left side-stream work unjoined"
            self.side_bwd["forked"] = False
        self.guard["have_stats"] = True      # (the spans of a whole pass -- inputs, weights, gradients -- exist once this one has run)
        self.mag.begin_backward()
        if self.half_operands:
            return                     # prepared by forward(); the weights have not changed since
        self.wt_batched = self.wt_table is not None
        if self.wt_batched:
            fn.weight_transpose_batch(*self.wt_table)

    def abandon_backward(self):
        """Drop what a backward pass that will not be finished (a failed graph recording) carries to the next one, waiting on
        nothing: the side streams' events, the BatchNorm backwards parked between their two halves, and their finalize jobs
        still parked in the library."""
        self.wg.reset()
        self.side_pending = False
        if self.side_bwd is not None:
            self.side_bwd["dirty"] = self.side_bwd["forked"] = False
        streams = set()
        for n in self.nodes:
            if isinstance(n, BatchNorm):
                streams.update(n.hand.parked_streams())
                n.hand.clear()
        for s in streams:      # (a job no apply half has run belongs to a node that is still pending)
            fn.bn_discard_parked(s)

    def backward(self):
        self.begin_backward()
        for idx in range(len(self.nodes) - 1, -1, -1):
            self.backward_node(idx)
        self.join_side_backward()
        self.flush_slabs()

    def num_params(self):
        return sum(p.size for p in self.param_order)

    # -- checkpoint exchange in the reference's shapes (mx.model.load_checkpoint -> arg_params) ----------------
    def set_params(self, arg_params, allow_missing=False, allow_extra=True):
        """arg_params: name -> numpy array in the reference's shape (Convolution weight (Cout, Cin, kh, kw),
        Deconvolution weight (in, out, kh, kw), vectors (C,)).  Converted to the device layout ([Cout][kh][kw][Cin
        padded to the input tensor's physical channels], pad channels zero) and copied into the arena.
        Shape mismatches raise; names the graph has no parameter for (the `*_gamma` of fix_gamma BatchNorms, the moving
        statistics, ...) are ignored unless allow_extra=False; graph parameters without a value keep their
        current contents if allow_missing else raise (Module.set_params semantics)."""
        missing = [p.name for p in self.param_order if p.name not in arg_params]
        if missing and not allow_missing:
            raise KeyError("set_params: no value for " + ", ".join(missing[:8]) + (" ..." if len(missing) > 8 else ""))
        extra = [k for k in arg_params if k not in self.params]
        if extra and not allow_extra:
            raise KeyError("set_params: graph has no parameter " + ", ".join(extra[:8]))
        for p in self.param_order:
            if p.name not in arg_params:
                continue
            v = np.asarray(arg_params[p.name], np.float32)
            logical = tuple(p.logical or p.shape)
            if tuple(v.shape) != logical:
                raise ValueError("set_params: %s has shape %s, the graph expects %s" % (p.name, tuple(v.shape), logical))
            dev = np.zeros(p.shape, np.float32)
            if p.kind == "raw":                                   # same values, only the shape differs ((1,6) <-> (6,))
                dev[:] = v.reshape(p.shape)
            elif p.kind in ("conv", "deconv"):
                t = v.transpose(0, 2, 3, 1)                       # -> [rows][kh][kw][cols]
                dev[:t.shape[0], :, :, :t.shape[3]] = t
            else:
                if v.shape[0] < p.shape[0]:                       # padded vector: keep the pad lanes as they are
                    dev[:] = p.data.detach().cpu().numpy()
                dev[:v.shape[0]] = v
            p.data.copy_(torch.from_numpy(dev))
            self.frozen_stale = self.frozen_stale or p.fixed

    def set_global_stats(self, names_or_pattern):
        """Switch BatchNorm nodes to their moving statistics -- mx.sym.BatchNorm(use_global_stats=True):
        the forward normalises with moving_mean / moving_var and leaves them alone, the backward treats them as constants.
        names_or_pattern: a regular expression matched (re.match) against the BatchNorm names of bn_nodes, or an iterable of
        names.  Before finalize().  -> the names switched, in graph order; a pattern or name without a BatchNorm raises"""
        if self.arena is not None:
            raise RuntimeError("set_global_stats: call it before finalize()")
        if isinstance(names_or_pattern, str):
            rx = re.compile(names_or_pattern)
            names = [n for n in self.bn_nodes if rx.match(n)]
            if not names:
                raise ValueError("set_global_stats: pattern %r matches no BatchNorm" % names_or_pattern)
        else:
            names = list(names_or_pattern)
            unknown = [n for n in names if n not in self.bn_nodes]
            if unknown:
                raise ValueError("set_global_stats: no BatchNorm named " + ", ".join(unknown[:8]))
        for n in names:
            self.bn_nodes[n].use_global_stats = True
        return names

    def get_aux(self):
        """-> the moving statistics in the reference's aux-state names and shapes: '<bn>_moving_mean' / '<bn>_moving_var'
        -> (channels,) float32 numpy arrays, pad channels dropped"""
        out = {}
        for name, channels, _ in self.bn_names:
            n = self.bn_nodes[name]
            out[name + "_moving_mean"] = n.moving_mean[:channels].detach().cpu().numpy().copy()
            out[name + "_moving_var"] = n.moving_var[:channels].detach().cpu().numpy().copy()
        return out

    def set_aux(self, aux_params, allow_missing=False):
        """copy aux states ('<bn>_moving_mean' / '<bn>_moving_var', shapes (channels,)) INTO the existing moving-statistics
        buffers (a recorded step keeps valid pointers); pad lanes keep 0 / 1.  Names the graph has no BatchNorm for are
        ignored; a BatchNorm without a value keeps its statistics if allow_missing else raises"""
        wanted = [name + suffix for name, _, _ in self.bn_names for suffix in ("_moving_mean", "_moving_var")]
        missing = [k for k in wanted if k not in aux_params]
        if missing and not allow_missing:
            raise KeyError("set_aux: no value for " + ", ".join(missing[:8]) + (" ..." if len(missing) > 8 else ""))
        for name, channels, _ in self.bn_names:
            n = self.bn_nodes[name]
            for suffix, buf in (("_moving_mean", n.moving_mean), ("_moving_var", n.moving_var)):
                if name + suffix not in aux_params:
                    continue
                v = np.asarray(aux_params[name + suffix], np.float32).reshape(-1)
                if v.shape[0] != channels:
                    raise ValueError("set_aux: %s%s has %d values, the graph expects %d" % (name, suffix, v.shape[0], channels))
                buf[:channels].copy_(torch.from_numpy(v))

    def get_params(self):
        """-> name -> numpy array in the reference's shapes (inverse of set_params; pad channels dropped)"""
        out = {}
        for p in self.param_order:
            v = p.data.detach().cpu().numpy()
            logical = tuple(p.logical or p.shape)
            if p.kind == "raw":
                v = v.reshape(logical)
            elif p.kind in ("conv", "deconv"):
                v = v[:logical[0], :, :, :logical[1]].transpose(0, 3, 1, 2)
            else:
                v = v[:logical[0]]
            out[p.name] = np.ascontiguousarray(v)
        return out


# ------------------------------------------------------------------ initialisers
def init_zeros(rng, shape):
    return np.zeros(shape, np.float32)


def init_ones(rng, shape):
    return np.ones(shape, np.float32)


def conv_weight_init(kind, cin_logical):
    """"maxdim": multi_init.py:74-76, U(+-1/sqrt(max(shape))) on the MXNet shape (Cout, Cin, kh, kw); "xavier":
    mx.init.Xavier(uniform, avg, magnitude 3).  Device layout (Cout, kh, kw, Cin_phys); pad channels stay 0."""
    def f(rng, shape):
        cout, r, s, cin_p = shape
        w = np.zeros(shape, np.float32)
        if kind == "maxdim":
            lim = 1.0 / math.sqrt(max(cout, cin_logical, r, s))
        else:  # "xavier": mx.init.Xavier(uniform, avg, magnitude 3) (train/train_multitask.py:313)
            fan_in, fan_out = cin_logical * r * s, cout * r * s
            lim = math.sqrt(3.0 / ((fan_in + fan_out) / 2.0))
        w[..., :cin_logical] = rng.uniform(-lim, lim, size=(cout, r, s, cin_logical))
        return w
    return f


def deconv_bilinear_init(channels):
    """multi_init.py:160-168 + upsample_filt: a diagonal bilinear kernel.  Device layout of the
    Deconvolution weight is [K = in channel][R][S][C = out channel] (phys channels)."""
    def f(rng, shape):
        k_p, r, s, c_p = shape
        factor = (r + 1) // 2
        center = factor - 1 if r % 2 == 1 else factor - 0.5
        og = np.ogrid[:r, :s]
        filt = (1 - abs(og[0] - center) / factor) * (1 - abs(og[1] - center) / factor)
        w = np.zeros(shape, np.float32)
        for i in range(channels):
            w[i, :, :, i] = filt
        return w
    return f


def init_affine_identity(rng, shape):
    """multi_init.py:72: affine_matrix = [[1, 0, 0, 0, 1, 0]]"""
    return np.array([1, 0, 0, 0, 1, 0], np.float32)


def affine_matrix_param(g, name="affine_matrix"):
    """mx.sym.var("affine_matrix", shape=(1,6)) (multitask_symbol_builder.py:574): an ordinary argument -- it gets
    a gradient through GridGenerator / BilinearSampler and the optimizer updates it (multi_solver.py:205-208,
    291-293), weight decay included.  Device shape (6,), checkpoint shape (1, 6)."""
    p = g.param(name, (6,), init_affine_identity)
    p.logical, p.kind = (1, 6), "raw"
    return p


# ------------------------------------------------------------------ nodes
class InputNCHW(Node):
    """data (B,3,H,W) -> NHWC with channels padded to 4 (symbol/resnet.py:89 `data`)"""

    def __init__(self, g, src, name="data_nhwc"):
        self.src = src
        N, C, H, W = src.shape
        self.out = g.tensor((N, H, W, fn.padc(C)), name, requires_grad=False)
        self.out.channels = C

    def forward(self):
        fn.nchw_to_nhwc(self.src.data, out=self.out.data)


# graph_plan.input_planes: a deferred BatchNorm output is ALSO written as piece planes when its readers would otherwise apply
# the affine to each element at least this many times (taps x 128-column tiles, summed over the readers)
FUSE_MAXPOOL_BACKWARD = os.environ.get("DSPN_FUSE_POOL_BWD", "1") != "0"      # (A/B switch)
X_PLANES_MIN_READS = int(os.environ.get("DSPN_X_PLANES_MIN_READS", "6"))


class BackwardHandoff:
    """The per-pass state between nodes: what a BatchNorm is left by other nodes, or by its own first half, during ONE backward
    pass.  Each field is taken (reset) by the step that uses it; clear() drops a pass that will not be finished."""
    __slots__ = ("sums_ready", "pooled", "parked", "recompute")

    def __init__(self):
        self.clear()

    def clear(self):
        self.sums_ready = False    # the data gradient of Conv.bn_bwd_node's convolution has gathered BatchNorm.bwd_sums
        self.pooled = None         # (argmax, pooled gradient, k, stride, pad) left by a MaxPool that folds this node
        # round 6: the finalize half is parked for / rode in the weight gradient of the convolution whose data gradient gathered
        # the sums: (args, kwargs, stream handle) of the apply half.  The coefficients wait in BatchNorm.bwd_ws, which no
        # other node writes
        self.parked = None
        # that data gradient stored no gradient for this node (backward_route.SUMS_ONLY): (conv, dy, planes, dy magnitude,
        # weight magnitude) of the apply pass that forms it again
        self.recompute = None

    def parked_streams(self):
        return () if self.parked is None else (self.parked[2],)


class BatchNorm(Node):
    """mx.sym.BatchNorm with batch statistics (the solver always runs is_train=True,
    multi_solver.py:284) optionally fused with the following ReLU.

    Moving statistics (MXNet's aux states): moving_mean / moving_var (C device floats, 0 / 1 at creation, pad lanes stay
    so) advance with `momentum` in the statistics finalize of a forward that the solver runs for a parameter update
    (Graph.bn_track); with Graph.bn_global the node normalises with them instead of the batch's (use_global_stats: the
    finalize folds them into scale / shift, no statistics pass).  include/dspn_nn.h dspn_bn_moving.
    A use_global_stats node of a TRAINING graph (Graph.set_global_stats, the training builders'
    global_stats_pattern) keeps its moving statistics through a step and runs the fixed-statistics backward:
    dx = gamma rstd dy', dgamma / dbeta the usual sums against the moving statistics."""

    def __init__(self, g, x, name, fix_gamma=False, eps=2e-5, relu=False, beta_grad_from_consumer=False,
                 defer_apply=False):
        """defer_apply: the output is only consumed by convolutions, which apply scale/shift(+ReLU) to x in their
        tile loaders (dspn_conv2d_forward_bn_f32 / dspn_conv2d_wgrad_bn_f32): forward is the statistics pass alone and
        the normalised tensor is never written"""
        C = x.shape[-1]
        if not FUSE_BATCHNORM:
            defer_apply = False
        self.x, self.eps, self.relu = x, eps, relu
        self.gamma = None if fix_gamma else g.param(name + "_gamma", (C,), init_ones)
        self.beta = g.param(name + "_beta", (C,), init_zeros)
        for p in (self.gamma, self.beta):
            if p is not None:
                p.logical = (x.channels or C,)
        g.bn_names.append((name, x.channels or C, bool(fix_gamma)))   # gamma / moving_* entries of a checkpoint
        g.bn_nodes[name] = self
        self.channels = x.channels or C
        self.momentum, self.use_global_stats = float(g.bn_momentum), bool(g.bn_global)
        self.moving_mean = torch.zeros(C, dtype=torch.float32, device=g.device)
        self.moving_var = torch.ones(C, dtype=torch.float32, device=g.device)
        self.mean = fn.zeros(C, device=g.device)
        self.rstd = fn.zeros(C, device=g.device)
        self.scale = fn.zeros(C, device=g.device)
        self.shift = fn.zeros(C, device=g.device)
        # an input BN whose data has no gradient only needs sum(dy) for beta: its consumer supplies it
        self.defer_apply = defer_apply
        # statistics gathered by the producing convolution's epilogue (one (mean, M2) pair per row tile) instead of a
        # separate pass over x
        self.tile_stats = (x.producer.enable_out_stats()
                           if FUSE_BATCHNORM and x.producer is not None else None)
        self.out = g.tensor(x.shape, name + ("_relu" if relu else "_out"), requires_grad=not beta_grad_from_consumer,
                            virtual=bool(defer_apply))
        if defer_apply:
            self.out.affine_src = (x, self.scale, self.shift, relu)
        self.out.bn_node = self
        # "f16x2" math: a MATERIALISED output leaves its magnitude as a by-product of the apply kernel
        self.am_out = g.mag.new() if (g.math == "f16x2" and self.out.dtype == torch.float32) else None
        self.out.am_slot = self.am_out
        self.conv_consumers = []     # convolutions reading self.out (deferred apply), in forward order
        self.mat_consumers = []      # plain convolutions reading a MATERIALISED self.out (their last data gradient can
                                     # still gather this BatchNorm's backward reductions in its epilogue)
        self.bwd_sums = None         # (buffer, tiles) written by the LAST data gradient into self.out.grad
        self.bwd_ws = None           # with bwd_sums: this node's workspace of the backward from them (coefficients, grouped tiles)
        # round 4 (graph_plan.gradient_planes): dx leaves as fp16 piece planes; x_ext = per-channel extremes of x from the
        # forward finalize, am_dyin = slot of the magnitude of this node's own output gradient (from the data gradient's epilogue)
        self.dx_planes, self.x_ext, self.am_dyin = False, None, None
        # round 4 (graph_plan.input_planes): the output as fp16 piece planes for the multi-tap convolutions behind a DEFERRED
        # apply; planes_ready: written by this step's forward (the magnitude they are cut by came out of the finalize)
        self.planes, self.planes_ready = None, False
        self.hand = BackwardHandoff()      # what other nodes, or this node's first half, leave here during a backward pass
        self._g = g
        # True when this node's backward is the LAST writer of x's gradient (set by Graph.finalize): only then is the dx it
        # stores the complete gradient whose magnitude the producing convolution may use
        self.completes_x_grad = False

    def _moving(self):
        """the dspn_bn_moving block of this forward's finalize, or None (batch statistics, nothing tracked)"""
        if self.use_global_stats:
            mode = fn.BN_GLOBAL
        elif self._g.bn_track:
            mode = fn.BN_TRACK
        else:
            return None
        return fn.bn_moving(self.moving_mean, self.moving_var, self.momentum, mode, self.channels)

    def forward(self):
        moving = self._moving()
        if self.tile_stats is not None:
            buf, tiles, tile_rows = self.tile_stats
            rows = int(np.prod(self.x.shape[:-1]))
            # "f16x2" math: the convolutions that fold this BatchNorm into their loaders multiply (relu)(x * scale + shift);
            # its magnitude comes out of this finalize kernel, from the extremes the producer wrote beside the statistics
            mag, mm = self._g.mag, getattr(self.x.producer, "out_minmax", None)
            slot = mag.input_slot(self.x, self.scale, create=False) if mm is not None else None
            am = mag.claim(slot)
            fn.bn_stats_from_tiles(buf, tiles, tile_rows, rows, self.x.shape[-1], self.eps,
                                   None if self.gamma is None else self.gamma.data, self.beta.data,
                                   self.mean, self.rstd, self.scale, self.shift,
                                   tile_minmax=mm if am is not None else None, relu=self.relu, out_absmax=am,
                                   out_absmin=None if am is None else mag.min_view(slot),
                                   out_chan_minmax=self.x_ext if am is not None else None, moving=moving)
            self.planes_ready = self.planes is not None and am is not None
            if self.planes_ready:
                fn.bn_apply_planes(self.x.data, self.scale, self.shift, am, relu=self.relu, out=self.planes)
        else:
            fn.bn_stats(self.x.data, self.eps, None if self.gamma is None else self.gamma.data, self.beta.data,
                        self.mean, self.rstd, self.scale, self.shift, moving=moving)
        if not self.defer_apply:
            fn.bn_apply(self.x.data, self.scale, self.shift, relu=self.relu, out=self.out.data,
                        out_absmax=self._g.mag.claim(self.am_out))

    def _x_ext_valid(self):
        """the per-channel extremes of x were written by this step's forward finalize (the magnitude slot they come with is done)"""
        mag = self._g.mag
        return mag.done(mag.input_slot(self.x, self.scale, create=False))

    def _dx_magnitude_slot(self):
        """"f16x2" math: dx is the output gradient of the convolution that produced x; where this node's backward completes it (it
        alone reads x, or x is the residual stream and it writes last), the apply kernel leaves its magnitude: that slot, or None"""
        prod, wanted = self.x.producer, self.x.requires_grad and self.completes_x_grad and self._g.mag.active
        return prod.am_dy if (wanted and isinstance(prod, Conv) and self.x.dtype == torch.float32) else None

    def _facts(self, beside):
        hand = self.hand
        return R.BnFacts(beside=beside, x_requires_grad=self.x.requires_grad, dx_planes=self.dx_planes,
                         cuda=self._g.device.type == "cuda", finalize_beside=bool(FINALIZE_BESIDE), out_written=self.out._gw,
                         x_written=self.x._gw, takes_magnitude=self._dx_magnitude_slot() is not None,
                         x_ext_valid=self.dx_planes and self._x_ext_valid(),
                         producer_guard_fb=bool(getattr(self.x.producer, "guard_fb", False)), sums_ready=hand.sums_ready,
                         pooled=hand.pooled is not None, parked=hand.parked is not None, recompute=hand.recompute is not None)

    def finalize_beside(self):
        """Round 6: called by the convolution whose data gradient has just gathered this node's backward
        sums in its epilogue, BEFORE it launches its weight gradient.  The finalize half of dspn_bn_backward_from_sums (one or
        two launches on 1 - 64 workgroups, 6 - 15 us of an otherwise idle chip) is PARKED in the library and rides in front of
        that weight gradient's grid (csrc/bn_final_job.h); backward() later launches the apply half.  (On a second stream
        instead -- two events per node -- the step LOST 1.5 %: profiles/r06_finalize_beside_ab.txt.)  -> True if it did."""
        route = R.bn_route(self._facts(beside=True))
        self._run(route)
        return route.finalize == R.PARKED

    def backward(self):
        self._run(R.bn_route(self._facts(beside=False)))

    def _run(self, route):
        hand, g = self.hand, self._g
        if route.kind == R.NOTHING:
            return
        if route.kind == R.APPLY_PARKED:
            (args, kw, _), hand.parked = hand.parked, None
            return self._apply(route.apply, args, kw)
        # what every entry point takes.  Frozen gamma / beta: not computed (NULL to the kernels); dgamma stays None without a gamma
        # (fix_gamma).  fixed_stats (use_global_stats under training): mean / rstd are the moving statistics, dx has no term through them
        gamma = None if self.gamma is None else self.gamma.data
        out = dict(dgamma=None if self.gamma is None else (fn.NO_OUTPUT if self.gamma.fixed else self.gamma.grad),
                   dbeta=fn.NO_OUTPUT if self.beta.fixed else self.beta.grad, relu=self.relu, fixed_stats=self.use_global_stats)
        if route.writes_dx:
            dx, acc = self.x.grad_target()
            out.update(dx=dx, dx_absmax=g.mag.claim(self._dx_magnitude_slot()))
        else:  # the parameters alone: reductions and finalize, no dx (the kernels take dx == NULL)
            acc = False
            out.update(dx=fn.NO_OUTPUT, dx_absmax=None)
        if hand.pooled is not None:
            (argmax, dyp, k, s, p), hand.pooled = hand.pooled, None
            if route.kind == R.POOLED:
                fn.bn_backward_maxpool(self.x.data, self.scale, self.shift, dyp, argmax, k, s, p, self.mean, self.rstd, gamma, **out)
                return
            assert route.unpool_first      # (a second writer of x's gradient: materialise the pooling backward after all)
            fn.maxpool_backward_argmax(argmax, dyp, self.out.shape, k, s, p, dx=self.out.own_grad())
            self.out.grad = self.out.own_grad()
        if route.kind == R.STANDALONE:
            fn.bn_backward(self.x.data, self.scale, self.shift, self.out.grad, self.mean, self.rstd, gamma, accumulate=acc, **out)
            return
        # the two reductions came out of the data-gradient kernel's epilogue
        hand.sums_ready = False
        args, kw = self._from_sums_call(route.kind == R.FROM_SUMS_PLANES, gamma, acc, out)
        phase = {R.WITH_APPLY: {}, R.ALONE: dict(phase=1), R.PARKED: dict(phase=1, park=True)}[route.finalize]
        fn.bn_backward_from_sums(*args, **phase, **kw)
        if route.finalize == R.PARKED:
            hand.parked = (args, kw, fn.stream())
        elif route.finalize == R.ALONE:
            self._apply(route.apply, args, kw)
        if route.kind == R.FROM_SUMS_PLANES:
            self.x.grad_planes = True

    def _from_sums_call(self, planes, gamma, acc, out):
        """(positional arguments, keywords) of fn.bn_backward_from_sums, whichever phase: the parked finalize and the finalize in
        front of a recomputed data gradient hand the same pair to their apply half"""
        g = self._g
        args = (self.x.data, self.scale, self.shift, self.out.grad, self.mean, self.rstd, gamma, self.bwd_sums[0], self.bwd_sums[1])
        kw = dict(out, accumulate=acc, workspace=self.bwd_ws)
        if planes:      # the gradient leaves as fp16 piece planes (same buffer): dx_absmax receives the BOUND it is cut by
            assert not acc
            kw.update(dy_absmax=g.mag.block(self.am_dyin), x_chan_minmax=self.x_ext, dx_planes=True,
                      dx_absmin=g.mag.min_view(self.x.producer.am_dy) if g.guard["enabled"] else None)
        return args, kw

    def _apply(self, how, args, kw):
        """the apply half from the coefficients the finalize left in bwd_ws: the apply kernel over the stored gradient, or --
        the data gradient stored none (backward_route.SUMS_ONLY) -- that data gradient again, with the apply in its epilogue"""
        rc, self.hand.recompute = self.hand.recompute, None
        if how == R.KERNEL:
            fn.bn_backward_from_sums(*args, phase=2, **kw)
            return
        conv, dy, planes, dya, wa = rc
        fn.conv2d_dgrad_bn_apply(dy, conv.wt, self.x.data, self.scale, self.shift, self.relu, self.bwd_ws, kw["dx"],
                                 accumulate=kw["accumulate"], dx_absmax=kw["dx_absmax"], wt_planes=conv.wtp, math=conv.math,
                                 dy_absmax=dya, w_absmax=wa, dy_planes=planes, wt_shape=conv.wt_shape)
        self._g.bn1_recompute_calls += 1


# round 6: the weight gradients of the step's stream on a stream of their own (Graph.wgrad_beside): nothing on the critical
# chain data gradient -> BatchNorm finalize -> apply -> next data gradient reads them, so they run BESIDE it -- in the gaps of
# the latency-bound finalize launches and under the HBM-bound apply passes -- and the bucket's slab sums follow them there;
# the step's stream waits for that stream once, at the end of the pass (and before an accumulation into a buffer one of
# them still reads: WgradSide.before_write).  Same kernels, same bits; +1.9 % on the step (profiles/r06_wgrad_beside_ab.txt).
# DSPN_WGRAD_SIDE=0: on the step's stream, with the BatchNorm finalize riding in their launches (below).  bench.py switches
# it off for its instrumented steps: a kernel timed beside another one measures the pair, not the kernel.
WGRAD_SIDE = int(os.environ.get("DSPN_WGRAD_SIDE", "1"))
WGRAD_SIDE_MIN_US = float(os.environ.get("DSPN_WGRAD_SIDE_MIN_US", "30"))      # (Conv._wgrad_worth_a_stream)

# round 6: the finalize half of a BatchNorm backward rides in the weight-gradient launch of the layer behind it
# (DSPN_FINALIZE_BESIDE=0: launches of its own, as round 5 -- same-box A/B; the results do not depend on it)
FINALIZE_BESIDE = os.environ.get("DSPN_FINALIZE_BESIDE", "1") != "0"

# round 5: convolutions no BatchNorm reads leave the magnitude of their output (forward epilogue) and of their masked gradient
# (the ReLU-backward / bias-gradient pass) as by-products; DSPN_CONV_MAGNITUDES=0 keeps the stand-alone passes (same-box A/B)
FUSE_CONV_MAGNITUDES = os.environ.get("DSPN_CONV_MAGNITUDES", "1") != "0"

# the projection units (conv1 and the 1 x 1 / stride-2 shortcut read one BatchNorm output): the shortcut's data gradient stays a
# compact (N, H/2, W/2, C) tensor and conv1's data gradient, the only writer of the full-resolution gradient, adds it at the
# even positions (graph_plan.shortcut_compaction); DSPN_SC_COMPACT=0: the shortcut writes the full tensor -- three quarters of
# it zeros -- and conv1 accumulates (same-box A/B; same bits either way)
SC_COMPACT = os.environ.get("DSPN_SC_COMPACT", "1") != "0"

# The bn1 of the dim-match residual units reads the residual stream; the gradient of its output has one writer (conv1's data
# gradient, a 1 x 1 product over C / 4 channels) and one reader (bn1's backward).  On marked pairs (graph_plan.bn1_recompute)
# that gradient is never stored: conv1's data gradient runs for the sums alone, and again with the apply pass in its epilogue
# (include/dspn_nn.h dspn_conv2d_dgrad_bn_sums_f32 / _apply_f32) -- four passes over the M x C tensor instead of six.
# DSPN_BN1_RECOMPUTE: 0 the data gradient + apply kernel pair everywhere, 1 the layers bn1_recompute_pays() names (default),
# 2 every layer that has the route (measurements).
BN1_RECOMPUTE = int(os.environ.get("DSPN_BN1_RECOMPUTE", "1"))


def bn1_recompute_pays(M, C, K):
    """The layers that take the route by default, by shape (M rows of C channels, K = channels of the product): the ONE place
    that decides.  Measured per stage of the resnet-50 step at 32 x 512 x 512 (profiles/bn1_recompute_last_step_by_kernel.txt,
    DESIGN.md section 7; data gradient + apply kernel -> sums pass + apply pass, ms per unit): stage 1 (524288, 256, 64) 0.607 ->
    0.495, stage 2 (131072, 512, 128) 0.317 -> 0.281, stage 3 (32768, 1024, 256) 0.188 -> 0.186 (inside the 0.008 spread of its
    launches), stage 4 (8192, 2048, 512) 0.136 -> 0.143.  The route pays where the second product is short beside the two passes
    it saves (K <= 128) and the M x C tensor does not fit the 256 MiB Infinity Cache, i.e. the saved passes are HBM traffic."""
    return K <= 128 and 4 * M * C >= 256 << 20


def xa_unavailable(conv):
    """the output-magnitude epilogue needs a dense output of whole float4 rows (every Conv output of the engine is one)"""
    return conv.out.data is None or conv.out.data.shape[-1] % 4 != 0


class Conv(Node):
    """mx.sym.Convolution (+ bias) (+ ReLU epilogue); weight [Cout, R, S, Cin_phys]"""

    def __init__(self, g, x, name, num_filter, kernel, stride=1, pad=0, dilate=1, no_bias=True, relu=False,
                 init="xavier", cin_logical=None, cout_phys=None, input_sum_grad=None, residual=None, out_name=None,
                 tap_expand=False):
        N, H, W, Cin = x.shape
        kh, kw = fn._hw(kernel)
        ph, pw = fn._hw(pad)
        self.x, self.stride, self.pad, self.dil, self.relu = x, stride, (ph, pw), dilate, relu
        # input produced by a deferred BatchNorm: read the raw tensor and apply the affine in the loader
        self.x_raw, self.in_affine = x, None
        if x.affine_src is not None:
            raw, sc, sh, arelu = x.affine_src
            self.x_raw, self.in_affine = raw, (sc, sh, arelu)
            assert not tap_expand
            x.bn_node.conv_consumers.append(self)
        elif x.bn_node is not None and not tap_expand:
            x.bn_node.mat_consumers.append(self)
        self.cout = num_filter
        # Param that receives sum_pixels(dx) instead of a full data gradient (see conv2d_input_sum_grad)
        self.input_sum_grad = input_sum_grad
        cin_meta = cin_logical if cin_logical is not None else (x.channels or Cin)   # channels a checkpoint holds
        cin_logical = Cin if cin_logical is None else cin_logical
        self.w = g.param(name + "_weight", (num_filter, kh, kw, Cin), conv_weight_init(init, cin_logical))
        self.b = None if no_bias else g.param(name + "_bias", (num_filter,), init_zeros)
        self.w.logical, self.w.kind = (num_filter, cin_meta, kh, kw), "conv"
        if self.b is not None:
            self.b.logical = (num_filter,)
        Ho, Wo = fn.conv_out_size(H, kh, stride, ph, dilate), fn.conv_out_size(W, kw, stride, pw, dilate)
        ldc = fn.padc(num_filter) if cout_phys is None else cout_phys
        self.out = g.tensor((N, Ho, Wo, ldc), out_name or (name + "_out"))
        self.out.channels = num_filter
        self.out.producer = self
        self.slabs, self.slabs_fresh = None, False     # deferred split-K slab reduction (Graph.flush_slabs)
        self.out_stats = None      # (buffer, tiles, rows per tile) once a BatchNorm asked for them
        self.out_minmax = None     # "f16x2" math: (tiles, 2, Cout) smallest / largest output value per tile (with out_stats)
        self._g = g
        # residual: a tensor of the output's shape added in the conv epilogue (`conv3 + shortcut`,
        # symbol/resnet.py:51); its gradient is the output gradient itself
        self.residual = residual
        assert residual is None or residual.shape == self.out.shape
        half = self.out.dtype == torch.bfloat16
        # data-gradient operand: the transposed weight -- as piece planes (wtp, below) where the split math contracts over whole
        # 32-channel blocks, else as a tensor of the storage type (no float transpose is kept beside planes: ~100 MB on resnet-50)
        self.wt_shape = (Cin, kh, kw, ldc)
        planes_t = g.device.type == "cuda" and x.requires_grad and fn.needs_planes(self.out.dtype, ldc, g.math)
        self.wt = None if (not x.requires_grad or planes_t) else fn.zeros(Cin, kh, kw, ldc, device=g.device, dtype=self.out.dtype)
        # bf16 operands: the copy of the float master the forward pass multiplies (refreshed once per step, Graph.forward)
        self.wh = fn.zeros(num_filter, kh, kw, Cin, device=g.device, dtype=torch.bfloat16) if half else None
        # split math: piece planes of the weight (forward operand) and of its transpose (data-gradient operand), cut once
        # per step by Graph.forward for the whole graph instead of once per tile inside the kernels
        self.math = g.math
        # "f16x2" math: slots of the operand magnitudes.  Readers of one (raw tensor, affine) pair share the input's slot
        # (act1 feeds conv1 and the projection shortcut); the gradient's and the weight's belong to this node.
        self.am_x = self.am_dy = self.am_w = None
        if g.math == "f16x2" and self.out.dtype == torch.float32:
            self.am_x = g.mag.input_slot(self.x_raw, None if self.in_affine is None else self.in_affine[0])
            self.am_dy, self.am_w = g.mag.new(backward=True), g.mag.new()
        # ... and of the OUTPUT as stored, where no BatchNorm reads it (no statistics epilogue: vgg16_reduced, the SSD extra layers):
        # the convolution's own epilogue leaves it (fn.conv2d_forward out_absmax), the next convolution needs no pass over the tensor
        self.am_out = g.mag.new() if (self.am_x is not None and not tap_expand) else None
        if self.am_out is not None:
            self.out.am_slot = self.am_out       # (pooled / aliased tensors built on it inherit the slot)
        if self.am_x is not None and self.in_affine is None:
            g.mag.want(self.x_raw)        # the producer of this input leaves its magnitude if it can
        self.x_planes_bn = None      # the deferred BatchNorm that also leaves this node's input as piece planes (graph_plan.input_planes)
        self.bn_bwd_node = None      # the BatchNorm whose backward sums this node's data gradient gathers (graph_plan.bn_backward_fusion)
        self._wg_worth = None        # _wgrad_worth_a_stream, once estimated
        self.guard_fb = False        # range guard (Graph._update_guard): this pass's calls run in the three-piece bf16 math
        self.bn1_recompute = False   # its data gradient may run sums-only, and again in bn_bwd_node's backward (graph_plan.bn1_recompute)
        self.sc_pair = None          # the other convolution of a (conv1, projection shortcut) pair (graph_plan.shortcut_compaction)
        self.wp = self.wtp = None
        if g.device.type == "cuda":
            npc = fn.plane_pieces(g.math)
            if fn.needs_planes(self.out.dtype, Cin, g.math):
                self.wp = fn.zeros(num_filter, kh * kw, Cin // 32, npc, 32, device=g.device, dtype=torch.bfloat16)
            if x.requires_grad and fn.needs_planes(self.out.dtype, ldc, g.math):
                self.wtp = fn.zeros(Cin, kh * kw, ldc // 32, npc, 32, device=g.device, dtype=torch.bfloat16)
        # tap-expanded evaluation (few output channels, stride 1): 1x1 convolution to Cout*kh*kw channels
        # on the same weight buffer + shifted sum over taps (include/dspn_nn.h, dspn_tap_sum_f32)
        self.tap_expand = bool(tap_expand) and kh * kw > 1
        if self.tap_expand:
            assert stride == 1 and dilate == 1 and not relu and residual is None
            assert (Ho, Wo) == (H, W), "tap expansion needs a 'same' convolution"
            self.z = fn.act_zeros(N, H, W, fn.padc(num_filter * kh * kw), device=g.device)   # also holds dz in backward
        # algorithmic FLOPs per batch (direct-conv count, logical channels)
        self.flops_fwd = 2.0 * cin_logical * num_filter * kh * kw * Ho * Wo * N
        self.flops_bwd = self.flops_fwd * (2 if x.requires_grad else 1)

    def alloc_slabs(self):
        if self.w.fixed:
            return                 # (a frozen weight has no weight gradient)
        cout, kh, kw, cin = self.w.shape
        wshape = (cout * kh * kw, 1, 1, cin) if self.tap_expand else self.w.shape
        xs = self.x.shape
        splits = fn.conv2d_wgrad_splits(xs, self.z.shape if self.tap_expand else self.out.shape, wshape,
                                        1 if self.tap_expand else self.stride)
        if splits > 0 and self.w.data.numel() % 4 == 0:
            self.slabs = fn.zeros(splits, self.w.data.numel(), device=self._g.device)

    def wop(self):
        """the weight operand of the forward kernels: the float master, or its bf16 copy"""
        return self.w.data if self.wh is None else self.wh

    def enable_out_stats(self):
        """called by a BatchNorm on self.out: have the epilogue write per-tile statistics (None if unavailable)"""
        if self.tap_expand or self.out.shape[3] != self.cout or self.cout % 4 != 0:
            return None
        if self.out_stats is None:
            rows = self.out.shape[0] * self.out.shape[1] * self.out.shape[2]
            tiles, tile_rows = fn.conv_stats_layout(rows, self.cout)
            if tiles == 0:
                return None
            self.out_stats = (fn.zeros(tiles, 2, self.cout, device=self._g.device), tiles, tile_rows)
            if self.math == "f16x2" and self.out.dtype == torch.float32:
                # per-tile extremes of the output next to its statistics: the magnitude of BatchNorm(+ReLU)(out), which
                # the next convolution multiplies, is then read off this table instead of off the whole tensor
                self.out_minmax = fn.zeros(tiles, 2, self.cout, device=self._g.device)
        return self.out_stats

    def _magnitudes(self, which):
        """device scalars of this node's operand magnitudes ("f16x2" math; None otherwise).  `x`: computed by the first
        reader of the (tensor, affine) pair in a step; `dy`: by backward(); `w`: by Graph.forward for all weights."""
        mag = self._g.mag
        if self.am_x is None or not mag.active:
            return None
        if which == "x" and not mag.done(self.am_x):
            src = self.x_raw
            while src.alias_of is not None:       # BlockGrad: the same values under another name
                src = src.alias_of
            prod = src.producer
            # the producer's per-tile extremes of x_raw (written when some BatchNorm reads it): with an affine, its extremes
            # sit at the extremes of x (monotone per channel); without one, |x| is largest at one of them
            table = getattr(prod, "out_minmax", None) if getattr(prod, "out", None) is src else None
            if table is not None:
                fn.absmax(table.view(-1, table.shape[-1]), self.in_affine, out=mag.claim(self.am_x))
            elif mag.done(src.am_slot):
                # round 4: a bound the producer left while it wrote the tensor (or the bound of what it was pooled from)
                if self.in_affine is None:
                    return mag.block(src.am_slot)
                fn.absmax_affine_bound(self.in_affine[0], self.in_affine[1], mag.block(src.am_slot), mag.claim(self.am_x))
            else:
                fn.absmax(self.x_raw.data, self.in_affine, out=mag.claim(self.am_x))
        return mag.block({"x": self.am_x, "dy": self.am_dy, "w": self.am_w}[which])

    def forward(self):
        xa, wa = self._magnitudes("x"), self._magnitudes("w")
        if self.tap_expand:
            cout, kh, kw, cin = self.w.shape
            fn.conv2d_forward(self.x.data, self.wop().view(cout * kh * kw, 1, 1, cin), None, 1, 0, 1, out=self.z,
                              w_planes=self.wp, math=self.math,     # (the planes of [Cout][taps][..] ARE those of the view)
                              x_absmax=xa, w_absmax=wa)
            fn.tap_sum(self.z, None if self.b is None else self.b.data, cout, kh, kw, self.pad, out=self.out.data)
            return
        if self.guard_fb:
            return self._forward_fallback()
        xp = self._x_planes()
        fn.conv2d_forward(self.x_raw.data if xp is None else xp, self.wop(), None if self.b is None else self.b.data, self.stride,
                          self.pad, self.dil, relu=self.relu, out=self.out.data,
                          residual=None if self.residual is None else self.residual.data,
                          in_affine=self.in_affine if xp is None else None,
                          out_stats=None if self.out_stats is None else self.out_stats[0], w_planes=self.wp,
                          math=self.math, x_absmax=xa, w_absmax=wa, out_minmax=self.out_minmax, x_planes=xp is not None,
                          out_absmax=self._out_magnitude())

    def _out_magnitude(self):
        """the magnitude block this call's epilogue fills, claimed (None where a BatchNorm takes statistics -- its finalize
        hands the magnitude on -- or the math is not "f16x2")"""
        mag = self._g.mag
        if (not FUSE_CONV_MAGNITUDES or self.am_out is None or not mag.active or self.out_stats is not None
                or not mag.wanted(self.am_out) or xa_unavailable(self)):
            return None
        return mag.claim(self.am_out)

    def _x_planes(self):
        """the input as piece planes, when the BatchNorm in front wrote them this step (cut by this node's x magnitude)"""
        bn = self.x_planes_bn
        if self.guard_fb:
            return None
        return bn.planes if (bn is not None and bn.planes_ready and self._g.mag.done(self.am_x)) else None

    def _w3(self, transposed):
        """the weight operand of a fallback call: three bf16 piece planes cut on the spot (None where the three-piece kernels
        read the float weights: contractions that are not whole 32-channel blocks)"""
        cols = self.wt_shape[3] if transposed else self.w.shape[3]
        if cols % 32 != 0:
            return None
        return fn.weight_planes(self.w.data, transposed=transposed, cols=cols, math="bf16x3")

    def _forward_fallback(self):
        """range guard: the same convolution in the three-piece bf16 math, on the float input (affine in the loader); the
        per-tile extremes the two-piece consumers take their magnitudes from are filled by a pass of their own"""
        fn.conv2d_forward(self.x_raw.data, self.wop(), None if self.b is None else self.b.data, self.stride, self.pad, self.dil,
                          relu=self.relu, out=self.out.data, residual=None if self.residual is None else self.residual.data,
                          in_affine=self.in_affine, out_stats=None if self.out_stats is None else self.out_stats[0],
                          w_planes=self._w3(False), math="bf16x3")
        if self.out_minmax is not None:
            fn.tile_minmax(self.out.data, self.out_stats[2], self.out_minmax)
        oa = self._out_magnitude()
        if oa is not None:
            fn.absmax(self.out.data, out=oa)
        self._g.guard_count_call()

    def backward(self):
        if not self.out._gw:
            return
        dy = self.out.grad
        planes = self.out.grad_planes            # fp16 piece planes from the BatchNorm behind this convolution (never with relu / bias / residual)
        if self.relu and self.b is not None:     # ReLU mask and bias gradient in one pass over dy
            # "f16x2" math: that pass also leaves the magnitude of the masked gradient, which both of its readers cut it by
            mag, dya0 = self._g.mag, None
            if FUSE_CONV_MAGNITUDES and not mag.done(self.am_dy) and dy.dtype == torch.float32:
                dya0 = mag.claim(self.am_dy)
            fn.relu_backward_colsum(self.out.data, dy, self.cout, dx=dy, out=self.b.grad, dx_absmax=dya0)
        elif self.relu:
            fn.relu_backward(self.out.data, dy, dx=dy)
        if self.residual is not None and self.residual.requires_grad:
            self.residual.give_grad(dy)
        if self.b is not None and not self.relu and not self.b.fixed:
            fn.colsum(dy, self.cout, out=self.b.grad)
        # "f16x2" math: the gradient's magnitude once (after the in-place ReLU mask above), for both of its readers
        xa, dya, wa = self._magnitudes("x"), self._magnitudes("dy"), self._magnitudes("w")
        if dya is not None and not self._g.mag.done(self.am_dy):       # (else: the BatchNorm backward that completed dy took it)
            fn.absmax(dy, out=self._g.mag.claim(self.am_dy))    # (a projection shortcut that shares this slot reads the same gradient)
        route = R.conv_route(self._facts(planes))
        step = {R.WGRAD: self._weight_gradient_step, R.ISG: self._input_sum_gradient, R.DGRAD: self._data_gradient,
                R.PARK: self._park_finalize}
        for s in route.steps:
            step[s](route, dy, planes, xa, dya, wa)

    def _facts(self, planes):
        """what backward_route.conv_route reads: the node and graph_plan's marks, the knobs as they stand now, this pass"""
        g, x, bn, pair = self._g, self.x, self.bn_bwd_node, self.sc_pair
        hand = None if bn is None else bn.hand
        cuda = g.device.type == "cuda"
        stride2_member = pair is not None and self.stride == 2
        (N, H, W, C), K = x.shape, self.wt_shape[3]
        return R.ConvFacts(
            stride=self.stride, bn_bwd_node=bn is not None, sc_pair=pair is not None, bn1_recompute=self.bn1_recompute,
            bn_dx_planes=bn is not None and bn.dx_planes, bn_x_requires_grad=bn is not None and bn.x.requires_grad,
            w_fixed=self.w.fixed, x_requires_grad=x.requires_grad,
            input_sum_grad=self.input_sum_grad is not None and not self.input_sum_grad.fixed, tap_expand=self.tap_expand,
            cuda=cuda, compact_buf=g.sc_compact_buf is not None,
            wgrad_side=bool(WGRAD_SIDE), wgrad_side_allowed=g.wgrad_side_allowed, finalize_beside=bool(FINALIZE_BESIDE),
            sc_compact=bool(SC_COMPACT), bn1_recompute_knob=BN1_RECOMPUTE, bn_chain=g.batchnorm_chain(),
            wgrad_worth=self._wgrad_worth_a_stream(), on_branch_stream=g.on_branch_stream,
            guard_fb=self.guard_fb, pair_guard_fb=pair is not None and pair.guard_fb, dy_planes=bool(planes), x_written=x._gw,
            pair_out_written=stride2_member and pair.out._gw, have_addend=x.sc_compact is not None,
            bn_pooled=hand is not None and hand.pooled is not None, bn_parked=hand is not None and hand.parked is not None,
            recompute_pays=self.bn1_recompute and bn1_recompute_pays(N * H * W, C, K),
            # (host-only queries of the library, asked for marked nodes only)
            addend_kernel=stride2_member and fn.conv2d_dgrad_addend_route(x.shape, pair.out.shape[3], pair.out.grad_planes),
            recompute_kernel=self.bn1_recompute and fn.conv2d_dgrad_recompute_route(x.shape, K, planes))

    def _weight_gradient_step(self, route, dy, planes, xa, dya, wa):
        if route.wgrad == R.ON_SIDE:
            went = self._g.wgrad_beside(self, dy, planes, xa, dya)
            assert went, "the route sent a weight gradient beside the chain that Graph.wgrad_beside refuses"
        else:
            self._weight_gradient(dy, planes, xa, dya)

    def _input_sum_gradient(self, route, dy, planes, xa, dya, wa):
        fn.conv2d_input_sum_grad(dy, self.w.data, self.x.shape, self.stride, self.pad, self.dil, out=self.input_sum_grad.grad)

    def _park_finalize(self, route, dy, planes, xa, dya, wa):
        """round 6: the data gradient that gathered the sums of the BatchNorm in front has gone FIRST; that node's finalize
        rides in front of the weight gradient's grid, which comes next (BatchNorm.finalize_beside)"""
        self.bn_bwd_node.finalize_beside()

    def _wgrad_worth_a_stream(self):
        """The weight gradient goes beside the chain only where that pays: behind a data gradient that feeds a BatchNorm
        backward (its finalize launches leave gaps, its apply pass is HBM-bound; the caller checks that) and where the kernel is
        long enough to carry the two events it costs.  Measured with every weight gradient beside: resnet-50 +1.9 %,
        vgg16_reduced (no BatchNorm: the chain is MFMA-bound like the weight gradients) -3.4 %, inceptionv3 1024 x 512 bs 8
        (launches of ~15 us) -7 % (profiles/r06_wgrad_beside_other_configs.txt).  Estimate: the larger of multiply-adds at
        250 TFLOP/s and operand bytes at 4 TB/s, at least WGRAD_SIDE_MIN_US."""
        w = self._wg_worth
        if w is None:
            P = float(np.prod(self.out.shape[:-1]))
            cout, kh, kw, cin = self.w.shape
            esz = 4.0 if self.out.dtype == torch.float32 else 2.0
            est = max(2.0 * P * cout * kh * kw * cin / 2.5e14, esz * (P * cout + float(np.prod(self.x.shape))) / 4e12)
            w = self._wg_worth = est * 1e6 >= WGRAD_SIDE_MIN_US
        return w

    def _weight_gradient(self, dy, planes, xa, dya):
        # each case chooses its operands once -- x, dy, the weight's shape, (stride, pad, dil) and what else the call names
        wshape, geom = self.w.shape, (self.stride, self.pad, self.dil)
        if self.tap_expand:
            cout, kh, kw, cin = self.w.shape
            fn.tap_spread(dy, cout, kh, kw, self.pad, out=self.z)
            # (the weight gradient multiplies the SPREAD gradient z: its magnitude is taken on the fly, these are small layers)
            x, dy, wshape, geom = self.x.data, self.z, (cout * kh * kw, 1, 1, cin), (1, 0, 1)
            how = dict(math=self.math, x_absmax=xa)
        elif self.guard_fb:
            assert not planes, "a convolution on the guard's fallback got its gradient as piece planes"
            x, how = self.x_raw.data, dict(in_affine=self.in_affine, math="bf16x3")
            self._g.guard_count_call()
        else:
            xp = self._x_planes()
            x = self.x_raw.data if xp is None else xp
            how = dict(in_affine=self.in_affine if xp is None else None, math=self.math, x_absmax=xa, dy_absmax=dya,
                       dy_planes=planes, x_planes=xp is not None)
        # ... and one site leaves the split-K slabs for the batched reduce, or writes the gradient
        if self.slabs is not None:
            fn.conv2d_wgrad_slabs(x, dy, wshape, self.slabs, *geom, **how)
        else:
            fn.conv2d_wgrad(x, dy, wshape, *geom, out=self.w.grad.view(wshape), **how)
        self.slabs_fresh = self.slabs is not None

    def _data_gradient(self, route, dy, planes, xa, dya, wa):
        g, kind = self._g, route.dgrad
        if self.wtp is not None and (g.wp_frozen if self.w.fixed else g.wp_table) is None:
            fn.weight_planes(self.w.data, transposed=True, cols=self.wtp.shape[2] * 32, out=self.wtp, math=self.math,
                             w_absmax=wa)
        elif self.wtp is None and not (g.wt_frozen is not None if self.w.fixed else g.wt_batched):
            fn.weight_transpose(self.w.data, out=self.wt, copy=self.wh)
        # each kind chooses its operands once -- the weight, dx's shape, (stride, pad, dil) and what else the call names
        wt, shape, geom = self.wt, self.x.shape, (self.stride, self.pad, self.dil)
        how = dict(wt_planes=self.wtp, math=self.math, dy_absmax=dya, w_absmax=wa, dy_planes=planes)
        bn, bn_dya = (self.bn_bwd_node if route.hands_sums else None), None
        if kind == R.COMPACT:
            # a projection shortcut (1 x 1, stride 2, pad 0) as the stride-1 1 x 1 data gradient on the subsampled grid, into the
            # graph's compact buffer, left on the input tensor for the pair's conv1 (which runs next among the writers of that
            # gradient and adds it in its epilogue).  A weight gradient of this node beside the chain reads dy, never the
            # compact buffer, which is written and read on the step's stream only
            (N, H, W, C), (Ho, Wo) = self.x.shape, dy.shape[1:3]
            dx = g.sc_compact_buf[:N * Ho * Wo * C].view(N, Ho, Wo, C)
            shape, geom = dx.shape, (1, 0, 1)
            how.update(out=dx)
        else:
            dx, acc = self.x.grad_target()
            if bn is not None:       # set by Graph.finalize on the LAST writer of a deferred BN's gradient
                how.update(bn_bwd=(bn.x.data, bn.scale, bn.shift, bn.mean, bn.rstd, bn.relu, bn.bwd_sums[0]))
                bn.hand.sums_ready = True
                if route.claims_dyin:    # that BatchNorm's backward bounds its dx from the largest gradient stored here
                    bn_dya = g.mag.claim(bn.am_dyin)
            if kind == R.SUMS_ONLY:      # dx stays unwritten; bn's backward runs this product again (BatchNorm._apply)
                how.update(sums_only=True)
                bn.hand.recompute = (self, dy, planes, dya, wa)
            elif kind == R.FALLBACK:
                w3 = self._w3(True)
                wt = self.wt if w3 is None else None
                how = dict(out=dx, accumulate=acc, bn_bwd=how.get("bn_bwd"), wt_planes=w3, math="bf16x3")
            else:      # (the addend: this call is then the first and only writer of dx)
                how.update(out=dx, accumulate=acc, bn_dy_absmax=bn_dya, strided_addend=self.x.sc_compact if kind == R.ADDEND else None)
        fn.conv2d_dgrad(dy, wt, shape, *geom, wt_shape=self.wt_shape, **how)
        if kind == R.COMPACT:
            self.x.sc_compact = dx
        elif kind == R.FALLBACK:
            if bn_dya is not None:       # (the two-piece data gradient leaves this by-product in its epilogue)
                fn.absmax(dx, out=bn_dya)
            g.guard_count_call()


class BilinearConcatConv(Node):
    """Convolution(kernel k x k, stride 1, 'same', no bias) of the channel concatenation of bilinearly resized maps
    -- `score3_conv` over `score3_concat` (multitask_symbol_builder.py:574-585) -- evaluated WITHOUT the
    concatenation.

    With the k x k taps expanded (dspn_tap_sum_f32) the convolution is a per-pixel linear map W (Cout*k*k x Cin)
    followed by a shifted sum, and a per-pixel linear map commutes with the resize U_c of each component (both are
    linear; U_c acts on pixels, W on channels):
        z = W . concat_c U_c(x_c) = sum_c U_c(W_c . x_c),          W_c = the columns of W that face component c.
    So each component is multiplied at ITS OWN resolution (4x4 ... 64x64 instead of 64x64 for all 3328 channels:
    9.3x fewer multiply-adds at 512x512), the small Cout*k*k-channel results are resized and added, and the
    3328-channel concatenation (1.7 GB per batch of 32, written once and read three times) never exists.  Backward
    is the transpose of the same chain: dz_c = U_c^T dz, dx_c = W_c^T dz_c, dW_c = dz_c^T x_c.
    Exact in real arithmetic; in fp32 the result differs from the direct form by rounding only (the graph-level
    parity tests against the direct-form oracle cover it).  The parameter keeps the reference's name and shape."""

    def __init__(self, g, inputs, name, num_filter, kernel, pad, target_hw, theta, init="maxdim"):
        N = inputs[0].shape[0]
        kh, kw = fn._hw(kernel)
        self.pad = fn._hw(pad)
        assert (kh - 1) // 2 == self.pad[0] and (kw - 1) // 2 == self.pad[1], "needs a 'same' convolution"
        Ht, Wt = target_hw
        self.inputs = inputs
        self.theta = theta            # Param "affine_matrix": the sampling grid of every component
        self.offsets = np.cumsum([0] + [t.shape[3] for t in inputs]).tolist()
        Cin = self.offsets[-1]
        self.cout, self.kh, self.kw = num_filter, kh, kw
        self.w = g.param(name + "_weight", (num_filter, kh, kw, Cin), conv_weight_init(init, Cin))
        self.w.logical, self.w.kind = (num_filter, Cin, kh, kw), "conv"
        T = num_filter * kh * kw
        Tp = fn.padc(T)
        self.T = T
        half = fn.ACT_DTYPE == torch.bfloat16
        self.z = fn.act_zeros(N, Ht, Wt, Tp, device=g.device)        # tap-expanded map at the target size (dz in backward)
        self.zc, self.wc, self.wct, self.dwc, self.wch, self.wcp = [], [], [], [], [], []
        self.math = g.math
        self._g = g
        # "f16x2" math: per component, slots for the magnitudes of its input, its weight slice and its output gradient --
        # each taken once per step and shared by the forward, weight-gradient and data-gradient calls that multiply it
        f16 = g.math == "f16x2"
        self.am = [(g.mag.new(), g.mag.new(), g.mag.new(backward=True)) if f16 else (None, None, None) for _ in inputs]
        # round 4: every weight slice is bounded by the magnitude of the whole weight, which the one batched launch at the top
        # of forward() takes with all the others (Magnitudes.am_table); the inputs are materialised BatchNorm outputs, which leave
        # theirs while they are written; the sampler's data-gradient passes leave the gradients'
        self.am_w = g.mag.new() if f16 else None
        for t in inputs:
            # W_c . x_c at the component's own resolution (its gradient in backward).  Every component goes through
            # the sampler, also the ones that already have the target size: once the optimizer has moved
            # affine_matrix off the identity they are resampled too, and their grid gradient is not zero
            self.zc.append(fn.act_zeros(N, t.shape[1], t.shape[2], Tp, device=g.device))
            self.wc.append(fn.zeros(T, 1, 1, t.shape[3], device=g.device))      # W_c, contiguous (float master slice)
            self.wct.append(fn.act_zeros(t.shape[3], 1, 1, Tp, device=g.device))    # its transpose (data-gradient operand)
            self.wch.append(fn.act_zeros(T, 1, 1, t.shape[3], device=g.device) if half else None)   # bf16 forward operand
            self.dwc.append(fn.zeros(T, 1, 1, t.shape[3], device=g.device))
            # split math: piece planes of W_c (the forward operand), refreshed after every gather of the slices
            self.wcp.append(fn.zeros(T, 1, t.shape[3] // 32, fn.plane_pieces(g.math), 32, device=g.device, dtype=torch.bfloat16)
                            if g.device.type == "cuda" and fn.needs_planes(self.zc[-1].dtype, t.shape[3], g.math) else None)
        self.sources = None           # fn.SamplerSources over zc, made at the first forward
        self.tpart = None             # (source pixels of all components, 6) float64: rows of the theta gradient
        self.out = g.tensor((N, Ht, Wt, fn.padc(num_filter)), name + "_out")
        self.out.channels = num_filter
        # multiply-adds actually executed (the direct form would be 2 * Cin * Cout * k * k * Ht * Wt * N)
        self.flops_fwd = sum(2.0 * t.shape[3] * T * t.shape[1] * t.shape[2] * N for t in inputs)
        self.flops_bwd = self.flops_fwd + sum(2.0 * t.shape[3] * T * t.shape[1] * t.shape[2] * N
                                              for t in inputs if t.requires_grad)
        self.flops_direct = 2.0 * Cin * T * Ht * Wt * N

    def _gather_weights(self):
        w2d = self.w.data
        Cin = self.offsets[-1]
        for c, t in enumerate(self.inputs):
            fn.copy_block(w2d, self.wc[c], 1, self.T, t.shape[3], 0, Cin, self.offsets[c], 0, t.shape[3], 0)

    def forward(self):
        self._gather_weights()
        for c, t in enumerate(self.inputs):
            if self.wch[c] is not None:      # bf16 operands of this slice: copy + transpose in one launch
                fn.weight_transpose(self.wc[c], out=self.wct[c], copy=self.wch[c])
            xa, wa = self._g.mag.take(self.am[c][0], t.data, src=t), self._g.mag.block(self.am_w)
            if self.wcp[c] is not None:
                fn.weight_planes(self.wc[c], out=self.wcp[c], math=self.math, w_absmax=wa)
            fn.conv2d_forward(t.data, self.wc[c] if self.wch[c] is None else self.wch[c], None, 1, 0, 1, out=self.zc[c],
                              w_planes=self.wcp[c], math=self.math, x_absmax=xa, w_absmax=wa)
        if self.sources is None:
            self.sources = fn.SamplerSources([(z, 0) for z in self.zc])
        fn.affine_sampler_forward(self.sources, self.theta.data, self.z)       # z = sum_c U_c(theta)(W_c x_c), one pass
        fn.tap_sum(self.z, None, self.cout, self.kh, self.kw, self.pad, out=self.out.data)

    def backward(self):
        if not self.out._gw:
            return
        fn.tap_spread(self.out.grad, self.cout, self.kh, self.kw, self.pad, out=self.z)
        # d L / d affine_matrix needs the forward values W_c x_c: every source's data-gradient pass reads them (its own
        # pixel's, before it overwrites zc with the gradient) and leaves its share of the theta gradient as rows of tpart
        if self.tpart is None:
            rows = [fn.affine_sampler_theta_rows(z.shape, self.z.shape[1], z.dtype) for z in self.zc]
            self.tpart = torch.zeros(sum(rows), 6, dtype=torch.float64, device=self.z.device)
            self.tpart_off = np.cumsum([0] + rows).tolist()
        Cin = self.offsets[-1]
        for c, t in enumerate(self.inputs):
            mag = self._g.mag      # (a gradient that is not float32 is never read through its block: written, not claimed)
            dza = mag.claim(self.am[c][2]) if self.zc[c].dtype == torch.float32 else mag.block(self.am[c][2])
            dz = fn.affine_sampler_backward_data_theta(self.z, self.theta.data, self.zc[c], 0,
                                                       self.tpart[self.tpart_off[c]:self.tpart_off[c + 1]], dx=self.zc[c],
                                                       dx_absmax=dza)
            xa, wa = self._g.mag.take(self.am[c][0], t.data, src=t), self._g.mag.block(self.am_w)
            dza = mag.take(self.am[c][2], dz)
            if not self.w.fixed:
                fn.conv2d_wgrad(t.data, dz, (self.T, 1, 1, t.shape[3]), 1, 0, 1, out=self.dwc[c], math=self.math,
                                x_absmax=xa, dy_absmax=dza)
                fn.copy_block(self.dwc[c], self.w.grad, 1, self.T, t.shape[3], 0, t.shape[3], 0, 0, Cin, self.offsets[c])
            if t.requires_grad:
                if self.wch[c] is None:
                    fn.weight_transpose(self.wc[c], out=self.wct[c])
                dx, acc = t.grad_target()
                fn.conv2d_dgrad(dz, self.wct[c], t.shape, 1, 0, 1, out=dx, accumulate=acc, math=self.math, dy_absmax=dza,
                                w_absmax=wa)
        if not self.theta.fixed:
            fn.affine_sampler_theta_reduce(self.tpart, self.theta.grad)


class Deconv4x4s2(Node):
    """mx.sym.Deconvolution(kernel 4, stride 2, pad 1, no bias) (multitask_symbol_builder.py:586):
    forward = data-gradient kernel of the 4x4/2 convolution with weight [K=in][R][S][C=out]."""

    def __init__(self, g, x, name, channels):
        N, H, W, Cp = x.shape
        self.x = x
        self.w = g.param(name + "_weight", (Cp, 4, 4, Cp), deconv_bilinear_init(channels))
        self.w.logical, self.w.kind = (channels, channels, 4, 4), "deconv"
        self.wt = fn.act_zeros(Cp, 4, 4, Cp, device=g.device)
        self.wh = fn.act_zeros(Cp, 4, 4, Cp, device=g.device) if fn.ACT_DTYPE == torch.bfloat16 else None
        self.out = g.tensor((N, 2 * H, 2 * W, Cp), name + "_out")
        self.out.channels = channels
        self.math = g.math
        self._g = g
        self.am = (g.mag.new(), g.mag.new(), g.mag.new(backward=True)) if g.math == "f16x2" else (None, None, None)   # x, w, dy
        self.am_w = self.am[1]      # (taken with every other weight's by the batched launch; a frozen weight's moves: Magnitudes.allocate)
        self.flops_fwd = 2.0 * channels * channels * 16 * H * W * N
        self.flops_bwd = self.flops_fwd * (2 if x.requires_grad else 1)

    def forward(self):
        fn.weight_transpose(self.w.data, out=self.wt, copy=self.wh)
        mag = self._g.mag
        xa, wa = mag.take(self.am[0], self.x.data, src=self.x), mag.take(self.am_w, self.w.data)
        fn.conv2d_dgrad(self.x.data, self.wt, self.out.shape, 2, 1, 1, out=self.out.data, math=self.math, dy_absmax=xa,
                        w_absmax=wa)

    def backward(self):
        if not self.out._gw:
            return
        dy = self.out.grad
        mag = self._g.mag
        xa, wa, dya = mag.take(self.am[0], self.x.data, src=self.x), mag.take(self.am_w, self.w.data), mag.take(self.am[2], dy)
        if not self.w.fixed:
            fn.conv2d_wgrad(dy, self.x.data, self.w.shape, 2, 1, 1, out=self.w.grad, math=self.math, x_absmax=dya,
                            dy_absmax=xa)
        if self.x.requires_grad:
            dx, acc = self.x.grad_target()
            fn.conv2d_forward(dy, self.w.data if self.wh is None else self.wh, None, 2, 1, 1, out=dx, accumulate=acc,
                              math=self.math, x_absmax=dya, w_absmax=wa)


class Add(Node):
    """elementwise sum of the residual unit (symbol/resnet.py:51)"""

    def __init__(self, g, a, b, name):
        self.a, self.b = a, b
        self.out = g.tensor(a.shape, name)

    def forward(self):
        fn.add(self.a.data, self.b.data, out=self.out.data)

    def backward(self):
        if not self.out._gw:
            return
        for t in (self.a, self.b):
            if t.requires_grad:
                t.give_grad(self.out.grad)


class BlockGrad(Node):
    """mx.sym.BlockGrad: same values, no gradient (multitask_symbol_builder.py:542,549)"""

    def __init__(self, g, x, name):
        self.out = g.tensor(x.shape, name, requires_grad=False, data=x.data)
        self.out.alias_of, self.out.am_slot, self.out.channels = x, x.am_slot, x.channels

    def forward(self):
        pass


class MaxPool(Node):
    """mx.sym.Pooling(pool_type='max'); pooling_convention='full' (symbol/vgg16_reduced.py:40-42) rounds the
    output size up, windows that stick out of the image just see fewer pixels"""

    def __init__(self, g, x, name, kernel, stride, pad, full=False):
        N, H, W, C = x.shape
        self.x, self.k, self.s, self.p = x, kernel, stride, pad

        def osz(h):
            if not full:
                return fn.conv_out_size(h, kernel, stride, pad)
            return -(-(h + 2 * pad - kernel) // stride) + 1
        self.out = g.tensor((N, osz(H), osz(W), C), name)
        self.out.am_slot = x.am_slot        # |max over a window| <= the input's magnitude
        # input produced by a deferred BatchNorm(+ReLU) (round 4: bn0 -> relu0 -> pooling0 of the resnet stem): the pooling pass
        # reads the raw tensor and applies the affine itself, the normalised tensor is never written
        self.x_raw, self.in_affine, self._g = x, None, g
        self.am_out = None
        if x.affine_src is not None:
            raw, sc, sh, arelu = x.affine_src
            self.x_raw, self.in_affine = raw, (sc, sh, arelu)
            if g.math == "f16x2" and self.out.dtype == torch.float32:
                self.am_out = g.mag.new()
                self.out.am_slot = self.am_out
        # one byte per output element: which window position held the maximum (read by backward
        # instead of x and y)
        self.argmax = (torch.zeros(self.out.shape, dtype=torch.uint8, device=g.device)
                       if x.requires_grad and kernel * kernel < 255 else None)

    def forward(self):
        if self.in_affine is not None:
            fn.maxpool_forward(self.x_raw.data, self.k, self.s, self.p, out=self.out.data, argmax=self.argmax,
                               in_affine=self.in_affine, out_absmax=self._g.mag.claim(self.am_out))
            return
        fn.maxpool_forward(self.x.data, self.k, self.s, self.p, out=self.out.data, argmax=self.argmax)

    def backward(self):
        if not self.out._gw or not self.x.requires_grad:
            return
        assert not self.x._gw, "maxpool input has a single consumer"
        bn = self.x.bn_node
        if (self.in_affine is not None and self.argmax is not None and bn is not None and FUSE_MAXPOOL_BACKWARD
                and self.out.grad.dtype == torch.float32 and self.out.grad.device.type == "cuda"):
            # round 4: the BatchNorm(+ReLU) folded into this pooling forms its output gradient from (pooled gradient, argmax)
            # itself (dspn_bn_backward_maxpool_f32): the dense gradient of the pooling input is never written
            bn.hand.pooled = (self.argmax, self.out.grad, self.k, self.s, self.p)
            self.x._gw = True
            return
        dx, _ = self.x.grad_target()
        if self.argmax is not None:
            fn.maxpool_backward_argmax(self.argmax, self.out.grad, self.x.shape, self.k, self.s, self.p, dx=dx)
        else:
            assert self.in_affine is None, "a pooling layer behind a deferred BatchNorm keeps its argmax record"
            fn.maxpool_backward(self.x.data, self.out.data, self.out.grad, self.k, self.s, self.p, dx=dx)


class AvgPool(Node):
    """mx.sym.Pooling(pool_type='avg', kernel=(k,k), stride=(k,k)) (multitask_symbol_builder.py:560-562)"""

    def __init__(self, g, x, name, k):
        N, H, W, C = x.shape
        self.x, self.k = x, k
        if k == 1:
            self.out = x
        else:
            self.out = g.tensor((N, H // k, W // k, C), name)
            self.out.am_slot = x.am_slot    # |mean over a window| <= the input's magnitude

    def forward(self):
        if self.k > 1:
            fn.avgpool_forward(self.x.data, self.k, out=self.out.data)

    def backward(self):
        if self.k == 1 or not self.out._gw or not self.x.requires_grad:
            return
        dx, acc = self.x.grad_target()
        fn.avgpool_backward(self.out.grad, self.x.shape, self.k, dx=dx, accumulate=acc)


class AvgPool2d(Node):
    """mx.sym.Pooling(pool_type='avg', kernel k, stride, pad) with overlapping windows
    (symbol/inceptionv3.py:31,74,115); the divisor is k*k including padding"""

    def __init__(self, g, x, name, kernel, stride, pad):
        N, H, W, C = x.shape
        self.x, self.k, self.s, self.p = x, kernel, stride, pad
        self.out = g.tensor((N, fn.conv_out_size(H, kernel, stride, pad), fn.conv_out_size(W, kernel, stride, pad), C),
                            name)

    def forward(self):
        fn.avgpool2d_forward(self.x.data, self.k, self.s, self.p, out=self.out.data)

    def backward(self):
        if not self.out._gw or not self.x.requires_grad:
            return
        dx, acc = self.x.grad_target()
        fn.avgpool2d_backward(self.out.grad, self.x.shape, self.k, self.s, self.p, dx=dx, accumulate=acc)


class Concat(Node):
    """mx.sym.Concat along channels (symbol/inceptionv3.py:33): each input is copied into its channel
    slice of the NHWC output; backward copies (or accumulates) the slice of the output gradient back"""

    def __init__(self, g, inputs, name):
        N, H, W, _ = inputs[0].shape
        assert all(t.shape[:3] == (N, H, W) for t in inputs), [t.shape for t in inputs]
        self.inputs = inputs
        self.offsets = np.cumsum([0] + [t.shape[3] for t in inputs]).tolist()
        self.out = g.tensor((N, H, W, self.offsets[-1]), name)

    def forward(self):
        N, H, W, C = self.out.shape
        for t, off in zip(self.inputs, self.offsets):
            c = t.shape[3]
            fn.copy_block(t.data, self.out.data, N, H * W, c, H * W * c, c, 0, H * W * C, C, off)

    def backward(self):
        if not self.out._gw:
            return
        N, H, W, C = self.out.shape
        for t, off in zip(self.inputs, self.offsets):
            if not t.requires_grad:
                continue
            c = t.shape[3]
            dx, acc = t.grad_target()
            fn.copy_block(self.out.grad, dx, N, H * W, c, H * W * C, C, off, H * W * c, c, 0, accumulate=acc)


class BilinearConcat(Node):
    """GridGenerator(affine_matrix, target) + BilinearSampler on each input, concatenated along
    channels (multitask_symbol_builder.py:574-582)."""

    def __init__(self, g, inputs, name, target_hw, theta):
        N = inputs[0].shape[0]
        self.inputs = inputs
        self.theta = theta
        self.offsets = np.cumsum([0] + [t.shape[3] for t in inputs]).tolist()
        self.out = g.tensor((N, target_hw[0], target_hw[1], self.offsets[-1]), name)
        self.sources = None           # made at the first forward (Graph.finalize may still re-allocate an input)

    def forward(self):
        if self.sources is None:
            self.sources = fn.SamplerSources([(t.data, off) for t, off in zip(self.inputs, self.offsets)])
        fn.affine_sampler_forward(self.sources, self.theta.data, self.out.data)

    def backward(self):
        if not self.out._gw:
            return
        if not self.theta.fixed:
            fn.affine_sampler_backward_theta(self.sources, self.theta.data, self.out.grad, self.theta.grad)
        for t, off in zip(self.inputs, self.offsets):
            if not t.requires_grad:
                continue
            dx, acc = t.grad_target()
            fn.affine_sampler_backward_data(self.out.grad, self.theta.data, t.shape, off, dx=dx, accumulate=acc)
