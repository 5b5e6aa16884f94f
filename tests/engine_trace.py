"""What the engine asks of the library in a pass, as text: a recorder of the calls into dspnet_amd.functional, and the small
graphs and settings whose traces tests/golden/engine_backward_trace.json pins (written by
tests/golden/make_engine_backward_trace_golden.py, replayed by tests/test_engine_trace_gpu.py).

The recorder wraps every public function DEFINED in dspnet_amd.functional except the helpers of SKIP (shapes, allocation,
descriptor tables, settings, and the two host-only route queries, which launch nothing).  Only outermost calls are recorded
(absmax inside conv2d_dgrad is that call's business).  One line per call:

    name|lane|argument=value,...

lane: the workspace lane of the call (0 the step's stream, 1 the branch stream, 2 weight gradients beside the chain).  Every
bound argument that is not None, defaults applied (so naming a default and leaving it out read the same): scalars and
strings literally, tuples element by element, tensors as dtype[shape]@k where k numbers the distinct data_ptr()s of the pass in
order of first appearance, anything else by its type's name.  The recorder keeps every tensor it has seen alive until the
pass ends, so no address is handed out twice within a pass and k depends on what the engine aliases, not on the allocator."""
import contextlib
import hashlib
import inspect

import numpy as np
import torch

from dspnet_amd import engine as E
from dspnet_amd import functional as fn

SKIP = frozenset("""L stream ptr workspace conv_out_size pad4 padc empty zeros act_zeros act_empty set_activation_dtype set_conv_math
get_conv_math needs_planes plane_pieces conv_stats_layout bn_moving bn_from_sums_workspace conv_dgrad_bn_tiles conv2d_wgrad_splits
conv2d_dgrad_addend_route conv2d_dgrad_recompute_route slice_bounds check_box_count render_chunk_rows tensor_stats_chunk_elems
tensor_stats_entry stats_records polygon_wave_entries affine_sampler_theta_rows absmax_table absmin_rows_table weight_planes_table
weight_transpose_table slab_reduce_table copy_block_table draw_table tensor_stats_table sgd_segment_table cityscapes_tables""".split())


def recorded_functions():
    return sorted(name for name, f in vars(fn).items()
                  if inspect.isfunction(f) and f.__module__ == fn.__name__ and not name.startswith("_") and name not in SKIP)


class Recorder:
    def __init__(self, pointers=True):
        self.pointers, self.lines, self.depth = pointers, [], 0
        self.new_pass()

    def new_pass(self):
        """a pass boundary: the pointer numbering starts again"""
        self.ids, self.alive = {}, []
        if self.lines:
            self.lines.append("-- pass")

    def text(self, v):
        if isinstance(v, torch.Tensor):
            s = "%s[%s]" % (str(v.dtype).replace("torch.", ""), ",".join(str(d) for d in v.shape))
            if self.pointers:
                if v.data_ptr() not in self.ids:
                    self.ids[v.data_ptr()] = len(self.ids)
                    self.alive.append(v)
                s += "@%d" % self.ids[v.data_ptr()]
            return s
        if isinstance(v, (bool, int, float, str)):
            return repr(v)
        if isinstance(v, np.generic):
            return repr(v.item())
        if isinstance(v, (tuple, list)):
            return "(" + ",".join("None" if e is None else self.text(e) for e in v) + ")"
        if isinstance(v, dict):
            return "{" + ",".join("%s=%s" % (k, self.text(e)) for k, e in sorted(v.items()) if e is not None) + "}"
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        return type(v).__name__

    def wrap(self, name, f):
        sig = inspect.signature(f)

        def wrapped(*a, **kw):
            if self.depth == 0:
                b = sig.bind(*a, **kw)
                b.apply_defaults()
                self.lines.append("%s|%d|%s" % (name, fn._WS_LANE, ",".join("%s=%s" % (k, self.text(v)) for k, v in b.arguments.items()
                                                                                if v is not None and not (isinstance(v, dict) and not v))))
            self.depth += 1
            try:
                return f(*a, **kw)
            finally:
                self.depth -= 1
        return wrapped

    @contextlib.contextmanager
    def recording(self):
        orig = {name: getattr(fn, name) for name in recorded_functions()}
        for name, f in orig.items():
            setattr(fn, name, self.wrap(name, f))
        try:
            yield self
        finally:
            for name, f in orig.items():
                setattr(fn, name, f)


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def call_counts(lines):
    counts = {}
    for ln in lines:
        if not ln.startswith("--"):
            name = ln.split("|", 1)[0]
            counts[name] = counts.get(name, 0) + 1
    return dict(sorted(counts.items()))


# ---------------------------------------------------------------------------------------------------------------------
# the graphs: B = 2, "f16x2" math, two forward / backward passes (the second reads the first one's magnitudes and piece planes)
B = 2


def _data(g, dev, size, channels, requires_grad=True):
    gen = torch.Generator().manual_seed(17)
    x0 = torch.randn(B, size, size, channels, generator=gen).to(dev)
    return g.tensor(x0.shape, "data", requires_grad=requires_grad, data=x0), gen


def build_recompute(g, dev):
    """tests/test_bn1_recompute_gpu.py toy_step: conv0 -> a stride-1 projection unit -> a dim-match unit (the bn1 / conv1 pair)"""
    from dspnet_amd.symbol import resnet
    x, gen = _data(g, dev, 128, 32)
    c0 = g.add(E.Conv(g, x, "conv0", 128, 3, pad=1)).out
    u1 = resnet.residual_unit(g, c0, 256, 1, False, "stage1_unit1", "_plus0")
    return resnet.residual_unit(g, u1, 256, 1, True, "stage1_unit2", "_plus1"), gen


def build_pair(g, dev):
    """tests/test_strided_addend_gpu.py toy_step at 128 x 128, C = 128: conv0 -> a stride-1 projection unit -> a stride-2 one"""
    from dspnet_amd.symbol import resnet
    x, gen = _data(g, dev, 128, 32)
    c0 = g.add(E.Conv(g, x, "conv0", 64, 3, pad=1)).out
    u1 = resnet.residual_unit(g, c0, 128, 1, False, "stage1_unit1", "_plus0")
    return resnet.residual_unit(g, u1, 256, 2, False, "stage2_unit1", "_plus1"), gen


def _stem(g, dev, input_grad):
    x, gen = _data(g, dev, 128, 32, requires_grad=input_grad)
    c0 = g.add(E.Conv(g, x, "conv0", 64, 3, pad=1)).out
    a0 = g.add(E.BatchNorm(g, c0, "bn0", relu=True, defer_apply=True)).out
    p0 = g.add(E.MaxPool(g, a0, "pooling0", 3, 2, 1)).out
    return g.add(E.Conv(g, p0, "conv1", 64, 1)).out, gen


def build_stem(g, dev):
    """conv -> deferred BatchNorm + ReLU -> MaxPool -> 1 x 1 conv; the input needs a gradient: the pooling-folded call"""
    return _stem(g, dev, True)


def build_stem_params_only(g, dev):
    """the same stem behind an input without a gradient and a frozen conv0: bn0's backward is its parameters alone"""
    return _stem(g, dev, False)


# name -> (builder, names the settings refer to, parameters frozen in every setting)
TOYS = {
    "recompute": (build_recompute, dict(conv1="stage1_unit2_conv1", bn1="stage1_unit2_bn1", sc="stage1_unit1_sc"), ()),
    "pair": (build_pair, dict(conv1="stage2_unit1_conv1", bn1="stage2_unit1_bn1", sc="stage2_unit1_sc"), ()),
    "stem": (build_stem, dict(conv1="conv1", bn1="bn0", sc=None), ()),
    "stem_params_only": (build_stem_params_only, dict(conv1="conv1", bn1="bn0", sc=None), ("conv0_weight",)),
}

# setting -> knobs of the engine module (chain: Graph.batchnorm_chain forced true), guard: conv1 on the range guard's fallback,
# frozen: which of the toy's names lose their parameters
SETTINGS = {
    "defaults": dict(),
    "wgrad_side_0": dict(WGRAD_SIDE=0),
    "wgrad_side_all": dict(WGRAD_SIDE=1, WGRAD_SIDE_MIN_US=0.0, chain=True),
    "one_stream_no_parking": dict(WGRAD_SIDE=0, FINALIZE_BESIDE=False),
    "bn1_recompute_0": dict(BN1_RECOMPUTE=0),
    "bn1_recompute_2": dict(BN1_RECOMPUTE=2),
    "bn1_recompute_2_one_stream": dict(BN1_RECOMPUTE=2, WGRAD_SIDE=0),
    "bn1_recompute_2_wgrad_side_all": dict(BN1_RECOMPUTE=2, WGRAD_SIDE=1, WGRAD_SIDE_MIN_US=0.0, chain=True),
    "sc_compact_0": dict(SC_COMPACT=False),
    "guard_fb_conv1": dict(guard=True),
    "conv1_weight_frozen": dict(frozen=("conv1",)),
    "bn1_frozen": dict(frozen=("bn1",)),
    "shortcut_frozen": dict(frozen=("sc",)),
}
KNOBS = ("WGRAD_SIDE", "WGRAD_SIDE_MIN_US", "FINALIZE_BESIDE", "SC_COMPACT", "BN1_RECOMPUTE")


def cases():
    """[(graph, setting)]: every setting on every toy that has what the setting names, and the network"""
    out = [(toy, s) for toy, (_, names, _) in TOYS.items() for s, kw in SETTINGS.items()
           if all(names[f] is not None for f in kw.get("frozen", ()))]
    return out + [("resnet-50", "defaults")]


@contextlib.contextmanager
def setting(name):
    kw = SETTINGS[name]
    prev = {k: getattr(E, k) for k in KNOBS}
    chain, math = E.Graph.batchnorm_chain, fn.get_conv_math()
    try:
        for k in KNOBS:
            if k in kw:
                setattr(E, k, kw[k])
        if kw.get("chain"):
            E.Graph.batchnorm_chain = lambda self: True
        fn.set_conv_math("f16x2")
        yield kw
    finally:
        for k, v in prev.items():
            setattr(E, k, v)
        E.Graph.batchnorm_chain = chain
        fn.set_conv_math(math)


def _frozen_params(names, which):
    out = []
    for f in which:
        out += [names[f] + "_gamma", names[f] + "_beta"] if f == "bn1" else [names[f] + "_weight"]
    return out


def trace(graph, setting_name, dev, pointers=True, passes=2):
    """-> the lines of `passes` forward / backward passes of one graph under one setting"""
    rec = Recorder(pointers)
    with setting(setting_name) as kw:
        if graph == "resnet-50":
            return _trace_network(rec, dev, passes)
        build, names, always_frozen = TOYS[graph]
        g = E.Graph(dev)
        frozen = list(always_frozen) + _frozen_params(names, kw.get("frozen", ()))
        if frozen:
            g.set_freeze(frozen)
        out, gen = build(g, dev)
        g.finalize(seed=5)
        g.guard["enabled"] = False
        conv1 = g.tensors[names["conv1"] + "_out"].producer
        dy = torch.randn(out.shape, generator=gen).to(dev)
        with rec.recording():
            for _ in range(passes):
                rec.new_pass()
                g.forward()
                conv1.guard_fb = bool(kw.get("guard"))
                g.begin_backward()
                out.give_grad(dy.clone())
                for idx in range(len(g.nodes) - 1, -1, -1):
                    g.backward_node(idx)
                g.join_side_backward()
                g.flush_slabs()
        torch.cuda.synchronize()
    return rec.lines


def _trace_network(rec, dev, passes):
    """get_multi_symbol_train("resnet-50", (3, 128, 128), num_classes=8, batch_size=2): eager solver.step()s -- side streams, tap
    expansion, the input-sum gradient, slabs"""
    from dspnet_amd import synthetic
    from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
    from dspnet_amd.train.solver import MultiTaskSolver
    net = get_multi_symbol_train("resnet-50", (3, 128, 128), num_classes=8, batch_size=B, device=dev, seed=0)
    gen = synthetic.rng(233)
    solver = MultiTaskSolver(net)
    solver.set_batch(torch.from_numpy(synthetic.images(B, 128, 128, gen)).to(dev),
                     torch.from_numpy(synthetic.det_labels(B, gen=gen, height=128, width=128)).to(dev),
                     torch.from_numpy(synthetic.seg_labels(B, 128, 128, gen=gen)).to(dev))
    with rec.recording():
        for _ in range(passes):
            rec.new_pass()
            solver.step()
    torch.cuda.synchronize()
    return rec.lines


# the routes a (graph, setting) is there for, read off its lines (the maker refuses a fixture in which one does not occur)
def routes_seen(lines):
    seen = set()
    compact_out = set()
    for ln in lines:
        name, lane, args = (ln.split("|", 2) + ["", ""])[:3]
        a = dict(p.split("=", 1) for p in _split_args(args))
        if name == "conv2d_dgrad":
            if a.get("sums_only") == "True":
                seen.add("sums-only")
            if a.get("math") == "'bf16x3'":
                seen.add("fallback")
            if "strided_addend" in a:
                seen.add("addend")
                if a["strided_addend"] in compact_out:
                    seen.add("compact")
            if "out" in a:
                compact_out.add(a["out"])
        elif name == "conv2d_dgrad_bn_apply":
            seen.add("recomputed apply")
        elif name == "bn_backward_from_sums":
            if a.get("park") == "True":
                seen.add("parked")
            if a.get("dx_planes") == "True":
                seen.add("planes")
            if a.get("dx") == "NoOutput":
                seen.add("parameters only")
        elif name == "bn_backward_maxpool":
            seen.add("pooled")
            if a.get("dx") == "NoOutput":
                seen.add("parameters only")
        elif name in ("conv2d_wgrad", "conv2d_wgrad_slabs") and lane == "2":
            seen.add("second stream")
        elif name == "conv2d_input_sum_grad":
            seen.add("input-sum gradient")
        if lane == "1":
            seen.add("branch stream")
    return seen


def _split_args(args):
    """the top-level k=v parts of a line's argument text (commas inside brackets belong to a value)"""
    parts, depth, cur = [], 0, ""
    for ch in args:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return [p for p in parts + [cur] if "=" in p]


EXPECT = {
    ("recompute", "defaults"): {"planes"},
    ("recompute", "wgrad_side_0"): {"parked"},
    ("recompute", "wgrad_side_all"): {"second stream"},
    ("recompute", "bn1_recompute_2"): {"sums-only", "recomputed apply"},
    ("recompute", "bn1_recompute_2_one_stream"): {"sums-only", "recomputed apply", "parked"},
    ("recompute", "bn1_recompute_2_wgrad_side_all"): {"sums-only", "recomputed apply", "second stream"},
    ("recompute", "guard_fb_conv1"): {"fallback"},
    ("pair", "defaults"): {"addend", "compact", "planes"},
    ("pair", "shortcut_frozen"): {"addend", "compact"},
    ("pair", "guard_fb_conv1"): {"fallback"},
    ("pair", "wgrad_side_0"): {"addend", "compact", "parked"},
    ("stem", "defaults"): {"pooled"},
    ("stem_params_only", "defaults"): {"pooled", "parameters only"},
    ("resnet-50", "defaults"): {"pooled", "input-sum gradient", "branch stream", "planes"},
}
# ... and what must NOT occur where the setting switches it off
FORBID = {
    ("recompute", "defaults"): {"sums-only"},           # (at this size bn1_recompute_pays says no)
    ("recompute", "bn1_recompute_0"): {"sums-only", "recomputed apply"},
    ("recompute", "guard_fb_conv1"): {"sums-only"},
    ("recompute", "one_stream_no_parking"): {"parked", "second stream"},
    ("recompute", "wgrad_side_0"): {"second stream"},
    ("pair", "sc_compact_0"): {"addend", "compact"},
    ("pair", "guard_fb_conv1"): {"addend", "compact"},
    ("stem", "defaults"): {"parameters only"},
}
