"""What Graph.finalize() decides from the graph's structure before anything runs.  Every pass reads ONE index of who reads
and who writes which tensor, built once from the nodes' wiring records (engine.Wiring: a node's outputs are the tensors its
constructor made, everything else it holds is a read); Graph keeps state and execution."""
import os

import torch

from . import engine as E, functional as fn


class WiringIndex:
    """tensor -> its readers and its writer over a complete node list; keys are id()s of engine Tensors"""

    def __init__(self, nodes):
        self.readers, self.writer = {}, {}     # -> [(node index, attribute)] in node order / -> node index
        for i, n in enumerate(nodes):
            for t in n.wiring.outputs:
                self.writer[id(t)] = i
            for k, t in n.wiring.reads:
                self.readers.setdefault(id(t), []).append((i, k))

    def reader_nodes(self, t, skip=()):
        """indices of the nodes that hold t as an input under an attribute not in `skip`"""
        return {i for i, k in self.readers.get(id(t), ()) if k not in skip}

    def first_reader(self, t):
        return min(self.reader_nodes(t), default=None)

    def repoint(self, i, node, attr, old, new):
        """node (index i) now holds `new` -- a tensor it already reads -- under `attr`: the one rewiring after Graph.add()"""
        node.wiring.reads[node.wiring.reads.index((attr, old))] = (attr, new)
        self.readers[id(old)].remove((i, attr))
        self.readers[id(new)] = sorted(self.readers[id(new)] + [(i, attr)])


def plan(g):      # (the passes in the order their decisions build on each other)
    index = WiringIndex(g.nodes)
    resolve_auto_deferred(g, index)
    side_sync(g, index)
    if os.environ.get("DSPN_X_PLANES", "1") != "0":       # (A/B switch)
        input_planes(g)
    bn_backward_fusion(g, index)
    gradient_magnitudes(g, index)
    if os.environ.get("DSPN_DY_PLANES", "1") != "0":      # (A/B switch)
        gradient_planes(g, index)
    shortcut_compaction(g, index)
    bn1_recompute(g, index)


def resolve_auto_deferred(g, index):
    """BatchNorm(defer_apply="auto"): keep the output virtual only if every reader is a plain convolution input;
    otherwise (a concat, a pooling layer, a residual operand ...) materialise it and unhook the convolutions."""
    def applies_in_loader(m, k, t):
        # bf16 tensors: a multi-tap convolution would re-apply the affine once per tap on a main loop that
        # is 3x shorter than in fp32 (scratch/fuse_cost.py bf16: +45 %); its input is materialised instead
        return (isinstance(m, E.Conv) and k == "x" and not m.tap_expand and not
                (E.MATERIALISE_MULTITAP_INPUT_BF16 and t.dtype == torch.bfloat16 and m.w.shape[1] * m.w.shape[2] > 1))

    for n in g.nodes:
        if not isinstance(n, E.BatchNorm) or n.defer_apply != "auto":
            continue
        # (x_raw: a convolution reading THROUGH another deferred BatchNorm reads that one's input, not this output as it is)
        rs = [(g.nodes[i], k) for i, k in index.readers.get(id(n.out), ()) if k != "x_raw"]
        if rs and all(applies_in_loader(m, k, n.out) for m, k in rs):
            n.defer_apply = True
            continue
        n.defer_apply = False
        n.out.affine_src = None
        n.out.data = fn.zeros(*n.out.shape, device=g.device, dtype=n.out.dtype)
        for c in n.conv_consumers:
            index.repoint(g.nodes.index(c), c, "x_raw", c.x_raw, c.x)
            c.x_raw, c.in_affine = c.x, None
        n.mat_consumers = list(n.conv_consumers)     # still candidates for gathering the backward reductions
        n.conv_consumers = []


def bn_backward_fusion(g, index):
    """For every BatchNorm whose output only convolutions read: the convolution that runs LAST in backward (the
    first in forward order) gathers the BatchNorm-backward reductions in its data-gradient epilogue."""
    for n in g.nodes:
        if not isinstance(n, E.BatchNorm) or not n.out.requires_grad:
            continue
        cons = n.conv_consumers if n.defer_apply else n.mat_consumers
        # every reader of the tensor: the convolutions must be the ONLY readers of a materialised BatchNorm output
        if not cons or (not n.defer_apply and index.reader_nodes(n.out) != {g.nodes.index(c) for c in cons}):
            continue
        last = min(cons, key=g.nodes.index)
        if last.stride not in (1, 2) or (last.stride == 2 and last.dil != 1) or last.x.shape[3] % 4 != 0:
            continue
        tiles = fn.conv_dgrad_bn_tiles(last.x.shape, last.stride)
        if tiles <= 0:
            continue
        n.bwd_sums = (fn.zeros(tiles, 2, last.x.shape[3], device=g.device), tiles)
        n.bwd_ws = fn.bn_from_sums_workspace(tiles, n.x.shape[-1], g.device)
        last.bn_bwd_node = n


def gradient_magnitudes(g, index):
    """"f16x2" math: a BatchNorm whose backward is the LAST writer of its input's gradient (backward runs the nodes in
    reverse: the reader with the smallest index) stores the complete gradient, so its apply kernel can also take the
    magnitude the producing convolution needs (BatchNorm.completes_x_grad)."""
    for idx, n in enumerate(g.nodes):
        if isinstance(n, E.BatchNorm):
            n.completes_x_grad = index.first_reader(n.x) == idx
        # a convolution read by nothing but another convolution's residual add (the projection shortcut of a unit) receives
        # that convolution's output gradient itself (Tensor.give_grad aliases it): one magnitude slot serves both
        elif isinstance(n, E.Conv) and n.am_dy is not None and n.residual is not None and n.residual.requires_grad:
            r, prod = n.residual, n.residual.producer
            if (prod is not None and prod.am_dy is not None and prod.out is r and index.reader_nodes(r) == {idx}
                    and not prod.relu and prod.b is None):
                prod.am_dy = n.am_dy


def gradient_planes(g, index):
    """"f16x2" math, round 4: a BatchNorm whose backward (from the sums its consumer's data gradient gathered) is the ONLY
    writer of its input's gradient, and whose input is the dense output of a plain convolution, writes that gradient as
    fp16 piece planes -- same buffer, same bytes -- cut by a bound it forms beforehand (dspn_bn_backward_from_sums_f32,
    dx_planes); the convolution's data gradient and weight gradient then copy their dy operand instead of cutting it
    once per tap and column tile.  In the residual units: bn2 -> conv1 and bn3 -> conv2."""
    if g.math != "f16x2" or g.device.type != "cuda":
        return
    gatherer = {id(n.bn_bwd_node): n for n in g.nodes if isinstance(n, E.Conv) and n.bn_bwd_node is not None}
    for idx, n in enumerate(g.nodes):
        if not isinstance(n, E.BatchNorm) or n.bwd_sums is None or id(n) not in gatherer:
            continue
        prod, x = n.x.producer, n.x
        # (x_raw: a convolution reading THROUGH a deferred BatchNorm; the gradient goes to the BatchNorm)
        if not (prod is not None and prod.out is x and index.reader_nodes(x, skip=("x_raw",)) == {idx} and x.requires_grad
                and x.dtype == torch.float32 and n.completes_x_grad and n.tile_stats is not None):
            continue
        if (prod.tap_expand or prod.relu or prod.b is not None or prod.residual is not None or prod.input_sum_grad is not None
                or prod.am_dy is None or x.shape[3] != prod.cout or prod.cout % 32 != 0 or prod.out_minmax is None
                or gatherer[id(n)].math != "f16x2"):
            continue
        n.dx_planes = True
        n.x_ext = fn.zeros(2, x.shape[3], device=g.device)
        n.am_dyin = g.mag.new(backward=True)


def shortcut_compaction(g, index):
    """The projection units of the ResNets: act1 feeds conv1 (1 x 1, stride 1) and the shortcut (1 x 1, stride 2, pad 0), and
    conv1 -- built first -- is the last writer of act1's gradient and gathers bn1's backward sums.  The shortcut's data
    gradient is the stride-1 1 x 1 data gradient on the subsampled grid; written at full resolution it is three quarters
    zeros that conv1's accumulate reads back.  Marked pairs keep it compact (backward_route.COMPACT) and conv1's data gradient
    adds it at the even positions (include/dspn_nn.h dspn_conv2d_dgrad_bn_sadd_f32).  A pair: the BatchNorm output's gradient
    has exactly these two writers, "f16x2" math, float tensors; whether a given pass takes the path is the nodes' decision."""
    if g.math != "f16x2" or g.device.type != "cuda":
        return
    largest = 0
    for n in g.nodes:
        if not isinstance(n, E.BatchNorm) or not n.out.requires_grad or n.out.dtype != torch.float32:
            continue
        readers = sorted(index.reader_nodes(n.out))
        if len(readers) != 2 or not all(isinstance(g.nodes[i], E.Conv) and g.nodes[i].x is n.out for i in readers):
            continue
        conv1, sc = g.nodes[readers[0]], g.nodes[readers[1]]
        one_by_one = lambda c: c.w.shape[1:3] == (1, 1) and c.pad == (0, 0) and c.dil == 1 and not c.tap_expand  # noqa: E731
        if not (one_by_one(conv1) and conv1.stride == 1 and conv1.bn_bwd_node is n and conv1.math == "f16x2"
                and one_by_one(sc) and sc.stride == 2 and sc.math == "f16x2" and sc.input_sum_grad is None
                and conv1.input_sum_grad is None and n.out.shape[3] == conv1.w.shape[3]):
            continue
        conv1.sc_pair, sc.sc_pair = sc, conv1
        N, H, W, C = n.out.shape
        largest = max(largest, N * ((H + 1) // 2) * ((W + 1) // 2) * C)
    if largest:
        g.sc_compact_buf = fn.zeros(largest, device=g.device)


def bn1_recompute(g, index):
    """The dim-match residual units: bn1 reads the residual stream and conv1 (1 x 1, stride 1, C -> C / 4) alone reads bn1's
    output, so the gradient of that output has ONE writer -- conv1's data gradient, which gathers bn1's backward sums -- and ONE
    reader, bn1's backward.  Marked pairs may leave it unwritten: the data gradient runs for the sums alone and again with the
    apply pass in its epilogue (include/dspn_nn.h dspn_conv2d_dgrad_bn_sums_f32 / _apply_f32).  A pair: "f16x2" math, float
    tensors, bn1's dx a float tensor (not piece planes) that is wanted, no projection shortcut beside conv1 (that is an
    sc_pair); whether a given pass takes the route is decided per pass (backward_route.conv_route)."""
    if g.math != "f16x2" or g.device.type != "cuda":
        return
    for idx, c in enumerate(g.nodes):
        n = c.bn_bwd_node if isinstance(c, E.Conv) else None
        if n is None or c.sc_pair is not None or c.math != "f16x2" or n.out.dtype != torch.float32:
            continue
        if not (c.w.shape[1:3] == (1, 1) and c.stride == 1 and c.pad == (0, 0) and c.dil == 1 and not c.tap_expand
                and c.input_sum_grad is None and c.x is n.out and n.out.shape[3] == c.w.shape[3]):
            continue
        if index.reader_nodes(n.out) != {idx} or n.dx_planes or not n.x.requires_grad:
            continue
        c.bn1_recompute = True


def input_planes(g):
    """"f16x2" math, round 4: a deferred BatchNorm whose readers re-read it often (X_PLANES_MIN_READS) also writes
    (relu)(x * scale + shift) as fp16 piece planes (dspn_bn_apply_planes_f32), cut by the magnitude its statistics finalize
    has just formed; that convolution's forward and weight gradient then copy their x operand into LDS instead of applying
    the affine and cutting every element once per (tap, column tile) -- 9 x Cout / 128 times for a 3 x 3.  The 1 x 1 readers
    (and the BatchNorm backward) keep reading the raw tensor.  In the residual units: bn2 -> conv2."""
    if g.math != "f16x2" or g.device.type != "cuda":
        return
    for n in g.nodes:
        if not isinstance(n, E.BatchNorm) or n.defer_apply is not True or n.tile_stats is None:
            continue
        x = n.x
        if (x.dtype != torch.float32 or x.shape[3] % 32 != 0 or x.data is None
                or x.producer is None or x.producer.out_minmax is None):
            continue
        cons = [c for c in n.conv_consumers if c.math == "f16x2" and c.wp is not None and c.x_raw is x]
        # how often the tile loaders would apply the affine to (and cut) one element: once per tap and 128-column tile
        reads = sum(c.w.shape[1] * c.w.shape[2] * ((c.cout + 127) // 128) for c in cons)
        if reads < E.X_PLANES_MIN_READS:
            continue
        n.planes = fn.zeros(*x.shape, device=g.device)
        for c in cons:
            c.x_planes_bn = n


def side_sync(g, index):
    """The builder only says WHICH nodes run beside the main stream; what orders the two streams is derived here from the
    tensors the nodes hold, so that a preset whose wiring differs (vgg16_reduced, inceptionv3, resnet-101: the decoder
    reads an SSD extra layer's output, symbol/multitask_symbol_builder.py `conv_feat`) cannot silently become a race:
    * forward: a main-stream node behind the segment that holds a tensor written inside it waits for an event recorded
      behind the in-segment node that writes (or, failing that, last holds) that tensor -- not for the whole branch;
    * backward: a node leaves the side set if it shares a tensor with a main-stream node that runs between the fork and
      itself (the decoder writes that tensor's gradient on the main stream while the side stream, which only waits for
      the fork event, would read or accumulate into it), repeated until nothing changes."""
    plan = g.side_plan
    g.side_fwd_events, g.side_fwd_waits = {}, {}
    if plan is None:
        return
    first, last = plan["first"], plan["last"]
    cuda = g.side_segment is not None
    refs = [g._node_tensors(n) for n in g.nodes]
    holders = {}
    for i, ts in enumerate(refs):
        for t in ts:
            holders.setdefault(id(t), []).append(i)
    before = {id(t) for ts in refs[:first] for t in ts}
    for tid, idxs in holders.items():
        inside = [i for i in idxs if first <= i <= last]
        outside = [i for i in idxs if i > last]
        if not inside or not outside or tid in before:
            continue
        # no writer among the nodes (a tensor the builder made): behind the LAST in-segment holder, which is safe whichever
        # of them writes
        src = index.writer.get(tid)
        if src not in inside:
            src = max(inside)
        if src not in g.side_fwd_events:
            g.side_fwd_events[src] = torch.cuda.Event() if cuda else None
        for r in outside:
            w = g.side_fwd_waits.setdefault(r, [])
            if src not in w:
                w.append(src)
    plan["fwd_waits"] = {r: list(w) for r, w in g.side_fwd_waits.items()}
    sb = plan["bwd"]
    if sb is None:
        return
    side, fork_after = set(sb["side"]), sb["fork_after"]
    has_bwd = [type(n).backward is not E.Node.backward for n in g.nodes]
    changed = True
    while changed:
        changed = False
        for i in sorted(side):
            mine = {id(t) for t in refs[i]}
            for x in range(i + 1, fork_after):
                if x in side or not has_bwd[x]:
                    continue
                if mine & {id(t) for t in refs[x]}:
                    side.discard(i)
                    changed = True
                    break
    sb["removed"] = frozenset(sb["side"]) - side
    sb["side"] = frozenset(side)
    if g.side_bwd is not None:
        g.side_bwd["side"] = frozenset(side)
        if not side:
            g.side_bwd = None
