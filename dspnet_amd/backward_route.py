"""What a Conv and the BatchNorm in front of it launch in ONE backward pass, decided from the facts of that pass.

graph_plan.py decides once, from the graph's structure, which nodes MAY take a route (its marks: bn_bwd_node, sc_pair,
bn1_recompute, dx_planes).  The two functions here decide every pass, from those marks, the engine's knobs and the state of
the pass, which route a node DOES take; engine.py gathers the facts (Conv._facts, BatchNorm._facts) and runs what comes back.
Nothing here launches, allocates or mutates, and nothing outside the standard library is imported: every route can be
tested without a device (tests/test_backward_route.py)."""
from typing import NamedTuple, Tuple

# steps of a convolution's backward, in the order the route lists them
WGRAD, ISG, DGRAD, PARK = "weight gradient", "input-sum gradient", "data gradient", "park the BatchNorm finalize"
# where the weight gradient runs
ON_STREAM, ON_SIDE, NO_WGRAD = "the step's stream", "the second stream", "no weight gradient"
# which data gradient runs
NO_DGRAD = "none"
FULL = "full"                      # the first writer of x's gradient, or accumulating
ADDEND = "full + strided addend"   # ... reading the compact gradient the pair's shortcut left
FALLBACK = "guard fallback"        # the three-piece math
SUMS_ONLY = "sums only"            # the gradient is not stored: bn's backward forms it again
COMPACT = "compact shortcut"       # the stride-1 product on the subsampled grid, into Graph.sc_compact_buf


class ConvFacts(NamedTuple):
    # the node, and the marks graph_plan left
    stride: int
    bn_bwd_node: bool              # its data gradient gathers a BatchNorm's backward sums
    sc_pair: bool                  # a member of a (conv1, projection shortcut) pair
    bn1_recompute: bool
    bn_dx_planes: bool             # bn_bwd_node.dx_planes
    bn_x_requires_grad: bool       # bn_bwd_node.x.requires_grad
    w_fixed: bool
    x_requires_grad: bool
    input_sum_grad: bool           # a Param takes sum_pixels(dx) and is not frozen
    tap_expand: bool
    cuda: bool
    compact_buf: bool              # Graph.sc_compact_buf exists
    # the knobs, as they stand at this call
    wgrad_side: bool               # engine.WGRAD_SIDE
    wgrad_side_allowed: bool       # Graph.wgrad_side_allowed
    finalize_beside: bool          # engine.FINALIZE_BESIDE
    sc_compact: bool               # engine.SC_COMPACT
    bn1_recompute_knob: int        # engine.BN1_RECOMPUTE: 0, 1, 2
    bn_chain: bool                 # Graph.batchnorm_chain()
    wgrad_worth: bool              # Conv._wgrad_worth_a_stream()
    on_branch_stream: bool
    # the pass
    guard_fb: bool
    pair_guard_fb: bool
    dy_planes: bool
    x_written: bool                # x's gradient has a writer already
    pair_out_written: bool         # (the stride-2 member) conv1's output gradient exists
    have_addend: bool              # x.sc_compact: the pair's shortcut left its gradient compact
    bn_pooled: bool                # the hand-off record of bn_bwd_node: a pooled gradient waits / its finalize is parked
    bn_parked: bool
    recompute_pays: bool           # engine.bn1_recompute_pays(M, C, K)
    addend_kernel: bool            # functional.conv2d_dgrad_addend_route, asked for the stride-2 member of a pair only
    recompute_kernel: bool         # functional.conv2d_dgrad_recompute_route, asked for marked nodes only


class ConvRoute(NamedTuple):
    steps: Tuple[str, ...]
    wgrad: str
    dgrad: str
    hands_sums: bool               # the data gradient gathers bn_bwd_node's sums and says so in its hand-off record
    claims_dyin: bool              # ... and leaves the magnitude of what it stores in that node's am_dyin slot


def conv_route(f):
    """Everything Conv.backward does behind its prologue (ReLU mask, bias gradient, magnitudes)."""
    gathers = f.bn_bwd_node and f.x_requires_grad
    dgrad = _data_gradient(f, gathers)
    isg = (ISG,) if f.input_sum_grad else ()
    dg = (DGRAD,) if dgrad != NO_DGRAD else ()
    if f.w_fixed:
        # no weight gradient: nothing for a BatchNorm finalize to ride in (it runs on its own) and no second stream
        steps, wgrad = isg + dg, NO_WGRAD
    elif (f.wgrad_side and f.wgrad_side_allowed and f.cuda and (gathers or f.bn_chain) and f.wgrad_worth
          and not f.on_branch_stream and not f.tap_expand):
        # beside the chain: nothing to ride in, and the finalize's gap is filled
        steps, wgrad = (WGRAD,) + isg + dg, ON_SIDE
    elif gathers and f.finalize_beside and not f.guard_fb and f.cuda and not f.bn_pooled:
        # the data gradient goes FIRST and the finalize of the BatchNorm in front rides in the weight gradient's launch
        steps, wgrad = (DGRAD, PARK, WGRAD) + isg, ON_STREAM
    else:
        steps, wgrad = (WGRAD,) + isg + dg, ON_STREAM
    return ConvRoute(steps, wgrad, dgrad, gathers, gathers and f.bn_dx_planes)


def _data_gradient(f, gathers):
    if not f.x_requires_grad:
        return NO_DGRAD
    if (f.sc_pair and f.stride == 2 and f.sc_compact and not f.guard_fb and not f.pair_guard_fb and not f.dy_planes
            and not f.x_written and f.pair_out_written and f.compact_buf and f.addend_kernel):
        assert not f.bn_bwd_node, "conv1, not the shortcut, gathers the sums of the pair's BatchNorm"
        return COMPACT
    # the addend was left for a first, only writer that gathers sums in the two-piece math
    assert not f.have_addend or (not f.x_written and not f.guard_fb and f.bn_bwd_node)
    if (gathers and f.bn1_recompute and f.bn1_recompute_knob and not f.x_written and not f.guard_fb and f.dy_planes and f.cuda
            and f.bn_x_requires_grad and not f.bn_pooled and not f.bn_dx_planes and not f.bn_parked
            and (f.bn1_recompute_knob >= 2 or f.recompute_pays) and f.recompute_kernel):
        assert not f.have_addend, "graph_plan marks no node for both the recompute and the compact shortcut"
        return SUMS_ONLY
    if f.guard_fb:
        return FALLBACK
    return ADDEND if f.have_addend else FULL


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm.backward / BatchNorm.finalize_beside
NOTHING = "nothing"
APPLY_PARKED = "apply half of a parked finalize"
POOLED = "pooling-folded"
FROM_SUMS_PLANES = "from sums, dx as piece planes"
FROM_SUMS = "from sums"
STANDALONE = "stand-alone"
# the finalize of a from-sums route
PARKED, ALONE, WITH_APPLY = "parked", "alone", "with the apply"
# its apply half
KERNEL, RECOMPUTE, NO_APPLY = "kernel", "recomputed data gradient", "no apply"


class BnFacts(NamedTuple):
    beside: bool                   # asked by finalize_beside (the gathering convolution, before its weight gradient)
    x_requires_grad: bool
    dx_planes: bool                # the mark of graph_plan.gradient_planes
    cuda: bool
    finalize_beside: bool          # engine.FINALIZE_BESIDE
    out_written: bool              # the output's gradient exists
    x_written: bool                # x's gradient has a writer already
    takes_magnitude: bool          # this call completes x's gradient and leaves its magnitude (a slot exists)
    x_ext_valid: bool              # the per-channel extremes of x are this step's
    producer_guard_fb: bool        # the convolution that reads dx is on the range guard's fallback
    # the hand-off record
    sums_ready: bool
    pooled: bool
    parked: bool
    recompute: bool                # the data gradient that gathered the sums stored nothing


class BnRoute(NamedTuple):
    kind: str
    unpool_first: bool = False     # a second writer: the pooling backward materialised first
    finalize: str = ""             # the from-sums routes
    apply: str = NO_APPLY          # the from-sums routes and APPLY_PARKED
    writes_dx: bool = False        # (parameters only: none)


def bn_route(f):
    acc = f.x_requires_grad and f.x_written
    apply = RECOMPUTE if f.recompute else KERNEL
    if f.beside:
        # (parameters only is the finalize alone: no apply half to park it for)
        if (not f.finalize_beside or not f.cuda or not f.sums_ready or f.pooled or not f.out_written or f.parked
                or not f.x_requires_grad):
            return BnRoute(NOTHING)
        return BnRoute(_from_sums_kind(f, acc), False, PARKED, apply, True)
    if f.parked:
        return BnRoute(APPLY_PARKED, apply=apply, writes_dx=True)
    if not f.out_written:
        return BnRoute(NOTHING)
    if f.pooled and not acc:
        return BnRoute(POOLED, writes_dx=f.x_requires_grad)
    assert not f.recompute or (f.sums_ready and f.x_requires_grad), "a sums-only data gradient without its sums, or without a dx"
    if not f.sums_ready:
        return BnRoute(STANDALONE, f.pooled, writes_dx=f.x_requires_grad)
    if not f.x_requires_grad:
        return BnRoute(FROM_SUMS, f.pooled, WITH_APPLY, NO_APPLY, False)
    # (the gradient was never stored: the finalize now, the apply pass in the data gradient that forms it again)
    return BnRoute(_from_sums_kind(f, acc), f.pooled, ALONE if f.recompute else WITH_APPLY, apply, True)


def _from_sums_kind(f, acc):
    """dx leaves as fp16 piece planes where the plan marked the node, this call is the first and last writer and the reader
    multiplies planes (a convolution on the guard's fallback reads a FLOAT gradient)"""
    planes = f.dx_planes and f.takes_magnitude and not acc and f.x_ext_valid and not f.producer_guard_fb
    return FROM_SUMS_PLANES if planes else FROM_SUMS
