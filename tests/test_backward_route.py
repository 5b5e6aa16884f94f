"""dspnet_amd/backward_route.py: which launches a Conv and the BatchNorm in front of it make in one backward pass, as a pure
function of the facts of that pass.  No device, no torch.

(a) A table of named cases, one per route the engine takes today, each asserting the whole route record.
(b) An exhaustive sweep.  A route function that never reads a fact cannot depend on it, so the sweep walks the decision tree:
    a facts object that reports the first field read without a value, both values tried in turn (BN1_RECOMPUTE: 0, 1, 2;
    stride: 1, 2).  Every leaf is a set of full assignments that share one route, and together the leaves are all of them.
    An invariant that needs a fact the leaf never read fails, because some assignment of the leaf then breaks it."""
import itertools

import pytest

from dspnet_amd import backward_route as R

CONV = R.ConvFacts(
    stride=1, bn_bwd_node=False, sc_pair=False, bn1_recompute=False, bn_dx_planes=False, bn_x_requires_grad=False, w_fixed=False,
    x_requires_grad=True, input_sum_grad=False, tap_expand=False, cuda=True, compact_buf=False, wgrad_side=True,
    wgrad_side_allowed=True, finalize_beside=True, sc_compact=True, bn1_recompute_knob=1, bn_chain=True, wgrad_worth=False,
    on_branch_stream=False, guard_fb=False, pair_guard_fb=False, dy_planes=False, x_written=False, pair_out_written=False,
    have_addend=False, bn_pooled=False, bn_parked=False, recompute_pays=False, addend_kernel=False, recompute_kernel=False)
GATHERS = dict(bn_bwd_node=True, bn_x_requires_grad=True)                        # a convolution behind a deferred BatchNorm
CONV1_OF_UNIT = dict(GATHERS, bn1_recompute=True, dy_planes=True, recompute_kernel=True)     # conv1 of a dim-match unit
SHORTCUT = dict(sc_pair=True, stride=2, compact_buf=True, pair_out_written=True, addend_kernel=True)
W, I, D, P = R.WGRAD, R.ISG, R.DGRAD, R.PARK

CONV_CASES = {
    # the four step orders
    "frozen weight": (dict(w_fixed=True, input_sum_grad=True), R.ConvRoute((I, D), R.NO_WGRAD, R.FULL, False, False)),
    "frozen weight, a gathered BatchNorm: its finalize is not parked":
        (dict(GATHERS, w_fixed=True), R.ConvRoute((D,), R.NO_WGRAD, R.FULL, True, False)),
    "weight gradient on the second stream": (dict(GATHERS, wgrad_worth=True, input_sum_grad=True),
                                             R.ConvRoute((W, I, D), R.ON_SIDE, R.FULL, True, False)),
    "second stream without a BatchNorm, in a BatchNorm chain": (dict(wgrad_worth=True), R.ConvRoute((W, D), R.ON_SIDE, R.FULL, False, False)),
    "no BatchNorm chain: the step's stream": (dict(wgrad_worth=True, bn_chain=False), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, False, False)),
    "the branch stream keeps its weight gradients": (dict(GATHERS, wgrad_worth=True, on_branch_stream=True),
                                                     R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "a tap-expanded node keeps its weight gradient": (dict(wgrad_worth=True, tap_expand=True), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, False, False)),
    "a solver with an all-reduce: one stream": (dict(GATHERS, wgrad_worth=True, wgrad_side_allowed=False),
                                                R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "finalize riding": (dict(GATHERS, input_sum_grad=True), R.ConvRoute((D, P, W, I), R.ON_STREAM, R.FULL, True, False)),
    "finalize riding, dx of the BatchNorm as planes": (dict(GATHERS, bn_dx_planes=True), R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, True)),
    "otherwise": (dict(input_sum_grad=True), R.ConvRoute((W, I, D), R.ON_STREAM, R.FULL, False, False)),
    "FINALIZE_BESIDE off": (dict(GATHERS, finalize_beside=False), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, True, False)),
    "a pooled gradient waits at the BatchNorm: nothing parked": (dict(GATHERS, bn_pooled=True), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, True, False)),
    "a CPU graph": (dict(GATHERS, cuda=False, wgrad_worth=True), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, True, False)),
    "the input needs no gradient": (dict(GATHERS, x_requires_grad=False, input_sum_grad=True),
                                    R.ConvRoute((W, I), R.ON_STREAM, R.NO_DGRAD, False, False)),
    # each data-gradient kind
    "accumulating": (dict(GATHERS, x_written=True), R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "strided addend": (dict(GATHERS, sc_pair=True, have_addend=True, dy_planes=True), R.ConvRoute((D, P, W), R.ON_STREAM, R.ADDEND, True, False)),
    "guard fallback": (dict(GATHERS, guard_fb=True, bn_dx_planes=True), R.ConvRoute((W, D), R.ON_STREAM, R.FALLBACK, True, True)),
    "sums only, forced": (dict(CONV1_OF_UNIT, bn1_recompute_knob=2), R.ConvRoute((D, P, W), R.ON_STREAM, R.SUMS_ONLY, True, False)),
    "sums only, where it pays": (dict(CONV1_OF_UNIT, recompute_pays=True), R.ConvRoute((D, P, W), R.ON_STREAM, R.SUMS_ONLY, True, False)),
    "sums only beside a weight gradient on the second stream":
        (dict(CONV1_OF_UNIT, recompute_pays=True, wgrad_worth=True), R.ConvRoute((W, D), R.ON_SIDE, R.SUMS_ONLY, True, False)),
    "marked, but the layer does not pay": (CONV1_OF_UNIT, R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "marked, knob off": (dict(CONV1_OF_UNIT, recompute_pays=True, bn1_recompute_knob=0), R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "marked, no kernel for the call": (dict(CONV1_OF_UNIT, bn1_recompute_knob=2, recompute_kernel=False),
                                       R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "marked, a float gradient": (dict(CONV1_OF_UNIT, bn1_recompute_knob=2, dy_planes=False), R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "marked, on the guard's fallback": (dict(CONV1_OF_UNIT, bn1_recompute_knob=2, guard_fb=True), R.ConvRoute((W, D), R.ON_STREAM, R.FALLBACK, True, False)),
    "marked, the BatchNorm writes no dx": (dict(CONV1_OF_UNIT, bn1_recompute_knob=2, bn_x_requires_grad=False),
                                           R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
    "compact shortcut": (SHORTCUT, R.ConvRoute((W, D), R.ON_STREAM, R.COMPACT, False, False)),
    "compact shortcut, frozen weight": (dict(SHORTCUT, w_fixed=True), R.ConvRoute((D,), R.NO_WGRAD, R.COMPACT, False, False)),
    "SC_COMPACT off": (dict(SHORTCUT, sc_compact=False), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, False, False)),
    "shortcut, conv1 on the guard's fallback": (dict(SHORTCUT, pair_guard_fb=True), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, False, False)),
    "shortcut on the guard's fallback": (dict(SHORTCUT, guard_fb=True), R.ConvRoute((W, D), R.ON_STREAM, R.FALLBACK, False, False)),
    "shortcut, no kernel takes the addend": (dict(SHORTCUT, addend_kernel=False), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, False, False)),
    "shortcut, conv1 has no gradient to propagate": (dict(SHORTCUT, pair_out_written=False), R.ConvRoute((W, D), R.ON_STREAM, R.FULL, False, False)),
    "conv1 of the pair does not take the compact kind": (dict(GATHERS, **dict(SHORTCUT, stride=1)), R.ConvRoute((D, P, W), R.ON_STREAM, R.FULL, True, False)),
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_route(name):
    facts, route = CONV_CASES[name]
    assert R.conv_route(CONV._replace(**facts)) == route


BN = R.BnFacts(beside=False, x_requires_grad=True, dx_planes=False, cuda=True, finalize_beside=True, out_written=True,
               x_written=False, takes_magnitude=False, x_ext_valid=False, producer_guard_fb=False, sums_ready=False, pooled=False,
               parked=False, recompute=False)
PLANES = dict(sums_ready=True, dx_planes=True, takes_magnitude=True, x_ext_valid=True)

BN_CASES = {
    "no gradient arrived": (dict(out_written=False), R.BnRoute(R.NOTHING)),
    "stand-alone": (dict(), R.BnRoute(R.STANDALONE, writes_dx=True)),
    "stand-alone, parameters only": (dict(x_requires_grad=False), R.BnRoute(R.STANDALONE)),
    "from sums, floats": (dict(sums_ready=True), R.BnRoute(R.FROM_SUMS, False, R.WITH_APPLY, R.KERNEL, True)),
    "from sums, accumulating into the residual stream": (dict(PLANES, x_written=True), R.BnRoute(R.FROM_SUMS, False, R.WITH_APPLY, R.KERNEL, True)),
    "from sums, planes": (PLANES, R.BnRoute(R.FROM_SUMS_PLANES, False, R.WITH_APPLY, R.KERNEL, True)),
    "planes refused: the producer is on the guard's fallback": (dict(PLANES, producer_guard_fb=True),
                                                                R.BnRoute(R.FROM_SUMS, False, R.WITH_APPLY, R.KERNEL, True)),
    "planes refused: the extremes of x are not this step's": (dict(PLANES, x_ext_valid=False), R.BnRoute(R.FROM_SUMS, False, R.WITH_APPLY, R.KERNEL, True)),
    "from sums, parameters only": (dict(sums_ready=True, x_requires_grad=False), R.BnRoute(R.FROM_SUMS, False, R.WITH_APPLY, R.NO_APPLY, False)),
    "finalize now + recomputed apply": (dict(sums_ready=True, recompute=True, x_written=True), R.BnRoute(R.FROM_SUMS, False, R.ALONE, R.RECOMPUTE, True)),
    "park + kernel apply": (dict(beside=True, sums_ready=True), R.BnRoute(R.FROM_SUMS, False, R.PARKED, R.KERNEL, True)),
    "park + kernel apply, planes": (dict(PLANES, beside=True), R.BnRoute(R.FROM_SUMS_PLANES, False, R.PARKED, R.KERNEL, True)),
    "park + recomputed apply": (dict(beside=True, sums_ready=True, recompute=True, x_written=True), R.BnRoute(R.FROM_SUMS, False, R.PARKED, R.RECOMPUTE, True)),
    "nothing parked: FINALIZE_BESIDE off": (dict(beside=True, sums_ready=True, finalize_beside=False), R.BnRoute(R.NOTHING)),
    "nothing parked: parameters only": (dict(beside=True, sums_ready=True, x_requires_grad=False), R.BnRoute(R.NOTHING)),
    "nothing parked: a pooled gradient waits": (dict(beside=True, sums_ready=True, pooled=True), R.BnRoute(R.NOTHING)),
    "nothing parked: parked already": (dict(beside=True, sums_ready=True, parked=True), R.BnRoute(R.NOTHING)),
    "nothing parked: no sums": (dict(beside=True), R.BnRoute(R.NOTHING)),
    "the apply half of a parked finalize": (dict(parked=True), R.BnRoute(R.APPLY_PARKED, apply=R.KERNEL, writes_dx=True)),
    "the recomputed apply half of a parked finalize": (dict(parked=True, recompute=True), R.BnRoute(R.APPLY_PARKED, apply=R.RECOMPUTE, writes_dx=True)),
    "pooling fold": (dict(pooled=True), R.BnRoute(R.POOLED, writes_dx=True)),
    "pooling fold, parameters only": (dict(pooled=True, x_requires_grad=False), R.BnRoute(R.POOLED)),
    "pooling fold with a second writer, then stand-alone": (dict(pooled=True, x_written=True), R.BnRoute(R.STANDALONE, True, writes_dx=True)),
    "pooling fold with a second writer, then from sums": (dict(pooled=True, x_written=True, sums_ready=True),
                                                          R.BnRoute(R.FROM_SUMS, True, R.WITH_APPLY, R.KERNEL, True)),
}


@pytest.mark.parametrize("name", list(BN_CASES))
def test_bn_route(name):
    facts, route = BN_CASES[name]
    assert R.bn_route(BN._replace(**facts)) == route


# ---------------------------------------------------------------------------------------------------------------------
class Partial(dict):
    """facts with some fields still open: reading an open one raises KeyError(name)"""
    __getattr__ = dict.__getitem__


def values(record, name):
    return {"bn1_recompute_knob": (0, 1, 2), "stride": (1, 2)}.get(name, (False, True))


def leaves(fn, record, known=None):
    """every (known facts, route) of fn's decision tree; `known` pins facts from the start.  A leaf that ends in one of the
    route function's own asserts is a combination the engine cannot reach: (known facts, the AssertionError)"""
    known = dict(known or {})
    try:
        yield known, fn(Partial(known))
    except AssertionError as e:
        yield known, e
    except KeyError as u:
        name = u.args[0]
        assert name in record._fields
        for v in values(record, name):
            yield from leaves(fn, record, dict(known, **{name: v}))


def need(known, **facts):
    """the leaf read these facts and they are what the invariant says (an unread fact could be anything)"""
    return all(name in known and known[name] == v for name, v in facts.items())


CONV_LEAVES = list(leaves(R.conv_route, R.ConvFacts))
BN_LEAVES = list(leaves(R.bn_route, R.BnFacts))


def test_sweep_reaches_every_route_and_the_asserts_are_the_known_ones():
    routes = [r for _, r in CONV_LEAVES if isinstance(r, R.ConvRoute)]
    assert {r.dgrad for r in routes} == {R.NO_DGRAD, R.FULL, R.ADDEND, R.FALLBACK, R.SUMS_ONLY, R.COMPACT}
    assert {r.steps for r in routes} >= {(I, D), (W, I, D), (D, P, W, I), (D, P, W), (W,), (D,), ()}
    assert {r.wgrad for r in routes} == {R.ON_STREAM, R.ON_SIDE, R.NO_WGRAD}
    for known, r in CONV_LEAVES:
        if isinstance(r, AssertionError):      # the addend left for a call that is not a first, two-piece, gathering writer of
            # an unmarked node; the shortcut of a pair gathering the sums that graph_plan gives to conv1
            assert (known.get("have_addend") and (known["x_written"] or known["guard_fb"] or not known["bn_bwd_node"]
                                                  or known.get("bn1_recompute"))) or (known["sc_pair"] and known["stride"] == 2
                                                                                      and known["bn_bwd_node"])
    bn = [r for _, r in BN_LEAVES if isinstance(r, R.BnRoute)]
    assert {r.kind for r in bn} == {R.NOTHING, R.APPLY_PARKED, R.POOLED, R.FROM_SUMS_PLANES, R.FROM_SUMS, R.STANDALONE}
    for known, r in BN_LEAVES:
        if isinstance(r, AssertionError):      # operands of a recomputed apply without sums or without a dx to write
            assert known["recompute"] and not (known.get("sums_ready") and known["x_requires_grad"])


def test_conv_invariants_hold_on_every_leaf():
    for known, r in CONV_LEAVES:
        if isinstance(r, AssertionError):
            continue
        # a route is its steps: one of each at most, the weight gradient and the data gradient exactly where they are wanted
        assert len(set(r.steps)) == len(r.steps)
        assert (W in r.steps) == (r.wgrad != R.NO_WGRAD) and (D in r.steps) == (r.dgrad != R.NO_DGRAD)
        assert (r.wgrad == R.NO_WGRAD) == known["w_fixed"]
        assert (r.dgrad != R.NO_DGRAD) == known["x_requires_grad"]
        assert (I in r.steps) == known["input_sum_grad"]
        # a frozen weight: no weight-gradient step and no parked finalize
        if known["w_fixed"]:
            assert W not in r.steps and P not in r.steps
        # a parked finalize: directly behind a data gradient that handed over sums, in front of a weight gradient on the step's
        # stream, on a node that is not on the guard's fallback
        if P in r.steps:
            i = r.steps.index(P)
            assert i > 0 and r.steps[i - 1] == D and r.steps[i + 1] == W and r.hands_sums and r.wgrad == R.ON_STREAM
            assert need(known, guard_fb=False, finalize_beside=True, cuda=True, bn_pooled=False)
        if r.wgrad == R.ON_SIDE:
            assert P not in r.steps and r.steps[0] == W
            assert need(known, wgrad_side=True, wgrad_side_allowed=True, cuda=True, wgrad_worth=True, on_branch_stream=False, tap_expand=False)
        # the guard's fallback never takes the compact, addend or sums-only kinds
        if known.get("guard_fb"):
            assert r.dgrad in (R.NO_DGRAD, R.FALLBACK)
        if r.dgrad in (R.COMPACT, R.ADDEND, R.SUMS_ONLY):
            assert need(known, guard_fb=False)
        # the addend is read only by a first, non-accumulating writer that gathers sums
        if r.dgrad == R.ADDEND:
            assert need(known, have_addend=True, x_written=False, bn_bwd_node=True) and r.hands_sums
        # the compact kind: the stride-2 member of a pair, nothing yet in x's gradient, conv1 not on the fallback
        if r.dgrad == R.COMPACT:
            assert need(known, sc_pair=True, stride=2, x_written=False, sc_compact=True, pair_guard_fb=False, dy_planes=False,
                        pair_out_written=True, compact_buf=True, addend_kernel=True) and not r.hands_sums
        # sums only: a marked node, first writer, planes in, a BatchNorm that writes a float dx and has nothing waiting
        if r.dgrad == R.SUMS_ONLY:
            assert r.hands_sums and not r.claims_dyin
            assert need(known, bn1_recompute=True, x_written=False, dy_planes=True, cuda=True, bn_x_requires_grad=True, bn_pooled=False,
                        bn_dx_planes=False, bn_parked=False, recompute_kernel=True)
            assert known["bn1_recompute_knob"] == 2 or need(known, bn1_recompute_knob=1, recompute_pays=True)
        assert r.hands_sums == (known["x_requires_grad"] and known["bn_bwd_node"]) and not (r.hands_sums and r.dgrad == R.COMPACT)
        if r.claims_dyin:
            assert r.hands_sums and need(known, bn_dx_planes=True)


def test_bn_invariants_hold_on_every_leaf():
    for known, r in BN_LEAVES:
        if isinstance(r, AssertionError):
            continue
        from_sums = r.kind in (R.FROM_SUMS, R.FROM_SUMS_PLANES)
        assert (r.finalize != "") == from_sums
        if known["beside"]:      # finalize_beside parks or does nothing: never a launch of the apply half, never without sums
            assert r.kind == R.NOTHING or (from_sums and r.finalize == R.PARKED and need(known, sums_ready=True, x_requires_grad=True,
                                                                                         pooled=False, parked=False, out_written=True))
        else:
            assert r.finalize != R.PARKED
        # planes leave only where the plan marked the node, to a reader that is not on the guard's fallback, from a first writer
        if r.kind == R.FROM_SUMS_PLANES:
            assert need(known, dx_planes=True, takes_magnitude=True, x_ext_valid=True, producer_guard_fb=False, x_written=False)
        # the recompute operands and the recomputed apply go together
        if r.kind not in (R.NOTHING, R.POOLED) and "recompute" in known:
            assert (r.apply == R.RECOMPUTE) == known["recompute"]
        if r.apply == R.RECOMPUTE:
            assert need(known, recompute=True) and r.writes_dx and r.finalize in ("", R.ALONE, R.PARKED)
        if r.finalize == R.ALONE:
            assert r.apply == R.RECOMPUTE
        # dx is written exactly where it is wanted (APPLY_PARKED: the route that parked it checked)
        if r.kind not in (R.NOTHING, R.APPLY_PARKED):
            assert r.writes_dx == known["x_requires_grad"] and (r.apply != R.NO_APPLY) == (from_sums and r.writes_dx)
        if r.unpool_first:
            assert need(known, pooled=True, x_written=True, x_requires_grad=True)


def test_a_conv_and_its_batchnorm_produce_every_wanted_gradient_exactly_once():
    """the two routes of one pass, chained through the hand-off record: the convolution's route, finalize_beside if its route
    parks, then the BatchNorm's backward.  dx of the BatchNorm is written once if wanted and never otherwise; a gradient
    that was not stored (sums only) is never read by the apply kernel or the stand-alone call, and the reverse."""
    carried = ("bn_x_requires_grad", "bn_dx_planes", "cuda", "finalize_beside", "bn_pooled")
    free = ("x_written", "takes_magnitude", "x_ext_valid", "producer_guard_fb")
    passes = set()      # (the carried facts, the convolution parks, its data gradient stored nothing) of every leaf that hands sums
    for known, r in CONV_LEAVES:
        if isinstance(r, AssertionError) or not r.hands_sums or known.get("bn_parked"):
            continue      # (a finalize parked from an earlier convolution: the BatchNorm's own apply half comes first)
        open_ = [c for c in carried if c not in known]
        for extra in itertools.product((False, True), repeat=len(open_)):
            k = dict(known, **dict(zip(open_, extra)))
            passes.add(tuple(k[c] for c in carried) + (P in r.steps, r.dgrad == R.SUMS_ONLY))
    assert len(passes) >= 32 and {p[-2:] for p in passes} == set(itertools.product((False, True), repeat=2))
    for *k, parks, sums_only in passes:
        x_requires_grad, dx_planes, cuda, finalize_beside, pooled = k
        for fr in itertools.product((False, True), repeat=len(free)):
            facts = BN._replace(x_requires_grad=x_requires_grad, dx_planes=dx_planes, cuda=cuda, finalize_beside=finalize_beside,
                                out_written=True, sums_ready=True, pooled=pooled, recompute=sums_only, **dict(zip(free, fr)))
            if parks and R.bn_route(facts._replace(beside=True)).finalize == R.PARKED:
                facts = facts._replace(parked=True, sums_ready=False, x_written=True)
            last = R.bn_route(facts)
            assert last.kind != R.NOTHING
            assert (last.kind == R.APPLY_PARKED or last.writes_dx) == x_requires_grad
            reads_stored = last.apply == R.KERNEL or last.kind in (R.STANDALONE, R.POOLED)
            assert (last.apply == R.RECOMPUTE) == sums_only and not (reads_stored and sums_only)
