"""The ledger of the "f16x2" operand magnitudes (dspnet_amd/magnitudes.py) on its own, without a GPU: the ledger is
built on the CPU device; the stand-alone pass (functional.absmax) and the batched weight launches are stubbed and
counted -- no kernel runs."""
from types import SimpleNamespace

import pytest
import torch

from dspnet_amd import functional as fn
from dspnet_amd.magnitudes import Magnitudes

CPU = torch.device("cpu")
S = fn.ABSMAX_SLOTS


@pytest.fixture()
def launches(monkeypatch):
    """stubs of every launch the ledger issues; -> the log of (name, argument) in issue order"""
    log = []

    def absmax(x, in_affine=None, out=None):
        log.append(("absmax", x))
        out.fill_(float(x.abs().max()))
        return out
    monkeypatch.setattr(fn, "absmax", absmax)
    monkeypatch.setattr(fn, "absmax_table", lambda pairs, device: ("am", [o for _, o in pairs]))
    monkeypatch.setattr(fn, "absmin_rows_table", lambda pairs, device: ("wmin", [o for _, o in pairs]))
    monkeypatch.setattr(fn, "absmax_batch", lambda name, outs: (log.append(("absmax_batch", len(outs))), [o.fill_(2.0) for o in outs]))
    monkeypatch.setattr(fn, "absmin_rows_batch", lambda name, outs: (log.append(("absmin_rows_batch", len(outs))), [o.fill_(0.5) for o in outs]))
    return log


def weight_node(mag, fixed):
    w = SimpleNamespace(fixed=fixed, data=torch.ones(4, 8), shape=(4, 8))
    return SimpleNamespace(w=w, am_w=mag.new())


def tensor(am_slot=None, alias_of=None):
    return SimpleNamespace(am_slot=am_slot, alias_of=alias_of)


def ledger(minima=True):
    """slots 0 x, 1 dy (backward), 2 w of a trained weight, 3 w of a frozen one (moves to 6), 4 dyin (backward), 5 out"""
    mag = Magnitudes("f16x2")
    x, dy = mag.new(), mag.new(backward=True)
    trained, frozen = weight_node(mag, False), weight_node(mag, True)
    dyin, out = mag.new(backward=True), mag.new()
    mag.allocate(CPU, [trained, frozen], minima=minima)
    return mag, SimpleNamespace(x=x, dy=dy, dyin=dyin, out=out, trained=trained, frozen=frozen)


def test_slots_are_numbered_in_creation_order_and_an_input_pair_shares_one():
    mag = Magnitudes("f16x2")
    assert [mag.new(), mag.new(backward=True), mag.new()] == [0, 1, 2]
    raw, scale, other = torch.zeros(1), torch.zeros(1), torch.zeros(1)
    assert mag.input_slot(raw, scale, create=False) is None
    a = mag.input_slot(raw, scale)
    assert a == 3 and mag.input_slot(raw, scale) == a and mag.input_slot(raw, scale, create=False) == a
    assert mag.input_slot(raw, other) == 4            # another affine of the same tensor: another magnitude
    assert mag.input_slot(raw, None) == 5 and mag.input_slot(raw, None) == 5
    assert mag.input_slot(other, scale) == 6
    assert mag.slots == 7


def test_frozen_weights_lie_behind_the_step_region_which_begin_step_resets(launches):
    mag, s = ledger()
    assert s.trained.am_w == 2 and s.frozen.am_w == 6 and mag.step_slots == 6 and mag.slots == 7
    assert mag.arena.numel() == 7 * S and mag.minima.numel() == 7
    assert not launches                               # allocate() builds tables, it launches nothing
    mag.refresh_frozen()
    assert launches == [("absmin_rows_batch", 1), ("absmax_batch", 1)]
    assert float(mag.block(6).min()) == 2.0 and float(mag.min_view(6)) == 0.5
    mag.claim(s.x).fill_(7.0)
    mag.min_view(s.x).fill_(0.25)
    del launches[:]
    mag.begin_step()
    assert launches == [("absmin_rows_batch", 1), ("absmax_batch", 1)]
    assert float(mag.arena[:2 * S].abs().max()) == 0.0 and float(mag.arena[3 * S:6 * S].abs().max()) == 0.0
    assert float(mag.block(s.trained.am_w).min()) == 2.0                 # (the trained weight's, taken by the batched launch)
    assert torch.isinf(mag.minima[:2]).all() and torch.isinf(mag.minima[3:6]).all() and float(mag.min_view(2)) == 0.5
    assert float(mag.block(6).min()) == 2.0 and float(mag.min_view(6)) == 0.5     # the frozen region: untouched
    # done: exactly the weight slots of the batched launches
    assert [i for i in range(mag.slots) if mag.done(i)] == [2, 6]
    del launches[:]
    mag.begin_step(minima=False)                      # (the guard asks for the weights' minima every few passes only)
    assert launches == [("absmax_batch", 1)]


def test_without_the_guard_no_minima_tables(launches):
    mag, s = ledger(minima=False)
    assert mag.wmin_table is None and mag.wmin_frozen is None and mag.am_table is not None and mag.am_frozen is not None
    mag.begin_step()
    mag.refresh_frozen()
    assert launches == [("absmax_batch", 1), ("absmax_batch", 1)]


def test_claim_marks_and_block_does_not(launches):
    mag, s = ledger()
    mag.begin_step()
    view = mag.block(s.x)
    assert view.numel() == S and view.data_ptr() == mag.arena[s.x * S:].data_ptr() and not mag.done(s.x)
    assert mag.claim(s.x).data_ptr() == view.data_ptr() and mag.done(s.x)
    assert mag.block(None) is None and mag.claim(None) is None and mag.min_view(None) is None and not mag.done(None)
    assert mag.min_view(s.x).data_ptr() == mag.minima[s.x:].data_ptr() and mag.min_view(s.x).numel() == 1


@pytest.mark.parametrize("math", ["bf16x3", "f16x2"])
def test_an_inactive_ledger_hands_out_nothing_and_marks_nothing(launches, math):
    """the other math modes never allocate; neither does an "f16x2" graph that is not on a GPU (no allocate() call)"""
    mag = Magnitudes(math)
    slot = mag.new(backward=True)
    if math != "f16x2":
        mag.allocate(CPU, [weight_node(mag, False)])
    assert not mag.active and mag.arena is None
    assert mag.block(slot) is None and mag.claim(slot) is None and mag.min_view(slot) is None
    assert mag.take(slot, torch.ones(4)) is None
    mag.begin_step(); mag.refresh_frozen(); mag.begin_backward(); mag.begin_backward()
    assert not mag.done(slot) and not launches
    assert mag.range_report() == (0, 0, 0.0)


def test_a_second_backward_pass_rezeroes_exactly_the_claimed_gradient_slots(launches):
    mag, s = ledger()
    mag.begin_step()
    mag.claim(s.x).fill_(3.0)
    mag.claim(s.out).fill_(4.0)
    mag.begin_backward()                              # the first pass after begin_step: nothing to retake
    assert float(mag.block(s.x).min()) == 3.0 and mag.done(s.x) and mag.done(s.out)
    mag.claim(s.dyin).fill_(5.0)                      # (the block a data gradient fills for the BatchNorm in front)
    mag.block(s.dy).fill_(6.0)                        # written but never claimed: not the ledger's to clear
    before = mag.arena.clone()
    mag.begin_backward()
    assert float(mag.block(s.dyin).abs().max()) == 0.0 and not mag.done(s.dyin) and not mag.done(s.dy)
    changed = (mag.arena != before).view(-1, S).any(dim=1).nonzero().flatten().tolist()
    assert changed == [s.dyin]
    assert float(mag.block(s.dy).min()) == 6.0
    assert [i for i in range(mag.slots) if mag.done(i)] == [s.x, s.trained.am_w, s.out, s.frozen.am_w]
    mag.claim(s.dy)
    mag.begin_step()                                  # a new forward pass: the next backward pass is a first one again
    mag.claim(s.dy).fill_(1.0)
    mag.begin_backward()
    assert mag.done(s.dy) and float(mag.block(s.dy).min()) == 1.0


def test_take_prefers_the_producers_block_and_passes_over_the_tensor_once_per_step(launches):
    mag, s = ledger()
    mag.begin_step()
    data = torch.full((2, 4), -3.0)

    def passes():
        return sum(name == "absmax" for name, _ in launches)
    src = tensor(am_slot=s.out)
    got = mag.take(s.x, data, src=src)                # nobody left a bound of the producer's output: a pass, into the reader's slot
    assert passes() == 1 and got.data_ptr() == mag.block(s.x).data_ptr() and float(got.max()) == 3.0
    assert mag.done(s.x) and not mag.done(s.out)
    assert mag.take(s.x, data, src=src).data_ptr() == got.data_ptr() and passes() == 1      # not again in the same step
    assert mag.take(s.x, data).data_ptr() == got.data_ptr() and passes() == 1
    mag.claim(s.out).fill_(9.0)                       # the producer left its bound: that block, no pass
    assert mag.take(s.dy, data, src=src).data_ptr() == mag.block(s.out).data_ptr()
    assert passes() == 1 and not mag.done(s.dy)
    assert mag.take(s.dy, data.to(torch.bfloat16)) is None and mag.take(None, data) is None and passes() == 1
    assert mag.take(s.dy, data, src=tensor(am_slot=None)).data_ptr() == mag.block(s.dy).data_ptr() and passes() == 2
    mag.begin_step()
    mag.take(s.x, data, src=src)
    assert passes() == 3                              # a new step: a new pass


def test_want_walks_the_aliases():
    mag = Magnitudes("f16x2")
    a, b = mag.new(), mag.new()
    pooled = tensor(am_slot=a)
    alias = tensor(am_slot=None, alias_of=tensor(am_slot=b, alias_of=pooled))
    mag.want(alias)
    assert mag.wanted(a) and mag.wanted(b) and not mag.wanted(mag.new()) and not mag.wanted(None)
    mag.want(None)


def test_spans_take_finite_maxima_and_the_minima(launches):
    mag, s = ledger()
    mag.refresh_frozen()
    mag.begin_step()
    mag.claim(s.x)[:3] = torch.tensor([1.0, 64.0, float("inf")])
    mag.min_view(s.x).fill_(2.0 ** -12)
    both = mag.spans_device()
    assert both.shape == (2, mag.slots) and float(both[0, s.x]) == 64.0 and float(both[1, s.x]) == 2.0 ** -12
    mag.block(s.x)[2] = 0.0
    seen, wide, bits = mag.range_report()             # x: 2^18; the two weights: 2 / 0.5
    assert (seen, wide, bits) == (3, 1, 18.0)
