"""The ledger of the operand magnitudes of a step ("f16x2" math).

The two-piece math cuts every convolution operand into fp16 pieces relative to a per-tensor magnitude block
(functional.absmax: ABSMAX_SLOTS partial maxima).  A block is meant to be the by-product of a kernel that touches the
tensor anyway -- a convolution epilogue, a BatchNorm finalize or apply, a pooling pass, a sampler backward, the ReLU mask
pass -- and a pass of its own runs only where nobody left one.  Which of the two happens is decided from this ledger:
nodes hold slot indices, the ledger holds the arena, what was written this step, and what somebody asked for.

Three verbs: `block` (the view for a kernel that READS the magnitude), `claim` (the view for a kernel that WRITES it;
marks the slot done -- the one write path) and `take` (the producer's bound if it left one, else a pass over the tensor,
once per step)."""
import numpy as np
import torch

from . import functional as fn


class Magnitudes:
    def __init__(self, math):
        self.math = math
        # one block per slot, all in one arena that begin_step() zeroes; slots are handed out while the graph is built
        # (new) and become views of the arena in allocate().  None: the ledger is inactive (other math modes, CPU graphs)
        self.slots = 0
        self.arena = None
        # range monitor / range guard: per slot the smallest non-zero per-channel magnitude travels beside the largest
        # (inputs from the BatchNorm finalize, weights from one batched launch per step, output gradients from the
        # BatchNorm backward's per-channel bounds); +inf where nobody saw the channels
        self.minima = None
        # the slots of FROZEN weights sit at the end of the arena, behind step_slots, which begin_step() does not zero:
        # their blocks are taken once and again only after the weights were set (refresh_frozen)
        self.step_slots = 0
        self.am_table = self.wmin_table = None      # descriptor tables of the weights' magnitudes / per-output-channel
        self.am_frozen = self.wmin_frozen = None    # minima: one launch per step, or per refresh (frozen weights)
        self._input = {}           # (id of the raw input tensor, id of its affine scale) -> slot shared by its readers
        self._wanted = set()       # slots some two-piece convolution will read off its input tensor (want)
        self._done = set()         # slots written in the current step
        self._backward, self._backward_ran = set(), False    # slots of gradient magnitudes: a second backward pass retakes them
        self._weights = set()      # weight slots, taken by the batched launches

    # -- allocation (while the graph is built) --------------------------------
    def new(self, backward=False):
        """index of a fresh slot.  backward=True: the magnitude of a gradient; a second backward pass after one forward
        pass takes those again (begin_backward)"""
        self.slots += 1
        if backward:
            self._backward.add(self.slots - 1)
        return self.slots - 1

    def input_slot(self, raw, affine_scale, create=True):
        """the slot shared by all readers of one (raw tensor, affine) pair (act1 feeds conv1 and the projection shortcut).
        create=False: None where no convolution reads that pair"""
        key = (id(raw), id(affine_scale))
        if key not in self._input and create:
            self._input[key] = self.new()
        return self._input.get(key)

    def want(self, t):
        """a two-piece convolution will multiply tensor t as it is: whoever produces it (or what it was pooled from) is
        asked to leave its magnitude block -- nobody takes one for tensors no convolution reads"""
        while t is not None:
            if t.am_slot is not None:
                self._wanted.add(t.am_slot)
            t = t.alias_of

    def wanted(self, slot):
        return slot in self._wanted

    def allocate(self, device, weights, minima=True):
        """Once the graph is complete.  weights: the nodes with a weight magnitude (n.am_w of n.w), taken by one batched
        launch per step; a frozen weight moves to a slot behind the step region.  minima: the weights' per-row minima too"""
        self.step_slots = self.slots
        for n in weights:
            if n.w.fixed:
                n.am_w = self.new()
        if self.math != "f16x2" or not self.slots:
            return
        self.arena = torch.zeros(self.slots * fn.ABSMAX_SLOTS, dtype=torch.float32, device=device)
        self.minima = torch.full((self.slots,), float("inf"), dtype=torch.float32, device=device)
        self._weights = {n.am_w for n in weights}
        for frozen in (False, True):
            sel = [n for n in weights if n.w.fixed == frozen]
            if not sel:
                continue
            am = fn.absmax_table([(n.w.data, self.block(n.am_w)) for n in sel], device)
            wmin = (fn.absmin_rows_table([(n.w.data.view(n.w.shape[0], -1), self.min_view(n.am_w)) for n in sel], device)
                    if minima else None)
            if frozen:
                self.am_frozen, self.wmin_frozen = am, wmin
            else:
                self.am_table, self.wmin_table = am, wmin

    # -- per-step state -------------------------------------------------------
    @property
    def active(self):
        return self.arena is not None

    def begin_step(self, minima=True):
        """every magnitude of the step starts from zero; the weights' are taken now (their minima where asked)"""
        if not self.active:
            return
        self.arena[:self.step_slots * fn.ABSMAX_SLOTS].zero_()
        self.minima[:self.step_slots].fill_(float("inf"))
        if self.wmin_table is not None and minima:
            fn.absmin_rows_batch(*self.wmin_table)
        self._done = set()
        self._backward_ran = False
        if self.am_table is not None:
            fn.absmax_batch(*self.am_table)
            self._done |= self._weights

    def refresh_frozen(self):
        """the frozen weights' blocks and minima, again"""
        if not self.active:
            return
        self.arena[self.step_slots * fn.ABSMAX_SLOTS:].zero_()
        self.minima[self.step_slots:].fill_(float("inf"))
        if self.wmin_frozen is not None:
            fn.absmin_rows_batch(*self.wmin_frozen)
        if self.am_frozen is not None:
            fn.absmax_batch(*self.am_frozen)

    def begin_backward(self):
        """a second backward pass on the same forward pass: new gradients, new magnitudes"""
        if not self.active:
            return
        if self._backward_ran:
            for slot in self._backward & self._done:
                self.block(slot).zero_()
            self._done -= self._backward
        self._backward_ran = True

    # -- blocks ---------------------------------------------------------------
    def block(self, slot):
        """the view of a slot for a kernel that reads it; None where there is nothing to read (inactive, no slot)"""
        if slot is None or self.arena is None:
            return None
        return self.arena[slot * fn.ABSMAX_SLOTS:(slot + 1) * fn.ABSMAX_SLOTS]

    def claim(self, slot):
        """the view of a slot for a kernel that writes it this step: the slot is done from here on"""
        out = self.block(slot)
        if out is not None:
            self._done.add(slot)
        return out

    def done(self, slot):
        return slot in self._done

    def min_view(self, slot):
        """the one-element view of a slot's smallest per-channel magnitude, for the kernel that sees the channels"""
        return None if (slot is None or self.minima is None) else self.minima[slot:slot + 1]

    def take(self, slot, tensor, src=None):
        """the magnitude block of `tensor` in the node-owned slot `slot`, taken by a pass over the tensor the first time a
        step asks for it and reused afterwards; None where the ledger is inactive or the tensor is not float32.
        src: the engine Tensor behind `tensor` -- if its producer has already left a bound of it this step, that block"""
        if slot is None or self.arena is None or tensor.dtype != torch.float32:
            return None
        if src is not None and src.am_slot in self._done:
            return self.block(src.am_slot)
        if slot in self._done:
            return self.block(slot)
        return fn.absmax(tensor, out=self.claim(slot))

    # -- spans (range monitor, range guard) -----------------------------------
    def spans_device(self):
        """(2, slots) device tensor: the largest (FINITE partial maxima, as the kernels read them) and the smallest non-zero
        per-channel magnitude per slot of the pass that has just been issued"""
        mx = self.arena.view(-1, fn.ABSMAX_SLOTS)
        mx = torch.where(mx < 3.0e38, mx, torch.zeros_like(mx)).max(dim=1).values
        return torch.stack([mx, self.minima])

    def range_report(self):
        """after a step (one device -> host copy): (tensors seen, tensors whose channel magnitudes span more than 2^16,
        largest span in bits) over the slots whose per-channel extremes somebody saw"""
        if self.arena is None:
            return (0, 0, 0.0)
        mx = self.arena.view(-1, fn.ABSMAX_SLOTS).max(dim=1).values.cpu().numpy()
        mn = self.minima.cpu().numpy()
        ok = np.isfinite(mn) & (mn > 0) & np.isfinite(mx) & (mx > 0)
        if not ok.any():
            return (0, 0, 0.0)
        span = np.log2(mx[ok] / mn[ok])
        return (int(ok.sum()), int((span > 16).sum()), float(span.max()))
