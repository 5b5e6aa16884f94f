"""Call-site audit of the "f16x2" magnitude blocks on a real training graph: does the block a two-piece convolution is
GIVEN bound the operand it MULTIPLIES?  tests/test_magnitudes.py checks the ledger with every launch stubbed; the by-product
producers have their own edge tests; this file watches the hand-over.  For one eager forward + backward pass the five
convolution entry points of dspnet_amd.functional are wrapped (the engine calls them through the module attribute); each
wrapper compares, with torch ops on the call's own stream, what the call is given against what it will multiply, then calls
through.

  float operand with a block (x / x_absmax, with the input affine applied; dy / dy_absmax; w or wt / w_absmax):
      true = max |operand| in float32;  block.max() >= true (1 - 2^-22)  -- the slack is the rounding of the bound kernel and of
      torch's unfused x * scale + shift;  the largest FINITE slot <= 2^17 true  -- the window of include/dspn_nn.h, beyond which
      a too-large block costs the small elements their relative accuracy.  An operand that is all zero has no accuracy to
      lose: any block serves it, the upper check is skipped (and counted).  The whole weight of a Conv node: equality.  (A slice
      of a weight read with the whole weight's block -- BilinearConcatConv -- gets the two-sided check.)
  operand passed as fp16 piece planes (x_planes, dy_planes, w_planes / wt_planes): every piece finite, and the SCALED VALUE
      h0 + h1 (exact in float64) below 2^15 in magnitude -- what a valid block guarantees through operand_scale -- with
      |h0| <= 2^15.  (First written as max |h0| < 2^15, which correct code misses: operand_scale puts the maximum u into
      [2^14, 2^15), and h0 = fp16(u) rounds every u above 32760 up to 32768 = 2^15 itself, a finite fp16 value that costs the
      products nothing.  On the first device run 24 (resnet-50) and 25 (vgg16_reduced) weight-plane operands, whose freshly
      initialised maxima sit a few 10^-6 under a power of two, had max |h0| = 32768.0 exactly and nothing else was found.
      A block that is too small still fails: its u is 2^15 or more, and so is h0 + h1.)
  a two-piece call that carries a float operand WITHOUT a block is a failure (functional would take the magnitude by a pass of
      its own: the ledger lost track of it).

Calls the range guard moved to the three-piece math carry no blocks and are only counted."""
import pytest
import torch

from dspnet_amd import engine, functional as fn, synthetic
from dspnet_amd.symbol.multitask_symbol_factory import get_multi_symbol_train
from dspnet_amd.train.solver import MultiTaskSolver

pytestmark = pytest.mark.gpu

LOW, WINDOW = 1.0 - 2.0 ** -22, 2.0 ** 17


class Audit:
    def __init__(self, g):
        self.g = g
        self.reset()
        self.owner, self.whole = {}, set()
        for n in g.nodes:
            if isinstance(n, engine.Conv):
                for t in (n.w.data, n.w.grad, n.wt, n.wh, n.wp, n.wtp, n.slabs):
                    if t is not None:
                        self.owner[t.data_ptr()] = n.w.name
                for t in (n.w.data, n.wt):
                    if t is not None:
                        self.whole.add(t.data_ptr())

    def reset(self):
        self.calls = {}                # Conv weight name -> {"forward": n, "dgrad": n, "wgrad": n}
        self.other = 0                 # audited calls of nodes that are no Conv (BilinearConcatConv, Deconv4x4s2)
        self.fallback = 0              # calls in another math (the range guard's)
        self.checked = dict(float=0, planes=0, zero=0)
        self.bad = []
        self.worst = (0.0, None)       # largest finite block maximum / true over the float operands
        self.tight = (float("inf"), None)

    # -- bookkeeping
    def node(self, *tensors):
        for t in tensors:
            if t is not None and t.data_ptr() in self.owner:
                return self.owner[t.data_ptr()]
        return None

    def count(self, name, kind):
        if name is None:
            self.other += 1
        else:
            self.calls.setdefault(name, dict(forward=0, dgrad=0, wgrad=0))[kind] += 1

    def two_piece(self, math, t):
        return fn._math_code(math) == 3 and t.dtype == torch.float32

    # -- the checks
    def float_operand(self, where, what, t, block, affine=None, exact=False):
        if block is None:
            self.bad.append(f"{where}: float operand {what} without a magnitude block")
            return
        u = t
        if affine is not None:
            sc, sh, relu = affine
            u = t * sc + sh
            if relu:
                u = u.clamp_min(0)
        true = float(u.abs().max())
        bmax = float(block.max())
        finite = block[block < 3.0e38]
        fmax = float(finite.max()) if finite.numel() else 0.0
        self.checked["float"] += 1
        if not bmax >= true * LOW:
            self.bad.append(f"{where}: {what} block.max() = {bmax!r} is below max |{what}| = {true!r} (ratio {bmax / true if true else 0:.6g})")
        if exact and bmax != true:
            self.bad.append(f"{where}: {what} block.max() = {bmax!r} differs from max |{what}| = {true!r} of the whole weight")
        if true == 0.0:
            self.checked["zero"] += 1
            return
        ratio = fmax / true
        if ratio > self.worst[0]:
            self.worst = (ratio, f"{where}: {what}")
        if ratio < self.tight[0]:
            self.tight = (ratio, f"{where}: {what}")
        if not fmax <= WINDOW * true:
            self.bad.append(f"{where}: {what} block (finite maximum {fmax!r}) is more than 2^17 above max |{what}| = {true!r} (ratio 2^{torch.log2(torch.tensor(ratio)).item():.1f})")

    def planes(self, where, what, t):
        h = t.view(torch.float16).reshape(-1, 2, 32)
        self.checked["planes"] += 1
        if not bool(torch.isfinite(h).all()):
            self.bad.append(f"{where}: {what} holds {int((~torch.isfinite(h)).sum())} non-finite pieces")
            return
        h0, u = float(h[:, 0].abs().max()), float(h.double().sum(dim=1).abs().max())
        if not (u < 2.0 ** 15 and h0 <= 2.0 ** 15):
            self.bad.append(f"{where}: {what} max |h0 + h1| = {u!r} is not below 2^15 (max |h0| = {h0!r})")

    def weight(self, where, what, w, planes, block):
        if w is not None and w.dtype == torch.float32:
            self.float_operand(where, what, w, block, exact=w.data_ptr() in self.whole)
        if planes is not None:
            if block is None:
                self.bad.append(f"{where}: {what} piece planes without the block they were cut by")
            self.planes(where, what + " planes", planes)

    def activation(self, where, what, t, block, is_planes, affine=None):
        if is_planes:
            if block is None:
                self.bad.append(f"{where}: {what} piece planes without the block they were cut by")
            self.planes(where, what + " planes", t)
        else:
            self.float_operand(where, what, t, block, affine)

    # -- the wrappers
    def install(self, monkeypatch):
        real = {k: getattr(fn, k) for k in ("conv2d_forward", "conv2d_dgrad", "conv2d_dgrad_bn_apply", "conv2d_wgrad", "conv2d_wgrad_slabs")}

        def forward(x, w, bias=None, stride=1, pad=0, dil=1, **kw):
            name = self.node(w, kw.get("w_planes"))
            self.count(name, "forward")
            if self.two_piece(kw.get("math"), x):
                where = f"conv2d_forward[{name or 'other node'}]"
                self.activation(where, "x", x, kw.get("x_absmax"), kw.get("x_planes", False), kw.get("in_affine"))
                self.weight(where, "w", w, kw.get("w_planes"), kw.get("w_absmax"))
            else:
                self.fallback += 1
            return real["conv2d_forward"](x, w, bias, stride, pad, dil, **kw)

        def dgrad_like(entry):
            def call(dy, wt, *args, **kw):
                name = self.node(wt, kw.get("wt_planes"))
                self.count(name, "dgrad")
                if self.two_piece(kw.get("math"), dy):
                    where = f"{entry}[{name or 'other node'}]"
                    self.activation(where, "dy", dy, kw.get("dy_absmax"), kw.get("dy_planes", False))
                    self.weight(where, "wt", wt, kw.get("wt_planes"), kw.get("w_absmax"))
                else:
                    self.fallback += 1
                return real[entry](dy, wt, *args, **kw)
            return call

        def wgrad_like(entry):
            def call(x, dy, w_shape, *args, **kw):
                name = self.node(kw.get("out"), args[0] if entry == "conv2d_wgrad_slabs" else None)
                self.count(name, "wgrad")
                if self.two_piece(kw.get("math"), x):
                    where = f"{entry}[{name or 'other node'}]"
                    self.activation(where, "x", x, kw.get("x_absmax"), kw.get("x_planes", False), kw.get("in_affine"))
                    self.activation(where, "dy", dy, kw.get("dy_absmax"), kw.get("dy_planes", False))
                else:
                    self.fallback += 1
                return real[entry](x, dy, w_shape, *args, **kw)
            return call

        monkeypatch.setattr(fn, "conv2d_forward", forward)
        monkeypatch.setattr(fn, "conv2d_dgrad", dgrad_like("conv2d_dgrad"))
        monkeypatch.setattr(fn, "conv2d_dgrad_bn_apply", dgrad_like("conv2d_dgrad_bn_apply"))
        monkeypatch.setattr(fn, "conv2d_wgrad", wgrad_like("conv2d_wgrad"))
        monkeypatch.setattr(fn, "conv2d_wgrad_slabs", wgrad_like("conv2d_wgrad_slabs"))

    # -- the verdict of one pass
    def verdict(self, label):
        convs = [n for n in self.g.nodes if isinstance(n, engine.Conv)]
        none = dict(forward=0, dgrad=0, wgrad=0)
        no_fwd = [n.w.name for n in convs if self.calls.get(n.w.name, none)["forward"] < 1]
        no_bwd = [n.w.name for n in convs if not n.w.fixed
                  and self.calls.get(n.w.name, none)["dgrad"] + self.calls.get(n.w.name, none)["wgrad"] < 1]
        total = sum(sum(c.values()) for c in self.calls.values()) + self.other
        print(f"{label}: {total} audited calls ({len(convs)} Conv nodes, {self.other} calls of other nodes, {self.fallback} in another math), "
              f"{self.checked['float']} float operands ({self.checked['zero']} all zero), {self.checked['planes']} plane operands; "
              f"largest finite block / true = {self.worst[0]:.6g} at {self.worst[1]}, smallest = {self.tight[0]:.9g} at {self.tight[1]}")
        assert convs and not no_fwd, f"{label}: Conv nodes without an audited forward call: {no_fwd[:8]}"
        assert not no_bwd, f"{label}: trained Conv nodes without an audited gradient call: {no_bwd[:8]}"
        assert self.checked["float"] > 0 and self.checked["planes"] > 0
        assert not self.bad, f"{label}: {len(self.bad)} findings:\n" + "\n".join(self.bad[:40])


def build(network, batch, size):
    dev = torch.device("cuda", 0)
    net = get_multi_symbol_train(network, (3, size, size), num_classes=8, batch_size=batch, device=dev, seed=1)
    gen = synthetic.rng(233)
    data = synthetic.images(batch, size, size, gen)
    lab = synthetic.det_labels(batch, gen=gen, height=size, width=size)
    seg = synthetic.seg_labels(batch, size, size, gen=gen)
    solver = MultiTaskSolver(net)
    solver.set_batch(torch.from_numpy(data).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(seg).to(dev))
    return net, solver


# resnet-50: the small training graph of tests/test_graph_gpu.py make(2, 128, 128); vgg16_reduced cannot be built below its SSD
# extra layers' reach: the 320 x 320 graph of test_other_backbone_graphs_match_cpu_restatement
@pytest.mark.parametrize("network,batch,size", [("resnet-50", 2, 128), ("vgg16_reduced", 2, 320)])
def test_every_block_bounds_the_operand_it_is_handed_with(gpu_device, monkeypatch, network, batch, size):
    """one eager forward + backward pass, audited; then (graphs with stage BatchNorms) every stage gamma times 2^+12 / 2^-12
    alternating per channel -- the jump of test_range_guard_acts_on_a_recorded_step -- and the pass again: a block left over
    from the first pass fails the lower bound on a tensor whose scale has moved"""
    if fn.get_conv_math() != "f16x2":
        pytest.skip("the magnitude blocks belong to the two-piece math")
    net, solver = build(network, batch, size)
    assert net.g.mag.active
    audit = Audit(net.g)
    audit.install(monkeypatch)
    solver.forward(); solver.backward(); torch.cuda.synchronize()
    audit.verdict(f"{network}, first pass")
    gammas = [p for p in net.g.param_order if p.name.endswith("_gamma") and p.name.startswith("stage")]
    assert bool(gammas) == (network == "resnet-50")
    if not gammas:
        return
    with torch.no_grad():
        for p in gammas:
            c = torch.arange(p.data.numel(), device=p.data.device)
            p.data.mul_(torch.where(c % 2 == 0, 2.0 ** 12, 2.0 ** -12).to(p.data.dtype))
    audit.reset()
    solver.forward(); solver.backward(); torch.cuda.synchronize()
    audit.verdict(f"{network}, after the gamma jump")
    assert bool(torch.isfinite(net.g.grad_arena).all())
