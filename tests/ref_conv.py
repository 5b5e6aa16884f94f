"""For tests/test_conv_edges_gpu.py: a Python restatement of the host dispatch of dspnet_amd/csrc/conv.hip (default
environment), the exact-sum input classes, and the float64 references (torch CPU; never a kernel of this library).

A case is (N, H, W, Cin, Cout, k, stride, pad, dil); k and pad an int or an (h, w) pair.  Cin / Cout are the LOGICAL channel
counts: the device tensors pad them with zeros to a 16-byte chunk (4 floats, 8 bfloat16)."""
import functools

import torch
import torch.nn.functional as F

F64 = torch.float64
FIT = 2.0 ** 22          # sum |a||b| per output, in units of the operands' last bit: every fp32 partial sum is exact below it


def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def out_hw(case):
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    (kh, kw), (ph, pw) = pair(k), pair(pad)
    return (H + 2 * ph - dil * (kh - 1) - 1) // stride + 1, (W + 2 * pw - dil * (kw - 1) - 1) // stride + 1


def padc(c, epc):
    return (c + epc - 1) // epc * epc


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated (conv.hip: nt_config, dispatch_nt, dgrad_tiles, wgrad_plan; conv_wide.hip: wide_tile_choice)
NT_BM, NT_BN = (128, 128, 64, 256), (128, 64, 64, 32)
NT_MIN_TILES = 256


def cdiv(a, b):
    return -(-a // b)


def nt_config(M, Cout):
    def tiles(bm, bn):
        return cdiv(M, bm) * cdiv(Cout, bn)
    if Cout <= 32:
        cfg = 3 if tiles(256, 32) >= NT_MIN_TILES else 2
    else:
        cfg = 0 if (Cout > 64 and tiles(128, 128) >= NT_MIN_TILES) else 2
    if cfg == 0 and cdiv(Cout, 64) * 64 < cdiv(Cout, 128) * 128:
        cfg = 1
    return cfg


def split_workspace_floats(M, Cout):
    return 32 * min(M * Cout, 192 * 64 * 64 * 4)


def nt_route(M, cols, kch, taps, epc=4, dense=True, fused=False, split_math=True):
    """one launch of dispatch_nt: M output rows, `cols` output columns, `kch` PHYSICAL channels per tap, `taps` taps.
    epc: elements per 16-byte chunk (4: float tensors, 8: bfloat16 tensors).  fused: statistics / BatchNorm sums asked for."""
    cfg = nt_config(M, cols)
    bm, bn = NT_BM[cfg], NT_BN[cfg]
    mt, nt = cdiv(M, bm), cdiv(cols, bn)
    nblk = mt * nt
    nk = (taps * (kch // epc) + 7) >> 3
    splits, per = 1, nk
    if dense and nblk < 192 and nk >= 16 and not fused:
        splits = max(1, min(min(cdiv(384, nblk), nk // 8), 32))
        while splits > 1 and splits * M * cols > split_workspace_floats(M, cols):
            splits -= 1
        per = cdiv(nk, splits)
        splits = cdiv(nk, per)
    uniform = ((kch // epc) & 7) == 0
    return dict(cfg=cfg, bm=bm, bn=bn, mt=mt, nt=nt, nblk=nblk, nk=nk, splits=splits, per=per, last=nk - (splits - 1) * per,
                uniform=uniform, planes=bool(split_math and epc == 4 and uniform), row_rem=M % bm, col_rem=cols % bn)


def wide_tile(M, Cout, nk, fused):
    """wide_tile_choice, automatic mode: None, or the (rows, columns) of the member's tile"""
    if Cout <= 64:
        return (256, 64) if nk >= 4 else None
    if nk < 4 and not (fused and nk >= 2):
        return None
    if Cout % 256 == 0 and nk >= 8 and cdiv(M, 128) * (Cout // 256) >= 256:
        return (128, 256)
    return (128, 128)


def wide_route(case, fused=False, aligned=True):
    """the wide member a default f16x2 float-tensor forward call of `case` takes (None: conv_nt_kernel), from dispatch_nt's
    wide_ok and wide_tile_choice; (rows, columns, direct epilogue legal)"""
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho, Wo = out_hw(case)
    M, (kh, kw) = N * Ho * Wo, pair(k)
    r = nt_route(M, Cout, padc(Cin, 4), kh * kw, fused=fused)
    ok = (r["splits"] == 1 and (r["cfg"] == 0 or (r["cfg"] == 2 and 32 < Cout <= 64)) and aligned and Cout % 4 == 0 and r["planes"])
    t = wide_tile(M, Cout, r["nk"], fused) if ok else None
    return None if t is None else (t[0], t[1], M % t[0] == 0)


def fwd_route(case, epc=4, fused=False):
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho, Wo = out_hw(case)
    kh, kw = pair(k)
    return nt_route(N * Ho * Wo, Cout, padc(Cin, epc), kh * kw, epc, fused=fused)


def dgrad_classes(N, H, W, stride):
    """(parity index, rows, cols) of the launches of one data gradient: the output rows of each class"""
    if stride == 1:
        return [(0, H, W)]
    return [(ph * 2 + pw, (H - ph + 1) // 2, (W - pw + 1) // 2) for ph in range(2) for pw in range(2)]


def dgrad_class_taps(k, pad, stride, cls):
    """(TR, TS) of parity class cls of a stride-2 data gradient (0: the class has no tap)"""
    (kh, kw), (ph_, pw_) = pair(k), pair(pad)
    if stride == 1:
        return kh, kw
    ph, pw = cls >> 1, cls & 1
    r0, s0 = (ph + ph_) & 1, (pw + pw_) & 1
    return ((kh - r0 + 1) // 2 if r0 < kh else 0), ((kw - s0 + 1) // 2 if s0 < kw else 0)


def dgrad_routes(case, epc=4):
    """[(class, route)] of the data gradient of `case` (empty classes and classes without a tap left out)"""
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    out = []
    for cls, hg, wg in dgrad_classes(N, H, W, stride):
        tr, ts = dgrad_class_taps(k, pad, stride, cls)
        if hg <= 0 or wg <= 0 or tr * ts == 0:
            continue
        out.append((cls, nt_route(N * hg * wg, Cin, padc(Cout, epc), tr * ts, epc, dense=(stride == 1))))
    return out


def dgrad_tiles(N, H, W, Cin, stride):
    """row tiles of all classes: what dspn_conv2d_dgrad_bn_tiles returns"""
    return sum(cdiv(N * hg * wg, NT_BM[nt_config(N * hg * wg, Cin)]) for _, hg, wg in dgrad_classes(N, H, W, stride)
               if hg > 0 and wg > 0)


def wgrad_plan(P, Cout, J, x_bytes=0):
    bm = 32 if Cout <= 32 else (64 if Cout <= 64 else 128)
    if bm == 128 and cdiv(Cout, 64) * 64 < cdiv(Cout, 128) * 128:
        bm = 64
    bn = 64 if (J <= 64 and bm == 128) else 128
    tiles = cdiv(Cout, bm) * cdiv(J, bn)
    lds = 4 * max(2 * 32 * (bm + bn), bm * (bn + 4))
    slots = 256 * min(8, (160 << 10) // lds)
    s_min = cdiv(x_bytes, 32 << 20) if x_bytes > 0 else 1
    s_max = max(1, min(P // 128, 1024))
    s_min = min(s_min, s_max)
    flop_per_pix, slot_rate, ovh = 2.0 * bm * bn, 120e12 / float(slots), 160.0
    best, splits = 1e30, s_min
    sp = s_min
    while sp <= s_max:
        pps = cdiv(cdiv(P, sp), 64) * 64
        real = cdiv(P, pps)
        rounds = cdiv(tiles * real, slots)
        t = float(rounds) * (float(pps) + ovh) * flop_per_pix / slot_rate + float(real) * Cout * J * 8.0 / 4e12
        if t < best * 0.999:
            best, splits = t, sp
        if tiles * sp > 8 * slots:
            break
        sp += 1
    splits = min(splits, s_max)
    pps = cdiv(cdiv(P, splits), 64) * 64
    return dict(bm=bm, bn=bn, splits=cdiv(P, pps), pps=pps, last=P - (cdiv(P, pps) - 1) * pps)


def wgrad_route(case, epc=4):
    N, H, W, Cin, Cout, k, stride, pad, dil = case
    Ho, Wo = out_hw(case)
    kh, kw = pair(k)
    P, cin_p = N * Ho * Wo, padc(Cin, epc)
    xb = 4 * P * cin_p * min(stride, 2) ** 2 if kh * kw > 1 else 0
    r = wgrad_plan(P, Cout, kh * kw * cin_p, xb)
    r.update(P=P, J=kh * kw * cin_p)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def _mantissa(shape, bits, g):
    """odd-rich integers m, 1 <= |m| < 2^bits: the top bit region and the last bit are both used"""
    m = torch.randint(1 << (bits - 2), 1 << bits, shape, generator=g) | 1
    m[torch.rand(shape, generator=g) < 0.25] >>= (bits - 3)             # some small magnitudes too (>= 1 after the | 1 below)
    m = (m | 1).double()
    return m * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()


def _sparse(shape, lim, expect, K, g):
    """integers in [-lim, lim], non-zero with probability expect / K (at most 1)"""
    v = torch.randint(1, lim + 1, shape, generator=g).double() * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    return v * (torch.rand(shape, generator=g) < min(1.0, expect / max(K, 1))).double()


def operands(shape_a, shape_b, cls, K, g):
    """(a, b, unit): the two operands of one contraction of length K in input class `cls`:
      "A"        integers in [-6, 6], both
      "B1"/"B2"  a (resp. b) = m 2^-6 with |m| < 2^13, the other a sparse integer in [-2, 2] (about 96 non-zeros per sum)
      "C1"/"C2"  a (resp. b) = m with |m| < 2^17, the other sparse in {-1, 0, 1} (about 14 non-zeros per sum: the largest
                 count of a few million sums stays below 32)
      "G"        randn and randn / sqrt(K), rounded to float32 (unit None)
    unit: the value of the last bit of a product; the sums are exact when sum|a||b| < 2^22 units (asserted by the caller)"""
    if cls == "A":
        return _ints(shape_a, 6, g), _ints(shape_b, 6, g), 1.0
    if cls == "G":
        return torch.randn(shape_a, generator=g, dtype=F64).float().double(), (torch.randn(shape_b, generator=g, dtype=F64) / K ** 0.5).float().double(), None
    bits, lim, expect, scale = (13, 2, 96, 2.0 ** -6) if cls[0] == "B" else (17, 1, 14, 1.0)
    if cls[1] == "1":
        return _mantissa(shape_a, bits, g) * scale, _sparse(shape_b, lim, expect, K, g), scale
    return _sparse(shape_a, lim, expect, K, g), _mantissa(shape_b, bits, g) * scale, scale


class Problem:
    """one case in one input class: the float64 tensors (NCHW / OIHW, logical channels) and, lazily, the references"""

    def __init__(self, case, cls, bf16=False):
        N, H, W, Cin, Cout, k, stride, pad, dil = case
        self.case, self.cls, self.bf16 = case, cls, bf16
        (kh, kw), (Ho, Wo) = pair(k), out_hw(case)
        flat = [int(v) for f in case for v in (f if isinstance(f, (tuple, list)) else (f,))]
        g = torch.Generator().manual_seed((sum((i + 1) * 7919 * v for i, v in enumerate(flat)) + 131 * sum(map(ord, cls))) % (1 << 31))
        exact = cls != "G"
        self.x, self.w, self.unit = operands((N, Cin, H, W), (Cout, Cin, kh, kw), cls, Cin * kh * kw, g)
        # the operands of the two gradients: dy in the role of the first operand
        if cls == "A":
            self.dy = _ints((N, Cout, Ho, Wo), 6, g)
        else:
            self.dy = operands((N, Cout, Ho, Wo), (1,), cls, Cout * kh * kw, g)[0]
        # for the weight gradient x and dy are contracted over P pixels: its own pair
        self.xg, self.dyg, _ = operands((N, Cin, H, W), (N, Cout, Ho, Wo), cls, N * Ho * Wo, g)
        if exact:
            self.bias = _ints((Cout,), 5, g) * self.unit
            self.res = _ints((N, Cout, Ho, Wo), 7, g) * self.unit
            self.prior = _ints((N, Cout, Ho, Wo), 7, g) * self.unit
            self.scale = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=F64)[torch.randint(0, 4, (Cin,), generator=g)]
            self.shift = _ints((Cin,), 3, g)
            self.prior_dx = _ints((N, Cin, H, W), 7, g) * self.unit
            self.prior_dw = _ints((Cout, Cin, kh, kw), 7, g) * self.unit
        else:
            r32 = lambda *s: torch.randn(*s, generator=g, dtype=F64).float().double()      # noqa: E731
            self.bias, self.res, self.prior = r32(Cout), r32(N, Cout, Ho, Wo), r32(N, Cout, Ho, Wo)
            self.scale, self.shift = (torch.rand(Cin, generator=g, dtype=F64) + 0.5).float().double(), 0.3 * r32(Cin)
            self.scale[1::3] *= -1.0
            self.prior_dx, self.prior_dw = r32(N, Cin, H, W), r32(Cout, Cin, kh, kw)
        if bf16:        # general values on bfloat16 tensors (and the operand-rounding "bf16" math): what the device is given
            for name in ("x", "w", "dy", "xg", "dyg", "res", "prior", "prior_dx"):
                setattr(self, name, getattr(self, name).to(torch.bfloat16).double())

    def conv(self, x, w):
        N, H, W, Cin, Cout, k, stride, pad, dil = self.case
        return F.conv2d(x, w, None, stride=stride, padding=pair(pad), dilation=dil)

    def affine(self, x, relu):
        """the input affine as the kernel applies it: fmaf(x, scale, shift) rounded once to float32 (exact for class A); on
        bfloat16 operands (the bf16 tensors and the operand-rounding "bf16" math) the MFMA is then fed its bfloat16 value"""
        a = (x * self.scale.view(1, -1, 1, 1) + self.shift.view(1, -1, 1, 1)).float().double()
        if self.bf16:
            a = a.to(torch.bfloat16).double()
        return a.clamp(min=0) if relu else a

    @functools.lru_cache(maxsize=None)
    def forward(self, affine=0):
        """(linear part y, S = the same sum over absolute values); affine: 0 none, 1 scale / shift, 2 with ReLU"""
        x = self.x if affine == 0 else self.affine(self.x, affine == 2)
        return self.conv(x, self.w), self.conv(x.abs(), self.w.abs())

    @functools.lru_cache(maxsize=None)
    def dgrad(self):
        """(dx, S) from autograd"""
        out = []
        for dy, w in ((self.dy, self.w), (self.dy.abs(), self.w.abs())):
            x = torch.zeros_like(self.x, requires_grad=True)
            out.append(torch.autograd.grad(self.conv(x, w), x, dy)[0])
        return tuple(out)

    @functools.lru_cache(maxsize=None)
    def wgrad(self, affine=0):
        """(dw, S) from autograd, of the weight-gradient pair (xg, dyg)"""
        x = self.xg if affine == 0 else self.affine(self.xg, affine == 2)
        out = []
        for xx, dy in ((x, self.dyg), (x.abs(), self.dyg.abs())):
            w = torch.zeros_like(self.w, requires_grad=True)
            out.append(torch.autograd.grad(self.conv(xx, w), w, dy)[0])
        return tuple(out)


@functools.lru_cache(maxsize=24)
def problem(case, cls, bf16=False):
    return Problem(case, cls, bf16)


def assert_fit(S, extra, unit, what):
    """the precondition of every bit-exact claim, on the reference alone"""
    worst = float((S + extra).max()) / unit
    assert worst < FIT, f"{what}: inputs unfit, sum|a||b| reaches {worst:.4g} units of the last bit (limit 2^22)"
