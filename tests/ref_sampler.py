"""Plain restatement of GridGenerator(affine) + BilinearSampler as dspnet_amd/csrc/sampler.hip states it at its top, in torch on
the CPU (float64 unless asked otherwise).  Shared by test_sampler_reference.py (which ties it to float64 affine_grid +
grid_sample autograd) and test_sampler_edges_gpu.py (which holds the kernels to it).  Tensors are NHWC.

  x_t = -1 + wo * 2 / (Wo - 1),  y_t = -1 + ho * 2 / (Ho - 1);  a target coordinate is 0 when that extent is 1 (tgt_coord)
  (gx, gy) = theta(2 x 3) . (x_t, y_t, 1)                       one grid for the whole batch
  xs = (gx + 1) (Win - 1) / 2,  ys likewise;  x0 = floor(xs), fx = xs - x0
  out = sum over the four neighbours (y0 + a, x0 + b) INSIDE the image of  wy_a wx_b x[neighbour]
        with wy_0 = 1 - fy, wy_1 = fy  (a neighbour outside the image contributes nothing)
  d weight / d xs = -wy_a (b = 0), +wy_a (b = 1);  d weight / d ys = -wx_b (a = 0), +wx_b (a = 1)

floor() makes this the RIGHT-hand derivative where a sample sits on a source pixel (fx == 0: x0 is that pixel, weight 1, slope
-1; x0 + 1 has weight 0 and slope +1), and a neighbour beyond the image has value and slope 0: a sample on the last pixel
sees the slope -x[last], one on the -1 border the slope +x[0].

A MATCH is a pair (target pixel, neighbour) whose neighbour lies inside the image, weight 0 included: what the gather kernels
enumerate from the source pixel's side.  Matches are ordered by target pixel (ho, wo), then neighbour (a, b); the k-th match
of a position counts in that order."""
import math

import torch

F64 = torch.float64


def tgt_coord(O, dtype=F64):
    """the O target coordinates of one axis"""
    if O <= 1:
        return torch.zeros(max(O, 1), dtype=dtype)
    return -1.0 + torch.arange(O, dtype=dtype) * (torch.tensor(2.0, dtype=dtype) / torch.tensor(float(O - 1), dtype=dtype))


class _threads:
    """`with _threads(1):` -- the many small tensor operations here only lose time to a thread pool"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.before = torch.get_num_threads()
        torch.set_num_threads(self.n)

    def __exit__(self, *exc):
        torch.set_num_threads(self.before)


class Geometry:
    """the matches of one (theta, source extent, target extent): t (target pixel ho * Wo + wo), p (source position
    h * Win + w), w (bilinear weight), coef (M, 6) = (d w / d xs (Win-1)/2 (x_t, y_t, 1), d w / d ys (Hin-1)/2 (x_t, y_t, 1))"""

    def __init__(self, theta, Hin, Win, Ho, Wo, dtype=F64):
        with _threads(1):
            self._build(theta, Hin, Win, Ho, Wo, dtype)

    def _build(self, theta, Hin, Win, Ho, Wo, dtype):
        th = torch.as_tensor(theta, dtype=F64).float().to(dtype)          # the kernels are handed theta as float32
        xt = tgt_coord(Wo, dtype).view(1, Wo).expand(Ho, Wo)
        yt = tgt_coord(Ho, dtype).view(Ho, 1).expand(Ho, Wo)
        gx = th[0] * xt + th[1] * yt + th[2]
        gy = th[3] * xt + th[4] * yt + th[5]
        xs = (gx + 1.0) * float(Win - 1) / 2.0
        ys = (gy + 1.0) * float(Hin - 1) / 2.0
        # (the kernel's band: nothing changes inside it, outside every neighbour is out of the image anyway)
        xs = xs.clamp(-2.0, Win + 1.0)
        ys = ys.clamp(-2.0, Hin + 1.0)
        self.xs, self.ys = xs, ys
        x0, y0 = torch.floor(xs), torch.floor(ys)
        fx, fy = xs - x0, ys - y0
        x0, y0 = x0.long(), y0.long()
        khw, khh = float(Win - 1) * 0.5, float(Hin - 1) * 0.5
        tt = torch.arange(Ho * Wo).view(Ho, Wo)
        ts, ps, ws, cs, ks = [], [], [], [], []
        for a in (0, 1):
            for b in (0, 1):
                yy, xx = y0 + a, x0 + b
                ok = (yy >= 0) & (yy < Hin) & (xx >= 0) & (xx < Win)
                wy = fy if a else 1.0 - fy
                wx = fx if b else 1.0 - fx
                cx = (wy if b else -wy) * khw
                cy = (wx if a else -wx) * khh
                coef = torch.stack([cx * xt, cx * yt, cx, cy * xt, cy * yt, cy], dim=-1)
                ts.append(tt[ok]); ps.append((yy * Win + xx)[ok]); ws.append((wy * wx)[ok]); cs.append(coef[ok])
                ks.append(torch.full((int(ok.sum()),), 2 * a + b))
        t, p, w, c, k = torch.cat(ts), torch.cat(ps), torch.cat(ws), torch.cat(cs), torch.cat(ks)
        order = torch.argsort(t * 4 + k)          # by target pixel, then neighbour (keys are distinct)
        self.t, self.p, self.w, self.coef = t[order], p[order], w[order], c[order]
        self.Hin, self.Win, self.Ho, self.Wo = Hin, Win, Ho, Wo

    def counts(self):
        """matches per source position"""
        return torch.bincount(self.p, minlength=self.Hin * self.Win)

    def matches_of(self, position):
        """indices (into t / p / w / coef) of the matches of one source position, in match order"""
        return torch.nonzero(self.p == position).flatten()

    def without(self, position, k):
        """the mutant: the k-th match of `position` left out"""
        drop = int(self.matches_of(position)[k])
        keep = torch.ones(self.t.numel(), dtype=torch.bool)
        keep[drop] = False
        g = object.__new__(Geometry)
        g.__dict__.update(self.__dict__)
        g.t, g.p, g.w, g.coef = self.t[keep], self.p[keep], self.w[keep], self.coef[keep]
        return g


def fraction_bits(v):
    """smallest f with v * 2^f integral for every entry of v (None: v is not dyadic within 40 bits)"""
    v = v.double().flatten()
    for f in range(41):
        s = v * 2.0 ** f
        if bool((s == torch.round(s)).all()):
            return f
    return None


class Result:
    """out (N, Ho, Wo, ldo); per source: dx[i] (N, Hin, Win, C), rows[i] (N * Hin * Win, 6), counts[i] (Hin * Win), the sums
    of |terms| abs_dx[i] / abs_rows[i] (the shapes of dx / rows) and geo[i]; dtheta (6), abs_out, abs_dtheta (6).  All float64."""


def sampler(sources, theta, Ho, Wo, dy=None, ldo=None, drop=None, dtype=F64, want_abs=True):
    """sources: [(x (N, Hin, Win, C), channel offset)], dy: (N, Ho, Wo, ldo) or None (forward only).  drop = (position, k) or
    (source index, position, k): the mutant that leaves one match out (of source 0 unless named).  dtype = torch.float32
    evaluates the same sums in float32 -- coordinates, weights, products, and sums in match order, i.e. by target pixel,
    where the gather kernels go by slice, row and column and the theta kernel by wave -- and returns them widened."""
    N = sources[0][0].shape[0]
    work = N * Ho * Wo * 4 * sum(x.shape[3] for x, _ in sources)
    with _threads(1 if work < (1 << 24) else torch.get_num_threads()):
        return _sampler(sources, theta, Ho, Wo, dy, ldo, drop, dtype, want_abs)


def _sampler(sources, theta, Ho, Wo, dy, ldo, drop, dtype, want_abs):
    N = sources[0][0].shape[0]
    ldo = ldo if ldo is not None else (dy.shape[3] if dy is not None else max(o + x.shape[3] for x, o in sources))
    if drop is not None and len(drop) == 2:
        drop = (0,) + tuple(drop)
    r = Result()
    r.out = torch.zeros(N, Ho * Wo, ldo, dtype=dtype)
    r.abs_out = torch.zeros(N, Ho * Wo, ldo, dtype=dtype) if want_abs else None
    r.dx, r.rows, r.counts, r.abs_dx, r.abs_rows, r.geo = [], [], [], [], [], []
    g_ = dy.to(dtype).reshape(N, Ho * Wo, ldo) if dy is not None else None
    r.abs_theta_tgt = torch.zeros(N, Ho * Wo, 6, dtype=F64) if want_abs and g_ is not None else None
    for si, (x, off) in enumerate(sources):
        _, Hin, Win, C = x.shape
        geo = Geometry(theta, Hin, Win, Ho, Wo, dtype)
        if drop is not None and drop[0] == si:
            geo = geo.without(drop[1], drop[2])
        r.geo.append(geo)
        r.counts.append(geo.counts())
        xv = x.to(dtype).reshape(N, Hin * Win, C)
        M = geo.t.numel()
        step = max(1, (1 << 24) // max(1, N * C))          # matches per pass: bounds the (N, step, C) temporaries
        dx = torch.zeros(N, Hin * Win, C, dtype=dtype)
        rows = torch.zeros(N, Hin * Win, 6, dtype=dtype)
        adx = torch.zeros_like(dx) if want_abs else None
        arows = torch.zeros_like(rows) if want_abs else None
        for m0 in range(0, M, step):
            t, p = geo.t[m0:m0 + step], geo.p[m0:m0 + step]
            w, coef = geo.w[m0:m0 + step].view(1, -1, 1), geo.coef[m0:m0 + step]
            xm = xv[:, p]                                            # (N, m, C)
            r.out[:, :, off:off + C].index_add_(1, t, w * xm)
            if want_abs:
                r.abs_out[:, :, off:off + C].index_add_(1, t, (w * xm).abs())
            if g_ is None:
                continue
            gm = g_[:, t, off:off + C]
            dx.index_add_(1, p, w * gm)
            dot = (gm * xm).sum(-1)                                   # (N, m)
            rows.index_add_(1, p, dot.unsqueeze(-1) * coef.unsqueeze(0))
            if want_abs:
                adx.index_add_(1, p, (w * gm).abs())
                aterm = (gm * xm).abs().sum(-1).unsqueeze(-1) * coef.abs().unsqueeze(0)
                arows.index_add_(1, p, aterm)
                r.abs_theta_tgt.index_add_(1, t, aterm.double())
        if g_ is not None:
            r.dx.append(dx.double().view(N, Hin, Win, C))
            r.rows.append(rows.double().view(N * Hin * Win, 6))
            if want_abs:
                r.abs_dx.append(adx.double().view(N, Hin, Win, C))
                r.abs_rows.append(arows.double().view(N * Hin * Win, 6))
    r.out = r.out.double().view(N, Ho, Wo, ldo)
    if want_abs:
        r.abs_out = r.abs_out.double().view(N, Ho, Wo, ldo)
    if g_ is not None:
        if dtype == F64:
            r.dtheta = sum(rows.sum(0) for rows in r.rows)
        else:        # the float32 evaluation keeps to float32 to the end
            r.dtheta = sum(rows.to(dtype).sum(0) for rows in r.rows).double()
        if want_abs:
            r.abs_dtheta = sum(a.sum(0) for a in r.abs_rows)
            r.abs_theta_tgt = r.abs_theta_tgt.view(N * Ho * Wo, 6)
    return r


def theta_waves(pixels):
    """waves of the stand-alone theta kernel (sampler.hip theta_blocks() x 4): wave v keeps FLOAT sums over the target pixels
    v, v + waves, ... and all sources"""
    return 4 * max(1, min((pixels + 15) // 16, 1024))


def inexact_in_fp32(res):
    """the premise of the bit-for-bit cases: x and dy are integers and every weight is dyadic, so every term is a multiple of
    2^-f (f = the fraction bits of the weights / coefficients); with (sum of |terms|) * 2^f < 2^24 every partial sum, in any
    order, is an integer below 2^24 in units of 2^-f: exact in float32.  Float sums are kept per output element (out, dx), per
    source pixel (the theta rows of the gather kernels; they go on in double: 29 bits to spare) and per wave over its target
    pixels (the stand-alone theta kernel, then double); d theta itself is rounded to float once, so IT must fit: |d theta| * 2^f
    < 2^24.  Returns None when the premise holds, else what breaks it."""
    cap = 2.0 ** 24
    fo, ft = 0, [0] * 6
    for i, geo in enumerate(res.geo):
        fw = fraction_bits(geo.w)
        if fw is None:
            return f"source {i}: weights are not dyadic"
        fo = max(fo, fw)
        if not float(res.abs_dx[i].max()) * 2.0 ** fw < cap:
            return f"dx of source {i} may round"
        for k in range(6):
            fk = fraction_bits(geo.coef[:, k])
            if fk is None:
                return f"source {i}: theta coefficient {k} is not dyadic"
            ft[k] = max(ft[k], fk)
            if not float(res.abs_rows[i][:, k].max()) * 2.0 ** fk < cap:
                return f"theta rows of source {i} may round"
    if not float(res.abs_out.max()) * 2.0 ** fo < cap:
        return "out may round"
    pixels = res.abs_theta_tgt.shape[0]
    waves = theta_waves(pixels)
    per_wave = torch.zeros(waves, 6, dtype=F64).index_add_(0, torch.arange(pixels) % waves, res.abs_theta_tgt)
    for k in range(6):
        if not float(per_wave[:, k].max()) * 2.0 ** ft[k] < cap:
            return f"a wave's sum for d theta[{k}] may round"
        if not float(res.abs_dtheta[k]) * 2.0 ** ft[k] < 2.0 ** 53:
            return f"the double sum for d theta[{k}] may round"
        if not abs(float(res.dtheta[k])) * 2.0 ** ft[k] < cap:
            return f"d theta[{k}] = {float(res.dtheta[k])} has more than 24 bits ({ft[k]} fraction bits)"
    return None


def assert_exact_in_fp32(res, what=""):
    why = inexact_in_fp32(res)
    assert why is None, f"{what}: {why}"


# ---------------------------------------------------------------------------------------------------------------------
# the exact grids (test_sampler_edges_gpu.py section a; test_sampler_reference.py checks their premise): Wo - 1, Ho - 1 and
# every source extent - 1 are powers of two and theta is dyadic, so every coordinate is exact in float32
EXACT_THETAS = {
    "identity": (1, 0, 0, 0, 1, 0),                      # multi_init.py:72; a same-size source is sampled ON its pixels
    "onto_border": (1, 0, -0.5, 0, 1, -0.5),             # a 5-wide source: target column 0 sits exactly on x = -1
    "onto_last": (1, 0, 0.5, 0, 1, 0.5),                 # a 5-wide source: samples exactly on the last pixel, then beyond it
    "zoom_out": (1.5, 0, 0, 0, 1.5, 0),                  # a border of zeros; a 5-wide source starts exactly on x = -1
    "zoom_in": (0.5, 0, 0, 0, 0.5, 0),
    "shear": (1, 0.25, 0, 0.5, 1, -0.25),
}
# (Ho, Wo), [(Hin, Win)]: the target's own size, extents 2 .. 65, square and not
EXACT_TARGETS = [((17, 17), [(17, 17), (5, 5), (9, 3)]),
                 ((33, 17), [(33, 17), (2, 2), (5, 9), (17, 33)]),
                 ((65, 65), [(65, 65), (33, 33), (3, 5)])]
EXACT_N, EXACT_C = 2, 4


def exact_case(target, shapes, theta, seed=0):
    """integer x and dy for one exact-grid case, thinned until inexact_in_fp32() passes: (sources, dy, reference)"""
    Ho, Wo = target
    ldo = EXACT_C * len(shapes) + 4
    for thin in (1, 2, 4, 8, 16, 32, 64):
        g = torch.Generator().manual_seed(seed + 1000 * thin)
        srcs = [(torch.randint(-3, 4, (EXACT_N, h, w, EXACT_C), generator=g).double(), 4 + EXACT_C * i) for i, (h, w) in enumerate(shapes)]
        dy = torch.randint(-3, 4, (EXACT_N, Ho, Wo, ldo), generator=g).double()
        if thin > 1:      # keep every thin-th target pixel (all channels), at random
            dy = dy * (torch.randint(0, thin, (EXACT_N, Ho, Wo, 1), generator=g) == 0)
        ref = sampler(srcs, theta, Ho, Wo, dy)
        if inexact_in_fp32(ref) is None:
            return srcs, dy, ref, thin
    raise AssertionError(f"no exact inputs for {target} {shapes} {theta}: {inexact_in_fp32(ref)}")


def coordinates_exact_in_fp32(theta, Hin, Win, Ho, Wo):
    """True when the source coordinates of every target pixel, computed in float32 step by step as tgt_coord / src_xy write
    them, equal the float64 ones -- with every intermediate exact, so that a fused multiply-add changes nothing either"""
    f32 = torch.float32
    th = torch.tensor(theta, dtype=F64)
    if not bool((th.float().double() == th).all()):
        return False
    ok = True

    def rnd(v):                     # a float64 result of float32 operands: must survive the rounding to float32
        nonlocal ok
        ok = ok and bool((v.to(f32).double() == v).all())
        return v.to(f32).double()

    def coord(O):
        if O <= 1:
            return torch.zeros(1, dtype=F64)
        k = rnd(torch.tensor(2.0, dtype=F64) / float(O - 1))
        return rnd(-1.0 + rnd(torch.arange(O, dtype=F64) * k))
    xt = coord(Wo).view(1, -1)
    yt = coord(Ho).view(-1, 1)
    out = []
    for a, b, c, ext in ((th[0], th[1], th[2], Win), (th[3], th[4], th[5], Hin)):
        g = rnd(rnd(rnd(a * xt) + rnd(b * yt)) + c)
        s = rnd(rnd(rnd(g + 1.0) * float(ext - 1)) / 2.0)
        out.append(s)
    geo = Geometry(theta, Hin, Win, Ho, Wo)
    return ok and torch.equal(out[0].expand(Ho, Wo).clamp(-2.0, Win + 1.0), geo.xs) and \
        torch.equal(out[1].expand(Ho, Wo).clamp(-2.0, Hin + 1.0), geo.ys)


def rows_per_pixel(part, pixels):
    """theta_partial as affine_sampler_backward_data_theta leaves it, (pixels * chunks, 6) with a pixel's chunks adjacent ->
    (pixels, 6)"""
    return part.view(pixels, -1, 6).sum(1)


def host_rows(Ho, Hin):
    """`rows` of the host routing in sampler.hip: the nominal height of a source pixel's pre-image box"""
    return 2 * math.ceil(Ho / Hin) + 2


# ---------------------------------------------------------------------------------------------------------------------
# the host-side routing of sampler.hip, restated
B1, B4 = "sampler_bwd_data_batched_kernel<1>", "sampler_bwd_data_batched_kernel<4>"
P1, P4, P16 = "sampler_bwd_data_kernel<1>", "sampler_bwd_data_kernel<4>", "sampler_bwd_data_kernel<16>"
CH = "sampler_bwd_data_kernel<4> x 8 chunks + sampler_bwd_reduce_kernel"


def route(N, Hin, Win, C, Ho, theta_rows=True, batched=True, half=False):
    """the kernel a data-gradient call reaches: affine_sampler_backward_data_theta (theta_rows) or affine_sampler_backward_data"""
    rows = host_rows(Ho, Hin)
    if theta_rows and not half and rows >= 32 and N * Hin * Win <= 4096:
        return "sampler_bwd_data_kernel<4> x 8 chunks + sampler_bwd_reduce_kernel"
    if batched and rows < 32 and C // 4 <= 64:
        return "sampler_bwd_data_batched_kernel<%d>" % (4 if rows >= 10 else 1)
    return "sampler_bwd_data_kernel<%d>" % (16 if rows >= 32 else 4 if rows >= 10 else 1)


def batched_gy(N, Hin, Win):
    """workgroups per source position of the batched kernel; each has 4 waves, one image per wave and trip"""
    pos = Hin * Win
    return max(1, min((N + 3) // 4, (2048 + pos - 1) // pos))



# ---------------------------------------------------------------------------------------------------------------------
# the long sums (test_sampler_edges_gpu.py section c; their premises are asserted in test_sampler_reference.py)
OUT_BAR, DX_BAR, ROWS_BAR, DTH_BAR = 1e-5, 1e-5, 1e-4, 1e-4      # the project's bars: test_nn_gpu.py


class Bars:
    """relative to the largest reference entry; None: bit for bit"""

    def __init__(self, out=OUT_BAR, dx=DX_BAR, rows=ROWS_BAR, dth=DTH_BAR):
        self.out, self.dx, self.rows, self.dth = out, dx, rows, dth


# id: theta, [(Hin, Win)], kernel of the data + theta call
LONG_CASES = {
    "minify": ((0.03, 0.01, 0.2, -0.02, 0.04, -0.1), [(16, 16)], B4, (64, 64)),        # thousands of matches per position: the list overflows
    "straddle": ((0.31, 0.02, 0.05, -0.03, 0.29, -0.04), [(16, 16)], B4, (64, 64)),    # listed and walked positions in one launch
    "degenerate": ((1e-12, 1e-12, 0.02, 1e-12, 1e-12, -0.04), [(8, 8)], B4, (32, 32)), # det == 0: the whole target is the box
    "chunked": ((0.97, 0.04, -0.03, -0.05, 1.04, 0.02), [(2, 2), (3, 5)], CH, (64, 64)),
}
LONG_N, LONG_C, LIST_CAP = 3, 8, 768


def long_case(name):
    """(sources, dy, float64 reference, bars, what was measured)"""
    theta, shapes, _, (LONG_HO, LONG_WO) = LONG_CASES[name]
    g = torch.Generator().manual_seed(7 + len(name))
    srcs = []
    for i, (h, w) in enumerate(shapes):
        ramp = 1.0 + 0.1 * torch.arange(h, dtype=F64).view(1, h, 1, 1) + 0.05 * torch.arange(w, dtype=F64).view(1, 1, w, 1) \
            + 0.02 * torch.arange(LONG_C, dtype=F64).view(1, 1, 1, LONG_C)
        srcs.append(((ramp + 0.1 * torch.randn(LONG_N, h, w, LONG_C, generator=g, dtype=F64)).float().double(), 4 + LONG_C * i))
    dy = (torch.rand(LONG_N, LONG_HO, LONG_WO, 4 + LONG_C * len(shapes) + 4, generator=g, dtype=F64) + 0.5).float().double()
    dy, _ = off_the_kinks(dy, theta, shapes, LONG_HO, LONG_WO)
    r64 = sampler(srcs, theta, LONG_HO, LONG_WO, dy, want_abs=False)
    r32 = sampler(srcs, theta, LONG_HO, LONG_WO, dy, want_abs=False, dtype=torch.float32)
    assert max(int(c.max()) for c in r64.counts) > 256, "not a long sum"

    def rel(a, b):
        return max(float((p - q).abs().max()) for p, q in zip(a, b)) / max(float(q.abs().max()) for q in b)
    measured = {"dx": rel(r32.dx, r64.dx), "rows": rel(r32.rows, r64.rows), "dth": rel([r32.dtheta], [r64.dtheta])}
    bars = Bars(OUT_BAR, max(DX_BAR, 4 * measured["dx"]), max(ROWS_BAR, 4 * measured["rows"]), max(DTH_BAR, 4 * measured["dth"]))
    return srcs, dy, r64, bars, measured


_long = {}


def long_case_once(name):
    if name not in _long:
        _long[name] = long_case(name)
    return _long[name]


def ambiguous_pixels(theta, shapes, Ho, Wo):
    """(Ho, Wo) mask of the target pixels for which a generic grid fixes NO reference for the gradients: float32 rounding can
    move the sample across a source pixel row or column of one of the sources, and which one-sided derivative is taken
    depends on that rounding.  A pixel counts when its floor cell differs from the float64 one under any float32 evaluation
    `fp contract(fast)` allows for tgt_coord and src_xy -- the coordinate -1 + o * k stepwise or as one fused multiply-add,
    t0 xt + t1 yt + t2 stepwise or with either product fused into the first addition (a fused multiply-add is emulated in
    double: the product of two floats is exact there) -- or when it lies within 16 float32 ulps of the largest coordinate
    from an integer without being computed exactly.  A sample computed exactly (the middle row of an odd target under a
    theta without shear, an exact grid) is on its pixel in any precision and stays in.  The tests zero dy at these
    pixels: the kinks themselves are checked bit for bit on the exact grids."""
    f32 = torch.float32
    th = torch.tensor(theta, dtype=F64).float().double()
    mask = torch.zeros(Ho, Wo, dtype=torch.bool)

    def rn(v):
        return v.to(f32).double()

    def coords(O):
        if O <= 1:
            return [torch.zeros(1, dtype=F64)]
        k = rn(torch.tensor(2.0, dtype=F64) / float(O - 1))
        o = torch.arange(O, dtype=F64)
        return [rn(-1.0 + rn(o * k)), rn(-1.0 + o * k)]
    for Hin, Win in shapes:
        want = Geometry(theta, Hin, Win, Ho, Wo)
        for xt in coords(Wo):
            for yt in coords(Ho):
                xt_, yt_ = xt.view(1, -1), yt.view(-1, 1)
                for (a, b, c, ext, ref) in ((th[0], th[1], th[2], Win, want.xs), (th[3], th[4], th[5], Hin, want.ys)):
                    if ext == 1:
                        continue          # pinned to exactly 0
                    for g in (rn(rn(a * xt_) + rn(b * yt_)), rn(rn(a * xt_) + b * yt_), rn(a * xt_ + rn(b * yt_))):
                        g = rn(g + c)
                        s = rn(rn(rn(g + 1.0) * float(ext - 1)) / 2.0).expand(Ho, Wo).clamp(-2.0, ext + 1.0)
                        close = ((ref - ref.round()).abs() <= 16 * 2.0 ** -24 * (ext + 1)) & (ref > -1.5) & (ref < ext + 0.5)
                        mask |= (s.floor() != ref.floor()) | (close & (s != ref))
    return mask


def off_the_kinks(dy, theta, shapes, Ho, Wo):
    """dy with the ambiguous target pixels zeroed"""
    m = ambiguous_pixels(theta, shapes, Ho, Wo)
    dy = dy.clone()
    dy[:, m] = 0
    return dy, int(m.sum())
