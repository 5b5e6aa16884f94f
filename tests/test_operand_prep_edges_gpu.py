"""The stand-alone kernels that prepare the operands of the two-piece ("f16x2") convolution math, at their edges, against the
numpy restatements of tests/ref_operand_prep.py: absmax_kernel (plain and both coefficient paths of the affine form, past its
2048-workgroup cap), absmax_batch_kernel, absmin_rows_batch_kernel, tile_minmax_kernel, absmax_affine_bound_kernel, the two
split-K slab reductions, the non-batch weight_transpose_kernel and the transposed weight planes of layers whose channel count
is no multiple of 32.

Every comparison is exact (bit for bit) -- these kernels are selections, fixed-order sums and exact splits -- except the
affine bound, whose bar (one fused or two separate roundings: 2^-23 relative) is derived in its test.  Every output buffer
sits between NaN guards and is pre-filled (NaN, or a known value where "max into" / "min into" is the contract).

PINNED, not derived (the code that defines each):
  * a NaN coefficient of absmax's affine form never reaches the block: fmaxf skips it with relu off, the ReLU's fmaxf(u, 0)
    turns it into 0 with relu on (csrc/conv.hip absmax_kernel) -- that channel contributes nothing either way;
  * a row whose only non-zero value is subnormal counts for absmin_rows (csrc/conv_wide.hip: m > 0.f, denormals kept);
  * a channel that is all NaN in a tile leaves tile_minmax's initial +inf / -inf (csrc/conv_wide.hip tile_minmax_kernel);
  * absmax_affine_bound: a NaN coefficient gives +inf, an inf slot of x_absmax gives +inf (csrc/nn.hip);
  * operand_scale clamps its exponent to [-100, 100] (csrc/dspn_pieces.h): a block whose maximum is just under 3e38 scales by
    2^-100 only, elements above 65504 * 2^100 overflow fp16 and leave the weight-plane kernel as repair_inf's +-65504 / +-inf."""
import numpy as np
import pytest
import torch

from dspnet_amd import functional as fn
import ref_operand_prep as P

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN, INF = float("nan"), float("inf")
S = fn.ABSMAX_SLOTS
ABSMAX_CAP, SLAB_CAP, WT_CAP = 2048, 16384, 4096       # workgroups of 256 threads: csrc/conv.hip dspn_absmax_f32, dspn_conv2d_slab_reduce_batch_f32, dspn_conv2d_weight_transpose_f32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Guarded:
    """an output of n elements between two guards of `guard` NaNs (n and guard multiples of 4 keep float4 alignment)"""

    def __init__(self, n, fill=NAN, guard=64, dtype=torch.float32):
        self.whole = torch.full((n + 2 * guard,), NAN, device="cuda", dtype=dtype)
        self.view = self.whole[guard:guard + n]
        self.view.fill_(fill)
        self.n, self.guard = n, guard

    def intact(self):
        g = self.guard
        return bool(torch.isnan(self.whole[:g]).all()) and bool(torch.isnan(self.whole[g + self.n:]).all())


def block(fill=0.0):
    return Guarded(S, fill)


# ---------------------------------------------------------------------------------------------------------------------
# fn.absmax, plain
PLAIN_N4 = [1, 63, 64, 255, 256, 257, 16385, ABSMAX_CAP * 256 + 1]


def plant_positions(n4):
    """(label, element index): first, last, each lane of the last float4, the first element of workgroup 64 (slot wrap)"""
    n = 4 * n4
    pos = [("first", 0), ("last", n - 1)] + [(f"lane {k} of the last float4", n - 4 + k) for k in range(4)]
    if n4 > 64 * 256:
        pos.append(("first of workgroup 64", 64 * 256 * 4))
    return pos


@pytest.mark.parametrize("n4", PLAIN_N4)
def test_absmax_plain_finds_a_planted_maximum_wherever_it_sits(gpu_device, n4):
    """one planted extreme (negative in every other case) among |values| < 1; past the 2048-workgroup cap the last float4 is
    reached only on the second grid trip"""
    g = torch.Generator(device="cuda").manual_seed(n4)
    x = (torch.rand(n4, 4, device="cuda", generator=g) * 2 - 1) * 0.999
    mags = torch.unique(x.abs())
    flat = x.view(-1)
    for k, (label, at) in enumerate(plant_positions(n4)):
        v = (1.5 + k) * (-1.0 if k % 2 else 1.0)
        keep = float(flat[at])
        flat[at] = v
        out = block()
        fn.absmax(x, out=out.view)
        b = out.view
        assert float(b.max()) == abs(v), (label, float(b.max()), v)
        assert bool(((b == 0) | (b == abs(v)) | torch.isin(b, mags)).all()), f"{label}: a slot holds a value that is no |element|"
        assert out.intact(), label
        flat[at] = keep


def test_absmax_takes_the_maximum_into_the_block(gpu_device):
    x = dev(np.linspace(-3.0, 2.0, 4 * 257, dtype=F32).reshape(257, 4))
    larger = block(5000.0)
    before = bits(larger.whole).clone()
    fn.absmax(x, out=larger.view)
    assert torch.equal(bits(larger.whole), before)                       # a larger block keeps every bit
    smaller = block(0.001)
    fn.absmax(x, out=smaller.view)
    assert float(smaller.view.max()) == 3.0 and float(smaller.view.min()) >= 0.001 and smaller.intact()
    pattern = Guarded(S)
    pattern.view.copy_(torch.arange(S, device="cuda") * 0.25)
    before = bits(pattern.whole).clone()
    fn.absmax(torch.zeros(257, 4, device="cuda"), out=pattern.view)
    assert torch.equal(bits(pattern.whole), before)                      # an all-zero tensor changes nothing
    fn.absmax(torch.full((257, 4), -0.0, device="cuda"), out=pattern.view)
    assert torch.equal(bits(pattern.whole), before)                      # -0.0 contributes nothing


@pytest.mark.parametrize("inf", [INF, -INF])
def test_absmax_special_values(gpu_device, inf):
    """NaN elements are skipped; one infinity makes the magnitude inf while the workgroups that did not see it still publish
    their finite maximum -- csrc/dspn_pieces.h: the operand scale comes from the finite slots"""
    n4 = 16385                                            # 65 workgroups: workgroup 64 shares slot 0 with workgroup 0
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (n4, 4)).astype(F32)
    x[rng.random((n4, 4)) < 0.01] = NAN
    x[5 * 256 + 17, 2] = -7.5                             # workgroup 5: the finite maximum
    x[5 * 256 + 18, 1] = NAN
    out = block()
    fn.absmax(dev(x), out=out.view)
    assert float(out.view.max()) == 7.5 == float(P.absmax_ref(x)) and not bool(torch.isnan(out.view).any())
    x[3 * 256 + 100, 3] = inf                             # workgroup 3
    out = block()
    fn.absmax(dev(x), out=out.view)
    assert float(out.view.max()) == INF == float(P.absmax_ref(x))
    assert int((out.view == INF).sum()) == 1 and bool((out.view == 7.5).any()) and out.intact()
    assert not bool(torch.isnan(out.view).any())
    all_nan = block(0.5)
    fn.absmax(torch.full((300, 4), NAN, device="cuda"), out=all_nan.view)
    assert bool((all_nan.view == 0.5).all())


# ---------------------------------------------------------------------------------------------------------------------
# fn.absmax with an input affine: both coefficient paths
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("kind", P.AFFINE_KINDS)
@pytest.mark.parametrize("rows,C", P.AFFINE_SHAPES, ids=str)
def test_absmax_affine_on_both_coefficient_paths(gpu_device, rows, C, kind, relu):
    """C = 64: the grid stride is a multiple of C / 4, every thread keeps one channel group (one trip at 5 rows, two at
    32769); C = 12: C / 4 = 3 divides no power of two, the general path (7 rows, and one float4 past the cap).  The planted
    element is in the last row.  A NaN scale (PINNED): that channel contributes nothing -- fmaxf skips the NaN with relu
    off, the ReLU's fmaxf(u, 0) makes it 0 with relu on."""
    n4 = rows * C // 4
    assert (min((n4 + 255) // 256, ABSMAX_CAP) * 256 % (C // 4) == 0) == (C == 64), "the shape is on the other path"
    assert (n4 > ABSMAX_CAP * 256) == (rows > 1000), "the trip count of the shape"
    x, scale, shift = P.affine_case(kind, rows, C)
    want = P.absmax_ref(x, scale, shift, relu)
    out = block()
    fn.absmax(dev(x), (dev(scale), dev(shift), relu), out=out.view)
    got = out.view
    assert float(got.max()) == float(want), (float(got.max()), float(want))
    assert not bool(torch.isnan(got).any()) and out.intact()
    if kind == "tiny_scale":
        assert float(got.max()) < 4096.0 * 2.0 ** -8      # the largest |x| is not the largest |u|
    if kind in ("negative_extreme", "nan_scale"):
        assert float(got.max()) == (9.25 if relu else 79.5)


# ---------------------------------------------------------------------------------------------------------------------
# fn.absmax_batch
BATCH_N4 = [1, 1023, 1024, 1025, 4096, 65 * 1024 + 1]


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_absmax_batch_keeps_every_tensor_to_itself(gpu_device, order):
    """the tensors lie back to back in one buffer; each maximum is the tensor's LAST element, and the element right behind
    it -- the next tensor's first -- is twice as large: a chunk that reads across the boundary, or a row search that is one
    off, shows.  65 * 1024 + 1 float4 are 66 chunks: the slot index wraps."""
    sizes = BATCH_N4 if order == "ascending" else BATCH_N4[::-1]
    rng = np.random.default_rng(len(order))
    buf = rng.uniform(-1, 1, 4 * sum(sizes) + 4).astype(F32)
    maxima, views, at = [], [], 0
    for i, n4 in enumerate(sizes):
        m = 10.0 * 3.0 ** i
        if i:
            buf[at] = -2.0 * maxima[-1]                   # the first element: twice the previous tensor's maximum
        buf[at + 4 * n4 - 1] = m if i % 2 else -m
        maxima.append(m)
        views.append((at, 4 * n4))
        at += 4 * n4
    buf[at] = 2.0 * maxima[-1]                            # (behind the last tensor)
    d = dev(buf)
    outs = Guarded(S * (2 * len(sizes) - 1), guard=64)
    blocks = [outs.view[2 * S * i:2 * S * i + S] for i in range(len(sizes))]       # a NaN sentinel block between two outputs
    for b in blocks:
        b.zero_()
    fn.absmax_batch(*fn.absmax_table([(d[a:a + n], b) for (a, n), b in zip(views, blocks)], d.device))
    for i, ((a, n), b) in enumerate(zip(views, blocks)):
        assert float(b.max()) == maxima[i] == float(P.absmax_ref(buf[a:a + n])), (order, sizes[i], float(b.max()), maxima[i])
        assert bool(((b == 0) | torch.isin(b, d[a:a + n].abs())).all()), (order, sizes[i])
    for i in range(len(sizes) - 1):
        assert bool(torch.isnan(outs.view[2 * S * i + S:2 * S * (i + 1)]).all()), "the sentinel between two blocks was written"
    assert outs.intact()
    # max into: a second launch over blocks that already hold more changes nothing
    for b in blocks:
        b.fill_(1e9)
    before = bits(outs.whole).clone()
    fn.absmax_batch(*fn.absmax_table([(d[a:a + n], b) for (a, n), b in zip(views, blocks)], d.device))
    assert torch.equal(bits(outs.whole), before)


# ---------------------------------------------------------------------------------------------------------------------
# fn.absmin_rows_batch
def absmin_weights(seed):
    rng = np.random.default_rng(seed)
    tiny = F32(5 * 2.0 ** -149)

    def rand(rows, n):
        return rng.uniform(0.5, 4.0, (rows, n)).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), (rows, n))
    ws = []
    ws.append(np.array([[-0.75]], F32) * (seed + 1))                               # (1, 1)
    w = rand(3, 255); w[0] = 0.0; w[1, 77] = INF; w[2, 254] = -8.0 - seed          # zero row, inf among finite values, a plain row
    ws.append(w)
    w = rand(4, 256); w[0] = NAN; w[1] = 0.0; w[1, 255] = -tiny                    # a row of NaNs, a row whose only value is subnormal
    ws.append(w)
    w = rand(5, 257) * F32(0.01); w[3] *= F32(0.001); w[3, 256] = 2.0 ** -10 / (seed + 1)   # the deciding value is element 256: the second pass of the row loop
    ws.append(w)
    w = rand(64, 4608); w[0] = 0.0; w[1, 4000] = -INF; w[2] = NAN; w[63] = 0.0; w[63, 4607] = tiny * (2 - seed)
    ws.append(w)
    w = rand(19, 1000); w[rng.random((19, 1000)) < 0.05] = NAN; w[18] *= F32(2.0 ** -(7 + seed)); w[18, 999] = NAN
    ws.append(w)
    w = rand(3, 255); w[0] = 0.0; w[1] = NAN; w[2, 0] = INF                        # no qualifying row
    ws.append(w)
    return ws


def test_absmin_rows_batch_takes_the_smallest_qualifying_row(gpu_device):
    """rows that are all zero, hold an inf, hold only NaNs, or hold one subnormal; the outputs start at +inf and only go down:
    the second launch, on other values, does not reset them"""
    shapes = [(1, 1), (3, 255), (4, 256), (5, 257), (64, 4608), (19, 1000), (3, 255)]
    first, second = absmin_weights(0), absmin_weights(1)
    assert [w.shape for w in first] == shapes
    outs = Guarded(4 * len(shapes), guard=4)
    cells = [outs.view[4 * i:4 * i + 1] for i in range(len(shapes))]                # NaN sentinels between the outputs
    for c in cells:
        c.fill_(INF)
    want = [P.absmin_rows_ref(w) for w in first]
    assert float(want[2]) == 5 * 2.0 ** -149 and float(want[4]) == 10 * 2.0 ** -149 and float(want[6]) == INF      # the cases are what they claim
    assert float(P.absmin_rows_ref(np.where(np.isinf(first[1]), F32(1.0), first[1]))) != float(want[1])              # the inf row would win were the inf a number
    d = [dev(w) for w in first]
    fn.absmin_rows_batch(*fn.absmin_rows_table(list(zip(d, cells)), "cuda"))
    got = [float(c) for c in cells]
    assert got == [float(v) for v in want], (got, want)
    d2 = [dev(w) for w in second]
    fn.absmin_rows_batch(*fn.absmin_rows_table(list(zip(d2, cells)), "cuda"))
    want2 = [min(float(a), float(P.absmin_rows_ref(w))) for a, w in zip(want, second)]
    got2 = [float(c) for c in cells]
    assert got2 == want2, (got2, want2)
    assert any(b < a for a, b in zip(got, got2)) and any(b == a and a < INF for a, b in zip(got, got2))       # some went down, some stayed
    mask = torch.ones(4 * len(shapes), dtype=torch.bool, device="cuda")
    mask[::4] = False
    assert bool(torch.isnan(outs.view[mask]).all()) and outs.intact()
    # "no row qualifies" means the output is not written at all: a cell that holds the NaN sentinel (as an unsigned word above
    # every float, +inf included) keeps it behind a weight whose rows are zero, NaN and inf; a qualifying weight replaces it
    cells[6].fill_(NAN)
    cells[1].fill_(NAN)
    fn.absmin_rows_batch(*fn.absmin_rows_table([(d[6], cells[6]), (d[1], cells[1])], "cuda"))
    assert bool(torch.isnan(cells[6]).all()) and float(cells[1]) == float(want[1])


# ---------------------------------------------------------------------------------------------------------------------
# fn.tile_minmax
@pytest.mark.parametrize("C", [4, 1024, 1028])
@pytest.mark.parametrize("rows,tile_rows", [(1, 1), (7, 3), (64, 64), (65, 64), (100, 256)])
def test_tile_minmax_at_ragged_tiles_and_channel_counts(gpu_device, rows, tile_rows, C):
    """C = 1028 is 257 float4 groups: one past a 256-thread pass, the second gridDim.y block.  Negatives, NaNs, +-inf; a
    channel that is all NaN in a tile leaves the initial +inf / -inf (PINNED: tile_minmax_kernel's initial values)."""
    rng = np.random.default_rng(rows * 1000 + C)
    x = rng.standard_normal((rows, C)).astype(F32)
    x[rng.random((rows, C)) < 0.05] = NAN
    x[rng.random((rows, C)) < 0.01] = INF
    x[rng.random((rows, C)) < 0.01] = -INF
    x[:tile_rows, C - 1] = NAN                          # all NaN in the first tile, last channel
    x[:, 1] = NAN                                       # ... and in every tile
    tiles = -(-rows // tile_rows)
    want = P.tile_minmax_ref(x, tile_rows)
    assert want[0, 0, C - 1] == INF and want[0, 1, C - 1] == -INF and not np.isnan(want).any()
    out = Guarded(tiles * 2 * C)
    fn.tile_minmax(dev(x), tile_rows, out.view.view(tiles, 2, C))
    assert np.array_equal(host(out.view).view(np.int32), want.reshape(-1).view(np.int32)) and out.intact()


def test_tile_minmax_reproduces_the_conv_epilogue_table(gpu_device):
    """the range guard's fallback refills out_minmax with tile_minmax over the stored output (engine.py Conv._forward_fallback):
    on a two-piece convolution's own output that pass must reproduce the table the epilogue wrote, bit for bit.  Shape: the
    "64 rows: 1" case of test_conv_edges_gpu.py STATS_CASES -- 65 output rows, the last tile holds one."""
    N, H, W, Cin, Cout = 1, 5, 13, 32, 64
    g = torch.Generator().manual_seed(65)
    x = torch.randn(N, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, 1, 1, Cin, generator=g) / Cin ** 0.5).cuda()
    M = N * H * W
    tiles, tile_rows = fn.conv_stats_layout(M, Cout)
    assert tiles >= 2 and M % tile_rows != 0, "the case has lost its ragged last tile"
    st = torch.full((tiles, 2, Cout), NAN, device="cuda")
    mm = torch.full((tiles, 2, Cout), NAN, device="cuda")
    y = fn.conv2d_forward(x, w, out_stats=st, out_minmax=mm, math="f16x2")
    again = Guarded(tiles * 2 * Cout)
    fn.tile_minmax(y.view(M, Cout), tile_rows, again.view.view(tiles, 2, Cout))
    assert not bool(torch.isnan(mm).any())
    assert torch.equal(bits(again.view), bits(mm.view(-1))) and again.intact()
    assert np.array_equal(host(mm).view(np.int32), P.tile_minmax_ref(host(y).reshape(M, Cout), tile_rows).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# fn.absmax_affine_bound
def magnitude_block(form, m):
    b = np.zeros(S, F32)
    if form == "slot 0":
        b[0] = m
    elif form == "slot 63":
        b[63] = m
    else:
        b[:] = np.linspace(0.0, 1.0, S, dtype=F32) * F32(m)
        b[37] = m
    return b


@pytest.mark.parametrize("form", ["slot 0", "slot 63", "spread"])
@pytest.mark.parametrize("C", [1, 4, 255, 256, 257, 2048])
def test_absmax_affine_bound_is_the_bound_it_says(gpu_device, C, form):
    """out.max() against B = max_c |scale_c| M + |shift_c| in float64.  BAR (derived, not measured): the kernel evaluates
    |scale| * M + |shift| in float32 as one fused operation (one rounding) or as a product and a sum (two); every term is
    non-negative, so the result is within (1 + 2^-24)^2 - 1 < 2^-23 of the exact value, relative; max is exact.  And it is a
    bound: for any x with |x| <= M the magnitude of (relu)(x * scale + shift) as the fmaf gives it is at most
    B (1 + 2^-24), so the result may not lie below absmax_ref(x, scale, shift, relu) * (1 - 2^-22)."""
    rng = np.random.default_rng(C)
    M = F32(3.7)
    scale, shift = rng.standard_normal(C).astype(F32), rng.standard_normal(C).astype(F32)
    c = C - 1                                             # the deciding channel: the last one (the second pass of the loop at C > 256)
    scale[c], shift[c] = F32(-1.25), F32(-50.0)           # a NEGATIVE shift decides
    want = P.affine_bound_f64(scale, shift, M)
    assert want == 1.25 * float(M) + 50.0
    out = block()
    fn.absmax_affine_bound(dev(scale), dev(shift), dev(magnitude_block(form, M)), out.view)
    got = float(out.view.max())
    assert abs(got - want) <= 2.0 ** -23 * want, (got, want)
    assert bool(((out.view == 0) | (out.view == got)).all()) and out.intact()
    x = rng.uniform(-1, 1, (50, C)).astype(F32) * M
    x[7, c] = M                                           # x * scale + shift = -(1.25 M + 50): the bound is attained
    for relu in (False, True):
        assert got >= float(P.absmax_ref(x, scale, shift, relu)) * (1 - 2.0 ** -22), relu


def test_absmax_affine_bound_special_cases(gpu_device):
    """PINNED (csrc/nn.hip absmax_affine_bound_kernel): a NaN coefficient gives +inf (no finite bound exists); an inf slot in
    x_absmax gives out.max() == inf -- and since the kernel writes ONE slot of out, a zeroed out block then holds no finite
    positive slot: operand_scale (csrc/dspn_pieces.h) reads the finite slots only and returns 1, the convolution runs
    unscaled."""
    C = 300
    rng = np.random.default_rng(9)
    scale, shift = rng.standard_normal(C).astype(F32), rng.standard_normal(C).astype(F32)
    xa = dev(magnitude_block("spread", 2.0))
    for which in ("scale", "shift"):
        s2, h2 = scale.copy(), shift.copy()
        (s2 if which == "scale" else h2)[299] = NAN
        out = block()
        fn.absmax_affine_bound(dev(s2), dev(h2), xa, out.view)
        assert float(out.view.max()) == INF and not bool(torch.isnan(out.view).any()) and out.intact(), which
    larger = block(1e6)
    before = bits(larger.whole).clone()
    fn.absmax_affine_bound(dev(scale), dev(shift), xa, larger.view)
    assert torch.equal(bits(larger.whole), before)
    untouched = Guarded(S)
    untouched.view.copy_(torch.arange(S, device="cuda") * 0.5)
    before = bits(untouched.whole).clone()
    fn.absmax_affine_bound(torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(S, device="cuda"), untouched.view)
    assert torch.equal(bits(untouched.whole), before)
    b = magnitude_block("spread", 2.0)
    b[5] = INF
    out = block()
    fn.absmax_affine_bound(dev(scale), dev(shift), dev(b), out.view)
    assert float(out.view.max()) == INF and out.intact()
    assert float(P.operand_scale_ref(host(out.view))) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# split-K slab reductions
SLAB_SPLITS = [1, 2, 15, 16, 17, 18, 32, 33, 49]      # around the 16-row batches, which start at k = 1


def slab_entries(seed=0):
    rng = np.random.default_rng(seed)
    es = []
    for i, (splits, n4) in enumerate((s, n) for s in SLAB_SPLITS for n in (1, 300)):
        acc = (i // 2 + i) % 2 == 1                      # mixed over the table, both values at every size
        es.append((P.wide_values((splits, 4 * n4), rng), P.wide_values((4 * n4,), rng), acc))
    return es


def run_slab_table(entries):
    """-> [(got, guard intact)] per entry: dw holds the prior value when accumulating, NaN otherwise"""
    outs, table = [], []
    for slabs, prior, acc in entries:
        o = Guarded(prior.size)
        if acc:
            o.view.copy_(dev(prior))
        outs.append(o)
        table.append((dev(slabs), o.view, acc))
    fn.slab_reduce_batch(*fn.slab_reduce_table(table, "cuda"))
    return [(host(o.view), o.intact()) for o in outs]


def test_slab_reduce_batch_adds_in_the_documented_order(gpu_device):
    """every entry of one table, then each entry as a table of one: bit-equal to slab[0] + slab[1] + ... (+ prior dw LAST)"""
    entries = slab_entries()
    assert {a for _, _, a in entries} == {False, True}
    want = [P.slab_sum_ref(s, p, a) for s, p, a in entries]
    bad = []
    for label, results in (("one table", run_slab_table(entries)), ("tables of one", [run_slab_table([e])[0] for e in entries])):
        for (s, p, a), w, (got, intact) in zip(entries, want, results):
            if not (np.array_equal(got.view(np.int32), w.view(np.int32)) and intact):
                bad.append((label, s.shape, a, int((got.view(np.int32) != w.view(np.int32)).sum())))
    assert not bad, bad


def test_slab_reduce_batch_past_its_grid_cap(gpu_device):
    """16384 * 256 + 1 float4 over two entries of two slabs: the last element belongs to the second grid trip"""
    total4 = SLAB_CAP * 256 + 1
    n4s = (3_000_000, total4 - 3_000_000)
    g = torch.Generator(device="cuda").manual_seed(1)
    table, ref = [], []
    for n4, acc in zip(n4s, (True, False)):
        slabs = torch.randn(2, 4 * n4, device="cuda", generator=g) * torch.exp(4 * torch.randn(2, 4 * n4, device="cuda", generator=g))
        o = Guarded(4 * n4)
        prior = None
        if acc:
            prior = torch.randn(4 * n4, device="cuda", generator=g)
            o.view.copy_(prior)
            prior = host(prior)
        table.append((slabs, o.view, acc))
        ref.append((host(slabs), prior, acc, o))
    fn.slab_reduce_batch(*fn.slab_reduce_table(table, "cuda"))
    for slabs, prior, acc, o in ref:
        want = P.slab_sum_ref(slabs, prior, acc)
        assert np.array_equal(host(o.view).view(np.int32), want.view(np.int32)) and o.intact(), (slabs.shape, acc)


@pytest.mark.parametrize("case", [(1, 48, 48, 8, 16, 3, 1), (1, 80, 80, 4, 4, 1, 0)], ids=str)
def test_single_launch_slab_reduce_of_conv2d_wgrad(gpu_device, case):
    """slab_reduce_kernel, reached through conv2d_wgrad on shapes the library cuts into 17 slabs or more (a 16-row batch and a
    tail): dw is the ordered float32 sum of the slabs conv2d_wgrad_slabs leaves for the same operands, prior value last"""
    N, H, W, Cin, Cout, k, pad = case
    g = torch.Generator().manual_seed(sum(case))
    x = (torch.randn(N, H, W, Cin, generator=g) * torch.exp(2 * torch.randn(N, H, W, Cin, generator=g))).cuda()
    dy = (torch.randn(N, H, W, Cout, generator=g) * torch.exp(2 * torch.randn(N, H, W, Cout, generator=g))).cuda()
    shape = (Cout, k, k, Cin)
    splits = fn.conv2d_wgrad_splits(tuple(x.shape), tuple(dy.shape), shape, 1)
    assert splits >= 17, f"{splits} slabs: the case no longer reaches the batched loop of slab_reduce_kernel"
    slabs = Guarded(splits * Cout * k * k * Cin)
    fn.conv2d_wgrad_slabs(x, dy, shape, slabs.view.view((splits,) + shape), stride=1, pad=pad, math="f16x2")
    sl = host(slabs.view).reshape(splits, -1)
    assert not np.isnan(sl).any() and slabs.intact()
    prior = P.wide_values((sl.shape[1],), np.random.default_rng(1))
    for acc in (False, True):
        o = Guarded(sl.shape[1])
        if acc:
            o.view.copy_(dev(prior))
        fn.conv2d_wgrad(x, dy, shape, stride=1, pad=pad, out=o.view.view(shape), accumulate=acc, math="f16x2")
        want = P.slab_sum_ref(sl, prior, acc)
        assert np.array_equal(host(o.view).view(np.int32), want.view(np.int32)) and o.intact(), acc


# ---------------------------------------------------------------------------------------------------------------------
# fn.weight_transpose (the non-batch kernel)
@pytest.mark.parametrize("half", [False, True], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("shape", [(19, 1, 1, 20), (8, 7, 7, 4), (64, 3, 3, 2048)], ids=str)
def test_weight_transpose_matches_permute_and_zero_padding(gpu_device, shape, half):
    """(64, 3, 3, 2048): C T Kp = 1 179 648 elements, past the 4096 workgroups of 256 the launch is capped at"""
    K, R, Sx, C = shape
    dtype = torch.bfloat16 if half else torch.float32
    Kp = fn.padc(K, dtype)
    if shape[3] == 2048:
        assert C * R * Sx * Kp > WT_CAP * 256
    g = torch.Generator().manual_seed(sum(shape))
    w = (torch.randn(shape, generator=g) * torch.exp(4 * torch.randn(shape, generator=g)))
    want = torch.zeros(C, R, Sx, Kp)
    want[..., :K] = w.permute(3, 1, 2, 0)
    out = Guarded(C * R * Sx * Kp, dtype=dtype)
    copy = Guarded(w.numel(), dtype=dtype) if half else None
    fn.weight_transpose(w.cuda(), out=out.view.view(C, R, Sx, Kp), copy=None if copy is None else copy.view.view(shape))
    assert torch.equal(bits(out.view).cpu(), bits(want.to(dtype).view(-1))) and out.intact()
    if half:
        assert torch.equal(bits(copy.view).cpu(), bits(w.to(dtype).view(-1))) and copy.intact()


# ---------------------------------------------------------------------------------------------------------------------
# fn.weight_planes, transposed, Cin % 32 != 0: the data-gradient operand of ragged layers
RAGGED = [(Cout, k, k, Cin) for Cin in (4, 20, 36) for Cout in (19, 40) for k in (1, 3)]


def ragged_weight(shape):
    rng = np.random.default_rng(sum(shape) + shape[1])
    return P.wide_values(shape, rng)


def planes_t_shape(shape, npc):
    Cout, R, Sx, Cin = shape
    return (Cin, R * Sx, (Cout + 31) // 32, npc, 32)


def one_block(m, slot=7):
    b = np.zeros(S, F32)
    b[slot] = m
    return b


@pytest.mark.parametrize("shape", RAGGED, ids=str)
def test_transposed_weight_planes_of_ragged_layers(gpu_device, shape):
    """three bf16 pieces and two fp16 pieces of the zero-padded transpose, stand-alone, bit-equal to the restatement"""
    Cout, R, Sx, Cin = shape
    w = ragged_weight(shape)
    cols = (Cout + 31) // 32 * 32
    wt = P.transposed_operand(w, cols)
    wd = dev(w)
    o3 = Guarded(wt.size * 3, dtype=torch.bfloat16)
    fn.weight_planes(wd, transposed=True, cols=cols, out=o3.view.view(planes_t_shape(shape, 3)), math="bf16x3")
    assert np.array_equal(host(bits(o3.view)), P.planes3_ref(wt).reshape(-1).view(np.int16)) and o3.intact()
    am = fn.absmax(wd)
    assert float(am.max()) == float(np.abs(w).max())
    o2 = Guarded(wt.size * 2, dtype=torch.bfloat16)
    fn.weight_planes(wd, transposed=True, cols=cols, out=o2.view.view(planes_t_shape(shape, 2)), math="f16x2", w_absmax=am)
    want2 = P.planes2_ref(wt, host(am))
    assert np.array_equal(host(bits(o2.view)), want2.reshape(-1).view(np.int16)) and o2.intact()
    assert np.isfinite(want2).all() and float(np.abs(want2[:, :, :, 0]).max()) < 2.0 ** 15


def test_ragged_rows_in_one_weight_planes_batch(gpu_device):
    """every ragged shape in both piece formats as rows of ONE table, beside a Cin % 32 == 0 row with forward planes"""
    entries, checks = [], []
    for shape in RAGGED + [(40, 3, 3, 64)]:
        Cout, R, Sx, Cin = shape
        w = ragged_weight(shape)
        wt = P.transposed_operand(w, (Cout + 31) // 32 * 32)
        wd = dev(w)
        am = fn.absmax(wd)
        for npc in (3, 2):
            o = Guarded(wt.size * npc, dtype=torch.bfloat16)
            fwd = Guarded(w.size * npc, dtype=torch.bfloat16) if Cin % 32 == 0 else None
            entries.append((wd, None if fwd is None else fwd.view.view(Cout, R * Sx, Cin // 32, npc, 32), o.view.view(planes_t_shape(shape, npc)))
                           + ((am,) if npc == 2 else ()))
            want = P.planes3_ref(wt) if npc == 3 else P.planes2_ref(wt, host(am))
            checks.append((shape, npc, "transposed", o, want))
            if fwd is not None:
                m = w.reshape(Cout, R * Sx, Cin)
                checks.append((shape, npc, "forward", fwd, P.planes3_ref(m) if npc == 3 else P.planes2_ref(m, host(am))))
    fn.weight_planes_batch(*fn.weight_planes_table(entries, "cuda"))
    bad = [(shape, npc, what) for shape, npc, what, o, want in checks
           if not (np.array_equal(host(bits(o.view)), want.reshape(-1).view(np.int16)) and o.intact())]
    assert not bad, bad


@pytest.mark.parametrize("edge", ["power of two", "subnormal", "just under 3e38", "inf slot"])
def test_two_piece_planes_at_edge_blocks(gpu_device, edge):
    """(19, 3, 3, 20) transposed, cut by hand-made blocks.  "just under 3e38": the exponent clamp at -100 leaves elements above
    65504 * 2^100 to overflow fp16 -- they come out as repair_inf's +-65504 / +-inf (PINNED, csrc/dspn_pieces.h).  "inf slot":
    the scale comes from the finite slots; the infinite element is +-65504 / +-inf, every other element the plain cut."""
    shape = (19, 3, 3, 20)
    rng = np.random.default_rng(len(edge))
    w = rng.uniform(-1, 1, shape).astype(F32)
    w[np.abs(w) < 1e-3] = F32(0.5)
    if edge == "power of two":
        w[18, 2, 2, 19] = -1.0
        w *= F32(2.0)                                     # max |w| = 2 exactly: 2 = 0.5 * 2^2, scale 2^13, the maximum lands ON 2^14
        blk = one_block(2.0)
        assert float(P.operand_scale_ref(blk)) == 2.0 ** 13
    elif edge == "subnormal":
        w = (rng.integers(-1000, 1001, shape).astype(np.float64) * 2.0 ** -149).astype(F32)
        w[0, 0, 0, 0] = F32(1000 * 2.0 ** -149)
        blk = one_block(np.abs(w).max())
        assert float(P.operand_scale_ref(blk)) == 2.0 ** 100        # 15 + 139 clamped
    elif edge == "just under 3e38":
        top = np.nextafter(F32(3.0e38), F32(0))
        w = (w.astype(np.float64) * float(top) * np.exp2(-rng.integers(0, 40, shape))).astype(F32)
        w[5, 1, 1, 3] = -top
        blk = one_block(top, slot=63)
        assert float(P.operand_scale_ref(blk)) == 2.0 ** -100
    else:
        w[7, 1, 0, 5], w[3, 2, 2, 0] = INF, -INF
        finite = float(np.abs(w[np.isfinite(w)]).max())
        blk = one_block(finite, slot=9)
        blk[3] = INF
        assert float(P.operand_scale_ref(blk)) == float(P.operand_scale_ref(one_block(finite)))
    cols = 32
    wt = P.transposed_operand(w, cols)
    want = P.planes2_ref(wt, blk)
    o = Guarded(wt.size * 2, dtype=torch.bfloat16)
    fn.weight_planes(dev(w), transposed=True, cols=cols, out=o.view.view(planes_t_shape(shape, 2)), math="f16x2", w_absmax=dev(blk))
    got = host(bits(o.view)).reshape(want.shape)
    assert np.array_equal(got, want.view(np.int16)) and o.intact()
    h = got.view(np.float16)                             # [c][tap][col block][piece][32]
    if edge == "inf slot":
        assert (h[5, 3, 0, 0, 7], h[5, 3, 0, 1, 7]) == (65504.0, INF) and (h[0, 8, 0, 0, 3], h[0, 8, 0, 1, 3]) == (-65504.0, -INF)
        assert int(np.isinf(h).sum()) == 2 and float(np.abs(h[:, :, :, 0]).max()) == 65504.0
    elif edge == "just under 3e38":
        assert int(np.isinf(h[:, :, :, 1]).sum()) > 1 and not np.isinf(h[:, :, :, 0]).any()      # the overflowed elements, repaired
    else:
        assert np.isfinite(h).all() and float(np.abs(h[:, :, :, 0]).max()) == (2.0 ** 14 if edge == "power of two" else 0.0)
