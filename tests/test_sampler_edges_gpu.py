"""The affine-sampler kernels of dspnet_amd/csrc/sampler.hip (and their bf16 twins, sampler_h.hip) at their dispatch edges,
against tests/ref_sampler.py: the float64 restatement of the semantics written at the top of sampler.hip, which
test_sampler_reference.py ties to float64 affine_grid + grid_sample autograd on the CPU.  Never against another kernel.

Every case runs the forward, affine_sampler_backward_data (overwriting and accumulating), affine_sampler_backward_data_theta
(overwriting, in place with dx = x, accumulating; with the magnitude block) followed by affine_sampler_theta_reduce, and the
stand-alone affine_sampler_backward_theta.  The theta_partial rows are compared ROW BY ROW with the reference's per-pixel
rows (a pixel's chunks summed), not only as six numbers.  The magnitude block must equal max|dx|, stay 0 for an all-zero dy
and keep a larger value that was in it.

a. Exact grids, bit for bit.  Wo - 1, Ho - 1 and every source extent - 1 are powers of two and theta is dyadic: every
   coordinate is exact in float32 (checked pixel by pixel in test_sampler_reference.py) and float32 and float64 take the
   same floor cell.  x and dy are small integers; ref_sampler.inexact_in_fp32() checks on the CPU that every sum of |terms|
   times 2^(fraction bits) stays below 2^24, so every partial sum in ANY order is exact and the kernels must return the
   float64 values themselves: out, dx, theta rows, d theta.  Samples on a pixel, on the last pixel and on the -1 border are
   all in there, and so is a source of the target's own size at the identity grid -- the kink that
   test_affine_sampler_matches_torch_grid_sample has to skip.  The 64-wide identity grid of training itself stays without
   a check: there the float32 coordinate -1 + wo * (2 / 63) falls into another floor cell than the float64 one for 11 of 64
   columns, the one-sided derivative taken depends on float32 rounding and no reference is fixed
   (test_sampler_reference.py::test_generic_grids_do_not).
   On a generic grid a sample can lie within float32 rounding of a source pixel row or column; which one-sided derivative
   is then taken depends on that rounding, in the kernel and in any float32 evaluation, and no reference is fixed for that
   target pixel's gradient terms.  The near-identity theta of the project's tests does this to target pixel (0, 0) on every
   target (-0.04 * -1 + 1.05 * -1 + 0.01 is -1 up to rounding), its rotation theta to 25 of 2560 pixels of a 64 x 40
   target over a 64 x 40 source.  ref_sampler.ambiguous_pixels() finds these pixels on the CPU -- every float32 evaluation
   order `fp contract(fast)` allows must give the float64 floor cell -- and sections b, c, e, f and g zero dy there (a
   handful of pixels per case, printed); `out` is continuous across a kink and is compared at every pixel.
b. Routing edges on generic thetas at the project's bars (test_nn_gpu.py): 1e-5 of the largest reference entry for out and
   dx, 1e-4 for theta rows and d theta.  test_edge_cases_meet_their_routes restates the host-side routing and asserts,
   without a GPU, that every case sits on the side it claims.
c. Long sums: thousands of matches per source position; x = ramp + 0.1 noise and dy = uniform + 0.5, so nothing cancels.
   The project has no bar for an element of more than 256 terms, so dx, theta rows and d theta are held to
   max(project bar, 4 x the error of the reference's own float32 evaluation), measured on the CPU when the test runs; the
   float32 evaluation sums in another order than the kernels, the factor 4 is for that.  Measured (relative to the largest
   float64 entry; `bar` is what the test then uses):
     case        target <- sources       fullest position   dx: err / bar        theta rows: err / bar   d theta: err / bar
     minify      64 x 64 <- 16 x 16      4096 matches       2.22e-06 / 1.00e-05  8.64e-07 / 1.00e-04     3.90e-06 / 1.00e-04
     straddle    64 x 64 <- 16 x 16      781 (some < 768)   1.49e-06 / 1.00e-05  1.00e-06 / 1.00e-04     1.02e-06 / 1.00e-04
     degenerate  32 x 32 <- 8 x 8        1024               1.21e-06 / 1.00e-05  7.58e-07 / 1.00e-04     3.74e-06 / 1.00e-04
     chunked     64 x 64 <- 2 x 2, 3 x 5 4024, 1956         2.94e-06 / 1.18e-05  1.66e-06 / 1.00e-04     1.63e-06 / 1.00e-04
   (4 x the measurement stays below the project's bar everywhere but for dx of the chunked case.)
   For each case the mutant with ONE match dropped at the fullest source position must lie outside the bars, for dx and for
   that position's theta row (test_sampler_reference.py::test_long_sum_cases_and_their_mutants, on the CPU from the reference
   alone; the smallest effect of a dropped match is 5.4e-4 of the largest dx entry and 3.2e-4 of the largest row entry).
d. Forward: more than 16384 x 256 float4 outputs (the grid-stride loop takes a second trip); 8 sources at once with summed,
   partly overlapping and uncovered channel slices; a 9th source is refused.
e. Stand-alone theta kernel past its 4096 waves x 4 pixels; affine_sampler_theta_reduce on float64 tables of 1 .. 65793 rows.
f. Target and source extents of 1.
g. bf16 twins (tests/bf16_twins.py): rows >= 32, which bf16 always runs as the 16-slice kernel with one row per pixel, and C = 260.
h. What the C ABI must refuse with an error code."""
import pytest
import torch

from dspnet_amd import functional as fn
from bf16_twins import BF, _same_stored
import ref_sampler as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
from ref_sampler import Bars, route, batched_gy, B1, B4, P1, P4, P16, CH, OUT_BAR, DX_BAR, ROWS_BAR, DTH_BAR
GENERIC = {"near_identity": (0.98, 0.03, -0.02, -0.04, 1.05, 0.01),       # test_nn_gpu.py THETAS[1:]
           "rotation": (0.71, 0.29, 0.23, -0.26, 0.83, -0.11),
           "zoom_out": (1.31, 0.0, 0.0, 0.0, 1.29, 0.0)}


EXACT = Bars(None, None, None, None)


def h64(t):
    return t.detach().cpu().double()


def held(got, exp, bar, what, scale=None):
    """got (device or host tensor) against the float64 reference exp: bit for bit (bar None), or within bar * the largest
    entry of the reference (plus the one float rounding of a result that is larger than the reference's scale)"""
    got = h64(got).reshape(exp.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    err = float((got - exp).abs().max())
    if bar is None:
        print(f"    {what}: exact case, {int((got != exp).sum())} of {exp.numel()} differ, worst {err:.3e}")
        assert torch.equal(got, exp), f"{what}: {int((got != exp).sum())} of {exp.numel()} differ, worst {err:.3e}"
        return
    scale = float(exp.abs().max()) if scale is None else scale
    print(f"    {what}: err {err:.3e} = {err / (scale + 1e-300):.3e} of {scale:.3e}, bar {bar:.1e}")
    assert err <= bar * scale + 2.0 ** -24 * float(exp.abs().max()) * (scale < float(exp.abs().max())), \
        f"{what}: {err:.3e} over {bar:.1e} of {scale:.3e}"


def covered(srcs, ldo):
    m = torch.zeros(ldo, dtype=torch.bool)
    for x, off in srcs:
        m[off:off + x.shape[3]] = True
    return m


def run_case(srcs, theta, Ho, Wo, dy, ref, bars, dtype=torch.float32, standalone=True):
    """every entry point on one case against ref = R.sampler(srcs, theta, Ho, Wo, dy); returns the device results of the
    overwriting data + theta call per source: [(dx, theta_partial)]"""
    N, ldo = dy.shape[0], dy.shape[3]
    th = torch.tensor(theta, dtype=torch.float32, device="cuda")
    xd = [x.to(dtype).cuda() for x, _ in srcs]
    offs = [off for _, off in srcs]
    dyd = dy.to(dtype).cuda()
    half = dtype != torch.float32
    nan = lambda *s: torch.full(s, float("nan"), dtype=dtype, device="cuda")      # noqa: E731
    table = fn.SamplerSources(list(zip(xd, offs)))
    if not half:
        out = torch.full((N, Ho, Wo, ldo), 7.0, device="cuda")
        fn.affine_sampler_forward(table, th, out)
        held(out, ref.out, bars.out, "out")
        bare = ~covered(srcs, ldo)
        assert not bool(bare.any()) or float(out[..., bare.cuda()].abs().max()) == 0, "uncovered channels are zeroed"
    g = torch.Generator().manual_seed(99)
    parts, kept = [], []
    for i, (xdev, off) in enumerate(zip(xd, offs)):
        shape, pix = tuple(xdev.shape), xdev.shape[0] * xdev.shape[1] * xdev.shape[2]
        prior = torch.randint(-3, 4, shape, generator=g).double()
        sc = float(ref.dx[i].abs().max())
        rows = fn.affine_sampler_theta_rows(shape, Ho, dtype)
        if not half:
            dx = fn.affine_sampler_backward_data(dyd, th, shape, off, dx=nan(*shape))
            held(dx, ref.dx[i], bars.dx, f"dx[{i}]")
            acc = fn.affine_sampler_backward_data(dyd, th, shape, off, dx=prior.to(dtype).cuda(), accumulate=True)
            held(acc, ref.dx[i] + prior, bars.dx, f"dx[{i}] accumulated", scale=sc)
        # data gradient + theta rows: overwritten, with the magnitude block
        part = torch.full((rows, 6), float("nan"), dtype=F64, device="cuda")
        am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
        dx = fn.affine_sampler_backward_data_theta(dyd, th, xdev, off, part, dx=nan(*shape), dx_absmax=am)
        kept.append((dx, part))
        if half:
            parts.append(part)
            continue
        held(dx, ref.dx[i], bars.dx, f"dx[{i}] with theta")
        held(R.rows_per_pixel(part.cpu(), pix), ref.rows[i], bars.rows, f"theta rows[{i}]")
        assert float(am.max()) == float(dx.abs().max()), "the magnitude block is not max|dx|"
        # in place: the forward values are read from the buffer dx overwrites
        buf, part_ip = xdev.clone(), torch.full((rows, 6), float("nan"), dtype=F64, device="cuda")
        dx = fn.affine_sampler_backward_data_theta(dyd, th, buf, off, part_ip, dx=buf)
        assert dx.data_ptr() == buf.data_ptr()
        held(dx, ref.dx[i], bars.dx, f"dx[{i}] in place")
        held(R.rows_per_pixel(part_ip.cpu(), pix), ref.rows[i], bars.rows, f"theta rows[{i}] in place")
        # accumulating, onto a block that already holds something larger
        big = 2.0 * sc + 10.0
        am = torch.full((fn.ABSMAX_SLOTS,), big, device="cuda")
        part_acc = torch.full((rows, 6), float("nan"), dtype=F64, device="cuda")
        dx = fn.affine_sampler_backward_data_theta(dyd, th, xdev, off, part_acc, dx=prior.float().cuda(), accumulate=True, dx_absmax=am)
        held(dx, ref.dx[i] + prior, bars.dx, f"dx[{i}] accumulated with theta", scale=sc)
        held(R.rows_per_pixel(part_acc.cpu(), pix), ref.rows[i], bars.rows, f"theta rows[{i}] accumulating")
        assert float(dx.abs().max()) < big and bool((am == am[0]).all()) and float(am[0]) == float(torch.tensor(big).float()), \
            "the block lost the larger value"
        # an all-zero dy: dx, the rows and the block stay 0
        am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
        part0 = torch.full((rows, 6), float("nan"), dtype=F64, device="cuda")
        dx = fn.affine_sampler_backward_data_theta(torch.zeros_like(dyd), th, xdev, off, part0, dx=nan(*shape), dx_absmax=am)
        assert float(dx.abs().max()) == 0 and float(part0.abs().max()) == 0 and float(am.max()) == 0
        parts.append(part)
    if half:
        return kept, parts
    table_rows = torch.cat(parts)
    dth = torch.full((6,), float("nan"), device="cuda")
    fn.affine_sampler_theta_reduce(table_rows, dth)
    held(dth, ref.dtheta.float().double() if bars.dth is None else ref.dtheta, bars.dth, "d theta (rows reduced)")
    again = torch.full((6,), float("nan"), device="cuda")
    fn.affine_sampler_theta_reduce(table_rows, again)
    assert torch.equal(dth, again)
    prior6 = torch.tensor([3., -2., 1., 0., -1., 2.], dtype=F64)
    sc = float(ref.dtheta.abs().max())
    exp = ref.dtheta + prior6
    acc = fn.affine_sampler_theta_reduce(table_rows, prior6.float().cuda(), accumulate=True)
    held(acc, exp.float().double() if bars.dth is None else exp, bars.dth, "d theta (rows reduced) accumulated", scale=sc)
    if standalone:
        dth = torch.full((6,), float("nan"), device="cuda")
        fn.affine_sampler_backward_theta(table, th, dyd, dth)
        held(dth, ref.dtheta.float().double() if bars.dth is None else ref.dtheta, bars.dth, "d theta (stand-alone)")
        acc = fn.affine_sampler_backward_theta(table, th, dyd, prior6.float().cuda(), accumulate=True)
        held(acc, exp.float().double() if bars.dth is None else exp, bars.dth, "d theta (stand-alone) accumulated", scale=sc)
        again = torch.full((6,), float("nan"), device="cuda")
        fn.affine_sampler_backward_theta(table, th, dyd, again)
        assert torch.equal(dth, again)
    return kept, parts


def random_case(N, shapes, C, Ho, Wo, seed, theta, coff=4, slack=8, dtype=F64):
    """randn sources on disjoint slices from channel coff on, ldo = coff + C * sources + slack: ldo > coff + C, coff > 0; dy is
    zero at the target pixels whose floor cell float32 rounding decides (ref_sampler.ambiguous_pixels)"""
    g = torch.Generator().manual_seed(seed)
    srcs = [(torch.randn(N, h, w, C, generator=g, dtype=F64), coff + C * i) for i, (h, w) in enumerate(shapes)]
    dy = torch.randn(N, Ho, Wo, coff + C * len(shapes) + slack, generator=g, dtype=F64)
    if dtype != F64:        # values the storage type holds exactly
        srcs = [(x.to(dtype).double(), o) for x, o in srcs]
        dy = dy.to(dtype).double()
    dy, dropped = R.off_the_kinks(dy, theta, shapes, Ho, Wo)
    print(f"  {dropped} of {Ho * Wo} target pixels carry no gradient: float32 rounding decides their floor cell")
    return srcs, dy


# ---------------------------------------------------------------------------------------------------------------------
# a. exact grids
@pytest.mark.parametrize("name", sorted(R.EXACT_THETAS))
@pytest.mark.parametrize("target,shapes", R.EXACT_TARGETS)
def test_exact_grids_bit_for_bit(gpu_device, name, target, shapes):
    theta = R.EXACT_THETAS[name]
    srcs, dy, ref, thin = R.exact_case(target, shapes, theta)
    R.assert_exact_in_fp32(ref, name)
    print(f"  {name} {target} <- {shapes}: every {thin}-th target pixel carries a gradient;",
          [route(R.EXACT_N, h, w, R.EXACT_C, target[0]) for h, w in shapes])
    run_case(srcs, theta, target[0], target[1], dy, ref, EXACT)


def test_exact_grids_reach_every_gather_kernel():
    got = {route(R.EXACT_N, h, w, R.EXACT_C, target[0]) for target, shapes in R.EXACT_TARGETS for h, w in shapes}
    assert got >= {"sampler_bwd_data_batched_kernel<1>", "sampler_bwd_data_batched_kernel<4>",
                   "sampler_bwd_data_kernel<4> x 8 chunks + sampler_bwd_reduce_kernel"}, got
    got = {route(R.EXACT_N, h, w, R.EXACT_C, target[0], theta_rows=False) for target, shapes in R.EXACT_TARGETS for h, w in shapes}
    assert "sampler_bwd_data_kernel<16>" in got, got


# ---------------------------------------------------------------------------------------------------------------------
# b. routing edges
# id: N, (Hin, Win), C, (Ho, Wo), batched setting, host `rows`, kernel of the data + theta call, kernel of the data-only call
EDGE_CASES = {
    "rows_8": (2, (11, 7), 8, (33, 20), 1, 8, B1, B1),
    "rows_10": (2, (9, 7), 8, (33, 20), 1, 10, B4, B4),
    "rows_30": (2, (4, 5), 8, (56, 12), 1, 30, B4, B4),
    "rows_32": (2, (4, 5), 8, (57, 12), 1, 32, CH, P16),
    "chunks_N256": (256, (4, 4), 4, (64, 8), 1, 34, CH, P16),          # N * Hin * Win = 4096: the last chunked size
    "chunks_N257": (257, (4, 4), 4, (64, 8), 1, 34, P16, P16),         # 4112: one 16-slice workgroup per source pixel
    "C_252": (2, (8, 8), 252, (24, 20), 1, 8, B1, B1),                 # 63 float4 columns: one idle lane
    "C_256": (2, (8, 8), 256, (24, 20), 1, 8, B1, B1),                 # 64: the widest the batched kernel takes
    "C_260": (2, (8, 8), 260, (24, 20), 1, 8, P1, P1),                 # 65: per-pixel kernel, second `cb += 64` trip with 1 lane
    "C_516": (2, (8, 8), 516, (24, 20), 1, 8, P1, P1),                 # 129: third trip; `c += 64` of the stand-alone theta kernel
    "C_260_rows_10": (2, (5, 6), 260, (24, 20), 1, 12, P4, P4),        # the channel loop around the 4-slice reduction
    "N_1": (1, (6, 5), 8, (20, 12), 1, 10, B4, B4),                    # three of the four waves idle
    "N_3": (3, (6, 5), 8, (20, 12), 1, 10, B4, B4),
    "N_5": (5, (6, 5), 8, (20, 12), 1, 10, B4, B4),                    # gy = 2: the second workgroup has one image
    "positions_2560": (6, (64, 40), 8, (64, 40), 1, 4, B1, B1),        # gy = 1: every wave takes a second trip over the batch
    "batched_off_rows_8": (2, (11, 7), 8, (33, 20), 0, 8, P1, P1),
    "batched_off_rows_10": (3, (9, 7), 8, (33, 20), 0, 10, P4, P4),
    "batched_off_rows_30": (2, (4, 5), 8, (56, 12), 0, 30, P4, P4),
}


def test_edge_cases_meet_their_routes():
    for name, (N, (Hin, Win), C, (Ho, Wo), batched, rows, with_theta, data_only) in EDGE_CASES.items():
        assert R.host_rows(Ho, Hin) == rows, name
        assert route(N, Hin, Win, C, Ho, True, bool(batched)) == with_theta, name
        assert route(N, Hin, Win, C, Ho, False, bool(batched)) == data_only, name
    E = EDGE_CASES
    assert 256 * 16 == 4096 and 257 * 16 > 4096
    assert [E[k][2] // 4 for k in ("C_252", "C_256", "C_260", "C_516")] == [63, 64, 65, 129]
    assert [batched_gy(E[k][0], *E[k][1]) for k in ("N_1", "N_3", "N_5")] == [1, 1, 2]
    N, (Hin, Win) = E["positions_2560"][:2]
    assert Hin * Win > 2048 and batched_gy(N, Hin, Win) == 1 and N > 4


@pytest.mark.parametrize("theta", sorted(GENERIC))
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_routing_edges_against_the_reference(gpu_device, case, theta):
    N, (Hin, Win), C, (Ho, Wo), batched, rows, with_theta, _ = EDGE_CASES[case]
    srcs, dy = random_case(N, [(Hin, Win)], C, Ho, Wo, len(case) * 31 + C, GENERIC[theta])
    ref = R.sampler(srcs, GENERIC[theta], Ho, Wo, dy, want_abs=False)
    # the library's own row count tells the chunked route from the others
    assert fn.affine_sampler_theta_rows((N, Hin, Win, C), Ho) == N * Hin * Win * (8 if with_theta == CH else 1)
    L = fn.L()
    try:
        assert L.dspn_affine_sampler_set_batched(batched) == 0
        run_case(srcs, GENERIC[theta], Ho, Wo, dy, ref, Bars())
    finally:
        L.dspn_affine_sampler_set_batched(1)


# ---------------------------------------------------------------------------------------------------------------------
# c. long sums
@pytest.mark.parametrize("name", sorted(R.LONG_CASES))
def test_long_sums_against_the_reference(gpu_device, name):
    """(what each case is, the measurement behind its bars and its mutant: test_sampler_reference.py, on the CPU)"""
    theta, shapes, kernel, (Ho, Wo) = R.LONG_CASES[name]
    srcs, dy, ref, bars, _ = R.long_case_once(name)
    for h, w in shapes:
        assert fn.affine_sampler_theta_rows((R.LONG_N, h, w, R.LONG_C), Ho) == R.LONG_N * h * w * (8 if kernel == CH else 1)
    run_case(srcs, theta, Ho, Wo, dy, ref, bars)


# ---------------------------------------------------------------------------------------------------------------------
# d. forward
def test_forward_grid_stride_second_trip(gpu_device):
    N, Ho, Wo, C = 9, 128, 128, 128
    assert N * Ho * Wo * (C // 4) > 16384 * 256            # the launch is capped at 16384 workgroups of 256 threads
    g = torch.Generator().manual_seed(41)
    srcs = [(torch.randn(N, 16, 16, C, generator=g).double(), 0)]
    theta = GENERIC["rotation"]
    ref = R.sampler(srcs, theta, Ho, Wo, want_abs=False)
    out = torch.full((N, Ho, Wo, C), 7.0, device="cuda")
    fn.affine_sampler_forward(fn.SamplerSources([(srcs[0][0].float().cuda(), 0)]), torch.tensor(theta, device="cuda"), out)
    held(out, ref.out, OUT_BAR, "out")


def test_forward_eight_sources_and_a_ninth(gpu_device):
    """three sources summed on one slice, two partly overlapping slices (channels 12 .. 16 carry both), 4 channels uncovered"""
    N, Ho, Wo, ldo = 2, 20, 12, 48
    layout = [((4, 4), 8, 0), ((8, 8), 8, 0), ((20, 12), 8, 0), ((5, 9), 8, 8), ((16, 16), 12, 12), ((2, 3), 8, 24), ((1, 1), 8, 32),
              ((7, 7), 4, 40)]
    g = torch.Generator().manual_seed(43)
    srcs = [(torch.randn(N, h, w, c, generator=g).double(), off) for (h, w), c, off in layout]
    assert len(srcs) == 8 and int((~covered(srcs, ldo)).sum()) == 4
    L = fn.L()
    for name, theta in GENERIC.items():
        ref = R.sampler(srcs, theta, Ho, Wo, ldo=ldo, want_abs=False)
        xd = [(x.float().cuda(), off) for x, off in srcs]
        out = torch.full((N, Ho, Wo, ldo), 7.0, device="cuda")
        fn.affine_sampler_forward(fn.SamplerSources(xd), torch.tensor(theta, device="cuda"), out)
        held(out, ref.out, OUT_BAR, f"out ({name})")
        assert float(out[..., 44:].abs().max()) == 0
    nine = fn.SamplerSources(xd + [xd[0]])
    th = torch.tensor(GENERIC["rotation"], device="cuda")
    before = out.clone()
    rc = L.dspn_affine_sampler_forward_f32(nine.x, nine.Hin, nine.Win, nine.C, nine.coff, 9, fn.ptr(th), fn.ptr(out), N, Ho, Wo, ldo, fn.stream())
    assert rc != 0 and b"sources" in L.dspn_last_error(), (rc, L.dspn_last_error())
    ws = torch.zeros(L.dspn_affine_sampler_theta_workspace_bytes(N, Ho, Wo), dtype=torch.uint8, device="cuda")
    dth = torch.zeros(6, device="cuda")
    rc = L.dspn_affine_sampler_backward_theta_f32(nine.x, nine.Hin, nine.Win, nine.C, nine.coff, 9, fn.ptr(th), fn.ptr(out), N, Ho, Wo, ldo,
                                                  fn.ptr(dth), 0, fn.ptr(ws), ws.numel(), fn.stream())
    assert rc != 0
    assert torch.equal(out, before) and float(dth.abs().max()) == 0          # a refused call touches nothing


# ---------------------------------------------------------------------------------------------------------------------
# e. the stand-alone theta kernel past its launch cap, and the two-level reduce
@pytest.mark.parametrize("theta", sorted(GENERIC))
def test_standalone_theta_past_its_launch_cap(gpu_device, theta):
    # (sources of at most 20: on a 64 x 64 source with randn data the float32 evaluation of the restatement itself is 1.0 to
    # 1.3e-5 of the largest entry off in `out` -- coordinate rounding times the slope -- and no float32 kernel can keep 1e-5)
    N, Ho, Wo, C = 5, 64, 64, 8
    assert N * Ho * Wo > 1024 * 4 * 4 and R.theta_waves(N * Ho * Wo) == 4096      # every wave takes a 5th pixel
    srcs, dy = random_case(N, [(16, 16), (12, 20)], C, Ho, Wo, 47, GENERIC[theta])
    ref = R.sampler(srcs, GENERIC[theta], Ho, Wo, dy, want_abs=False)
    run_case(srcs, GENERIC[theta], Ho, Wo, dy, ref, Bars())


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 65536, 65793])
def test_theta_reduce_on_float64_tables(gpu_device, rows):
    """the double sum is held to 1e-12 relative; the ONE rounding of the float result (2^-24 relative) is the reference's too.
    The entries are positive, so `relative` is relative to the sum of |entries| as well"""
    groups = min(256, (rows + 255) // 256)
    assert {1: 1, 255: 1, 256: 1, 257: 2, 65536: 256, 65793: 256}[rows] == groups and (rows != 65793 or rows % groups)
    g = torch.Generator().manual_seed(rows)
    table = torch.rand(rows, 6, generator=g, dtype=F64) + 0.25
    ref = table.sum(0)
    dev = table.cuda()
    dth = fn.affine_sampler_theta_reduce(dev, torch.full((6,), float("nan"), device="cuda"))
    err = (h64(dth) - ref).abs()
    assert bool((err <= (2.0 ** -24 + 1e-12) * ref.abs()).all()), (err / ref)
    assert torch.equal(dth, fn.affine_sampler_theta_reduce(dev, torch.full((6,), float("nan"), device="cuda")))
    prior = torch.tensor([1.5, -2.0, 0.25, 1e3, -1e3, 0.0])
    acc = fn.affine_sampler_theta_reduce(dev, prior.cuda(), accumulate=True)
    exp = ref + prior.double()
    err = (h64(acc) - exp).abs()
    assert bool((err <= 2.0 ** -24 * exp.abs() + 1e-12 * (ref.abs() + prior.double().abs())).all()), (err / exp)
    assert torch.equal(acc, fn.affine_sampler_theta_reduce(dev, prior.cuda(), accumulate=True))


# ---------------------------------------------------------------------------------------------------------------------
# f. extents of 1
@pytest.mark.parametrize("theta", sorted(GENERIC) + ["identity"])
@pytest.mark.parametrize("Ho,Wo", [(1, 9), (9, 1)])
def test_extents_of_one(gpu_device, Ho, Wo, theta):
    """a target coordinate is 0 where that extent is 1; a source extent of 1 pins that coordinate to pixel 0 and gives the
    theta components of that axis nothing"""
    th = GENERIC.get(theta, (1, 0, 0, 0, 1, 0))
    srcs, dy = random_case(3, [(1, 5), (4, 1), (3, 3), (1, 1)], 8, Ho, Wo, 53, th)
    ref = R.sampler(srcs, th, Ho, Wo, dy, want_abs=False)
    assert float(ref.rows[0][:, 3:].abs().max()) == 0 and float(ref.rows[1][:, :3].abs().max()) == 0
    run_case(srcs, th, Ho, Wo, dy, ref, Bars())


# ---------------------------------------------------------------------------------------------------------------------
# g. bf16 twins
BF16_CASES = {
    "rows_34_small": (3, (4, 4), 8, (64, 8)),            # float: 8 chunks + reduce; bf16: the 16-slice kernel, one row per pixel
    "rows_34_N257": (257, (4, 4), 4, (64, 8)),           # both builds: the 16-slice kernel
    "C_260": (2, (8, 8), 260, (24, 20)),                 # per-pixel kernel, second channel trip
    "C_256": (2, (8, 8), 256, (24, 20)),                 # batched kernel, all 64 lanes
}


@pytest.mark.parametrize("case", sorted(BF16_CASES))
def test_bf16_twins(gpu_device, case):
    """on bf16-representable inputs a stored bf16 result == round_to_bf16(float result) wherever both builds add in the same
    order (every route but the float build's chunked one, which is held to the reference's bar instead); the float64 theta
    rows of the two builds agree to 1e-6 (as test_bf16_storage_gpu.py: the builds may contract multiply-adds differently)"""
    N, (Hin, Win), C, (Ho, Wo) = BF16_CASES[case]
    theta = GENERIC["near_identity"]
    srcs, dy = random_case(N, [(Hin, Win)], C, Ho, Wo, 59 + C, theta, dtype=BF)
    ref = R.sampler(srcs, theta, Ho, Wo, dy, want_abs=False)
    pix = N * Hin * Win
    assert fn.affine_sampler_theta_rows((N, Hin, Win, C), Ho, BF) == pix
    assert route(N, Hin, Win, C, Ho, half=True) == {"rows_34_small": P16, "rows_34_N257": P16, "C_260": P1, "C_256": B1}[case]
    same_order = route(N, Hin, Win, C, Ho, half=True) == route(N, Hin, Win, C, Ho)
    assert same_order == (case != "rows_34_small")
    (kf, pf), (kh, ph) = [run_case(srcs, theta, Ho, Wo, dy, ref, Bars(), dtype=d) for d in (torch.float32, BF)]
    th = torch.tensor(theta, device="cuda")
    xf, xh = srcs[0][0].float().cuda(), srcs[0][0].to(BF).cuda()
    dyf, dyh = dy.float().cuda(), dy.to(BF).cuda()
    off = srcs[0][1]
    outf, outh = torch.empty(N, Ho, Wo, dy.shape[3], device="cuda"), torch.empty(N, Ho, Wo, dy.shape[3], dtype=BF, device="cuda")
    fn.affine_sampler_forward(fn.SamplerSources([(xf, off)]), th, outf)
    fn.affine_sampler_forward(fn.SamplerSources([(xh, off)]), th, outh)
    _same_stored(outh, outf, "sampler forward")
    # the data-only entry point never splits: the same kernel and order in both builds
    df = fn.affine_sampler_backward_data(dyf, th, xf.shape, off)
    dh = fn.affine_sampler_backward_data(dyh, th, xh.shape, off)
    _same_stored(dh, df, "sampler backward data")
    prior = torch.randn(xf.shape, generator=torch.Generator().manual_seed(3)).to(BF).cuda()
    _same_stored(fn.affine_sampler_backward_data(dyh, th, xh.shape, off, dx=prior.clone(), accumulate=True),
                 fn.affine_sampler_backward_data(dyf, th, xf.shape, off, dx=prior.float(), accumulate=True), "accumulated")
    (dxf, partf), (dxh, parth) = kf[0], kh[0]
    if same_order:
        _same_stored(dxh, dxf, "sampler backward data with theta")
    bound = ref.dx[0].abs() * 2.0 ** -8 + DX_BAR * float(ref.dx[0].abs().max())          # test_bf16_storage_gpu.close_stored
    assert bool(((h64(dxh) - ref.dx[0]).abs() <= bound).all())
    buf = xh.clone()
    part_ip = torch.full((pix, 6), float("nan"), dtype=F64, device="cuda")
    assert torch.equal(fn.affine_sampler_backward_data_theta(dyh, th, buf, off, part_ip, dx=buf), dxh) and torch.equal(part_ip, parth)
    held(parth, ref.rows[0], ROWS_BAR, "bf16 theta rows")
    rf = R.rows_per_pixel(partf.cpu(), pix)
    assert float((parth.cpu() - rf).abs().max()) <= 1e-6 * float(rf.abs().max()) or not same_order
    dth = fn.affine_sampler_theta_reduce(parth, torch.zeros(6, device="cuda"))
    held(dth, ref.dtheta, DTH_BAR, "bf16 d theta (rows reduced)")
    dth = fn.affine_sampler_backward_theta(fn.SamplerSources([(xh, off)]), th, dyh, torch.zeros(6, device="cuda"))
    held(dth, ref.dtheta, DTH_BAR, "bf16 d theta (stand-alone)")


# ---------------------------------------------------------------------------------------------------------------------
# h. what the C ABI refuses
def test_c_abi_refusals(gpu_device):
    L = fn.L()
    P, st = fn.ptr, fn.stream()
    N, Hin, Win, C, Ho, Wo, ldo = 2, 4, 4, 8, 64, 8, 16
    x, dx = torch.ones(N, Hin, Win, C, device="cuda"), torch.full((N, Hin, Win, C), 5.0, device="cuda")
    dy, th = torch.ones(N, Ho, Wo, ldo, device="cuda"), torch.tensor([1., 0, 0, 0, 1, 0], device="cuda")
    rows = fn.affine_sampler_theta_rows(x.shape, Ho)
    assert rows == 8 * N * Hin * Win                      # the chunked route: it needs a workspace
    part = torch.full((rows, 6), 5.0, dtype=F64, device="cuda")
    nbytes = L.dspn_affine_sampler_backward_workspace_bytes(N, Hin, Win, C, Ho)
    assert nbytes == 4 * 8 * N * Hin * Win * C
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    tws = torch.zeros(L.dspn_affine_sampler_theta_workspace_bytes(N, Ho, Wo), dtype=torch.uint8, device="cuda")
    dth, y = torch.full((6,), 5.0, device="cuda"), torch.full((N, Ho, Wo, ldo), 5.0, device="cuda")

    def forward(c=C, coff=0):
        t = fn.SamplerSources([(x, coff)])
        t.C[0] = c
        return L.dspn_affine_sampler_forward_f32(t.x, t.Hin, t.Win, t.C, t.coff, 1, P(th), P(y), N, Ho, Wo, ldo, st)

    def theta(c=C, coff=0):
        t = fn.SamplerSources([(x, coff)])
        t.C[0] = c
        return L.dspn_affine_sampler_backward_theta_f32(t.x, t.Hin, t.Win, t.C, t.coff, 1, P(th), P(dy), N, Ho, Wo, ldo, P(dth), 0, P(tws),
                                                        tws.numel(), st)

    def data(c=C, coff=0):
        return L.dspn_affine_sampler_backward_data_f32(P(dy), P(th), P(dx), N, Hin, Win, c, Ho, Wo, ldo, coff, 0, st)

    def data_theta(c=C, coff=0, dx_=dx, accumulate=0, part_bytes=part.numel() * 8, ws_=ws, ws_bytes=nbytes):
        return L.dspn_affine_sampler_backward_data_theta_f32(P(dy), P(th), P(x), P(dx_), N, Hin, Win, c, Ho, Wo, ldo, coff, accumulate,
                                                             P(part), part_bytes, None, P(ws_), ws_bytes, st)

    def refused(rc, text=b""):
        assert rc != 0 and text in L.dspn_last_error(), (rc, L.dspn_last_error())

    for call in (forward, theta, data, data_theta):
        refused(call(c=6))                                 # C not a multiple of 4
        refused(call(coff=2))                              # coff not a multiple of 4
        refused(call(coff=12))                             # coff + C > ldo
        refused(call(c=0))
    refused(data_theta(dx_=x, accumulate=1), b"alias")     # x is dx, accumulating
    refused(data_theta(part_bytes=part.numel() * 8 - 1), b"theta_partial")
    refused(data_theta(ws_bytes=nbytes - 1), b"workspace")
    refused(data_theta(ws_=None), b"workspace")
    torch.cuda.synchronize()
    for t in (dx, dth, y):                                # a refused call touches nothing
        assert bool((t == 5.0).all())
    assert bool((part == 5.0).all()) and bool((x == 1.0).all())
    assert forward() == 0 and theta() == 0 and data() == 0 and data_theta() == 0 and data_theta(dx_=x) == 0
    torch.cuda.synchronize()
