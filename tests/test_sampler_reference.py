"""tests/ref_sampler.py, the float64 restatement the affine-sampler kernels are held to in test_sampler_edges_gpu.py, against
float64 affine_grid + grid_sample(align_corners=True, zeros) autograd -- generic thetas, the exact (dyadic) grids with every
sample on a pixel, on the last pixel or on the -1 border, extents of 1 -- and against a loop over matches written out in
Python; and the premise of the bit-for-bit GPU cases: on those grids the float32 coordinates, computed as the kernel writes
them, ARE the float64 ones.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import ref_sampler as R

F64 = torch.float64
GENERIC_THETAS = [(0.98, 0.03, -0.02, -0.04, 1.05, 0.01), (0.71, 0.29, 0.23, -0.26, 0.83, -0.11), (1.31, 0.0, 0.0, 0.0, 1.29, 0.0),
                  (0.03, 0.01, 0.2, -0.02, 0.04, -0.1), (0.31, 0.02, 0.05, -0.03, 0.29, -0.04)]


def autograd(sources, theta, Ho, Wo, dy):
    """out (N, Ho, Wo, ldo), [dx], d theta from torch's own operators in float64"""
    N, ldo = dy.shape[0], dy.shape[3]
    th = torch.tensor(theta, dtype=F64).float().double().requires_grad_()          # the restatement takes theta as the float32 the kernels get
    xs = [x.permute(0, 3, 1, 2).clone().requires_grad_() for x, _ in sources]
    grid = F.affine_grid(th.view(1, 2, 3).expand(N, 2, 3), (N, 1, Ho, Wo), align_corners=True)
    out = torch.zeros(N, ldo, Ho, Wo, dtype=F64)
    for x, (_, off) in zip(xs, sources):
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        out = out + F.pad(s, (0, 0, 0, 0, off, ldo - off - x.shape[1]))
    out.backward(dy.permute(0, 3, 1, 2))
    return out.detach().permute(0, 2, 3, 1), [x.grad.permute(0, 2, 3, 1) for x in xs], th.grad


def agree(got, exp, tol, what):
    err, scale = float((got - exp).abs().max()), float(exp.abs().max()) + 1e-300
    assert err <= tol * scale, f"{what}: {err:.3e} of {scale:.3e}"


def check_against_autograd(sources, theta, Ho, Wo, dy, tol=1e-12):
    ref = R.sampler(sources, theta, Ho, Wo, dy)
    out, dxs, dth = autograd(sources, theta, Ho, Wo, dy)
    agree(ref.out, out, tol, "out")
    for i, dx in enumerate(dxs):
        agree(ref.dx[i], dx, tol, f"dx[{i}]")
    agree(ref.dtheta, dth, tol, "d theta")
    # the rows are the same gradient, one source pixel at a time: per source they add up to that source's d theta
    for i, (x, off) in enumerate(sources):
        _, _, dth_i = autograd([(x, off)], theta, Ho, Wo, dy)
        agree(ref.rows[i].sum(0), dth_i, tol, f"rows[{i}]")
        assert int(ref.counts[i].sum()) == ref.geo[i].t.numel()
    return ref


def random_case(shapes, Ho, Wo, N=2, C=4, seed=0, overlap=False):
    g = torch.Generator().manual_seed(seed)
    offs = [0 if overlap else 4 + C * i for i in range(len(shapes))]
    srcs = [(torch.randn(N, h, w, C, generator=g, dtype=F64), o) for (h, w), o in zip(shapes, offs)]
    dy = torch.randn(N, Ho, Wo, max(offs) + C + 4, generator=g, dtype=F64)
    return srcs, dy


@pytest.mark.parametrize("theta", GENERIC_THETAS)
@pytest.mark.parametrize("overlap", [False, True])
def test_restatement_equals_grid_sample_autograd(theta, overlap):
    srcs, dy = random_case([(4, 4), (16, 12), (5, 9), (2, 3)], 16, 12, seed=3, overlap=overlap)
    check_against_autograd(srcs, theta, 16, 12, dy)


@pytest.mark.parametrize("name", sorted(R.EXACT_THETAS))
@pytest.mark.parametrize("target,shapes", R.EXACT_TARGETS)
def test_restatement_equals_grid_sample_autograd_on_exact_grids(name, target, shapes):
    """kinks included: samples on a pixel, on the last pixel, on the -1 border (torch takes the same one-sided derivative)"""
    theta = R.EXACT_THETAS[name]
    srcs, dy, ref, _ = R.exact_case(target, shapes, theta)
    check_against_autograd(srcs, theta, target[0], target[1], dy)
    on_pixel = sum(int(((g.xs == g.xs.floor()) | (g.ys == g.ys.floor())).sum()) for g in ref.geo)
    assert on_pixel > 0, "an exact grid without a single sample on a pixel row or column"


def test_exact_grids_reach_the_border_and_the_last_pixel():
    geo = R.Geometry(R.EXACT_THETAS["onto_border"], 5, 5, 17, 17)
    assert float(geo.xs.min()) == -1.0 and float(geo.ys.min()) == -1.0
    geo = R.Geometry(R.EXACT_THETAS["onto_last"], 5, 5, 17, 17)
    assert bool((geo.xs == 4.0).any()) and float(geo.xs.max()) == 5.0
    geo = R.Geometry(R.EXACT_THETAS["zoom_out"], 5, 5, 17, 17)
    assert float(geo.xs.min()) == -1.0 and float(geo.xs.max()) == 5.0
    geo = R.Geometry(R.EXACT_THETAS["identity"], 17, 17, 17, 17)
    assert torch.equal(geo.xs, torch.arange(17, dtype=F64).expand(17, 17))


@pytest.mark.parametrize("name", sorted(R.EXACT_THETAS))
@pytest.mark.parametrize("target,shapes", R.EXACT_TARGETS)
def test_exact_grids_have_exact_float32_coordinates(name, target, shapes):
    for h, w in shapes:
        assert R.coordinates_exact_in_fp32(R.EXACT_THETAS[name], h, w, target[0], target[1]), (name, target, (h, w))


def test_generic_grids_do_not():
    """the check above can fail: the 64-wide identity grid of training is NOT exact (why it has no fixed reference)"""
    assert not R.coordinates_exact_in_fp32((1, 0, 0, 0, 1, 0), 64, 64, 64, 64)
    assert not R.coordinates_exact_in_fp32((0.98, 0.03, -0.02, -0.04, 1.05, 0.01), 5, 5, 17, 17)


@pytest.mark.parametrize("Ho,Wo,shapes", [(1, 9, [(1, 5), (4, 1), (3, 3)]), (9, 1, [(1, 5), (4, 1), (3, 3)]), (1, 1, [(1, 1), (2, 2)])])
@pytest.mark.parametrize("theta", GENERIC_THETAS[:3] + [(1, 0, 0, 0, 1, 0)])
def test_extents_of_one(Ho, Wo, shapes, theta):
    """a target coordinate is 0 when that extent is 1 (torch: the same); a source extent of 1 pins that coordinate to 0"""
    srcs, dy = random_case(shapes, Ho, Wo, seed=5)
    check_against_autograd(srcs, theta, Ho, Wo, dy)


def test_rows_counts_and_abs_sums_against_a_loop_over_matches():
    theta, (Hin, Win), (Ho, Wo), N, C = (0.9, 0.2, 0.1, -0.15, 1.2, -0.05), (3, 4), (6, 5), 2, 4
    theta = [float(v) for v in torch.tensor(theta).float()]          # (as the restatement: the float32 the kernels get)
    srcs, dy = random_case([(Hin, Win)], Ho, Wo, N=N, C=C, seed=9)
    x, off = srcs[0]
    ref = R.sampler(srcs, theta, Ho, Wo, dy)
    rows, arows = torch.zeros(N * Hin * Win, 6, dtype=F64), torch.zeros(N * Hin * Win, 6, dtype=F64)
    dx, adx, counts = torch.zeros_like(x), torch.zeros_like(x), torch.zeros(Hin * Win, dtype=torch.long)
    aout = torch.zeros_like(ref.out)
    for ho in range(Ho):
        for wo in range(Wo):
            xt, yt = -1 + wo * 2 / (Wo - 1), -1 + ho * 2 / (Ho - 1)
            xs = (theta[0] * xt + theta[1] * yt + theta[2] + 1) * (Win - 1) / 2
            ys = (theta[3] * xt + theta[4] * yt + theta[5] + 1) * (Hin - 1) / 2
            x0, y0 = int(xs // 1), int(ys // 1)
            fx, fy = xs - x0, ys - y0
            for a in (0, 1):
                for b in (0, 1):
                    h, w = y0 + a, x0 + b
                    if not (0 <= h < Hin and 0 <= w < Win):
                        continue
                    counts[h * Win + w] += 1
                    wy, wx = (fy if a else 1 - fy), (fx if b else 1 - fx)
                    cx, cy = (wy if b else -wy) * (Win - 1) / 2, (wx if a else -wx) * (Hin - 1) / 2
                    coef = torch.tensor([cx * xt, cx * yt, cx, cy * xt, cy * yt, cy], dtype=F64)
                    for n in range(N):
                        g = dy[n, ho, wo, off:off + C]
                        dx[n, h, w] += wy * wx * g
                        adx[n, h, w] += (wy * wx * g).abs()
                        aout[n, ho, wo, off:off + C] += (wy * wx * x[n, h, w]).abs()
                        r = (n * Hin + h) * Win + w
                        rows[r] += float((g * x[n, h, w]).sum()) * coef
                        arows[r] += float((g * x[n, h, w]).abs().sum()) * coef.abs()
    assert torch.equal(counts, ref.counts[0])
    for got, exp, what in ((ref.dx[0], dx, "dx"), (ref.rows[0], rows, "rows"), (ref.abs_dx[0], adx, "abs dx"),
                           (ref.abs_rows[0], arows, "abs rows"), (ref.abs_out, aout, "abs out")):
        agree(got, exp, 1e-13, what)
    agree(ref.abs_dtheta, arows.sum(0), 1e-13, "abs d theta")


def test_the_mutant_leaves_out_exactly_one_match():
    theta, Ho, Wo = (0.31, 0.02, 0.05, -0.03, 0.29, -0.04), 16, 16
    srcs, dy = random_case([(6, 6)], Ho, Wo, seed=13)
    ref = R.sampler(srcs, theta, Ho, Wo, dy)
    pos = int(ref.counts[0].argmax())
    k = 3
    mut = R.sampler(srcs, theta, Ho, Wo, dy, drop=(pos, k))
    assert int(mut.counts[0][pos]) == int(ref.counts[0][pos]) - 1 and int(mut.counts[0].sum()) == int(ref.counts[0].sum()) - 1
    m = int(ref.geo[0].matches_of(pos)[k])
    t, w = int(ref.geo[0].t[m]), ref.geo[0].w[m]
    N, C, off = 2, 4, srcs[0][1]
    exp = ref.dx[0].clone().view(N, 36, C)
    exp[:, pos] -= w * dy.view(N, Ho * Wo, -1)[:, t, off:off + C]
    agree(mut.dx[0].view(N, 36, C), exp, 1e-13, "mutant dx")
    other = torch.ones(36, dtype=torch.bool); other[pos] = False
    assert torch.equal(mut.rows[0].view(N, 36, 6)[:, other], ref.rows[0].view(N, 36, 6)[:, other])
    assert not torch.equal(mut.rows[0].view(N, 36, 6)[:, pos], ref.rows[0].view(N, 36, 6)[:, pos])


def test_float32_evaluation_is_close_and_not_identical():
    theta, Ho, Wo = (0.31, 0.02, 0.05, -0.03, 0.29, -0.04), 32, 32
    srcs, dy = random_case([(8, 8)], Ho, Wo, seed=17)
    r64, r32 = R.sampler(srcs, theta, Ho, Wo, dy), R.sampler(srcs, theta, Ho, Wo, dy, dtype=torch.float32)
    for a, b in ((r32.out, r64.out), (r32.dx[0], r64.dx[0]), (r32.rows[0], r64.rows[0]), (r32.dtheta, r64.dtheta)):
        err = float((a - b).abs().max()) / float(b.abs().max())
        assert 0 < err < 1e-4, err


def test_exactness_premise_can_fail():
    srcs, dy = random_case([(5, 5)], 17, 17, seed=19)
    assert R.inexact_in_fp32(R.sampler(srcs, R.EXACT_THETAS["identity"], 17, 17, dy * 2.0 ** 30)) is not None     # sums too large
    assert "dyadic" in R.inexact_in_fp32(R.sampler(srcs, GENERIC_THETAS[0], 17, 17, dy))


@pytest.mark.parametrize("name", sorted(R.LONG_CASES))
def test_long_sum_cases_and_their_mutants(name):
    """CPU only: the case is what it claims to be, and one dropped match at the fullest position is outside the bars"""
    theta, shapes, kernel, (Ho, Wo) = R.LONG_CASES[name]
    srcs, dy, ref, bars, measured = R.long_case_once(name)
    print(f"  {name}: float32 reference off by dx {measured['dx']:.2e} rows {measured['rows']:.2e} d theta {measured['dth']:.2e};"
          f" bars dx {bars.dx:.2e} rows {bars.rows:.2e} d theta {bars.dth:.2e}; fullest position {max(int(c.max()) for c in ref.counts)}")
    for (h, w), cnt in zip(shapes, ref.counts):
        assert R.route(R.LONG_N, h, w, R.LONG_C, Ho) == kernel
    cnt = ref.counts[0]
    if name == "minify":
        assert int(cnt.max()) > 4 * R.LIST_CAP and int((cnt > R.LIST_CAP).sum()) >= 5          # thousands of matches: most positions overflow
    if name == "straddle":
        assert bool(((cnt > 0) & (cnt <= R.LIST_CAP)).any()) and bool((cnt > R.LIST_CAP).any())
    if name == "degenerate":
        assert int((cnt > 0).sum()) == 4 and int(cnt.max()) == Ho * Wo
    for si, ((h, w), cnt) in enumerate(zip(shapes, ref.counts)):
        pos = int(cnt.argmax())
        idx = ref.geo[si].matches_of(pos)
        live = ~R.ambiguous_pixels(theta, shapes, Ho, Wo).flatten()[ref.geo[si].t[idx]]          # dy is zero at the others
        k = int((ref.geo[si].w[idx] * live).argmax())
        mut = R.sampler(srcs, theta, Ho, Wo, dy, drop=(si, pos, k), want_abs=False)
        ddx = float((mut.dx[si] - ref.dx[si]).abs().max())
        drow = float((mut.rows[si] - ref.rows[si]).view(R.LONG_N, h * w, 6)[:, pos].abs().max())
        sdx, srow = float(ref.dx[si].abs().max()), float(ref.rows[si].abs().max())
        print(f"    source {si}: one match of {int(cnt[pos])} moves dx by {ddx / sdx:.2e}, its theta row by {drow / srow:.2e}")
        assert ddx > bars.dx * sdx and drow > bars.rows * srow, "the bar would let a dropped match pass: change the inputs"


def test_ambiguous_pixels_are_the_kinks_float32_cannot_decide():
    """the near-identity theta of the project's tests puts target pixel (0, 0) on source row 0 up to rounding (-0.04 * -1 +
    1.05 * -1 + 0.01); its zoom-out theta puts the middle row of an odd target exactly on a row, in any precision"""
    m = R.ambiguous_pixels(GENERIC_THETAS[0], [(6, 5)], 20, 12)
    assert bool(m[0, 0]) and int(m.sum()) == 1
    assert int(R.ambiguous_pixels(GENERIC_THETAS[2], [(11, 7)], 33, 20).sum()) == 0
    assert float(R.Geometry(GENERIC_THETAS[2], 11, 7, 33, 20).ys[16, 0]) == 5.0
    for name, theta in R.EXACT_THETAS.items():
        for target, shapes in R.EXACT_TARGETS:
            assert int(R.ambiguous_pixels(theta, shapes, target[0], target[1]).sum()) == 0, (name, target)
    assert int(R.ambiguous_pixels((1, 0, 0, 0, 1, 0), [(64, 64)], 64, 64).sum()) > 1000          # training's own grid
    g = torch.Generator().manual_seed(1)
    dy, n = R.off_the_kinks(torch.randn(2, 20, 12, 8, generator=g, dtype=F64), GENERIC_THETAS[0], [(6, 5)], 20, 12)
    assert n == 1 and float(dy[:, 0, 0].abs().max()) == 0 and float(dy[:, 0, 1].abs().min()) > 0
