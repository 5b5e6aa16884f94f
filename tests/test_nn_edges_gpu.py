"""Pooling, loss, layout, column-sum and SGD kernels of dspnet_amd/csrc/nn.hip and nn_float_ops.hip at their edges, against plain float64
references written here (torch CPU / numpy; never another kernel of this library): every pooling geometry the three symbols
use, odd and tiny maps, launches past the workgroup cap of `grid_for` (where only the grid-stride loop covers the tensor),
the softmax dispatch boundaries, and the limits the C ABI refuses.

Bars.  What only selects or moves data (max pooling, the argmax record, layout, copies, fill, ReLU masks, counts, pad
columns, ignored rows) is bit exact against the reference rounded to float.  A sum of n float terms carries at most n
roundings: |err| <= n * 2^-24 * sum|terms| (average pooling: (k*k + 2) * 2^-24 * sum|terms| / (k*k) -- k*k - 1 adds, the
rounded 1 / (k*k) and the product; max-pooling gradients: k*k * 2^-24 * sum|routed dy|), plus one rounding of the result
when accumulating.  Softmax, smooth-L1, SGD, column sums and cross-entropy keep the 1e-6 / 1e-5 / 1e-4 (of the largest
entry) that tests/test_nn_gpu.py uses for the same operators.

What max pooling promises for non-finite input ("Pooling and softmax: the edges of the contract"): a value
wins a window only by comparing GREATER than what came before, starting from -inf.  So NaN never wins and is skipped -- a
window with a NaN among finite values yields the maximum of the finite ones, records its position and routes the gradient
there.  A window that holds nothing above -inf (all -inf, all NaN, or both) yields -inf, records 255 and routes NO gradient,
in `maxpool_backward_argmax` and in `maxpool_backward` alike; dx is finite wherever dy is.  (+inf is an ordinary maximum.)

What softmax_output admits: at most 64 columns (C <= ld <= 64, refused beyond); logits of any finite size; -inf entries as
long as one entry of the row is finite (their probability is exactly 0).  A row of only -inf, or any NaN / +inf, is outside
the contract."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dspnet_amd import functional as fn
from bf16_twins import BF, _pair, _same_stored

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of float32


def _grid_cap_items():
    """work items one launch covers without its grid-stride loop, read from the source:
    `inline int grid_for(long long n, int per_block = kT, int cap = 8192)` with `constexpr int kT = 256` -> 2 097 152"""
    src = open(os.path.join(os.path.dirname(fn.__file__), "csrc", "nn_launch.h")).read()
    cap = re.search(r"inline int grid_for\(long long n, int per_block = kT, int cap = (\d+)\)", src)
    kt = re.search(r"constexpr int kT = (\d+);", src)
    assert cap and kt, "grid_for / kT not found in nn_launch.h: update this reader"
    return int(cap.group(1)) * int(kt.group(1))


CAP = _grid_cap_items()
BWD_CAP = 65535 * 256   # the two max-pooling backward launches pass cap = 65535 explicitly (grid_for(total, kT, 65535))


def close(got, exp, tol):
    """tests/test_nn_gpu.py's `close`: max error relative to the largest entry of the reference"""
    scale = float(exp.abs().max()) + 1e-30
    err = float((got - exp).abs().max())
    print(f"    close: max err {err:.3e}, scale {scale:.3e}, bar {tol * scale:.3e}")
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


def within(got, exp, bound, what):
    """element-wise derived bound; got / exp / bound: float64 tensors or arrays of one shape"""
    got, exp, bound = (torch.as_tensor(np.asarray(t)) if not torch.is_tensor(t) else t for t in (got, exp, bound))
    over = (got - exp).abs() - bound
    print(f"    {what}: max err {float((got - exp).abs().max()):.3e}, largest bound {float(bound.max()):.3e}")
    assert not bool((over > 0).any()), f"{what}: {int((over > 0).sum())} elements over the bound, worst by {float(over.max()):.3e}"


def dev(a):
    """numpy / torch array -> float32 device tensor"""
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).float().contiguous().cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def to_nchw(a):     # NHWC numpy -> NCHW float64 torch
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))).double()


def to_nhwc(t):     # NCHW torch -> NHWC float64 numpy
    return t.detach().double().permute(0, 2, 3, 1).contiguous().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# references (NHWC numpy)
def pool_out(h, k, s, p, full=False):
    """MXNet Pooling output size; 0 where the padded map is smaller than the kernel"""
    if h + 2 * p < k:
        return 0
    return -(-(h + 2 * p - k) // s) + 1 if full else (h + 2 * p - k) // s + 1


def np_maxpool(x, k, s, p, Ho, Wo):
    """max pooling as the operator defines it: scan the window in (r, q) order from -inf, take what compares GREATER.
    -> (y, record): record = r * k + q of the first maximum, 255 where nothing compared above -inf"""
    N, H, W, C = x.shape
    Hp, Wp = max(H + 2 * p, (Ho - 1) * s + k), max(W + 2 * p, (Wo - 1) * s + k)
    xp = np.full((N, Hp, Wp, C), -np.inf, x.dtype)
    xp[:, p:p + H, p:p + W] = x
    m = np.full((N, Ho, Wo, C), -np.inf, x.dtype)
    rec = np.full((N, Ho, Wo, C), 255, np.uint8)
    for r in range(k):
        for q in range(k):
            v = xp[:, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s]
            with np.errstate(invalid="ignore"):
                upd = v > m
            m = np.where(upd, v, m)
            rec = np.where(upd, np.uint8(r * k + q), rec)
    return m, rec


def np_maxpool_bwd(rec, dy, x_shape, k, s, p):
    """dx[pixel] = sum of dy over the windows whose record names the pixel (float64)"""
    N, H, W, C = x_shape
    Ho, Wo = dy.shape[1:3]
    Hp, Wp = max(H + 2 * p, (Ho - 1) * s + k), max(W + 2 * p, (Wo - 1) * s + k)
    dxp = np.zeros((N, Hp, Wp, C), np.float64)
    for r in range(k):
        for q in range(k):
            dxp[:, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s] += np.where(rec == r * k + q, dy, 0.0)
    return dxp[:, p:p + H, p:p + W]


def avg2d_bwd_ref(dy_nchw, x_shape_nchw, k, s, p):
    """gradient of F.avg_pool2d(count_include_pad=True) by autograd (the operator is linear: x itself does not matter)"""
    x0 = torch.zeros(x_shape_nchw, dtype=torch.float64, requires_grad=True)
    F.avg_pool2d(x0, k, s, p, count_include_pad=True).backward(dy_nchw)
    return x0.grad


def randn32(g, *shape):
    """float32-representable standard normal data as float64"""
    return torch.randn(*shape, generator=g).double()


# ---------------------------------------------------------------------------------------------------------------------
# 1. pooling geometry table
# (N, C, H, W): odd and unequal maps, a 1-pixel-high map, a map smaller than the kernel; channels 4, 20, 64, 288; batch 1, 3
POOL_SHAPES = [(1, 4, 35, 35), (3, 20, 17, 17), (1, 64, 8, 8), (3, 288, 75, 38), (1, 20, 13, 14), (3, 4, 1, 9), (1, 4, 2, 2)]
# k, stride, pad, pooling_convention == 'full': resnet pooling0; plain 2/2/0; vgg pool3; vgg pool5; inception
MAXPOOL_GEOMS = [(3, 2, 1, False), (2, 2, 0, False), (2, 2, 0, True), (3, 1, 1, False), (3, 2, 0, False)]
# inception 3/1/1, and two geometries the API allows and no symbol uses
AVGPOOL2D_GEOMS = [(3, 1, 1), (3, 2, 1), (2, 2, 0)]


def _legal(shape, k, s, p, full=False):
    return pool_out(shape[2], k, s, p, full) > 0 and pool_out(shape[3], k, s, p, full) > 0


def _id(v):
    return "-".join(str(int(e)) if isinstance(e, bool) else str(e) for e in v)


MAXPOOL_CASES = [(g_, s_) for g_ in MAXPOOL_GEOMS for s_ in POOL_SHAPES if _legal(s_, *g_)]
AVGPOOL2D_CASES = [(g_, s_) for g_ in AVGPOOL2D_GEOMS for s_ in POOL_SHAPES if _legal(s_, *g_)]


def _maxpool_data(kind, shape, g):
    N, C, H, W = shape
    n = N * C * H * W
    if kind == "distinct":          # no two elements equal (n < 2^24: every value is exact in float32)
        assert n < 2 ** 24
        return ((torch.randperm(n, generator=g).double() - n // 2) / 8).view(N, C, H, W)
    x = randn32(g, N, C, H, W)
    if kind == "relu":              # post-ReLU zeros: many windows tie at 0
        return x.clamp(min=0)
    x[:, 0] = 1.5                   # plateau: a constant channel and a constant block in the last channel
    x[:, -1, H // 3:, W // 4:] = -2.0
    return x


@pytest.mark.parametrize("kind", ["distinct", "relu", "plateau"])
@pytest.mark.parametrize("geom,shape", MAXPOOL_CASES, ids=[_id(g_) + "_" + _id(s_) for g_, s_ in MAXPOOL_CASES])
def test_maxpool_geometries(gpu_device, geom, shape, kind):
    k, s, p, full = geom
    N, C, H, W = shape
    Ho, Wo = pool_out(H, k, s, p, full), pool_out(W, k, s, p, full)
    g = torch.Generator().manual_seed(sum(shape) + 10 * k + s + p)
    x = _maxpool_data(kind, shape, g)
    dy = randn32(g, N, C, Ho, Wo)
    xn, dyn = to_nhwc(x), to_nhwc(dy)
    y_ref, rec_ref = np_maxpool(xn, k, s, p, Ho, Wo)
    dx_ref = np_maxpool_bwd(rec_ref, dyn, xn.shape, k, s, p)
    xt = x.clone().requires_grad_()
    y_t = F.max_pool2d(xt, k, s, p, ceil_mode=full)
    assert tuple(y_t.shape) == (N, C, Ho, Wo)
    assert torch.equal(y_t.detach(), to_nchw(y_ref))                    # the value does not depend on the tie rule
    if kind == "distinct":                                              # nor does the gradient on tie-free data
        y_t.backward(dy)
        assert float((xt.grad - to_nchw(dx_ref)).abs().max()) <= 1e-12

    xd, dyd = dev(xn), dev(dyn)
    rec = torch.full((N, Ho, Wo, C), 77, dtype=torch.uint8, device="cuda")
    y = fn.maxpool_forward(xd, k, s, p, out=fn.empty(N, Ho, Wo, C), argmax=rec)
    assert np.array_equal(host(y), y_ref), "forward value"
    assert torch.equal(fn.maxpool_forward(xd, k, s, p, out=fn.empty(N, Ho, Wo, C)), y), "forward without the record"
    assert np.array_equal(rec.cpu().numpy(), rec_ref), "argmax record != first maximum in (r, s) scan order"
    bound = k * k * U * np_maxpool_bwd(rec_ref, np.abs(dyn), xn.shape, k, s, p)
    dx_rec = fn.maxpool_backward_argmax(rec, dyd, tuple(xd.shape), k, s, p)
    dx_val = fn.maxpool_backward(xd, y, dyd, k, s, p)
    within(host(dx_rec), dx_ref, bound, "maxpool_backward_argmax")
    within(host(dx_val), dx_ref, bound, "maxpool_backward")
    assert torch.equal(dx_rec, dx_val)                                  # same windows in the same order: same bits


@pytest.mark.parametrize("geom,shape", AVGPOOL2D_CASES, ids=[_id(g_) + "_" + _id(s_) for g_, s_ in AVGPOOL2D_CASES])
def test_avgpool2d_geometries(gpu_device, geom, shape):
    """divisor k*k everywhere, the padding counted (MXNet's Pooling with pool_type='avg')"""
    k, s, p = geom
    N, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 100 * k + s + p)
    x = randn32(g, N, C, H, W)
    y_ref = F.avg_pool2d(x, k, s, p, count_include_pad=True)
    Ho, Wo = y_ref.shape[2:]
    assert (Ho, Wo) == (pool_out(H, k, s, p), pool_out(W, k, s, p))
    dy = randn32(g, N, C, Ho, Wo)                                       # a gradient of its own, also where Ho == H
    dx_ref = avg2d_bwd_ref(dy, x.shape, k, s, p)
    kk = k * k
    xd, dyd = dev(to_nhwc(x)), dev(to_nhwc(dy))
    y = fn.avgpool2d_forward(xd, k, s, p)
    assert tuple(y.shape) == (N, Ho, Wo, C)
    within(to_nchw(host(y)), y_ref, (kk + 2) * U * F.avg_pool2d(x.abs(), k, s, p, count_include_pad=True), "avgpool2d_forward")
    bound_g = (kk + 2) * U * avg2d_bwd_ref(dy.abs(), x.shape, k, s, p)
    dx = fn.avgpool2d_backward(dyd, tuple(xd.shape), k, s, p, dx=torch.full_like(xd, float("nan")))
    within(to_nchw(host(dx)), dx_ref, bound_g, "avgpool2d_backward")
    base = randn32(g, N, C, H, W)
    acc = fn.avgpool2d_backward(dyd, tuple(xd.shape), k, s, p, dx=dev(to_nhwc(base)), accumulate=True)
    exp = base + dx_ref
    within(to_nchw(host(acc)), exp, bound_g + U * (exp.abs() + bound_g), "avgpool2d_backward accumulate")


AVGPOOL_CASES = [(k, s_) for k in (1, 2, 4) for s_ in [(2, 8, 16, 16)] + POOL_SHAPES if s_[2] >= k and s_[3] >= k]


@pytest.mark.parametrize("k,shape", AVGPOOL_CASES, ids=[f"{k}_" + _id(s_) for k, s_ in AVGPOOL_CASES])
def test_avgpool_floor_output_and_zero_gradient_beyond_it(gpu_device, k, shape):
    N, C, H, W = shape
    Ho, Wo = H // k, W // k
    g = torch.Generator().manual_seed(sum(shape) + k)
    x = randn32(g, N, C, H, W).requires_grad_()
    y_ref = F.avg_pool2d(x, k, k)
    assert tuple(y_ref.shape[2:]) == (Ho, Wo)
    dy = randn32(g, N, C, Ho, Wo)
    y_ref.backward(dy)
    xa = x.detach().abs().requires_grad_()
    F.avg_pool2d(xa, k, k).backward(dy.abs())
    kk = k * k
    xd, dyd = dev(to_nhwc(x)), dev(to_nhwc(dy))
    y = fn.avgpool_forward(xd, k)
    within(to_nchw(host(y)), y_ref.detach(), (kk + 2) * U * F.avg_pool2d(x.detach().abs(), k, k), "avgpool_forward")
    bound_g = (kk + 2) * U * xa.grad
    dx = fn.avgpool_backward(dyd, tuple(xd.shape), k, dx=torch.full_like(xd, float("nan")))
    within(to_nchw(host(dx)), x.grad, bound_g, "avgpool_backward")
    beyond = torch.ones(N, H, W, C, dtype=torch.bool)
    beyond[:, :Ho * k, :Wo * k] = False
    assert float(dx.cpu()[beyond].abs().sum()) == 0.0                   # rows / columns past Ho*k: exactly zero
    base = randn32(g, N, C, H, W)
    acc = fn.avgpool_backward(dyd, tuple(xd.shape), k, dx=dev(to_nhwc(base)), accumulate=True)
    exp = base + x.grad
    within(to_nchw(host(acc)), exp, bound_g + U * (exp.abs() + bound_g), "avgpool_backward accumulate")
    assert torch.equal(acc.cpu()[beyond], dev(to_nhwc(base)).cpu()[beyond])


# ---------------------------------------------------------------------------------------------------------------------
# 2. non-finite inputs to max pooling (the promise: module docstring)
@pytest.mark.parametrize("geom", MAXPOOL_GEOMS, ids=_id)
def test_maxpool_non_finite_windows(gpu_device, geom):
    k, s, p, full = geom
    N, H, W, C = 2, 6, 7, 8
    Ho, Wo = pool_out(H, k, s, p, full), pool_out(W, k, s, p, full)
    g = torch.Generator().manual_seed(k + s + p)
    x = torch.randn(N, H, W, C, generator=g).numpy()
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x[..., 0] = -inf                                    # every window all -inf
    x[:, 1, 1, 1] = nan; x[:, 4, 5, 1] = nan; x[:, 0, 0, 1] = nan       # one NaN among finite values
    x[..., 2] = nan                                     # every window all NaN
    x[..., 3] = -inf; x[:, ::2, ::3, 3] = nan           # -inf and NaN mixed, nothing finite
    x[..., 4] = -inf; x[:, 2, 3, 4] = 0.25              # one finite value in a sea of -inf
    x[..., 5] = nan; x[:, 3, 2, 5] = -1.0               # one finite value in a sea of NaN
    x[:, 2, 2, 6] = inf                                 # +inf is an ordinary maximum
    dy = torch.randn(N, Ho, Wo, C, generator=g).numpy()
    y_ref, rec_ref = np_maxpool(x, k, s, p, Ho, Wo)
    dx_ref = np_maxpool_bwd(rec_ref, dy, x.shape, k, s, p)
    # the same promise said another way: NaN counts as -inf for the value
    y_alt = F.max_pool2d(to_nchw(np.where(np.isnan(x), -inf, x)), k, s, p, ceil_mode=full)
    assert torch.equal(y_alt, to_nchw(y_ref))

    xd, dyd = dev(x), dev(dy)
    rec = torch.full((N, Ho, Wo, C), 77, dtype=torch.uint8, device="cuda")
    y = fn.maxpool_forward(xd, k, s, p, out=fn.empty(N, Ho, Wo, C), argmax=rec)
    yh, rh = host(y), rec.cpu().numpy()
    assert not np.isnan(yh).any() and np.array_equal(yh, y_ref)
    assert np.array_equal(rh, rec_ref)
    for c in (0, 2, 3):                                 # nothing above -inf: value -inf, record 255
        assert (yh[..., c] == -np.inf).all() and (rh[..., c] == 255).all()
    assert (rh[..., 1] != 255).all() and np.isfinite(yh[..., 1]).all()
    dx_rec = fn.maxpool_backward_argmax(rec, dyd, tuple(xd.shape), k, s, p)
    dx_val = fn.maxpool_backward(xd, y, dyd, k, s, p)
    bound = k * k * U * np_maxpool_bwd(rec_ref, np.abs(dy), x.shape, k, s, p)
    for name, dx in (("maxpool_backward_argmax", dx_rec), ("maxpool_backward", dx_val)):
        d = host(dx)
        assert np.isfinite(d).all(), name
        within(d, dx_ref, bound, name + " on non-finite input")
        for c in (0, 2, 3):
            assert not d[..., c].any(), f"{name}: a window without a maximum routed a gradient (channel {c})"
    assert torch.equal(dx_rec, dx_val)


# ---------------------------------------------------------------------------------------------------------------------
# 3. past the grid cap: grid_for caps a launch at 8192 workgroups of kT = 256 threads = 2 097 152 work items (CAP, read
# from the source above); beyond it only the grid-stride loop reaches the rest of the tensor.  Whole tensors are compared.
def test_grid_cap_is_what_these_cases_were_sized_for():
    assert CAP <= 2_097_152, "grid_for's cap grew: grow the `past the cap` cases below with it"


def test_maxpool_past_the_grid_cap(gpu_device):
    """3/2/1 as resnet's pooling0: 16.9 M float4 inputs (past the 65535-workgroup cap of the two backward launches), 4.2 M
    float4 outputs (past the forward's); the first four samples again with the folded BatchNorm + ReLU (2.1 M outputs)"""
    k, s, p = 3, 2, 1
    N, H, W, C = 8, 257, 256, 128                        # 269 MB
    Ho, Wo = pool_out(H, k, s, p), pool_out(W, k, s, p)
    assert N * H * W * C // 4 > BWD_CAP and N * Ho * Wo * C // 4 > CAP and 4 * Ho * Wo * C // 4 > CAP
    g = torch.Generator().manual_seed(71)
    x = torch.randn(N, H, W, C, generator=g)
    dy = torch.randn(N, Ho, Wo, C, generator=g)
    xd, dyd = x.cuda(), dy.cuda()
    rec = torch.full((N, Ho, Wo, C), 77, dtype=torch.uint8, device="cuda")
    y = fn.maxpool_forward(xd, k, s, p, argmax=rec)
    dx_rec = fn.maxpool_backward_argmax(rec, dyd, tuple(xd.shape), k, s, p).cpu()      # (one large result alive at a time)
    assert torch.equal(fn.maxpool_backward(xd, y, dyd, k, s, p).cpu(), dx_rec)
    # folded affine: scale with 5 significant bits, shift a multiple of 1/16 -- x * scale + shift is then exact in float64
    # and its rounding to float is the kernel's single fmaf rounding
    sc = (torch.randint(-16, 17, (C,), generator=g).float() / 8)
    sh = (torch.randint(-16, 17, (C,), generator=g).float() / 16)
    rec_a = torch.full((4, Ho, Wo, C), 77, dtype=torch.uint8, device="cuda")
    am = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    y_a = fn.maxpool_forward(xd[:4], k, s, p, argmax=rec_a, in_affine=(sc.cuda(), sh.cuda(), True), out_absmax=am)
    y, rec, y_a, rec_a = y.cpu(), rec.cpu(), y_a.cpu(), rec_a.cpu()
    del xd, dyd
    torch.cuda.empty_cache()
    # at most ceil(k/s)^2 = 4 windows cover a pixel: |err| <= k*k * 2^-24 * 4 * max|dy|
    bound = k * k * U * 4 * float(dy.abs().max())
    amax = 0.0
    for n in range(N):                                   # the reference one sample at a time (memory)
        xn, dyn = x[n:n + 1].numpy(), dy[n:n + 1].numpy()
        y_ref, rec_ref = np_maxpool(xn, k, s, p, Ho, Wo)
        assert np.array_equal(y[n:n + 1].numpy(), y_ref), f"forward, sample {n}"
        assert np.array_equal(rec[n:n + 1].numpy(), rec_ref), f"record, sample {n}"
        dx_ref = np_maxpool_bwd(rec_ref, dyn.astype(np.float64), xn.shape, k, s, p)
        err = float(np.abs(dx_rec[n:n + 1].numpy() - dx_ref).max())
        assert err <= bound, f"backward, sample {n}: {err:.3e} > {bound:.3e}"
        if n < 4:
            u = np.maximum(xn.astype(np.float64) * sc.double().numpy() + sh.double().numpy(), 0.0).astype(np.float32)
            ya_ref, reca_ref = np_maxpool(u, k, s, p, Ho, Wo)
            assert np.array_equal(y_a[n:n + 1].numpy(), ya_ref), f"forward with in_affine, sample {n}"
            assert np.array_equal(rec_a[n:n + 1].numpy(), reca_ref), f"record with in_affine, sample {n}"
            amax = max(amax, float(np.abs(ya_ref).max()))
    assert float(am.max()) == amax


def test_avgpool2d_past_the_grid_cap(gpu_device):
    k, s, p = 3, 1, 1
    N, C, H, W = 2, 256, 131, 130                        # 2.18 M float4 in and out
    assert N * H * W * C // 4 > CAP
    g = torch.Generator().manual_seed(72)
    x, dy = randn32(g, N, C, H, W), randn32(g, N, C, H, W)
    xd, dyd = dev(to_nhwc(x)), dev(to_nhwc(dy))
    y = fn.avgpool2d_forward(xd, k, s, p)
    within(to_nchw(host(y)), F.avg_pool2d(x, k, s, p, count_include_pad=True),
           11 * U * F.avg_pool2d(x.abs(), k, s, p, count_include_pad=True), "avgpool2d_forward")
    dx = fn.avgpool2d_backward(dyd, tuple(xd.shape), k, s, p)
    within(to_nchw(host(dx)), avg2d_bwd_ref(dy, x.shape, k, s, p), 11 * U * avg2d_bwd_ref(dy.abs(), x.shape, k, s, p),
           "avgpool2d_backward")


def test_elementwise_past_the_grid_cap(gpu_device):
    g = torch.Generator().manual_seed(73)
    n = 4 * (CAP + 1000) + 3                             # add: float4 items past the cap, and a 3-element tail
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    assert torch.equal(fn.add(a.cuda(), b.cuda()).cpu(), (a.double() + b.double()).float())
    n = CAP + 1001                                       # relu_backward, fill: one element per item
    y, dy = a[:n].clamp(min=0), b[:n]
    exp = torch.where(y > 0, dy, torch.zeros_like(dy))
    assert torch.equal(fn.relu_backward(y.cuda(), dy.cuda()).cpu(), exp)
    base = a[n:2 * n]
    assert torch.equal(fn.relu_backward(y.cuda(), dy.cuda(), dx=base.clone().cuda(), accumulate=True).cpu(),
                       (exp.double() + base.double()).float())
    t = torch.full((n,), float("nan"), device="cuda")
    assert torch.equal(fn.fill(t, 2.5).cpu(), torch.full((n,), 2.5))


def test_layout_kernels_past_the_grid_cap(gpu_device):
    g = torch.Generator().manual_seed(74)
    N, C, H, W = 2, 3, 1025, 1024                        # 2 099 200 pixels (one item each), 6.3 M elements back
    assert N * H * W > CAP
    x = torch.randn(N, C, H, W, generator=g)
    xd = fn.nchw_to_nhwc(x.cuda(), out=torch.full((N, H, W, 4), float("nan"), device="cuda"))
    assert torch.equal(xd[..., :C].cpu(), x.permute(0, 2, 3, 1)) and not bool(xd[..., C:].cpu().any())
    assert torch.equal(fn.nhwc_to_nchw(xd, C).cpu(), x)
    del xd
    t = torch.randn(32, 6132, 21, generator=g)           # the SSD head shape: 4.1 M elements
    assert t.numel() > CAP
    assert torch.equal(fn.transpose_bnc(t.cuda()).cpu(), t.permute(0, 2, 1).contiguous())


@pytest.mark.parametrize("C,lds,soff,ldd,doff,rows", [(30, 32, 1, 40, 7, 36000),      # by element: 2.16 M items
                                                      (64, 80, 8, 72, 4, 66000)])     # 16-byte units: 2.11 M float4
def test_copy_block_past_the_grid_cap(gpu_device, C, lds, soff, ldd, doff, rows):
    samples = 2
    vec = C % 4 == 0 and soff % 4 == 0 and doff % 4 == 0
    assert samples * rows * C // (4 if vec else 1) > CAP
    g = torch.Generator().manual_seed(75 + C)
    src = torch.randn(samples, rows, lds, generator=g)
    dss = rows * ldd + 12
    dst = torch.randn(samples, dss, generator=g)
    exp = dst.clone()
    for s_ in range(samples):
        blk = exp[s_, :rows * ldd].view(rows, ldd)
        blk[:, doff:doff + C] = src[s_, :, soff:soff + C]
    out = fn.copy_block(src.cuda(), dst.cuda(), samples, rows, C, rows * lds, lds, soff, dss, ldd, doff)
    assert torch.equal(out.cpu(), exp)


def test_softmax_output_past_the_grid_cap(gpu_device):
    """the rows of a 512 x 1024 segmentation batch and five more: past 8192 workgroups of 128 rows"""
    rows, C, ld = 2 * 512 * 1024 + 5, 19, 20
    assert rows > 128 * (CAP // 256)
    g = torch.Generator().manual_seed(76)
    logits = (randn32(g, rows, C) * 3).float().double()
    label = torch.randint(0, C, (rows,), generator=g).double()
    label[torch.rand(rows, generator=g) < 0.1] = 255
    p_ref = torch.softmax(logits, dim=1)
    onehot = F.one_hot(label.clamp(max=C - 1).long(), C).double()
    g_ref = (p_ref - onehot) * 4.0 * (label != 255).double().unsqueeze(1)
    lg = torch.full((rows, ld), 1e30)
    lg[:, :C] = logits.float()
    prob, grad = fn.softmax_output(lg.cuda(), label.float().cuda(), C, 255.0, 4.0, None)
    prob, grad = prob.cpu(), grad.cpu()
    close(prob[:, :C].double(), p_ref, 1e-6)
    close(grad[:, :C].double(), g_ref, 1e-5)
    assert not bool(prob[:, C:].any()) and not bool(grad[:, C:].any())
    assert not bool(grad[label == 255].any())


def test_losses_count_and_sgd_past_the_grid_cap(gpu_device):
    g = torch.Generator().manual_seed(77)
    n = CAP + 1003
    pred, target = randn32(g, n) * 2, randn32(g, n)
    mask = (torch.rand(n, generator=g) < 0.3).double()
    x = mask * (pred - target)
    loss_ref = torch.where(x.abs() < 1, 0.5 * x * x, x.abs() - 0.5)
    d_ref = mask * torch.where(x.abs() < 1, x, torch.sign(x)) * (0.5 / 7.0)
    pd, td, md = dev(pred), dev(target), dev(mask)
    loss = fn.smooth_l1_forward(pd, td, md)
    close(loss.cpu().double(), loss_ref, 1e-6)
    close(fn.smooth_l1_backward(pd, td, md, torch.tensor([7.0], device="cuda"), grad_scale=0.5).cpu().double(), d_ref, 1e-4)
    # count: its launch is capped at 1024 workgroups (262 144 items); n is far past that and past CAP
    lab = torch.randint(-1, 3, (n,), generator=g).float()
    assert float(fn.count(lab.cuda(), "ne", -1.0)) == float((lab != -1).sum())
    assert float(fn.count(lab.cuda(), "gt", 0.0)) == float((lab > 0).sum())
    np.testing.assert_allclose(float(fn.sum_all(loss)), float(loss.cpu().double().sum()), rtol=1e-5)
    n = 4 * (CAP + 1000)                                 # sgd: float4 items; one large arena
    w, gr, mom = randn32(g, n), randn32(g, n), randn32(g, n)
    lr, mu, wd, rs = 0.0005, 0.9, 0.0005, 1 / 32
    m_ref = mu * mom - lr * (rs * gr + wd * w)
    wd_, gd, md_ = dev(w), dev(gr), dev(mom)
    fn.sgd_momentum(wd_, gd, md_, lr, mu, wd, rs)
    close(md_.cpu().double(), m_ref, 1e-6)
    close(wd_.cpu().double(), w + m_ref, 1e-6)
    assert torch.equal(gd.cpu().double(), gr)


# ---------------------------------------------------------------------------------------------------------------------
# 4. losses and read-outs
def _softmax_case(ld, C, g, rows=261):
    """logits (float32-representable), labels with ignored rows, and the special rows: large logits around +-1e4, equal
    logits, one -inf entry (admitted: module docstring); pad columns hold 1e30 -- were one read, every probability of its
    row would collapse to 0"""
    logits = randn32(g, rows, C) * 3
    logits[0] = torch.linspace(-1e4, 1e4, C).float().double() if C > 1 else 1e4
    logits[1] = 1e4 + randn32(g, C)
    logits[2] = -1e4
    logits[3] = 0.75                                    # equal logits: 1 / C each
    logits[4, C // 2] = -float("inf")
    logits = logits.float().double()                    # what the device is given, exactly
    label = torch.randint(0, C, (rows,), generator=g).double()
    label[torch.rand(rows, generator=g) < 0.2] = 255
    label[:5] = torch.tensor([C - 1, 0, 0, C - 1, (C // 2 + 1) % C]).double()
    lg = torch.full((rows, ld), 1e30)
    lg[:, :C] = logits.float()
    return logits, label, lg


SOFTMAX_LD_C = [(ld, C) for ld in (4, 12, 13, 24, 25, 63, 64) for C in sorted({ld, ld - 1, 2})]


@pytest.mark.parametrize("ld,C", SOFTMAX_LD_C)
def test_softmax_output_dispatch_boundaries(gpu_device, ld, C):
    g = torch.Generator().manual_seed(100 * ld + C)
    logits, label, lg = _softmax_case(ld, C, g)
    rows = logits.shape[0]
    p_ref = torch.softmax(logits, dim=1)
    assert abs(float(p_ref[3, 0]) - 1.0 / C) < 1e-15 and float(p_ref[4, C // 2]) == 0.0
    valid = (label != 255).double().unsqueeze(1)
    onehot = F.one_hot(label.clamp(max=C - 1).long(), C).double()
    lgd, labd = lg.cuda(), label.float().cuda()
    for cnt, gs in ((None, 1.0), (0.0, 3.0), (1.0, 3.0), (37.0, 0.25)):      # scale = grad_scale / max(1, count)
        vc = None if cnt is None else torch.tensor([cnt], device="cuda")
        prob = torch.full((rows, ld), float("nan"), device="cuda")
        grad = torch.full((rows, ld), float("nan"), device="cuda")
        fn.softmax_output(lgd, labd, C, 255.0, gs, vc, prob=prob, grad=grad)
        prob, grad = prob.cpu(), grad.cpu()
        g_ref = (p_ref - onehot) * valid * (gs / max(1.0, cnt or 0.0))
        close(prob[:, :C].double(), p_ref, 1e-6)
        close(grad[:, :C].double(), g_ref, 1e-5)
        assert not bool(prob[:, C:].any()) and not bool(grad[:, C:].any()), "pad column not exactly 0"
        assert not bool(grad[label == 255].any()), "ignored row with a gradient"
    # all rows ignored: the gradient is exactly 0; the probabilities are unchanged
    _, grad0 = fn.softmax_output(lgd, torch.full((rows,), 255.0, device="cuda"), C, 255.0, 2.0, None)
    assert not bool(grad0.cpu().any())
    # label=None: probabilities only
    prob1, none = fn.softmax_output(lgd, None, C, 255.0, want_grad=False)
    assert none is None and torch.equal(prob1.cpu(), prob)


def test_softmax_output_refuses_more_than_64_columns(gpu_device):
    from dspnet_amd._lib import DspnError
    L = fn.L()
    for ld, C in ((65, 65), (65, 19), (68, 64)):
        lg = torch.zeros(8, ld, device="cuda"); prob = torch.zeros(8, ld, device="cuda")
        rc = L.dspn_softmax_output_f32(fn.ptr(lg), 0, fn.ptr(prob), 0, 8, C, ld, 255.0, 1.0, 0, fn.stream())
        assert rc != 0 and b"<= 64" in L.dspn_last_error()
        with pytest.raises(DspnError):
            fn.softmax_output(lg, None, C, 255.0, want_grad=False)
    lg = torch.zeros(8, 20, device="cuda")
    with pytest.raises(DspnError):                       # a gradient needs labels
        fn.softmax_output(lg, None, 19, 255.0, grad=torch.zeros_like(lg))


@pytest.mark.parametrize("rows", [1, 1023, 1025, 1030, 5000])
def test_cross_entropy_sum_skips_and_eps(gpu_device, rows):
    g = torch.Generator().manual_seed(rows)
    C, ld = 9, 12
    prob = torch.rand(rows, ld, generator=g)
    prob[rows // 2, :] = 0.0                             # log(0 + eps)
    label = torch.randint(0, C, (rows,), generator=g).float()
    if rows > 1:
        label[1::7] = -1.0; label[2::7] = -3.0; label[3::7] = float(C); label[4::7] = 11.0; label[5::7] = 255.0
    for ignore, eps in ((-1.0, 1e-3), (255.0, 1e-8)):
        keep = (label != ignore) & (label >= 0) & (label < C)
        picked = prob[torch.arange(rows)[keep], label[keep].long()]
        ref = -(torch.log((picked + np.float32(eps)).double())).sum()    # the operator adds eps in float, then takes the log
        ce = fn.cross_entropy_sum(prob.cuda(), label.cuda(), C, ignore, eps).cpu()
        assert float(ce[1]) == float(keep.sum())
        np.testing.assert_allclose(float(ce[0]), float(ref), rtol=1e-5, atol=1e-30)


def test_count_modes_and_its_2_pow_24_limit(gpu_device):
    """float accumulation of ones is exact below 2^24 only: the entry point refuses n >= 2^24 instead of rounding"""
    from dspnet_amd._lib import DspnError
    one = torch.tensor([3.0], device="cuda")
    assert float(fn.count(one, "ne", 3.0)) == 0.0 and float(fn.count(one, "ne", 2.0)) == 1.0
    assert float(fn.count(one, "gt", 3.0)) == 0.0 and float(fn.count(one, "gt", 2.0)) == 1.0
    g = torch.Generator().manual_seed(5)
    for n in (262_143, 262_144, 262_145, 300_001):       # around the launch's own cap of 1024 workgroups
        a = torch.randint(-1, 4, (n,), generator=g).float()
        out = torch.full((1,), float("nan"), device="cuda")
        assert float(fn.count(a.cuda(), "ne", -1.0, out=out)) == float((a != -1).sum())
        assert float(fn.count(a.cuda(), "gt", 1.0, out=out)) == float((a > 1).sum())
    n = 2 ** 24 - 1                                      # the largest n it takes, every element counted: still exact
    ones = torch.ones(2 ** 24 + 1000, device="cuda")
    assert float(fn.count(ones[:n], "gt", 0.0)) == float(n)
    for n in (2 ** 24, 2 ** 24 + 1000):                  # every element counted would not fit a float: an error
        rc = fn.L().dspn_count_f32(fn.ptr(ones), n, 1, 0.0, fn.ptr(one), fn.stream())
        assert rc != 0 and b"2^24" in fn.L().dspn_last_error()
        with pytest.raises(DspnError):
            fn.count(ones[:n], "gt", 0.0)


def test_smooth_l1_at_the_kink_and_with_no_valid_element(gpu_device):
    g = torch.Generator().manual_seed(6)
    n = 4099
    target = randn32(g, n)
    res = randn32(g, n) * 2
    res[:9] = torch.tensor([1.0, -1.0, 0.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20, -1.0 - 2.0 ** -20, -1.0 + 2.0 ** -20, 5.0, -5.0]).double()
    target[:9] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, -2.0]).double()     # pred - target exact
    pred = (res + target).float().double()
    mask = (torch.rand(n, generator=g) < 0.5).double()
    mask[:9] = 1.0
    x = mask * (pred.float() - target.float()).double()                 # the float difference, as the operator forms it
    loss_ref = torch.where(x.abs() < 1, 0.5 * x * x, x.abs() - 0.5)
    pd, td, md = dev(pred), dev(target), dev(mask)
    loss = fn.smooth_l1_forward(pd, td, md).cpu()
    close(loss.double(), loss_ref, 1e-6)
    assert loss[:3].tolist() == [0.5, 0.5, 0.0]
    assert not bool(loss[mask == 0].any())                              # mask 0: exactly no loss
    for cnt, gs in ((0.0, 1.0), (1.0, 2.5), (123.0, 2.5)):              # scale = grad_scale / max(1, valid_count)
        d_ref = mask * torch.where(x.abs() < 1, x, torch.sign(x)) * (gs / max(1.0, cnt))
        grad = fn.smooth_l1_backward(pd, td, md, torch.tensor([cnt], device="cuda"), grad_scale=gs).cpu()
        close(grad.double(), d_ref, 1e-4)
        assert not bool(grad[mask == 0].any())
        assert grad[:3].tolist() == [np.float32(gs / max(1.0, cnt)), -np.float32(gs / max(1.0, cnt)), 0.0]
    zero = fn.smooth_l1_backward(pd, td, torch.zeros(n, device="cuda"), torch.tensor([0.0], device="cuda")).cpu()
    assert not bool(zero.any())


@pytest.mark.parametrize("n", [1, 1023, 1025, 3_000_001])
def test_sum_all(gpu_device, n):
    g = torch.Generator().manual_seed(n)
    a = torch.rand(n, generator=g) + torch.randn(n, generator=g) * 0.1
    np.testing.assert_allclose(float(fn.sum_all(a.cuda())), float(a.double().sum()), rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# 5. element-wise, column sums, layout, SGD
@pytest.mark.parametrize("n", [1, 3, 1000, 1001, 1002, 1003])
def test_add_any_length_and_relu_backward_accumulate(gpu_device, n):
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    assert torch.equal(fn.add(a.cuda(), b.cuda()).cpu(), (a.double() + b.double()).float())     # one rounding
    y = torch.randn(n, generator=g).clamp(min=0)
    y[::5] = 0.0; y[1::5] = -0.0                         # y exactly 0 (either sign): no gradient
    exp = torch.where(y > 0, b, torch.zeros_like(b))
    assert torch.equal(fn.relu_backward(y.cuda(), b.cuda(), dx=torch.full((n,), float("nan"), device="cuda")).cpu(), exp)
    assert torch.equal(fn.relu_backward(y.cuda(), b.cuda(), dx=a.clone().cuda(), accumulate=True).cpu(),
                       (exp.double() + a.double()).float())


@pytest.mark.parametrize("rows", [1, 31, 33, 100, 1000])      # 100, 1000: not a multiple of the 64-row slab
@pytest.mark.parametrize("C,ld", [(1, 4), (30, 32), (256, 256), (300, 300), (2048, 2048)])
def test_colsum_and_relu_backward_colsum_shapes(gpu_device, rows, C, ld):
    g = torch.Generator().manual_seed(rows + C)
    a = torch.randn(rows, ld, generator=g)
    out = torch.full((C,), float("nan"), device="cuda")
    close(fn.colsum(a.cuda(), C, out=out).cpu().double(), a.double().sum(0)[:C], 1e-5)
    y = torch.randn(rows, ld, generator=g).clamp(min=0)
    ref_dx = torch.where(y > 0, a, torch.zeros_like(a))
    block = torch.zeros(fn.ABSMAX_SLOTS, device="cuda")
    dx, s = fn.relu_backward_colsum(y.cuda(), a.clone().cuda(), C, out=torch.full((C,), float("nan"), device="cuda"), dx_absmax=block)
    assert torch.equal(dx.cpu(), ref_dx)
    close(s.cpu().double(), ref_dx.double().sum(0)[:C], 1e-5)
    assert float(block.max()) == float(ref_dx.abs().max())


@pytest.mark.parametrize("C,Cp", [(1, 4), (3, 4), (1, 8), (3, 8), (5, 8)])
def test_layout_pad_channels(gpu_device, C, Cp):
    g = torch.Generator().manual_seed(10 * C + Cp)
    x = torch.randn(3, C, 37, 53, generator=g)
    xd = fn.nchw_to_nhwc(x.cuda(), out=torch.full((3, 37, 53, Cp), float("nan"), device="cuda"))
    assert torch.equal(xd[..., :C].cpu(), x.permute(0, 2, 3, 1)) and not bool(xd[..., C:].cpu().any())
    junk = xd.clone(); junk[..., C:] = float("nan")      # C < Cp: the pad channels are never read
    assert torch.equal(fn.nhwc_to_nchw(junk, C).cpu(), x)
    t = torch.randn(1, 1, 1, generator=g)
    assert torch.equal(fn.transpose_bnc(t.cuda()).cpu(), t)


@pytest.mark.parametrize("n", [4, 8, 4092, 4100])
@pytest.mark.parametrize("mu,wd", [(0.9, 0.0005), (0.0, 0.0005), (0.9, 0.0), (0.0, 0.0)])
def test_sgd_momentum_rule(gpu_device, n, mu, wd):
    """MXNet's sgd_mom_update: mom = momentum * mom - lr * (rescale * grad + wd * w); w += mom"""
    g = torch.Generator().manual_seed(n)
    w, gr, mom = randn32(g, n), randn32(g, n), randn32(g, n)
    lr, rs = 0.01, 1 / 8
    m_ref = mu * mom - lr * (rs * gr + wd * w)
    wd_, gd, md = dev(w), dev(gr), dev(mom)
    fn.sgd_momentum(wd_, gd, md, lr, mu, wd, rs)
    close(md.cpu().double(), m_ref, 1e-6)
    close(wd_.cpu().double(), w + m_ref, 1e-6)


def test_sgd_momentum_refuses_a_length_that_is_no_multiple_of_4(gpu_device):
    from dspnet_amd._lib import DspnError
    for n in (3, 4097, 4098):
        w = torch.ones(n, device="cuda")
        with pytest.raises(DspnError):
            fn.sgd_momentum(w, torch.ones_like(w), torch.zeros_like(w), 0.1, 0.9, 0.0, 1.0)
        assert torch.equal(w.cpu(), torch.ones(n))       # refused, not partly applied


# ---------------------------------------------------------------------------------------------------------------------
# 6. bf16 twins of the geometries and boundary lengths above: bf16 kernel == round_to_bf16(float kernel), bit for bit
TWIN_SHAPES = [(2, 13, 14, 24), (1, 35, 35, 64), (3, 1, 9, 8), (1, 2, 2, 8)]        # NHWC, channels in 16-byte chunks of bf16


@pytest.mark.parametrize("shape", TWIN_SHAPES, ids=_id)
def test_pooling_geometries_bf16_twins(gpu_device, shape):
    N, H, W, C = shape
    nchw_shape = (N, C, H, W)
    xh, xf = _pair(shape, 40)
    for k, s, p, full in MAXPOOL_GEOMS:
        if not _legal(nchw_shape, k, s, p, full):
            continue
        Ho, Wo = pool_out(H, k, s, p, full), pool_out(W, k, s, p, full)
        rh = torch.zeros(N, Ho, Wo, C, dtype=torch.uint8, device="cuda"); rf = torch.zeros_like(rh)
        yh = fn.maxpool_forward(xh, k, s, p, out=torch.empty(N, Ho, Wo, C, dtype=BF, device="cuda"), argmax=rh)
        yf = fn.maxpool_forward(xf, k, s, p, out=torch.empty(N, Ho, Wo, C, device="cuda"), argmax=rf)
        _same_stored(yh, yf, f"maxpool {k}/{s}/{p}")
        assert torch.equal(rh, rf)
        gh, gf = _pair((N, Ho, Wo, C), 41)
        _same_stored(fn.maxpool_backward_argmax(rh, gh, shape, k, s, p), fn.maxpool_backward_argmax(rf, gf, shape, k, s, p),
                     f"maxpool_backward_argmax {k}/{s}/{p}")
        _same_stored(fn.maxpool_backward(xh, yh, gh, k, s, p), fn.maxpool_backward(xf, yf, gf, k, s, p),
                     f"maxpool_backward {k}/{s}/{p}")
    for k, s, p in AVGPOOL2D_GEOMS:
        if not _legal(nchw_shape, k, s, p):
            continue
        yh, yf = fn.avgpool2d_forward(xh, k, s, p), fn.avgpool2d_forward(xf, k, s, p)
        _same_stored(yh, yf, f"avgpool2d {k}/{s}/{p}")
        gh, gf = _pair(tuple(yf.shape), 42)
        for acc in (False, True):
            bh, bf_ = _pair(shape, 43)
            _same_stored(fn.avgpool2d_backward(gh, shape, k, s, p, dx=bh, accumulate=acc),
                         fn.avgpool2d_backward(gf, shape, k, s, p, dx=bf_, accumulate=acc), f"avgpool2d_backward {k}/{s}/{p} acc={acc}")
    for k in (1, 2, 4):
        if H < k or W < k:
            continue
        yh, yf = fn.avgpool_forward(xh, k), fn.avgpool_forward(xf, k)
        _same_stored(yh, yf, f"avgpool {k}")
        gh, gf = _pair(tuple(yf.shape), 44)
        for acc in (False, True):
            bh, bf_ = _pair(shape, 45)
            _same_stored(fn.avgpool_backward(gh, shape, k, dx=bh, accumulate=acc),
                         fn.avgpool_backward(gf, shape, k, dx=bf_, accumulate=acc), f"avgpool_backward {k} acc={acc}")


@pytest.mark.parametrize("ld,C", SOFTMAX_LD_C)
def test_softmax_output_boundaries_bf16_twins(gpu_device, ld, C):
    lh, lf = _pair((261, ld), 50 + ld, 3.0)
    g = torch.Generator().manual_seed(ld + C)
    label = torch.randint(0, C, (261,), generator=g).float().cuda(); label[::7] = 255.0
    ph, gh = fn.softmax_output(lh, label, C, 255.0, 0.25)
    pf, gf = fn.softmax_output(lf, label, C, 255.0, 0.25)
    assert ph.dtype == torch.float32 and torch.equal(ph, pf)
    _same_stored(gh, gf, f"softmax gradient ld={ld} C={C}")
