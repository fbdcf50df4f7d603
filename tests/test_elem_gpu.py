"""Elementwise, pooling and loss kernels (pool_elem.hip, softmax_opt.hip,
dropout_ln.hip) against fp64 references at model layouts and edges.

Convention: inputs are rounded to the 16-bit dtype first; the reference is
fp64 on those rounded values, on the CPU. Every case runs in bf16 and fp16.
Where the operation is a selection or an exactly representable sum the
result must be bit-equal (torch.equal) to the fp64 result rounded to the
dtype; otherwise it must agree within N units in the last place of the output
dtype at the reference's magnitude (`ulp`). Small-integer inputs ([-4,4])
make the references exact. Each test prints its figures before asserting.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CL = torch.channels_last
DTYPES = [torch.bfloat16, torch.float16]
dtype_ids = ["bf16", "fp16"]
both_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)


def ext():
    from dtmx.ops.hip import require_ext
    return require_ext()


def DFm():
    from dtmx.ops import functional as DF
    return DF


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed)) * scale


def ints(shape, seed, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def ulp(dtype, ref):
    """Spacing of `dtype` at the magnitude of each element of the fp64 tensor
    `ref`: 2^(floor(log2|ref|) - mantissa bits), and below the smallest
    normal number the subnormal step (fp16: 2^-24, bf16: 2^-133)."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(ref.double().abs())[1] - 1     # |ref| = m * 2^(e+1), m in [.5,1)
    e = torch.where(ref == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - mant).double())


def ulp_err(got, ref, dtype, at=None):
    """Largest |got - ref| in ulps of dtype at |ref| (or at `at`)."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    u = ulp(dtype, ref if at is None else at.detach().double().cpu())
    return ((got - ref).abs() / u).max().item()


def check_ulp(got, ref, dtype, n, name, at=None):
    e = ulp_err(got, ref, dtype, at)
    print(f"{name}: max error {e:.3f} ulp (bound {n})")
    assert got.dtype == dtype, (name, got.dtype)
    assert e <= n, f"{name}: {e:.3f} ulp > {n}"


def check_equal(got, ref64, dtype, name):
    """Bit equality with the fp64 reference rounded to dtype."""
    want = ref64.detach().cpu().to(dtype)
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == want.shape, (name, got.dtype,
                                                             got.shape)
    bad = (got != want).sum().item()
    print(f"{name}: {bad} of {want.numel()} elements differ")
    assert torch.equal(got, want), f"{name}: {bad} elements differ"


def test_ulp_helper():
    one = torch.tensor([1.0, 1.999, 2.0, 0.75, 0.0, 1e-30, 6e-8, -3.0],
                       dtype=torch.float64)
    assert ulp(torch.bfloat16, one).tolist() == [
        2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133,
        2.0 ** (-100 - 7), 2.0 ** (-24 - 7), 2.0 ** -6]
    assert ulp(torch.float16, one).tolist() == [
        2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24,
        2.0 ** -24, 2.0 ** -9]
    for dt in DTYPES:   # agrees with the spacing torch itself rounds to
        x = torch.tensor([1.0, 3.0, 0.3, 100.0], dtype=dt)
        nxt = torch.nextafter(x, torch.full_like(x, 1e4))
        assert torch.equal((nxt.double() - x.double()), ulp(dt, x.double()))


# ===================================================== A. relu / add+relu ==

def _relu_inputs(shape, seed, dtype):
    x = randn(shape, seed).to(dtype)
    x.view(-1)[::7] = 0                       # relu'(0) = 0 on both sides
    return x


def _cat_halves(f, *xs):
    C = xs[0].shape[1]
    return torch.cat([f(*(x[:, :C // 2] for x in xs)),
                      f(*(x[:, C // 2:] for x in xs))], dim=1)


@both_dtypes
@pytest.mark.parametrize("sliced", [True, False], ids=["slices", "dense"])
def test_elem_relu_cat_backward(dtype, sliced):
    """conv -> relu -> cat(dim=1) (googlenet): cat's backward hands each relu
    a channel narrow of the NHWC gradient, strides (400,1,80,16)."""
    DF = DFm()
    x = _relu_inputs((2, 16, 5, 5), 1, dtype)
    dy = randn((2, 16, 5, 5), 2).to(dtype)

    def graph(relu, x, dy):
        x = x.requires_grad_(True)
        if sliced:
            y = _cat_halves(relu, x)
        else:   # each branch owns a dense NHWC tensor, as after a conv
            y = torch.cat([relu((x[:, :8] * 1).contiguous(memory_format=CL)),
                           relu((x[:, 8:] * 1).contiguous(memory_format=CL))], 1)
        y.backward(dy)
        return y, x.grad

    y, dx = graph(DF.relu, nhwc(x), nhwc(dy))
    yr, dxr = graph(torch.relu, x.float().contiguous(memory_format=CL),
                    dy.float().contiguous(memory_format=CL))
    check_equal(y, yr, dtype, "relu cat y")
    check_equal(dx, dxr, dtype, "relu cat dx")


@both_dtypes
def test_elem_relu_reshape_backward(dtype):
    """relu -> flatten: the gradient comes back as an NCHW block while the
    saved activation is NHWC."""
    DF = DFm()
    x = _relu_inputs((2, 16, 5, 5), 3, dtype)
    dy = randn((2, 400), 4).to(dtype)
    xg = nhwc(x).requires_grad_(True)
    y = DF.relu(xg).reshape(2, -1)
    y.backward(dy.to(DEV))
    xr = x.float().contiguous(memory_format=CL).requires_grad_(True)
    yr = torch.relu(xr).reshape(2, -1)
    yr.backward(dy.float())
    check_equal(y, yr, dtype, "relu reshape y")
    check_equal(xg.grad, xr.grad, dtype, "relu reshape dx")


@both_dtypes
@pytest.mark.parametrize("via_cat", [True, False], ids=["cat", "direct"])
@pytest.mark.parametrize("b_nhwc", [False, True], ids=["b_nchw", "b_nhwc"])
def test_elem_add_relu_layouts(dtype, b_nhwc, via_cat):
    DF = DFm()
    a = _relu_inputs((2, 16, 5, 5), 5, dtype)
    b = randn((2, 16, 5, 5), 6).to(dtype)
    dy = randn((2, 16, 5, 5), 7).to(dtype)

    def graph(f, a, b, dy):
        a = a.detach().clone().contiguous(memory_format=CL).requires_grad_(True)
        b = b.detach().clone()
        b = (b.contiguous(memory_format=CL) if b_nhwc
             else b.contiguous()).requires_grad_(True)
        y = _cat_halves(f, a, b) if via_cat else f(a, b)
        y.backward(dy.contiguous(memory_format=CL))
        return y, a.grad, b.grad

    y, da, db = graph(DF.add_relu, a.to(DEV), b.to(DEV), dy.to(DEV))
    # the kernel adds in fp32 and rounds once; so does fp64 on 16-bit inputs
    yr, dar, dbr = graph(lambda p, q: torch.relu(p + q), a.double(),
                         b.double(), dy.double())
    check_equal(y, yr, dtype, "add_relu y")
    check_equal(da, dar, dtype, "add_relu da")
    check_equal(db, dbr, dtype, "add_relu db")


@both_dtypes
def test_elem_relu_channel_slice(dtype):
    """A channel slice of an NHWC tensor has gaps; reading numel elements
    from its data_ptr would read the neighbours' channels."""
    DF = DFm()
    x = _relu_inputs((2, 32, 5, 5), 8, dtype)
    dy = randn((2, 16, 5, 5), 9).to(dtype)
    xg = nhwc(x).requires_grad_(True)
    y = DF.relu(xg[:, 8:24])
    y.backward(nhwc(dy))
    xr = x.double().requires_grad_(True)
    yr = torch.relu(xr[:, 8:24])
    yr.backward(dy.double())
    check_equal(y, yr, dtype, "relu slice y")
    check_equal(xg.grad, xr.grad, dtype, "relu slice dx")


@both_dtypes
def test_elem_relu_numel_not_multiple_of_8(dtype):
    DF = DFm()
    x = _relu_inputs((3, 5, 3, 3), 10, dtype)
    dy = randn((3, 5, 3, 3), 11).to(dtype)
    xg = nhwc(x).requires_grad_(True)
    y = DF.relu(xg)
    y.backward(nhwc(dy))
    xr = x.double().requires_grad_(True)
    yr = torch.relu(xr)
    yr.backward(dy.double())
    check_equal(y, yr, dtype, "relu 135 y")
    check_equal(xg.grad, xr.grad, dtype, "relu 135 dx")
    b = randn((3, 5, 3, 3), 12).to(dtype)
    z = DF.add_relu(nhwc(x), b.to(DEV))
    check_equal(z, torch.relu(x.double() + b.double()), dtype, "add_relu 135")


def test_elem_add_relu_mixed_dtypes_take_torch_path():
    DF = DFm()
    a = _relu_inputs((2, 16, 5, 5), 13, torch.bfloat16)
    b = randn((2, 16, 5, 5), 14)
    z = DF.add_relu(nhwc(a), nhwc(b))
    assert z.dtype == torch.float32
    assert torch.equal(z.cpu(), torch.relu(a.float() + b))


def test_elem_relu_host_checks_raise():
    """The checks are on the host: nothing is launched."""
    e = ext()
    y = nhwc(_relu_inputs((2, 16, 5, 5), 15, torch.bfloat16))
    dy = y.contiguous()                              # NCHW against NHWC
    with pytest.raises(RuntimeError, match="same strides"):
        e.relu_bwd(dy, y)
    with pytest.raises(RuntimeError, match="same strides"):
        e.add_relu_fwd(y, dy)
    with pytest.raises(RuntimeError, match="same dtype"):
        e.relu_bwd(y.half(), y)
    with pytest.raises(RuntimeError, match="same dtype"):
        e.add_relu_fwd(y, y.half())
    with pytest.raises(RuntimeError, match="same sizes"):
        e.relu_bwd(y.reshape(2, 16, 25, 1), y)
    big = nhwc(_relu_inputs((2, 32, 5, 5), 16, torch.bfloat16))
    with pytest.raises(RuntimeError, match="dense"):
        e.relu_fwd(big[:, 8:24])
    with pytest.raises(RuntimeError, match="dense"):
        e.relu_bwd(big[:, :16], y)
    with pytest.raises(RuntimeError, match="dense"):
        e.add_relu_fwd(y, big[:, :16])
    with pytest.raises(RuntimeError, match="multiple of 8"):
        e.relu_fwd(torch.zeros(135, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="16-bit"):
        e.relu_fwd(torch.zeros(16, device=DEV))
    # dense operands that agree still run, whatever their dim order
    p = y.permute(3, 1, 0, 2)
    assert torch.equal(e.relu_bwd(p, p), (p * (p > 0)))


# ============================================================ B. max pool ==

MAXPOOL_CASES = [
    # (N, C, H, W, K, stride, pad)
    (2, 8, 7, 10, 3, 2, 1),        # H != W
    (2, 24, 8, 8, 3, 2, 0),        # row/col 7 reached by no window: dx = 0
    (2, 16, 6, 9, 2, 2, 0),        # H != W, 2/2/0 (vgg, lenet)
    (1, 8, 5, 5, 3, 1, 1),         # 3/1/1 (googlenet)
    (2, 20, 6, 7, 2, 2, 0),        # scalar path, C = 20
    (2, 3, 9, 9, 3, 2, 1),         # scalar path, C = 3
    (8, 128, 130, 130, 2, 2, 0),   # vector path, fwd items > 2048*256
    (2, 20, 240, 240, 2, 2, 0),    # scalar path, same grid-stride condition
]
GRID_CAP_ITEMS = 2048 * 256


def test_elem_maxpool_big_cases_pass_the_grid_cap():
    for (N, C, H, W, K, s, p) in MAXPOOL_CASES[-2:]:
        P, Q = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        per = C // 8 if C % 8 == 0 else C
        assert N * P * Q * per > GRID_CAP_ITEMS      # forward
        assert N * H * W * per > GRID_CAP_ITEMS      # backward


@functools.lru_cache(maxsize=None)
def _maxpool_ref(case):
    """Integer inputs are the same in both dtypes: one fp64 reference."""
    N, C, H, W, K, s, p = case
    x = ints((N, C, H, W), 100)
    xr = x.double().requires_grad_(True)
    y, flat = F.max_pool2d(xr, K, s, p, return_indices=True)
    P, Q = y.shape[2], y.shape[3]
    # torch's index is ih*W+iw; the kernel stores the window-local kh*K+kw
    ih, iw = flat // W, flat % W
    kh = ih - (torch.arange(P).view(1, 1, P, 1) * s - p)
    kw = iw - (torch.arange(Q).view(1, 1, 1, Q) * s - p)
    assert kh.min() >= 0 and kh.max() < K and kw.min() >= 0 and kw.max() < K
    code = (kh * K + kw).to(torch.uint8)
    dy = ints((N, C, P, Q), 101)
    y.backward(dy.double())
    return x, y.detach(), code, dy, xr.grad


@both_dtypes
@pytest.mark.parametrize("case", MAXPOOL_CASES, ids=str)
def test_elem_maxpool_exact(case, dtype):
    N, C, H, W, K, s, p = case
    x, yr, code, dy, dxr = _maxpool_ref(case)
    y, idx = ext().maxpool_fwd(nhwc(x.to(dtype)), K, s, p)
    dx = ext().maxpool_bwd(nhwc(dy.to(dtype)), idx, H, W, K, s, p)
    assert y.is_contiguous(memory_format=CL) and dx.is_contiguous(memory_format=CL)
    check_equal(y, yr, dtype, "maxpool y")
    idx = idx.cpu()
    bad = (idx != code).sum().item()
    print(f"maxpool idx: {bad} of {code.numel()} differ")
    assert idx.dtype == torch.uint8 and torch.equal(idx, code)
    check_equal(dx, dxr, dtype, "maxpool dx")
    if case == MAXPOOL_CASES[1]:
        assert dxr[:, :, 7].abs().max() == 0 and dxr[:, :, :, 7].abs().max() == 0
        assert dx[:, :, 7].abs().max() == 0 and dx[:, :, :, 7].abs().max() == 0


@both_dtypes
@pytest.mark.parametrize("case", [(2, 16, 9, 11, 3, 2, 1), (2, 20, 9, 11, 3, 1, 1)],
                         ids=str)
def test_elem_maxpool_random(case, dtype):
    """Random normal values through autograd; overlapping windows sum up to
    nine gradients in fp32 before the one rounding."""
    N, C, H, W, K, s, p = case
    x = randn((N, C, H, W), 102).to(dtype)
    xg = nhwc(x).requires_grad_(True)
    y = DFm().max_pool2d(xg, K, s, p)
    xr = x.double().requires_grad_(True)
    yr = F.max_pool2d(xr, K, s, p)
    dy = randn(tuple(yr.shape), 103).to(dtype)
    y.backward(dy.to(DEV))                           # NCHW gradient
    yr.backward(dy.double())
    check_ulp(y, yr, dtype, 1, "maxpool random y")
    check_ulp(xg.grad, xr.grad, dtype, 1, "maxpool random dx")


# ================================================== C. global average pool ==

GAP_CASES = [(2, 8, 1, 1), (2, 1000, 8, 8), (3, 20, 5, 7), (2, 2048, 7, 7)]


@both_dtypes
@pytest.mark.parametrize("case", GAP_CASES, ids=str)
def test_elem_global_avgpool(case, dtype):
    """Inputs are post-ReLU-like (max(N(0,1), 0), the only thing the zoo
    feeds this layer), so the mean is well conditioned and one ulp at the
    reference's magnitude is a meaningful bound for an fp32 sum; sums that
    cancel are the integer-exact test's."""
    N, C, H, W = case
    x = randn(case, 200).clamp_min(0).to(dtype)
    dy = randn((N, C), 201).to(dtype)
    xg = nhwc(x).requires_grad_(True)
    y = DFm().global_avg_pool(xg)
    y.backward(dy.to(DEV))
    assert y.shape == (N, C) and xg.grad.is_contiguous(memory_format=CL)
    check_ulp(y, x.double().mean(dim=(2, 3)), dtype, 1, "gap y")
    dxr = (dy.double() / (H * W)).view(N, C, 1, 1).expand(N, C, H, W)
    check_ulp(xg.grad, dxr, dtype, 1, "gap dx")


@both_dtypes
def test_elem_global_avgpool_exact(dtype):
    """|sum| <= 256 and the divisor is 64: exact in both dtypes."""
    N, C, H, W = 2, 64, 8, 8
    x = ints((N, C, H, W), 202)
    dy = ints((N, C), 203)
    y = ext().global_avgpool_fwd(nhwc(x.to(dtype)))
    dx = ext().global_avgpool_bwd(dy.to(dtype).to(DEV), H, W)
    check_equal(y, x.double().mean(dim=(2, 3)), dtype, "gap exact y")
    check_equal(dx, (dy.double() / 64).view(N, C, 1, 1).expand(N, C, H, W),
                dtype, "gap exact dx")


# ================================================================= D. LRN ==

# Largest error measured on an MI355X over all cases below, forward and
# backward, against fp64 F.local_response_norm and its autograd on the
# rounded inputs: see the docstring of test_elem_lrn. The bound is twice
# that, rounded up to a whole ulp.
LRN_MEASURED_ULP = 0.516
LRN_BOUND_ULP = math.ceil(2 * LRN_MEASURED_ULP)     # 2
LRN_CASES = [(8, 5.0), (16, 5.0), (24, 5.0), (192, 5.0), (16, 1e-4)]


def _lrn_ref(x64, dy64, alpha, size):
    xr = x64.clone().requires_grad_(True)
    y = F.local_response_norm(xr, size, alpha=alpha * size / 5, beta=0.75, k=2.0)
    y.backward(dy64)
    return y.detach(), xr.grad


@both_dtypes
@pytest.mark.parametrize("C,alpha", LRN_CASES, ids=str)
def test_elem_lrn(C, alpha, dtype):
    """Window-5 cross-channel LRN with alpha = 5, where the window term is of
    the order of knorm, so a wrong window is visible (and one alpha = 1e-4
    case). C = 8: no halo; 16: one-sided halos; 24, 192: both.

    The kernels use __powf, so the bound is measured: largest error over all
    cases and both dtypes against the fp64 reference 0.516 ulp of the output
    dtype (fp16, C = 192, backward; forward at most 0.500), bound 2 ulp =
    twice that rounded up to a whole ulp.
    The same bound must reject the fp64 reference computed with window 3
    (alpha rescaled so only the window differs)."""
    x = randn((2, C, 3, 3), 300 + C).to(dtype)
    dy = randn((2, C, 3, 3), 301 + C).to(dtype)
    xg = nhwc(x).requires_grad_(True)
    y = DFm().local_response_norm(xg, 5, alpha=alpha, beta=0.75, knorm=2.0)
    y.backward(nhwc(dy))
    yr, dxr = _lrn_ref(x.double(), dy.double(), alpha, 5)
    ef, eb = ulp_err(y, yr, dtype), ulp_err(xg.grad, dxr, dtype)
    print(f"lrn C={C} alpha={alpha} {dtype}: fwd {ef:.3f} ulp, bwd {eb:.3f} ulp")
    if alpha == 5.0:
        y3, dx3 = _lrn_ref(x.double(), dy.double(), alpha, 3)
        s3f = ulp_err(y3.to(dtype), yr, dtype)
        s3b = ulp_err(dx3.to(dtype), dxr, dtype)
        print(f"  window-3 reference: fwd {s3f:.1f} ulp, bwd {s3b:.1f} ulp")
        assert s3f > LRN_BOUND_ULP and s3b > LRN_BOUND_ULP
    assert ef <= LRN_BOUND_ULP, f"lrn fwd {ef:.3f} ulp"
    assert eb <= LRN_BOUND_ULP, f"lrn bwd {eb:.3f} ulp"


# ========================================================= E. softmax + CE ==

SOFTMAX_SHAPES = [(1, 1), (3, 7), (2, 255), (2, 256), (2, 257), (64, 1000),
                  (2, 4099)]
# Largest relative loss error measured on an MI355X per logit set over all
# shapes, dtypes and dloss values, against fp64 cross_entropy(reduction="sum")
# on the rounded logits; the bound is twice that.
LOSS_MEASURED_REL = {"normal": 9.32e-8, "large": 2.307e-7, "peaked": 2.431e-3}
LOSS_BOUND_REL = {k: 2 * v for k, v in LOSS_MEASURED_REL.items()}


def _labels(B, V, seed):
    lab = torch.randint(0, V, (B,), generator=gen(seed))
    lab[0] = 0
    lab[-1] = V - 1
    return lab


def _logits(kind, B, V, lab, dtype, seed):
    if kind == "normal":
        lg = randn((B, V), seed, 2.0)
    elif kind == "large":   # bf16 values up to +-80
        lg = ((torch.rand((B, V), generator=gen(seed)) * 160 - 80)
              .to(torch.bfloat16).float())
    else:                   # label logit +12, the rest 0: the true loss is small
        lg = torch.zeros(B, V)
        lg[torch.arange(B), lab] = 12.0
    return lg.to(dtype)


@both_dtypes
@pytest.mark.parametrize("dloss", [1.0, 0.125])
@pytest.mark.parametrize("kind", ["normal", "large", "peaked"])
@pytest.mark.parametrize("shape", SOFTMAX_SHAPES, ids=str)
def test_elem_softmax_ce(shape, kind, dloss, dtype):
    """Probabilities within 1 ulp of the fp64 softmax (fp16 with an absolute
    floor of one subnormal step, which `ulp` has built in; bf16's range is
    fp32's). dlogits within 1 ulp at max(|p|, |p - onehot|) * dloss: it is
    computed from the stored 16-bit p and inherits p's rounding. The loss
    uses __expf/__logf; its relative error against fp64
    cross_entropy(reduction="sum") is bounded at twice the largest value
    measured per logit set (LOSS_MEASURED_REL). The loss is an fp32 number
    summed over rows by atomics, so on the normal and large sets the figure
    is one to two fp32 ulps of the total and moves with the order of the
    adds. On the peaked set the true loss per row is log(1 + (V-1)e^-12),
    down to 3.7e-5, and the absolute error per row is that of one fp32
    log(1 + tiny): at most 3.4e-7 measured (V = 4099), 9e-8 at V = 7, which
    is where the largest relative figure comes from."""
    B, V = shape
    lab = _labels(B, V, 400 + V)
    lg = _logits(kind, B, V, lab, dtype, 401 + V)
    lgg = lg.to(DEV).requires_grad_(True)
    loss = DFm().softmax_cross_entropy_sum(lgg, lab.to(DEV))     # int64 labels
    (loss * dloss).backward()
    loss2, probs = ext().softmax_ce_fwd(lgg.detach(), lab.to(DEV).int())
    assert loss.dtype == torch.float32 and probs.dtype == dtype

    l64 = lg.double()
    p64 = torch.softmax(l64, dim=1)
    ref_rows = F.cross_entropy(l64, lab, reduction="none")
    ref_loss = ref_rows.sum().item()
    onehot = F.one_hot(lab, V).double()
    d64 = (p64 - onehot) * dloss

    err = abs(loss.item() - ref_loss)
    rel = err / ref_loss if ref_loss > 0 else (0.0 if err == 0 else math.inf)
    print(f"softmax {shape} {kind} dloss={dloss} {dtype}: loss {loss.item():.9g} "
          f"ref {ref_loss:.9g} rel {rel:.3e} abs/row {err / B:.3e}")
    check_ulp(probs, p64, dtype, 1, "probs")
    at = torch.maximum(p64.abs(), (p64 - onehot).abs()) * dloss
    check_ulp(lgg.grad, d64, dtype, 1, "dlogits", at=at)
    assert loss2.item() == pytest.approx(loss.item(), rel=1e-6, abs=1e-9)
    assert rel <= LOSS_BOUND_REL[kind], f"loss rel {rel:.3e}"


# =========================================================== F. layer norm ==

LN_D = [8, 63, 64, 65, 255, 256, 257, 1000, 4097]


def _ln_check(x, dtype, name):
    """x: (B, D) already rounded to dtype. gamma/beta random fp32, dy
    integers in [-4,4]."""
    B, D = x.shape
    gamma = randn((D,), 500 + D, 0.2) + 1.0
    beta = randn((D,), 501 + D, 0.1)
    dy = ints((B, D), 502 + D)
    xg = x.to(DEV).requires_grad_(True)
    gg = gamma.to(DEV).requires_grad_(True)
    bg = beta.to(DEV).requires_grad_(True)
    y = DFm().layer_norm(xg, gg, bg, 1e-5)
    y.backward(dy.to(dtype).to(DEV))

    xr = x.double().requires_grad_(True)
    gr = gamma.double().requires_grad_(True)
    br = beta.double().requires_grad_(True)
    yr = F.layer_norm(xr, (D,), gr, br, 1e-5)
    yr.backward(dy.double())
    xhat = ((x.double() - x.double().mean(1, keepdim=True))
            / (x.double().var(1, unbiased=False, keepdim=True) + 1e-5).sqrt())
    terms = (dy.double() * xhat).abs().sum(0)
    dg_tol = B * 2.0 ** -23 * terms

    _, mean, rstd = ext().layer_norm_fwd(xg.detach(), gg.detach(), bg.detach(), 1e-5)
    rs64 = (x.double().var(1, unbiased=False) + 1e-5).rsqrt()
    rs_rel = ((rstd.double().cpu() - rs64).abs() / rs64).max().item()
    ey, edx = ulp_err(y, yr, dtype), ulp_err(xg.grad, xr.grad, dtype)
    dg_err = (gg.grad.double().cpu() - gr.grad).abs()
    dg_ratio = (dg_err / dg_tol.clamp_min(1e-300)).max().item() \
        if (dg_err > 0).any() else 0.0
    print(f"{name}: rstd rel err {rs_rel:.3e}, y {ey:.3f} ulp, dx {edx:.3f} ulp, "
          f"dgamma err/bound {dg_ratio:.3f}")
    assert y.dtype == dtype and xg.grad.dtype == dtype
    assert gg.grad.dtype == torch.float32 and bg.grad.dtype == torch.float32
    assert ey <= 2, f"{name}: y {ey:.3f} ulp"
    assert edx <= 2, f"{name}: dx {edx:.3f} ulp"
    assert torch.equal(bg.grad.cpu(), br.grad.float()), f"{name}: dbeta"
    assert (dg_err <= dg_tol).all(), f"{name}: dgamma err/bound {dg_ratio:.3f}"


@both_dtypes
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("D", LN_D)
def test_elem_layer_norm(D, B, dtype):
    """Centred N(0,1) rows. y and dx within 2 ulp of fp64; dbeta bit-equal
    (integer dy); dgamma within B * 2^-23 * sum|dy * xhat|. The dgamma bound
    needs each term correct to an fp32 rounding, also where x is close to
    the row mean; an fp32 mean misses it at B = 1 (up to 306x the bound at
    D = 4097 measured), the fp64 statistics give at most 0.50x."""
    _ln_check(randn((B, D), 503 + D).to(dtype), dtype, f"ln D={D} B={B}")


LN_OFFSET = [(torch.float16, 64.0, 1 / 16), (torch.float16, 256.0, 1 / 4),
             (torch.bfloat16, 64.0, 1 / 2)]


@pytest.mark.parametrize("dtype,base,step", LN_OFFSET,
                         ids=["fp16-64", "fp16-256", "bf16-64"])
def test_elem_layer_norm_offset_rows(dtype, base, step):
    """Rows base + k*step, k in [-4,4], exactly representable: the mean is
    large against the spread, where var = E[x^2] - mean^2 cancels in fp32.
    Same tolerances as the centred rows (the fp64 reference is well
    conditioned). Measured on an MI355X against the fp64 reference, with the
    one-pass fp32 statistics the kernel had before: rstd off by 8.6e-3
    (both fp16 rows) and 1.2e-4 (bf16), y 411 / 411 / 2.3 ulp, dx 442 / 442
    / 1.4 ulp. With the two-pass fp64 statistics: rstd 4e-14, y and dx
    0.500 ulp on all three."""
    x = base + ints((5, 1000), 504) * step
    assert torch.equal(x.to(dtype).float(), x)
    _ln_check(x.to(dtype), dtype, f"ln offset {base}+k*{step}")


# =============================================================== G. dropout ==

DROPOUT_N = [1, 7, 1001, 2 ** 20, 2 ** 21 + 3]
DROPOUT_P = [0.1, 0.5, 0.9]


def test_elem_dropout_largest_n_needs_a_second_pass():
    assert DROPOUT_N[-1] > 4096 * 256 * 2


def _dropout_check(x, p, seed, dtype, dy):
    """x, dy on the device, already rounded. Returns the logical keep mask."""
    xg = x.clone().requires_grad_(True)
    y = DFm().dropout(xg, p, training=True, seed=seed)
    y.backward(dy)
    y2, mask = ext().dropout_fwd(x, p, seed)
    assert torch.equal(y2.view_as(y), y.detach())      # same seed, same result
    keep = mask.view(x.contiguous().shape).bool().cpu()
    assert set(mask.unique().tolist()) <= {0, 1}
    yc, dxc = y.detach().cpu(), xg.grad.cpu()
    assert yc.shape == x.shape and yc.dtype == dtype
    assert (yc[~keep] == 0).all() and (dxc[~keep] == 0).all()
    yr = x.double().cpu() / (1 - p)
    dxr = dy.double().cpu() / (1 - p)
    if p == 0.5:
        assert torch.equal(yc[keep], yr[keep].to(dtype))
        assert torch.equal(dxc[keep], dxr[keep].to(dtype))
    else:
        check_ulp(yc[keep], yr[keep], dtype, 1, "dropout kept y")
        check_ulp(dxc[keep], dxr[keep], dtype, 1, "dropout kept dx")
    return keep


@both_dtypes
@pytest.mark.parametrize("p", DROPOUT_P)
@pytest.mark.parametrize("n", DROPOUT_N)
def test_elem_dropout_values(n, p, dtype):
    """Kept values within 1 ulp of x/(1-p) (bit-equal at p = 0.5), dropped
    ones exactly 0, backward the same mask and scale."""
    x = randn((n,), 600).to(dtype).to(DEV)
    dy = randn((n,), 601).to(dtype).to(DEV)
    _dropout_check(x, p, 1234 + n, dtype, dy)


@both_dtypes
def test_elem_dropout_nhwc_and_sliced_dy(dtype):
    x = nhwc(randn((2, 16, 6, 6), 602).to(dtype))
    dy = randn((2, 16, 6, 12), 603).to(dtype).to(DEV)[..., ::2]
    assert not dy.is_contiguous()
    _dropout_check(x, 0.5, 77, dtype, dy)
    _dropout_check(x, 0.1, 78, dtype, dy)


def _within(rate, want, n, name):
    sigma = math.sqrt(want * (1 - want) / n)
    z = (rate - want) / sigma
    print(f"{name}: rate {rate:.6f} expected {want:.6f} ({z:+.2f} sigma)")
    assert abs(z) <= 5, f"{name}: {z:+.2f} sigma"


@pytest.mark.parametrize("p", DROPOUT_P)
def test_elem_dropout_statistics(p):
    """n = 2^20. One hash yields the uniforms of elements 2i and 2i+1, so
    the even and the odd half and their joint rate are checked on their own;
    sigma = sqrt(q(1-q)/count) for an event of probability q."""
    n = 2 ** 20
    x = torch.ones(n, dtype=torch.bfloat16, device=DEV)
    k1 = ext().dropout_fwd(x, p, 4321)[1].bool().cpu()
    k1b = ext().dropout_fwd(x, p, 4321)[1].bool().cpu()
    k2 = ext().dropout_fwd(x, p, 8765)[1].bool().cpu()
    assert torch.equal(k1, k1b)
    q = 1 - p
    _within(k1.float().mean().item(), q, n, "keep rate")
    _within(k1[0::2].float().mean().item(), q, n // 2, "keep rate, even")
    _within(k1[1::2].float().mean().item(), q, n // 2, "keep rate, odd")
    _within((k1[0::2] & k1[1::2]).float().mean().item(), q * q, n // 2,
            "joint rate of (2i, 2i+1)")
    _within((k1 == k2).float().mean().item(), p * p + q * q, n,
            "agreement of two seeds")


# =================================================================== H. SGD ==

SGD_N = [1, 1000, 2 ** 20 + 5]          # the last is past the 4096-block cap
SGD_HYPER = dict(lr=0.1, mu=0.9, wd=1e-4, rs=0.5)


def assert_close(got, want, rtol, atol, name):
    torch.testing.assert_close(got.double().cpu(), want.double(), rtol=rtol,
                               atol=atol, msg=lambda m: f"{name}: {m}")


def _sgd_ref(g, master, mom, clip):
    h = SGD_HYPER
    gv = g.double() * h["rs"]
    if clip > 0:
        assert (gv.abs() > clip).any() or g.numel() == 1
        gv = gv.clamp(-clip, clip)
    gv = gv + h["wd"] * master.double()
    mom_ref = h["mu"] * mom.double() - h["lr"] * gv
    return master.double() + mom_ref, mom_ref


@both_dtypes
@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("n", SGD_N)
def test_elem_sgd_mom_mp(n, clip, dtype):
    """fp64 update rule on the rounded inputs; the device-hyperparameter
    variant must be bit-equal to the host-argument one.

    Weights are +-(1 + |N(0,1)|) and momenta 0.1 * N(0,1), so that no update
    cancels its weight: master is fp32 state with an absolute error near
    2^-24 of the operands, and one 16-bit ulp at the magnitude of the result
    only means something where the result is not a difference of much larger
    numbers. (With N(0,1) weights a few of the 2^20 results land within 1e-5
    of zero and the fp32 master, correct to rtol 1e-5 / atol 1e-6, is several
    16-bit ulps of that from the fp64 value: 6.7 measured.)"""
    h = SGD_HYPER
    master = randn((n,), 700)
    master = torch.where(master < 0, master - 1, master + 1)
    mom = randn((n,), 701, 0.1)
    g = (randn((n,), 702, 2.0) + (3.0 if n == 1 else 0.0)).to(dtype)
    master_ref, mom_ref = _sgd_ref(g, master, mom, clip)

    w, m, v = master.to(dtype).to(DEV), master.to(DEV), mom.to(DEV)
    ext().sgd_mom_mp(w, g.to(DEV), m, v, h["lr"], h["mu"], h["wd"], h["rs"], clip)
    assert_close(m, master_ref, 1e-5, 1e-6, "sgd master")
    assert_close(v, mom_ref, 1e-5, 1e-6, "sgd mom")
    check_ulp(w, master_ref, dtype, 1, "sgd w")
    assert torch.equal(w, m.to(dtype))          # w is the rounded master

    w2, m2, v2 = master.to(dtype).to(DEV), master.to(DEV), mom.to(DEV)
    hyper = torch.tensor([h["lr"], h["mu"], h["wd"], h["rs"], clip],
                         dtype=torch.float32, device=DEV)
    ext().sgd_mom_mp_dev(w2, g.to(DEV), m2, v2, hyper)
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(v2, v)


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("n", SGD_N)
def test_elem_sgd_mom_f32(n, clip):
    h = SGD_HYPER
    w0 = randn((n,), 703)
    mom = randn((n,), 704)
    g = randn((n,), 705, 2.0) + (3.0 if n == 1 else 0.0)
    w_ref, mom_ref = _sgd_ref(g, w0, mom, clip)
    w, v = w0.to(DEV), mom.to(DEV)
    ext().sgd_mom_f32(w, g.to(DEV), v, h["lr"], h["mu"], h["wd"], h["rs"], clip)
    assert_close(w, w_ref, 1e-5, 1e-6, "sgd f32 w")
    assert_close(v, mom_ref, 1e-5, 1e-6, "sgd f32 mom")
