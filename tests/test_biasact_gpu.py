"""Fused bias + ReLU: ext.bias_act_bwd, ext.conv_fwd_act / linear_fwd_act on
each GEMM route, and DF.conv2d_bias_act / DF.linear(relu=True) through
autograd, against fp64.

Integer cases are bit-exact: every product and partial sum is an exactly
represented integer, so the only roundings are the two 16-bit ones of the
epilogue, round16(relu(round16(acc) + bias)), which the reference repeats.
Random cases: the any-order fp32 bound n * 2^-24 * sum|terms| (plus half an
ulp for each 16-bit rounding of the forward), no further slack.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                                 ids=["bf16", "fp16"])


def ext():
    from dtmx.ops.hip import require_ext
    return require_ext()


def ints(g, shape, lo, hi, dtype):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype).to(DEV)


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def act64(gemm64, bias, relu, dtype):
    """round16(relu(round16(gemm64) + bias)) as an fp64 tensor; bias broadcasts
    over dim 1"""
    shape = (1, -1) + (1,) * (gemm64.dim() - 2)
    v = gemm64.to(dtype).double() + bias.double().reshape(shape)
    return (v.clamp_min(0) if relu else v).to(dtype).double()


# ------------------------------------------------------------- bias_act_bwd

BWD_SHAPES = [(1, 8), (7, 24), (300, 40), (1030, 208), (5, 4096), (70001, 8),
              (2, 48, 5, 7)]


def bwd_ref(dy, y, relu):
    g = torch.where(y.float() > 0, dy, torch.zeros_like(dy)) if relu else dy
    rows = g.permute(0, 2, 3, 1) if g.dim() == 4 else g
    return g, rows.reshape(-1, g.shape[1]).double()


@dtypes
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "sum"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=str)
def test_bias_act_bwd_integer_exact(shape, relu, dtype):
    gen = torch.Generator().manual_seed(3)
    dy, y = ints(gen, shape, -4, 4, dtype), ints(gen, shape, -2, 2, dtype)
    if len(shape) == 4:
        dy, y = nhwc(dy), nhwc(y)
    g, db = ext().bias_act_bwd(dy, y, relu)
    g2, db2 = ext().bias_act_bwd(dy, y, relu)
    gref, rows = bwd_ref(dy, y, relu)
    assert db.dtype == torch.float32 and tuple(db.shape) == (shape[1],)
    assert g.stride() == dy.stride() and torch.equal(g, gref)
    assert (g.data_ptr() == dy.data_ptr()) == (not relu)
    assert torch.equal(db.double(), rows.sum(0))
    assert torch.equal(g2, g) and torch.equal(db2, db)
    if relu:
        assert torch.equal(g, ext().relu_bwd(dy, y))


@dtypes
def test_bias_act_bwd_random_within_bound(dtype):
    gen = torch.Generator().manual_seed(5)
    dy = torch.randn(1030, 208, generator=gen).to(dtype).to(DEV)
    y = torch.randn(1030, 208, generator=gen).to(dtype).to(DEV)
    g, db = ext().bias_act_bwd(dy, y, True)
    gref, rows = bwd_ref(dy, y, True)
    assert torch.equal(g, gref)
    bound = rows.shape[0] * 2.0 ** -24 * rows.abs().sum(0)
    err = (db.double() - rows.sum(0)).abs()
    print(f"bias_act_bwd {dtype}: max err / bound = {(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ forward

# name -> ((N, C, H, W), Ko, (R, S), stride, (ph, pw), split-K?, gemm kernel)
FWD_ROUTES = {
    "tn2": ((1, 8, 6, 6), 16, (3, 3), 1, (1, 1), False, 2),
    "tn4": ((1, 8, 6, 7), 72, (3, 3), 2, (1, 1), False, 4),
    "256f": ((2, 32, 102, 203), 192, (2, 2), 1, (0, 0), False, 256),
    "dense1x1": ((2, 16, 5, 7), 72, (1, 1), 1, (0, 0), False, 4),
    "splitk": ((2, 64, 5, 5), 24, (3, 3), 1, (1, 1), True, None),
    "im2col_c3": ((2, 3, 9, 11), 16, (3, 3), 1, (1, 1), False, 2),
    "per_axis": ((1, 8, 6, 7), 16, (3, 5), 1, (0, 2), False, 2),
}


def conv_case(name, gen, dtype, integer):
    xs, Ko, (R, S), stride, pad, small, kernel = FWD_ROUTES[name]
    ws = (Ko, xs[1], R, S)
    if integer:
        x, w = ints(gen, xs, -2, 2, dtype), ints(gen, ws, -2, 2, dtype)
        # alternating signs and distinct magnitudes: about half the outputs
        # end below zero, and a channel shift moves every column differently
        bias = (torch.arange(Ko) % 7 + 1.0) * (1 - 2 * (torch.arange(Ko) % 2))
    else:
        x = torch.randn(xs, generator=gen).to(dtype).to(DEV)
        w = (torch.randn(ws, generator=gen) * 0.2).to(dtype).to(DEV)
        bias = torch.randn(Ko, generator=gen)
    bias = bias.to(dtype).to(DEV)
    P = (xs[2] + 2 * pad[0] - R) // stride + 1
    Q = (xs[3] + 2 * pad[1] - S) // stride + 1
    M, K = xs[0] * P * Q, R * S * xs[1]
    K = K if xs[1] % 8 == 0 else -(-K // 64) * 64  # im2col pads K to 64
    small_got = xs[1] % 8 == 0 and ext().smallgrid_plan(M, Ko, K)[0]
    assert bool(small_got) == small
    if not small:
        assert ext().gemm_plan(M, Ko, K)[0] == kernel
    if name == "256f":
        assert 1 <= M % 256 <= 128
    return nhwc(x), nhwc(w), bias, stride, pad, R * S * xs[1]


@dtypes
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "bias"])
@pytest.mark.parametrize("name", list(FWD_ROUTES))
def test_conv_fwd_act_integer_exact(name, relu, dtype):
    x, w, bias, stride, pad, _ = conv_case(name, torch.Generator().manual_seed(1),
                                           dtype, True)
    y = ext().conv_fwd_act(x, w, bias, relu, stride, *pad)
    conv64 = F.conv2d(x.double().cpu(), w.double().cpu(), None, stride, pad)
    ref = act64(conv64, bias.cpu(), relu, dtype)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.double().cpu(), ref)
    if relu:
        frac = (ref == 0).double().mean().item()
        assert 0.2 < frac < 0.8, frac  # ReLU is visible


@dtypes
def test_linear_fwd_act_integer_exact(dtype):
    gen = torch.Generator().manual_seed(2)
    M, N, K = 129, 132, 200  # tails in all three
    x, w = ints(gen, (M, K), -2, 2, dtype), ints(gen, (N, K), -2, 2, dtype)
    bias = ((torch.arange(N) % 7 + 1.0) * (1 - 2 * (torch.arange(N) % 2))).to(dtype).to(DEV)
    assert ext().gemm_plan(M, N, K)[0] == 4
    for relu in (True, False):
        y = ext().linear_fwd_act(x, w, bias, relu)
        assert torch.equal(y.double(), act64(x.double() @ w.double().T, bias, relu, dtype))


def ulp(v, dtype):
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(v.clamp_min(2.0 ** emin))[1] - 1
    return torch.ldexp(torch.ones_like(v), e - p)


@dtypes
@pytest.mark.parametrize("name", ["splitk", "linear"])
def test_fwd_act_random_within_bound(name, dtype):
    """|y - relu(gemm64 + bias)| <= a + half an ulp at |gemm64| + a + half an
    ulp at |ref| + all before it, a = K * 2^-24 * sum|x*w| (relu contracts)."""
    gen = torch.Generator().manual_seed(9)
    if name == "linear":
        K = 200
        x = torch.randn(129, K, generator=gen).to(dtype).to(DEV)
        w = (torch.randn(136, K, generator=gen) * 0.2).to(dtype).to(DEV)
        bias = torch.randn(136, generator=gen).to(dtype).to(DEV)
        y = ext().linear_fwd_act(x, w, bias, True).double()
        gemm, S = x.double() @ w.double().T, x.double().abs() @ w.double().abs().T
    else:
        x, w, bias, stride, pad, K = conv_case(name, gen, dtype, False)
        y = ext().conv_fwd_act(x, w, bias, True, stride, *pad).double().cpu()
        xd, wd, bias = x.double().cpu(), w.double().cpu(), bias.cpu()
        gemm = F.conv2d(xd, wd, None, stride, pad)
        S = F.conv2d(xd.abs(), wd.abs(), None, stride, pad)
    pre = gemm + bias.double().reshape((1, -1) + (1,) * (gemm.dim() - 2))
    a = K * 2.0 ** -24 * S
    b = a + 0.5 * ulp(gemm.abs() + a, dtype)
    bound = b + 0.5 * ulp(pre.abs() + b, dtype)
    err = (y - pre.clamp_min(0)).abs()
    print(f"fwd_act {name} {dtype}: max err / bound = {(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


# ----------------------------------------------------------------- autograd

def ste16(v, dtype):
    """round to dtype, gradient passed straight through"""
    return v + (v.detach().to(dtype).double() - v.detach())


@dtypes
@pytest.mark.parametrize("op", ["conv", "conv256f", "linear"])
def test_autograd_integer_exact(op, dtype):
    """conv256f: a shape of the 256f route, whose forward DF keeps unfused"""
    from dtmx.ops import functional as DF
    gen = torch.Generator().manual_seed(4)
    if op == "linear":
        x, w = ints(gen, (9, 40), -2, 2, dtype), ints(gen, (24, 40), -2, 2, dtype)
        dy = ints(gen, (9, 24), -2, 2, dtype)
        run = lambda x, w, b: DF.linear(x, w, b, relu=True)
        run64 = lambda x, w: x @ w.T
    else:
        xs, ws, pad = (((2, 16, 9, 11), (24, 16, 3, 3), 1) if op == "conv" else
                       (FWD_ROUTES["256f"][0], (192, 32, 2, 2), 0))
        x, w = nhwc(ints(gen, xs, -2, 2, dtype)), nhwc(ints(gen, ws, -2, 2, dtype))
        run = lambda x, w, b: DF.conv2d_bias_act(x, w, b, True, 1, pad)
        run64 = lambda x, w: F.conv2d(x, w, None, 1, pad)
        dy = nhwc(ints(gen, run64(x.double().cpu(), w.double().cpu()).shape, -2, 2, dtype))
        assert DF._biasact_fwd_routed(ext(), x, w, 1, pad, pad) == (op == "conv")
    Ko = w.shape[0]
    b = ((torch.arange(Ko) % 7 + 1.0) * (1 - 2 * (torch.arange(Ko) % 2))).to(dtype).to(DEV)
    leaves = [t.requires_grad_() for t in (x, w, b)]
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = run(*leaves)
        grads = torch.autograd.grad(y, leaves, dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    x64, w64, b64 = (t.detach().double().cpu().requires_grad_() for t in leaves)
    shape = (1, -1) + (1,) * (y.dim() - 2)
    y64 = ste16(F.relu(ste16(run64(x64, w64), dtype) + b64.reshape(shape)), dtype)
    grads64 = torch.autograd.grad(y64, [x64, w64, b64], dy.double().cpu())
    assert torch.equal(y.detach().double().cpu(), y64.detach())
    for got, want, leaf in zip(grads, grads64, leaves):
        assert got.dtype == dtype and got.shape == leaf.shape
        assert torch.equal(got.double().cpu(), want.to(dtype).double())
