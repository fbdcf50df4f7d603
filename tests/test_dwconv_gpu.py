"""Depthwise 3x3 HIP kernels (dwconv.hip) vs fp32 CPU references.

Conventions of test_ops_gpu.py: inputs are bf16/fp16-rounded first, the
reference is fp32 F.conv2d(groups=C) / torch.nn.grad.conv2d_* on the CPU on
the same rounded values, tolerances rtol=0.02, atol=0.02*mean|ref|+1e-3.
The small-integer variants assert exact equality: every output is an integer
of magnitude <= 9*3*2 = 54, which bf16/fp16 represent exactly.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

CASES = [
    # (N, C, H, W, stride, pad)
    (2, 8, 5, 5, 1, 1),       # one channel vector; borders dominate
    (1, 136, 1, 1, 1, 1),     # 1x1 image: centre tap only; C not a power of 2
    (2, 24, 7, 9, 2, 1),      # odd, non-square, stride 2
    (2, 16, 8, 8, 2, 1),      # even + stride 2: last row/col reached by one tap
    (2, 32, 8, 8, 2, 0),      # pad 0 stride 2: last row/col reached by no output
    (3, 40, 13, 6, 1, 1),     # W not a multiple of the output strip
    (2, 32, 17, 17, 1, 0),    # pad 0, stride 1
    (4, 64, 28, 28, 1, 1),    # several blocks contribute wgrad partials
    (4, 64, 28, 28, 2, 1),    # same, stride 2
]
FP16_CASES = [CASES[2], CASES[7]]
IDS = [str(c) for c in CASES]


def ext():
    from dtmx.ops.hip import require_ext
    return require_ext()


def assert_close(got, want, rtol=0.02, atol=None, name=""):
    got = got.float().cpu()
    want = want.float().cpu()
    if atol is None:
        atol = 0.02 * want.abs().mean().item() + 1e-3
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol,
                               msg=lambda m: f"{name}: {m}")


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def out_hw(H, W, stride, pad):
    return (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1


@functools.lru_cache(maxsize=None)
def problem(case, dtype=torch.bfloat16, integer=False):
    """Rounded CPU inputs and the fp32 CPU references for one case, computed
    once and shared (never modified) by the tests that use the case."""
    N, C, H, W, stride, pad = case
    P, Q = out_hw(H, W, stride, pad)
    g = torch.Generator().manual_seed(1234)
    if integer:
        x = torch.randint(-3, 4, (N, C, H, W), generator=g).to(dtype)
        dy = torch.randint(-3, 4, (N, C, P, Q), generator=g).to(dtype)
        w = torch.randint(-2, 3, (C, 1, 3, 3), generator=g).to(dtype)
    else:
        x = torch.randn(N, C, H, W, generator=g).to(dtype)
        dy = torch.randn(N, C, P, Q, generator=g).to(dtype)
        w = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).to(dtype)
    y = F.conv2d(x.float(), w.float(), None, stride, pad, 1, C)
    dx = torch.nn.grad.conv2d_input((N, C, H, W), w.float(), dy.float(),
                                    stride=stride, padding=pad, groups=C)
    dw = torch.nn.grad.conv2d_weight(x.float(), (C, 1, 3, 3), dy.float(),
                                     stride=stride, padding=pad, groups=C)
    return dict(x=x, dy=dy, w=w, y=y, dx=dx, dw=dw)


def run_fwd(case, pr):
    return ext().dwconv_fwd(nhwc(pr["x"]), pr["w"].to(DEV), case[4], case[5])


def run_dgrad(case, pr):
    return ext().dwconv_dgrad(nhwc(pr["dy"]), pr["w"].to(DEV), case[4], case[5],
                              case[2], case[3])


def run_wgrad(case, pr):
    return ext().dwconv_wgrad(nhwc(pr["x"]), nhwc(pr["dy"]), case[4], case[5])


# ------------------------------------------------------- fp32 reference

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_fwd(case):
    pr = problem(case)
    y = run_fwd(case, pr)
    assert y.dtype == torch.bfloat16 and y.shape == pr["y"].shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert_close(y, pr["y"], name=f"dwconv_fwd{case}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_dgrad(case):
    pr = problem(case)
    dx = run_dgrad(case, pr)
    assert dx.shape == pr["dx"].shape
    assert_close(dx, pr["dx"], name=f"dwconv_dgrad{case}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_wgrad(case):
    pr = problem(case)
    dw = run_wgrad(case, pr)
    assert dw.shape == (case[1], 1, 3, 3) and dw.dtype == torch.bfloat16
    assert_close(dw, pr["dw"], name=f"dwconv_wgrad{case}")


# ------------------------------------------------- small integers, exact

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_fwd_integer_exact(case):
    pr = problem(case, integer=True)
    assert pr["y"].abs().max() <= 54
    y = run_fwd(case, pr)
    assert torch.equal(y.float().cpu(), pr["y"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dwconv_dgrad_integer_exact(case):
    pr = problem(case, integer=True)
    assert pr["dx"].abs().max() <= 54
    dx = run_dgrad(case, pr)
    assert torch.equal(dx.float().cpu(), pr["dx"])


def test_dwconv_dgrad_unreached_edge_is_zero():
    """pad 0, stride 2, even size: no output reaches the last input row and
    column, so dx there is exactly 0 (written, not left as allocated)."""
    case = (2, 32, 8, 8, 2, 0)
    pr = problem(case)
    assert pr["dx"][:, :, -1, :].abs().max() == 0
    dx = run_dgrad(case, pr).float().cpu()
    assert dx[:, :, -1, :].abs().max() == 0
    assert dx[:, :, :, -1].abs().max() == 0


# ------------------------------------------------------------------ fp16

@pytest.mark.parametrize("case", FP16_CASES, ids=[str(c) for c in FP16_CASES])
def test_dwconv_fp16(case):
    pr = problem(case, dtype=torch.float16)
    y = run_fwd(case, pr)
    assert y.dtype == torch.float16
    assert_close(y, pr["y"], name=f"dwconv_fwd_fp16{case}")
    assert_close(run_dgrad(case, pr), pr["dx"], name=f"dwconv_dgrad_fp16{case}")
    dw = run_wgrad(case, pr)
    assert dw.dtype == torch.float16
    assert_close(dw, pr["dw"], name=f"dwconv_wgrad_fp16{case}")


# ----------------------------------------------------------- determinism

def test_dwconv_wgrad_deterministic():
    case = (4, 64, 28, 28, 1, 1)
    pr = problem(case)
    x, dy = nhwc(pr["x"]), nhwc(pr["dy"])
    a = ext().dwconv_wgrad(x, dy, 1, 1)
    b = ext().dwconv_wgrad(x, dy, 1, 1)
    assert torch.equal(a, b)


# -------------------------------------------------------------- autograd

@pytest.mark.parametrize("case", [CASES[3], CASES[7]],
                         ids=[str(CASES[3]), str(CASES[7])])
def test_dwconv_autograd(case):
    from dtmx.ops import functional as DF
    N, C, H, W, stride, pad = case
    pr = problem(case)
    x = nhwc(pr["x"]).requires_grad_(True)
    w = pr["w"].to(DEV).requires_grad_(True)
    y = DF.depthwise_conv2d(x, w, stride, pad)
    assert type(y.grad_fn).__name__ == "_DepthwiseConvNHWCBackward"
    # a non-channels_last upstream gradient: backward must re-lay it out
    y.backward(pr["dy"].to(DEV).contiguous())
    xr = pr["x"].float().requires_grad_(True)
    wr = pr["w"].float().requires_grad_(True)
    F.conv2d(xr, wr, None, stride, pad, 1, C).backward(pr["dy"].float())
    assert w.grad.shape == (C, 1, 3, 3) and w.grad.dtype == torch.bfloat16
    assert_close(y, pr["y"], name="autograd y")
    assert_close(x.grad, xr.grad, name="autograd x.grad")
    assert_close(w.grad, wr.grad, name="autograd w.grad")


def test_dwconv_autograd_needs_input_grad():
    """Only the requested gradients are computed."""
    from dtmx.ops import functional as DF
    case = CASES[0]
    pr = problem(case)
    x = nhwc(pr["x"])
    w = pr["w"].to(DEV).requires_grad_(True)
    DF.depthwise_conv2d(x, w, case[4], case[5]).backward(nhwc(pr["dy"]))
    assert x.grad is None
    assert_close(w.grad, pr["dw"], name="w.grad only")


# --------------------------------------------------------------- routing

def _record_calls(monkeypatch):
    from dtmx.ops import functional as DF
    calls = []
    real = DF.depthwise_conv2d

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(DF, "depthwise_conv2d", wrapper)
    return calls


def test_grouped_layer_routes_depthwise(monkeypatch):
    from dtmx.ops.layers import GroupedConv2dNHWC
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=32).to(DEV).to(torch.bfloat16)
    x = nhwc(torch.randn(2, 32, 9, 9).bfloat16()).requires_grad_(True)
    y = layer(x)
    assert len(calls) == 1
    assert type(y.grad_fn).__name__ == "_DepthwiseConvNHWCBackward"
    ref = F.conv2d(x.detach().float().cpu(), layer.weight.detach().float().cpu(),
                   None, 1, 1, 1, 32)
    assert_close(y, ref, name="layer fwd")


def test_grouped_layer_non_depthwise_keeps_library_path(monkeypatch):
    from dtmx.ops.layers import GroupedConv2dNHWC
    calls = _record_calls(monkeypatch)
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=4).to(DEV).to(torch.bfloat16)
    x = nhwc(torch.randn(2, 32, 9, 9).bfloat16()).requires_grad_(True)
    y = layer(x)
    assert calls == []
    assert type(y.grad_fn).__name__ != "_DepthwiseConvNHWCBackward"
    ref = F.conv2d(x.detach().float().cpu(), layer.weight.detach().float().cpu(),
                   None, 1, 1, 1, 4)
    assert_close(y, ref, name="grouped layer fwd")


# -------------------------------------------------------------- envelope

def test_envelope_fallback_c12():
    from dtmx.ops import functional as DF
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 12, 7, 7, generator=g).bfloat16()
    w = (torch.randn(12, 1, 3, 3, generator=g) * 0.3).bfloat16()
    y = DF.depthwise_conv2d(nhwc(x), w.to(DEV), 1, 1)
    assert_close(y, F.conv2d(x.float(), w.float(), None, 1, 1, 1, 12), name="C=12")
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        ext().dwconv_fwd(nhwc(x), w.to(DEV), 1, 1)


def test_envelope_fallback_5x5():
    from dtmx.ops import functional as DF
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 16, 9, 9, generator=g).bfloat16()
    w = (torch.randn(16, 1, 5, 5, generator=g) * 0.2).bfloat16()
    y = DF.depthwise_conv2d(nhwc(x), w.to(DEV), 1, 2)
    assert_close(y, F.conv2d(x.float(), w.float(), None, 1, 2, 1, 16), name="5x5")
    with pytest.raises(RuntimeError, match="3x3"):
        ext().dwconv_fwd(nhwc(x), w.to(DEV), 1, 1)


def test_envelope_rejects_bad_stride_pad_layout_dtype():
    pr = problem(CASES[0])
    x, w = nhwc(pr["x"]), pr["w"].to(DEV)
    with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
        ext().dwconv_fwd(x, w, 3, 1)
    with pytest.raises(RuntimeError, match="padding must be 0 or 1"):
        ext().dwconv_fwd(x, w, 1, 2)
    with pytest.raises(RuntimeError, match="channels_last"):
        ext().dwconv_fwd(pr["x"].to(DEV).contiguous(), w, 1, 1)
    with pytest.raises(RuntimeError, match="bfloat16/float16"):
        ext().dwconv_fwd(x.float(), w.float(), 1, 1)


def test_weight_channels_last_view_accepted():
    """contiguous and channels_last views of (C,1,3,3) share memory order."""
    case = CASES[0]
    pr = problem(case)
    w = pr["w"].to(DEV).contiguous(memory_format=torch.channels_last)
    y = ext().dwconv_fwd(nhwc(pr["x"]), w, case[4], case[5])
    assert_close(y, pr["y"], name="w channels_last view")
