"""Grouped 3x3 HIP kernels (gconv.hip) vs fp32 CPU references.

Conventions of test_dwconv_gpu.py: inputs are bf16/fp16-rounded first, the
reference is fp32 F.conv2d(groups=G) / torch.nn.grad.conv2d_* on the CPU on
the same rounded values, tolerances rtol=0.02, atol=0.02*mean|ref|+1e-3.
The small-integer variants assert exact equality: x, dy in {-1,0,1}, w in
{-2..2}; every reference value is asserted to be an integer of magnitude
<= 256, which bf16 holds exactly (fp32 accumulation of integers is exact).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

CASES = [
    # (N, C, groups, H, W, stride, pad)
    (2, 32, 8, 5, 5, 1, 1),        # Cg 4: one channel tile; borders dominate
    (1, 96, 12, 1, 1, 1, 1),       # Cg 8: 1x1 image, centre tap; 3 tiles; 1 px
    (2, 64, 4, 7, 9, 2, 1),        # Cg 16: odd, non-square, stride 2
    (2, 64, 2, 8, 8, 2, 1),        # Cg 32: even + stride 2: last row/col, one tap
    (2, 32, 8, 8, 8, 2, 0),        # Cg 4: pad 0 stride 2: last row/col unreached
    (3, 64, 8, 13, 6, 1, 1),       # Cg 8: W and N*P*Q (234) not tile multiples
    (2, 128, 4, 17, 17, 1, 0),     # Cg 32: pad 0, stride 1; 450 output pixels
    (4, 128, 32, 28, 28, 1, 1),    # Cg 4: stage-1 grouping; several wgrad blocks
    (4, 128, 8, 28, 28, 2, 1),     # Cg 16: same, stride 2
    (2, 160, 5, 9, 9, 1, 1),       # Cg 32: 5 channel tiles
]
CL_WEIGHT_CASES = [CASES[2], CASES[7], CASES[9]]
FP16_CASES = [CASES[2], CASES[7]]
IDS = [str(c) for c in CASES]


def ids(cases):
    return [str(c) for c in cases]


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
    N, C, G, H, W, stride, pad = case
    Cg = C // G
    P, Q = out_hw(H, W, stride, pad)
    g = torch.Generator().manual_seed(1234)
    if integer:
        x = torch.randint(-1, 2, (N, C, H, W), generator=g).to(dtype)
        dy = torch.randint(-1, 2, (N, C, P, Q), generator=g).to(dtype)
        w = torch.randint(-2, 3, (C, Cg, 3, 3), generator=g).to(dtype)
    else:
        x = torch.randn(N, C, H, W, generator=g).to(dtype)
        dy = torch.randn(N, C, P, Q, generator=g).to(dtype)
        w = (torch.randn(C, Cg, 3, 3, generator=g) * 0.2).to(dtype)
    y = F.conv2d(x.float(), w.float(), None, stride, pad, 1, G)
    dx = torch.nn.grad.conv2d_input((N, C, H, W), w.float(), dy.float(),
                                    stride=stride, padding=pad, groups=G)
    dw = torch.nn.grad.conv2d_weight(x.float(), (C, Cg, 3, 3), dy.float(),
                                     stride=stride, padding=pad, groups=G)
    return dict(x=x, dy=dy, w=w, y=y, dx=dx, dw=dw)


def run_fwd(case, pr, w=None):
    w = pr["w"].to(DEV) if w is None else w
    return ext().gconv_fwd(nhwc(pr["x"]), w, case[5], case[6], case[2])


def run_dgrad(case, pr, w=None):
    w = pr["w"].to(DEV) if w is None else w
    return ext().gconv_dgrad(nhwc(pr["dy"]), w, case[5], case[6], case[2],
                             case[3], case[4])


def run_wgrad(case, pr, w_cl=False):
    return ext().gconv_wgrad(nhwc(pr["x"]), nhwc(pr["dy"]), case[5], case[6],
                             case[2], w_cl)


# ------------------------------------------------------- fp32 reference

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_fwd(case):
    pr = problem(case)
    y = run_fwd(case, pr)
    assert y.dtype == torch.bfloat16 and y.shape == pr["y"].shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert_close(y, pr["y"], name=f"gconv_fwd{case}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_dgrad(case):
    pr = problem(case)
    dx = run_dgrad(case, pr)
    assert dx.dtype == torch.bfloat16 and dx.shape == pr["dx"].shape
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert_close(dx, pr["dx"], name=f"gconv_dgrad{case}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_wgrad(case):
    pr = problem(case)
    dw = run_wgrad(case, pr)
    assert dw.shape == pr["dw"].shape and dw.dtype == torch.bfloat16
    assert dw.is_contiguous()
    assert_close(dw, pr["dw"], name=f"gconv_wgrad{case}")


@pytest.mark.parametrize("case", CL_WEIGHT_CASES, ids=ids(CL_WEIGHT_CASES))
def test_gconv_weight_channels_last(case):
    """The weight as Module.bind leaves it: memory [C][3][3][Cg]. fwd and
    dgrad read it through its strides; wgrad returns dw in that layout."""
    pr = problem(case)
    w = pr["w"].to(DEV).contiguous(memory_format=torch.channels_last)
    assert not w.is_contiguous()
    assert_close(run_fwd(case, pr, w), pr["y"], name=f"fwd w_cl{case}")
    assert_close(run_dgrad(case, pr, w), pr["dx"], name=f"dgrad w_cl{case}")
    dw = run_wgrad(case, pr, True)
    assert dw.shape == pr["dw"].shape and dw.stride() == w.stride()
    assert_close(dw, pr["dw"], name=f"wgrad w_cl{case}")


# ------------------------------------------------- small integers, exact

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_fwd_integer_exact(case):
    pr = problem(case, integer=True)
    assert pr["y"].abs().max() <= 256
    y = run_fwd(case, pr)
    assert torch.equal(y.float().cpu(), pr["y"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_dgrad_integer_exact(case):
    pr = problem(case, integer=True)
    assert pr["dx"].abs().max() <= 256
    dx = run_dgrad(case, pr)
    assert torch.equal(dx.float().cpu(), pr["dx"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gconv_wgrad_integer_exact(case):
    pr = problem(case, integer=True)
    assert pr["dw"].abs().max() <= 256
    dw = run_wgrad(case, pr)
    assert torch.equal(dw.float().cpu(), pr["dw"])
    if case in CL_WEIGHT_CASES:
        dw = run_wgrad(case, pr, True)
        assert torch.equal(dw.float().cpu(), pr["dw"])


# ------------------------------------------------------- group isolation

def test_gconv_group_isolation():
    """x (dy) non-zero in one group only: every other group's output (input
    gradient) channels are exactly zero — nothing leaks through the zero
    blocks of the expanded weight."""
    case = CASES[2]
    N, C, G, H, W, stride, pad = case
    Cg = C // G
    pr = problem(case)
    keep = slice(2 * Cg, 3 * Cg)
    mask = torch.zeros(1, C, 1, 1, dtype=torch.bool)
    mask[:, keep] = True
    w = pr["w"].to(DEV)
    x1 = torch.where(mask, pr["x"], torch.zeros_like(pr["x"]))
    y = ext().gconv_fwd(nhwc(x1), w, stride, pad, G).float().cpu()
    assert y[:, keep].abs().max() > 0
    assert y[~mask.expand_as(y)].abs().max() == 0
    dy1 = torch.where(mask, pr["dy"], torch.zeros_like(pr["dy"]))
    dx = ext().gconv_dgrad(nhwc(dy1), w, stride, pad, G, H, W).float().cpu()
    assert dx[:, keep].abs().max() > 0
    assert dx[~mask.expand_as(dx)].abs().max() == 0


def test_gconv_dgrad_unreached_edge_is_zero():
    """pad 0, stride 2, even size: no output reaches the last input row and
    column, so dx there is exactly 0 (written, not left as allocated)."""
    case = CASES[4]
    pr = problem(case)
    assert pr["dx"][:, :, -1, :].abs().max() == 0
    dx = run_dgrad(case, pr).float().cpu()
    assert dx[:, :, -1, :].abs().max() == 0
    assert dx[:, :, :, -1].abs().max() == 0


# ------------------------------------------------------------------ fp16

@pytest.mark.parametrize("case", FP16_CASES, ids=ids(FP16_CASES))
def test_gconv_fp16(case):
    pr = problem(case, dtype=torch.float16)
    y = run_fwd(case, pr)
    assert y.dtype == torch.float16
    assert_close(y, pr["y"], name=f"gconv_fwd_fp16{case}")
    dx = run_dgrad(case, pr)
    assert dx.dtype == torch.float16
    assert_close(dx, pr["dx"], name=f"gconv_dgrad_fp16{case}")
    dw = run_wgrad(case, pr)
    assert dw.dtype == torch.float16
    assert_close(dw, pr["dw"], name=f"gconv_wgrad_fp16{case}")


# ----------------------------------------------------------- determinism

def test_gconv_wgrad_deterministic():
    case = CASES[7]
    pr = problem(case)
    x, dy = nhwc(pr["x"]), nhwc(pr["dy"])
    a = ext().gconv_wgrad(x, dy, case[5], case[6], case[2], False)
    b = ext().gconv_wgrad(x, dy, case[5], case[6], case[2], False)
    assert torch.equal(a, b)


# -------------------------------------------------------------- autograd

@pytest.mark.parametrize("case", [CASES[3], CASES[7]],
                         ids=[str(CASES[3]), str(CASES[7])])
def test_gconv_autograd(case):
    from dtmx.ops import functional as DF
    N, C, G, H, W, stride, pad = case
    pr = problem(case)
    x = nhwc(pr["x"]).requires_grad_(True)
    w = pr["w"].to(DEV).requires_grad_(True)
    y = DF.grouped_conv2d(x, w, stride, pad, G)
    assert type(y.grad_fn).__name__ == "_GroupedConvNHWCBackward"
    # a non-channels_last upstream gradient: backward must re-lay it out
    y.backward(pr["dy"].to(DEV).contiguous())
    xr = pr["x"].float().requires_grad_(True)
    wr = pr["w"].float().requires_grad_(True)
    F.conv2d(xr, wr, None, stride, pad, 1, G).backward(pr["dy"].float())
    assert w.grad.shape == (C, C // G, 3, 3) and w.grad.dtype == torch.bfloat16
    assert_close(y, pr["y"], name="autograd y")
    assert_close(x.grad, xr.grad, name="autograd x.grad")
    assert_close(w.grad, wr.grad, name="autograd w.grad")


def test_gconv_autograd_needs_input_grad():
    """Only the requested gradients are computed."""
    from dtmx.ops import functional as DF
    case = CASES[0]
    pr = problem(case)
    x = nhwc(pr["x"])
    w = pr["w"].to(DEV).requires_grad_(True)
    DF.grouped_conv2d(x, w, case[5], case[6], case[2]).backward(nhwc(pr["dy"]))
    assert x.grad is None
    assert_close(w.grad, pr["dw"], name="w.grad only")


# --------------------------------------------------------------- routing

def _layer_and_ref(bias, channels_last):
    from dtmx.ops.layers import GroupedConv2dNHWC
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(64, 64, 3, 1, 1, groups=16, bias=bias)
    if bias:
        with torch.no_grad():
            layer.bias.copy_(torch.randn(64))
    layer = layer.to(DEV).to(torch.bfloat16)
    if channels_last:
        layer = layer.to(memory_format=torch.channels_last)
    x = nhwc(torch.randn(2, 64, 9, 9).bfloat16()).requires_grad_(True)
    ref = F.conv2d(x.detach().float().cpu(), layer.weight.detach().float().cpu(),
                   layer.bias.detach().float().cpu() if bias else None,
                   1, 1, 1, 16)
    return layer, x, ref


@pytest.mark.parametrize("bias", [False, True])
def test_grouped_layer_routes_native(bias):
    layer, x, ref = _layer_and_ref(bias, False)
    assert layer.weight.is_contiguous()
    y = layer(x)
    fn = y.grad_fn if not bias else y.grad_fn.next_functions[0][0]
    assert type(fn).__name__ == "_GroupedConvNHWCBackward"
    assert_close(y, ref, name="layer fwd")


def test_grouped_layer_channels_last_weight_routes_native():
    layer, x, ref = _layer_and_ref(False, True)
    assert not layer.weight.is_contiguous()
    assert layer.weight.is_contiguous(memory_format=torch.channels_last)
    y = layer(x)
    assert type(y.grad_fn).__name__ == "_GroupedConvNHWCBackward"
    assert_close(y, ref, name="layer fwd, channels_last weight")
    y.float().sum().backward()
    assert layer.weight.grad.stride() == layer.weight.stride()
    dw = torch.nn.grad.conv2d_weight(x.detach().float().cpu(), (64, 4, 3, 3),
                                     torch.ones_like(ref), stride=1, padding=1,
                                     groups=16)
    assert_close(layer.weight.grad, dw, name="layer w.grad, channels_last weight")


def test_grouped_layer_depthwise_still_depthwise():
    from dtmx.ops.layers import GroupedConv2dNHWC
    torch.manual_seed(0)
    layer = GroupedConv2dNHWC(32, 32, 3, 1, 1, groups=32).to(DEV).to(torch.bfloat16)
    x = nhwc(torch.randn(2, 32, 9, 9).bfloat16()).requires_grad_(True)
    assert type(layer(x).grad_fn).__name__ == "_DepthwiseConvNHWCBackward"


# -------------------------------------------------------------- envelope

OUTSIDE = [
    # (C_in, C_out, groups, k, pad, message of the raw entry point)
    (96, 96, 8, 3, 1, "channels per group"),             # Cg = 12
    (64, 64, 8, 5, 2, "3x3"),                            # 5x5
    (64, 128, 4, 3, 1, "in_channels == out_channels"),   # C_in != C_out
    (48, 48, 6, 3, 1, "C % 32 == 0"),                    # Cg = 8, C % 32 != 0
]


@pytest.mark.parametrize("cin,cout,G,k,pad,msg", OUTSIDE,
                         ids=[o[5] for o in OUTSIDE])
def test_envelope_fallback(cin, cout, G, k, pad, msg):
    from dtmx.ops import functional as DF
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, cin, 7, 7, generator=g).bfloat16()
    w = (torch.randn(cout, cin // G, k, k, generator=g) * 0.2).bfloat16()
    y = DF.grouped_conv2d(nhwc(x).requires_grad_(True), w.to(DEV), 1, pad, G)
    assert type(y.grad_fn).__name__ != "_GroupedConvNHWCBackward"
    assert_close(y, F.conv2d(x.float(), w.float(), None, 1, pad, 1, G), name=msg)
    with pytest.raises(RuntimeError, match=msg):
        ext().gconv_fwd(nhwc(x), w.to(DEV), 1, 1, G)


def test_envelope_rejects_bad_stride_pad_layout_dtype():
    case = CASES[0]
    pr = problem(case)
    x, w, G = nhwc(pr["x"]), pr["w"].to(DEV), case[2]
    with pytest.raises(RuntimeError, match="stride must be 1 or 2"):
        ext().gconv_fwd(x, w, 3, 1, G)
    with pytest.raises(RuntimeError, match="padding must be 0 or 1"):
        ext().gconv_fwd(x, w, 1, 2, G)
    with pytest.raises(RuntimeError, match="channels_last"):
        ext().gconv_fwd(pr["x"].to(DEV).contiguous(), w, 1, 1, G)
    with pytest.raises(RuntimeError, match="bfloat16/float16"):
        ext().gconv_fwd(x.float(), w.float(), 1, 1, G)


# --------------------------------------------------------- graph capture

def test_gconv_graph_capture():
    """fwd + dgrad + wgrad (and their pack / finalize kernels) launch on the
    capture stream without a host sync; replays equal the eager results."""
    case = CASES[0]
    N, C, G, H, W, stride, pad = case
    pr = problem(case)
    x, dy, w = nhwc(pr["x"]), nhwc(pr["dy"]), pr["w"].to(DEV)
    e = ext()
    want = (e.gconv_fwd(x, w, stride, pad, G),
            e.gconv_dgrad(dy, w, stride, pad, G, H, W),
            e.gconv_wgrad(x, dy, stride, pad, G, False))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = e.gconv_fwd(x, w, stride, pad, G)
        dx = e.gconv_dgrad(dy, w, stride, pad, G, H, W)
        dw = e.gconv_wgrad(x, dy, stride, pad, G, False)
    for _ in range(2):
        for t in (y, dx, dw):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip((y, dx, dw), want):
            assert torch.equal(got, ref)
