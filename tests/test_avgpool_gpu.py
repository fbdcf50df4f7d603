"""Windowed average pool HIP kernels (avgpool.hip) vs fp32 CPU references.

Conventions of test_dwconv_gpu.py: inputs are bf16/fp16-rounded first, the
reference is fp32 F.avg_pool2d and its autograd on the CPU on the same rounded
values, tolerances rtol=0.02, atol=0.02*mean|ref|+1e-3.

The small-integer variants assert exact equality against the fp64 reference.
Inputs are L * {-1, 0, 1} with L the least common multiple of the divisors
that occur in the case, so every window mean and every dy/div term is an
integer: |y| <= L and |dx| <= L * (windows per element) / min divisor, at
most 225 over the listed cases (the K = 5 case), and bf16 (8 significant
bits) and fp16 hold every integer up to 256 exactly. A kernel is exact here
if it divides each term, or if it scales by exact small integers and applies
one reciprocal to an exact sum (an fp32 rounding away from a nonzero integer
still rounds to it); per-term reciprocals of 3 or 9 would leave a residue
where terms cancel to 0. The K = 8 whole-image case is
left out: there L = 3136 and |y| reaches the hundreds beyond 256, which bf16
cannot represent exactly.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

CASES = [
    # (N, C, H, W, K, stride, pad)
    (2, 8, 5, 5, 3, 1, 1),       # one channel vector; borders dominate
    (1, 136, 1, 1, 3, 1, 1),     # 1x1 image: divisor 1 vs 9; C not a power of 2
    (3, 40, 13, 6, 3, 1, 1),     # W not a multiple of the output strip
    (2, 24, 11, 3, 3, 1, 1),     # W smaller than a strip
    (4, 64, 28, 28, 3, 1, 1),    # several blocks
    (2, 16, 8, 8, 3, 2, 1),      # generic path
    (2, 32, 8, 8, 3, 2, 0),      # last row/col reached by no window
    (1, 8, 7, 7, 2, 2, 0),       # generic path, even window
    (1, 8, 12, 12, 5, 3, 2),     # generic path, pad 2
    (2, 16, 8, 8, 8, 1, 0),      # whole-image window
]
# 3x3 s1 p1 with more work items than the strip kernels' grid cap of
# 2048 blocks x 256 threads = 524288: 65 rows x 64 strips x 128 channel
# vectors = 532480, so the grid-stride loop runs a second pass for some.
BIG = (1, 1024, 65, 256, 3, 1, 1)
GRID_CAP_ITEMS = 2048 * 256
ALL_CASES = CASES + [BIG]
EXACT_CASES = [c for c in CASES if c[4] != 8]
MODES = [True, False]
HOT, GENERIC = CASES[2], CASES[8]


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


def out_hw(H, W, K, stride, pad):
    return (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1


def divisors(case, cip):
    """(P, Q) map of each window's divisor. Without ceil mode a window never
    leaves the padded extent, so the include-pad divisor is K*K everywhere."""
    N, C, H, W, K, stride, pad = case
    P, Q = out_hw(H, W, K, stride, pad)
    if cip:
        return torch.full((P, Q), K * K, dtype=torch.int64)
    ones = torch.ones(1, 1, H, W, dtype=torch.float64)
    return F.avg_pool2d(ones, K, stride, pad, divisor_override=1)[0, 0].round().long()


@functools.lru_cache(maxsize=None)
def problem(case, cip, dtype=torch.bfloat16, integer=False):
    """Rounded CPU inputs and the CPU references for one case and count mode,
    computed once and shared (never modified) by the tests that use them.
    References are fp32, fp64 for the integer variant."""
    N, C, H, W, K, stride, pad = case
    P, Q = out_hw(H, W, K, stride, pad)
    g = torch.Generator().manual_seed(1234)
    if integer:
        L = math.lcm(*divisors(case, cip).unique().tolist())
        x = (L * torch.randint(-1, 2, (N, C, H, W), generator=g)).to(dtype)
        dy = (L * torch.randint(-1, 2, (N, C, P, Q), generator=g)).to(dtype)
        ref_t = torch.float64
    else:
        x = torch.randn(N, C, H, W, generator=g).to(dtype)
        dy = torch.randn(N, C, P, Q, generator=g).to(dtype)
        ref_t = torch.float32
    xr = x.to(ref_t).requires_grad_(True)
    y = F.avg_pool2d(xr, K, stride, pad, False, cip)
    (dx,) = torch.autograd.grad(y, xr, dy.to(ref_t))
    return dict(x=x, dy=dy, y=y.detach(), dx=dx)


def run_fwd(case, cip, pr):
    return ext().avgpool_fwd(nhwc(pr["x"]), case[4], case[5], case[6], cip)


def run_bwd(case, cip, pr):
    return ext().avgpool_bwd(nhwc(pr["dy"]), case[2], case[3], case[4], case[5],
                             case[6], cip)


def test_big_case_exceeds_grid_cap():
    N, C, H, W, K, stride, pad = BIG
    assert (K, stride, pad) == (3, 1, 1)
    assert N * H * ((W + 3) // 4) * (C // 8) > GRID_CAP_ITEMS


# ------------------------------------------------------- fp32 reference

@pytest.mark.parametrize("cip", MODES)
@pytest.mark.parametrize("case", ALL_CASES, ids=ids(ALL_CASES))
def test_avgpool_fwd(case, cip):
    pr = problem(case, cip)
    y = run_fwd(case, cip, pr)
    assert y.dtype == torch.bfloat16 and y.shape == pr["y"].shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert_close(y, pr["y"], name=f"avgpool_fwd{case} cip={cip}")


@pytest.mark.parametrize("cip", MODES)
@pytest.mark.parametrize("case", ALL_CASES, ids=ids(ALL_CASES))
def test_avgpool_bwd(case, cip):
    pr = problem(case, cip)
    dx = run_bwd(case, cip, pr)
    assert dx.dtype == torch.bfloat16 and dx.shape == pr["dx"].shape
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert_close(dx, pr["dx"], name=f"avgpool_bwd{case} cip={cip}")


# ------------------------------------------------------------------ fp16

@pytest.mark.parametrize("cip", MODES)
@pytest.mark.parametrize("case", [HOT, GENERIC], ids=ids([HOT, GENERIC]))
def test_avgpool_fp16(case, cip):
    pr = problem(case, cip, dtype=torch.float16)
    y = run_fwd(case, cip, pr)
    assert y.dtype == torch.float16
    assert_close(y, pr["y"], name=f"avgpool_fwd_fp16{case} cip={cip}")
    dx = run_bwd(case, cip, pr)
    assert dx.dtype == torch.float16
    assert_close(dx, pr["dx"], name=f"avgpool_bwd_fp16{case} cip={cip}")


# ------------------------------------------------- small integers, exact

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cip", MODES)
@pytest.mark.parametrize("case", EXACT_CASES, ids=ids(EXACT_CASES))
def test_avgpool_fwd_integer_exact(case, cip, dtype):
    pr = problem(case, cip, dtype=dtype, integer=True)
    assert torch.equal(pr["y"], pr["y"].round()) and pr["y"].abs().max() <= 256
    y = run_fwd(case, cip, pr)
    assert torch.equal(y.cpu(), pr["y"].to(dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cip", MODES)
@pytest.mark.parametrize("case", EXACT_CASES, ids=ids(EXACT_CASES))
def test_avgpool_bwd_integer_exact(case, cip, dtype):
    pr = problem(case, cip, dtype=dtype, integer=True)
    assert torch.equal(pr["dx"], pr["dx"].round()) and pr["dx"].abs().max() <= 256
    dx = run_bwd(case, cip, pr)
    assert torch.equal(dx.cpu(), pr["dx"].to(dtype))


@pytest.mark.parametrize("cip", MODES)
def test_avgpool_bwd_unreached_edge_is_zero(cip):
    """pad 0, stride 2, even size: no window reaches the last input row and
    column, so dx there is exactly 0 (written, not left as allocated)."""
    case = (2, 32, 8, 8, 3, 2, 0)
    pr = problem(case, cip)
    assert pr["dx"][:, :, -1, :].abs().max() == 0
    assert pr["dx"][:, :, :, -1].abs().max() == 0
    dx = run_bwd(case, cip, pr).float().cpu()
    assert dx[:, :, -1, :].abs().max() == 0
    assert dx[:, :, :, -1].abs().max() == 0
    assert dx[:, :, :-1, :-1].abs().max() > 0


def test_avgpool_count_modes_differ():
    """Guards against a swapped template argument: the two modes agree in the
    interior and differ on the border by exactly the divisor ratio. Integer
    inputs (multiples of 36) make both results exact integers."""
    case = CASES[0]
    K = case[4]
    pr = problem(case, False, integer=True)
    x = nhwc(pr["x"])
    incl = ext().avgpool_fwd(x, K, case[5], case[6], True).float().cpu()
    excl = ext().avgpool_fwd(x, K, case[5], case[6], False).float().cpu()
    assert torch.equal(incl[:, :, 1:-1, 1:-1], excl[:, :, 1:-1, 1:-1])
    cnt = divisors(case, False).float()
    assert cnt[0, 0] == 4 and cnt[0, 1] == 6 and cnt[1, 1] == 9
    assert torch.equal(excl * cnt, incl * (K * K))
    assert not torch.equal(incl, excl)
    assert torch.equal(excl, pr["y"].float())
    # the same for the backward's per-source weights
    dy = nhwc(pr["dy"])
    bi = ext().avgpool_bwd(dy, case[2], case[3], K, case[5], case[6], True)
    be = ext().avgpool_bwd(dy, case[2], case[3], K, case[5], case[6], False)
    assert torch.equal(be.float().cpu(), pr["dx"].float())
    xr = pr["x"].double().requires_grad_(True)
    (dxi,) = torch.autograd.grad(F.avg_pool2d(xr, K, case[5], case[6], False, True),
                                 xr, pr["dy"].double())
    assert torch.equal(bi.float().cpu(), dxi.float())
    assert not torch.equal(bi, be)


# ----------------------------------------------------------- determinism

@pytest.mark.parametrize("case", [CASES[4], CASES[5]], ids=ids([CASES[4], CASES[5]]))
def test_avgpool_deterministic(case):
    pr = problem(case, False)
    dy = nhwc(pr["dy"])
    a = ext().avgpool_bwd(dy, case[2], case[3], case[4], case[5], case[6], False)
    b = ext().avgpool_bwd(dy, case[2], case[3], case[4], case[5], case[6], False)
    assert torch.equal(a, b)


# -------------------------------------------------------------- autograd

@pytest.mark.parametrize("cip", MODES)
@pytest.mark.parametrize("case,layout", [(CASES[4], "nhwc"), (CASES[2], "nchw"),
                                         (CASES[5], "nchw")],
                         ids=["hot-nhwc", "hot-nchw", "generic-nchw"])
def test_avgpool_autograd(case, layout, cip):
    from dtmx.ops import functional as DF
    N, C, H, W, K, stride, pad = case
    pr = problem(case, cip)
    x = pr["x"].to(DEV).contiguous() if layout == "nchw" else nhwc(pr["x"])
    x.requires_grad_(True)
    y = DF.avg_pool2d(x, K, stride, pad, cip)
    assert type(y.grad_fn).__name__ == "_AvgPoolNHWCBackward"
    assert y.is_contiguous(memory_format=torch.channels_last)
    # a non-channels_last upstream gradient: backward must re-lay it out
    y.backward(pr["dy"].to(DEV).contiguous())
    assert x.grad.shape == x.shape and x.grad.dtype == torch.bfloat16
    assert_close(y, pr["y"], name="autograd y")
    assert_close(x.grad, pr["dx"], name="autograd x.grad")


# --------------------------------------------------------------- routing

def _record_native(monkeypatch):
    e = ext()
    calls = []
    real = e.avgpool_fwd

    def wrapper(*a, **k):
        calls.append(a[1:])
        return real(*a, **k)

    monkeypatch.setattr(e, "avgpool_fwd", wrapper)
    return calls


def test_layer_routes_native(monkeypatch):
    from dtmx.ops.layers import AvgPool2dNHWC
    calls = _record_native(monkeypatch)
    case = CASES[0]
    pr = problem(case, False)
    y = AvgPool2dNHWC(3, 1, 1, count_include_pad=False)(nhwc(pr["x"]))
    assert calls == [(3, 1, 1, False)]
    assert_close(y, pr["y"], name="layer fwd")


def test_default_stride_is_kernel(monkeypatch):
    from dtmx.ops import functional as DF
    calls = _record_native(monkeypatch)
    case = CASES[7]  # K = 2, stride 2
    pr = problem(case, True)
    y = DF.avg_pool2d(nhwc(pr["x"]), 2)
    assert calls == [(2, 2, 0, True)]
    assert_close(y, pr["y"], name="default stride")


def test_envelope_fallback(monkeypatch):
    from dtmx.ops import functional as DF
    calls = _record_native(monkeypatch)
    g = torch.Generator().manual_seed(5)
    # C = 20
    x = torch.randn(2, 20, 7, 7, generator=g).bfloat16()
    y = DF.avg_pool2d(nhwc(x), 3, 1, 1, False)
    assert torch.equal(y, F.avg_pool2d(nhwc(x), 3, 1, 1, False, False))
    assert_close(y, F.avg_pool2d(x.float(), 3, 1, 1, False, False), name="C=20")
    # fp32
    x32 = torch.randn(2, 16, 7, 7, generator=g)
    y = DF.avg_pool2d(nhwc(x32), 3, 1, 1, True)
    assert y.dtype == torch.float32
    assert torch.equal(y, F.avg_pool2d(nhwc(x32), 3, 1, 1, False, True))
    # tuple arguments
    xb = nhwc(x32.bfloat16())
    y = DF.avg_pool2d(xb, (3, 3), (1, 1), (1, 1), False)
    assert torch.equal(y, F.avg_pool2d(xb, (3, 3), (1, 1), (1, 1), False, False))
    # forced fallback
    monkeypatch.setattr(DF, "_FALLBACK", {"avgpool"})
    y = DF.avg_pool2d(xb, 3, 1, 1, False)
    assert torch.equal(y, F.avg_pool2d(xb, 3, 1, 1, False, False))
    assert calls == []
    monkeypatch.setattr(DF, "_FALLBACK", set())
    DF.avg_pool2d(xb, 3, 1, 1, False)
    assert calls == [(3, 1, 1, False)]


def test_entry_points_name_the_violated_condition():
    e = ext()
    pr = problem(CASES[0], True)
    x, dy = nhwc(pr["x"]), nhwc(pr["dy"])
    x20 = nhwc(torch.zeros(2, 20, 5, 5).bfloat16())
    for fwd in (True, False):
        def call(t, K=3, stride=1, pad=1):
            if fwd:
                return e.avgpool_fwd(t, K, stride, pad, True)
            return e.avgpool_bwd(t, 5, 5, K, stride, pad, True)
        good = x if fwd else dy
        with pytest.raises(RuntimeError, match="C % 8 == 0"):
            call(x20)
        with pytest.raises(RuntimeError, match="kernel must be in"):
            call(good, K=9, pad=0)
        with pytest.raises(RuntimeError, match="kernel must be in"):
            call(good, K=1, pad=0)
        with pytest.raises(RuntimeError, match="padding must be in"):
            call(good, pad=2)
        with pytest.raises(RuntimeError, match="stride must be in"):
            call(good, stride=9)
        with pytest.raises(RuntimeError, match="channels_last"):
            call(pr["x"].to(DEV).contiguous())
        with pytest.raises(RuntimeError, match="bfloat16/float16"):
            call(good.float())
    with pytest.raises(RuntimeError, match="empty output"):
        e.avgpool_fwd(nhwc(torch.zeros(1, 8, 2, 5).bfloat16()), 4, 1, 0, True)
    with pytest.raises(RuntimeError, match="does not match"):
        e.avgpool_bwd(dy, 6, 5, 3, 1, 1, True)


# ----------------------------------------------------------- graph capture

def test_avgpool_graph_capture():
    """fwd + bwd of both paths launch on the capture stream without a host
    sync; replays into zeroed outputs equal the eager results."""
    e = ext()
    jobs = []
    for case, cip in [(CASES[2], False), (CASES[2], True), (CASES[8], False)]:
        pr = problem(case, cip)
        jobs.append((case, cip, nhwc(pr["x"]), nhwc(pr["dy"])))

    def run():
        outs = []
        for (N, C, H, W, K, s, p), cip, x, dy in jobs:
            outs.append(e.avgpool_fwd(x, K, s, p, cip))
            outs.append(e.avgpool_bwd(dy, H, W, K, s, p, cip))
        return outs

    want = run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for _ in range(2):
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
