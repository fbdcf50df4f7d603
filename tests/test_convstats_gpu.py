"""BatchNorm statistics fused into the depthwise / grouped conv forward
(dwconv_fwd_stats, gconv_fwd_stats) against fp64 sums of the stored output.

Integer cases: x, w in [-4, 4], so y and every partial sum is an exactly
represented integer and the slab column totals must equal the fp64 sums over
the rounded y bit for bit. Random cases: any-order fp32 summation bound
|sum_slab - sum_64| <= n * 2^-24 * sum|v|, no further slack.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]

DW_CASES = [  # (N, H, W, C, stride, pad)
    (2, 5, 7, 8, 1, 1),         # one channel vector; strip tail at Q = 7; batch seam
    (1, 9, 9, 24, 2, 0),        # C/8 = 3 does not divide 256; far edge, s2 p0
    (2, 3, 3, 2056, 1, 1),      # C/8 = 257 > 256: rest of the row is zeroed
    (8, 128, 256, 64, 1, 1),    # exactly 2048 * 256 items: the full capped grid
    (9, 128, 256, 64, 1, 1),    # 2304 * 256 items: some threads walk twice
    (12, 256, 256, 24, 1, 1),   # C/8 = 3, 2304 * 256 items: the grid is rounded
                                # to 2046 blocks, or a second step changes vector
    (1, 33, 224, 2056, 1, 1),   # C/8 = 257, 1856 * 256 items: 2056 blocks would
                                # pass the cap, rounded down to 1799 that walk on
]
GC_CASES = [  # (N, H, W, C, Cg, stride, pad)
    (2, 5, 7, 32, 4, 1, 1),     # one channel tile; 70 pixels: pixel-step tail
    (1, 9, 11, 160, 32, 2, 0),  # five tiles: second block has one live wave
    (3, 6, 6, 64, 16, 1, 0),    # two tiles; diagonal-block width 16
    (5, 120, 120, 32, 4, 1, 1),  # 1125 pixel steps on 1024 walkers: a second step
]
DW_RANDOM = (2, 9, 11, 72, 1, 1)
GC_RANDOM = (2, 9, 11, 96, 8, 1, 1)


def ext():
    from dtmx.ops.hip import require_ext
    return require_ext()


def operands(case, dtype, integer):
    """x (NHWC), w and the (plain, stats) entry closures of a dw or gc case."""
    grouped = len(case) == 7
    N, H, W, C = case[:4]
    Cg = case[4] if grouped else 1
    stride, pad = case[-2:]
    g = torch.Generator().manual_seed(7)
    if integer:
        x = torch.randint(-4, 5, (N, C, H, W), generator=g).to(dtype)
        w = torch.randint(-4, 5, (C, Cg, 3, 3), generator=g).to(dtype)
    else:
        x = torch.randn(N, C, H, W, generator=g).to(dtype)
        w = (torch.randn(C, Cg, 3, 3, generator=g) * 0.3).to(dtype)
    x = x.to(DEV).contiguous(memory_format=torch.channels_last)
    w = w.to(DEV)
    tail = (stride, pad, C // Cg) if grouped else (stride, pad)
    e = ext()
    plain, stats = ((e.gconv_fwd, e.gconv_fwd_stats) if grouped
                    else (e.dwconv_fwd, e.dwconv_fwd_stats))
    return x, w, (lambda: plain(x, w, *tail)), (lambda: stats(x, w, *tail))


def sums64(y):
    v = y.double().permute(1, 0, 2, 3).reshape(y.shape[1], -1)
    return v.sum(1), (v * v).sum(1), v.abs().sum(1), v.shape[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", DW_CASES + GC_CASES, ids=str)
def test_integer_exact(case, dtype):
    x, w, plain, stats = operands(case, dtype, integer=True)
    y, ps, pss = stats()
    y2, ps2, pss2 = stats()
    assert torch.equal(y, plain()), "y differs from the plain entry"
    C = x.shape[1]
    assert ps.dtype == pss.dtype == torch.float32
    assert ps.dim() == 2 and ps.shape[1] == C and ps.shape == pss.shape
    assert 1 <= ps.shape[0] <= (2048 if len(case) == 6 else 1024)
    s, q, _, _ = sums64(y)
    assert torch.equal(ps.double().sum(0), s)
    assert torch.equal(pss.double().sum(0), q)
    # every element written, the same way, by both calls
    assert torch.equal(ps, ps2) and torch.equal(pss, pss2) and torch.equal(y, y2)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [DW_RANDOM, GC_RANDOM], ids=str)
def test_random_summation_bound(case, dtype):
    x, w, plain, stats = operands(case, dtype, integer=False)
    y, ps, pss = stats()
    assert torch.equal(y, plain())
    s, q, a, n = sums64(y)
    u = n * 2.0 ** -24
    es, eq = (ps.double().sum(0) - s).abs(), (pss.double().sum(0) - q).abs()
    print(f"{case} {dtype}: max err/bound sum {(es / (u * a)).max().item():.3e} "
          f"sumsq {(eq / (u * q)).max().item():.3e}")
    assert (es <= u * a).all() and (eq <= u * q).all()


# depthwise: just inside the routed class (_dwconv_stats_routed: 25 M elements)
@pytest.mark.parametrize("case", [(28, 112, 112, 72, 1, 1), GC_RANDOM], ids=str)
def test_public_path_conv_bn(case, monkeypatch):
    """GroupedConv2dNHWC -> BatchNorm2dNHWC carries the slabs; statistics and
    output agree with the BatchNorm's own pass on the same conv output, and a
    captured graph replays the eager bits."""
    from dtmx.ops import functional as DF
    from dtmx.ops.layers import BatchNorm2dNHWC, GroupedConv2dNHWC
    monkeypatch.setenv("DTMX_FUSE_BN_STATS", "1")
    grouped = len(case) == 7
    N, H, W, C = case[:4]
    torch.manual_seed(3)
    conv = GroupedConv2dNHWC(C, C, 3, case[-2], case[-1],
                             groups=C // case[4] if grouped else C)
    conv = conv.to(DEV).bfloat16().train()
    bn = BatchNorm2dNHWC(C, momentum=0.0).to(DEV).bfloat16().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C))
    ref = copy.deepcopy(bn)
    x = torch.randn(N, C, H, W).bfloat16().to(DEV).contiguous(
        memory_format=torch.channels_last)
    with torch.no_grad():
        yc = conv(x)
        assert hasattr(yc, "_dtmx_bn_stats")
        out = bn(yc)
        want = DF.batch_norm(yc, ref.weight, ref.bias, ref.running_mean,
                             ref.running_var, True, 0.0, ref.eps, False, None, None)
    # momentum 0: running_mean is the batch mean, running_var the unbiased var
    s, q, a, n = sums64(yc)
    bm, bq = 2.0 ** -24 * a, 2.0 ** -24 * q    # the bound of the sums, over n
    mean = (s / n).abs()
    bvar = (bq + 2 * mean * bm + bm * bm) * n / (n - 1)
    assert ((bn.running_mean - ref.running_mean).abs().double() <= bm).all()
    assert ((bn.running_var - ref.running_var).abs().double() <= bvar).all()
    # y = (x - mean) * invstd * gamma + beta moves by dz before the bf16
    # rounding, which can then flip by one ulp (<= 2^-7 |y|)
    invstd = (q / n - (s / n) ** 2 + bn.eps).rsqrt()
    dev = (yc.double() - (s / n).view(1, -1, 1, 1)).abs().amax((0, 2, 3))
    dz = bn.weight.double().abs() * invstd * (bm + dev * invstd ** 2 * bvar / 2)
    tol = 2.0 ** -7 * want.double().abs() + dz.view(1, -1, 1, 1)
    assert ((out.double() - want.double()).abs() <= tol).all()

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(side):
        bn(conv(x))
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad(), torch.cuda.graph(g):
        got = bn(conv(x))
    for _ in range(3):
        got.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, out)
