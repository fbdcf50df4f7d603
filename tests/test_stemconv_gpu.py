"""First-layer convolution (stemconv.hip: fwd with fused BN statistics, wgrad)
and its DF.conv2d routing, against fp64 F.conv2d / conv2d_weight on the CPU on
the same 16-bit-rounded inputs.

Integer-exact cases: |x|, |w|, |dy| <= 3 keep every fp32 sum an exact integer
(at most 7 * 7 * 4 terms forward, N * P * Q <= 456 pixels in wgrad): bit-equal
to the fp64 result rounded once. Random cases: |got - ref| <= K 2^-24 S +
1/2 ulp(|ref| + K 2^-24 S), K the contraction length, S the same op on
magnitudes (tests/test_gemm_conv_gpu.py).
"""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

pytestmark = pytest.mark.gpu

DEV = "cuda"
_dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                                  ids=["bf16", "fp16"])
# (N, H, W, C, Ko, R = S, stride, pad): what each breaks is listed in
# docs/KERNELS.md
CASES = [(2, 9, 11, 3, 8, 7, 2, 3), (1, 23, 37, 3, 64, 7, 2, 3),
         (2, 19, 35, 3, 72, 3, 2, 0), (1, 18, 18, 3, 32, 3, 2, 1),
         (2, 10, 21, 3, 16, 3, 1, 1), (1, 12, 12, 1, 8, 5, 1, 0),
         (1, 9, 10, 2, 8, 3, 1, (1, 0)), (1, 9, 10, 4, 8, 7, 1, 3)]
RANDOM = (2, 23, 37, 3, 64, 7, 2, 3)
_case_id = lambda c: "x".join(str(v).replace(", ", "_") for v in c)


def _ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dtmx.ops.hip import require_ext

    return require_ext()


def _dev(t, dtype, offset=0, cl=True):
    """on the device `offset` elements into its buffer, NHWC (cl) or NCHW"""
    buf = torch.empty(t.numel() + offset, device=DEV, dtype=dtype)
    N, C, H, W = t.shape
    out = buf[offset:].view(N, H, W, C).permute(0, 3, 1, 2) if cl else \
        buf[offset:].view(N, C, H, W)
    return out.copy_(t)


@functools.lru_cache(maxsize=None)
def _data(case, ints=True, dtype=None):
    """x, w, dy and the fp64 y, dw of a case; values are dtype-representable"""
    N, H, W, C, Ko, RS, stride, pad = case
    pad = pad if isinstance(pad, tuple) else (pad, pad)
    g = torch.Generator().manual_seed(7)
    P, Q = ((d + 2 * p - RS) // stride + 1 for d, p in zip((H, W), pad))
    sizes = [(N, C, H, W), (Ko, C, RS, RS), (N, Ko, P, Q)]
    if ints:
        x, w, dy = (torch.randint(-3, 4, s, generator=g).double() for s in sizes)
    else:
        x, w, dy = (torch.randn(s, generator=g).to(dtype).double() for s in sizes)
    return (x, w, dy, F.conv2d(x, w, None, stride, pad),
            conv2d_weight(x, w.shape, dy, stride, pad), stride, pad)


def _assert_bits(got, want64, dtype):
    assert got.dtype == dtype and got.shape == want64.shape
    torch.testing.assert_close(got.double().cpu(), want64.to(dtype).double(),
                               rtol=0, atol=0)


def _bound(ref, S, K, dtype):
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    a = K * 2.0 ** -24 * S
    v = ref.abs() + a
    e = torch.frexp(v.clamp_min(2.0 ** emin))[1] - 1
    return a + 0.5 * torch.ldexp(torch.ones_like(v), e - p)


@_dtypes
@pytest.mark.parametrize("w_cl", [True, False], ids=["KRSC", "KCRS"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_stem_exact(case, w_cl, dtype):
    """x and w one element into their buffers; dw in the layout of w; slices
    1, 2, 3 (3 exceeds the two tiles of the first case), twice in a row"""
    ext = _ext()
    from dtmx.ops import functional as DF

    x64, w64, dy64, y64, dw64, stride, pad = _data(case)
    x, w, dy = _dev(x64, dtype, 1), _dev(w64, dtype, 1, w_cl), _dev(dy64, dtype)
    assert DF._stemconv_in_envelope(x, w, stride, *pad)
    y, ps, pss = ext.stemconv_fwd(x, w, stride, *pad)
    assert ps.numel() == 0 and pss.numel() == 0
    _assert_bits(y, y64, dtype)
    for slices in (0, 1, 2, 3, 1, 2, 3):
        dw = ext.stemconv_wgrad(x, dy, *w.shape[2:], stride, *pad,
                                not w.is_contiguous(), slices)
        assert dw.stride() == w.stride() or 1 in w.shape[1:]
        assert dw.is_contiguous() == w.is_contiguous()
        _assert_bits(dw, dw64, dtype)


@_dtypes
@pytest.mark.parametrize("case", CASES[1:3], ids=_case_id)
def test_stem_stats(case, dtype):
    """one exclusive fp32 slab row per tile over the rounded y; BatchNorm on
    the slabs equals BatchNorm on its own statistics pass (tolerance of the
    fused-against-plain comparison in tests/test_bnfuse_gpu.py)"""
    ext = _ext()
    from dtmx.ops import functional as DF

    x64, w64, _, y64, _, stride, pad = _data(case)
    Ko = case[4]
    y, ps, pss = ext.stemconv_fwd(_dev(x64, dtype, 1), _dev(w64, dtype, 1), stride,
                                  *pad, True)
    _assert_bits(y, y64, dtype)
    yr = y64.to(dtype).double()
    assert (yr * yr).sum((0, 2, 3)).max() < 2 ** 24  # fp32 sums exact in any order
    tiles = case[0] * -(-y64.shape[2] // 8) * -(-y64.shape[3] // 16)
    for slab, want in ((ps, yr), (pss, yr * yr)):
        assert slab.dtype == torch.float32 and slab.shape == (tiles, Ko)
        torch.testing.assert_close(slab.double().sum(0).cpu(), want.sum((0, 2, 3)),
                                   rtol=0, atol=0)
    g = torch.Generator().manual_seed(8)
    gamma, beta = (torch.randn(Ko, generator=g).to(dtype).to(DEV) for _ in range(2))
    outs = []
    for pre in ((ps, pss), None):
        rm, rv = torch.zeros(Ko, device=DEV), torch.ones(Ko, device=DEV)
        outs.append((DF.batch_norm(y, gamma, beta, rm, rv, True, pre_stats=pre), rm, rv))
    for a, b in zip(*outs):
        torch.testing.assert_close(a.float(), b.float(), rtol=0.01, atol=0.01)


@_dtypes
@pytest.mark.parametrize("entry", ["fwd", "wgrad"])
def test_stem_random(entry, dtype):
    ext = _ext()
    x64, w64, dy64, y64, dw64, stride, pad = _data(RANDOM, False, dtype)
    N, _, _, C, _, RS = RANDOM[:6]
    x, w, dy = _dev(x64, dtype, 1), _dev(w64, dtype, 1), _dev(dy64, dtype)
    if entry == "fwd":
        got, ref, K = ext.stemconv_fwd(x, w, stride, *pad)[0], y64, RS * RS * C
        S = F.conv2d(x64.abs(), w64.abs(), None, stride, pad)
    else:
        got = ext.stemconv_wgrad(x, dy, RS, RS, stride, *pad, True)
        ref, K = dw64, N * dy64.shape[2] * dy64.shape[3]
        S = conv2d_weight(x64.abs(), w64.shape, dy64.abs(), stride, pad)
    bound = _bound(ref, S, K, dtype)
    err = (got.double().cpu() - ref).abs()
    print(f"stemconv_{entry} {dtype}: max err / bound = "
          f"{(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


@_dtypes
@pytest.mark.parametrize("native_fwd", [False, True], ids=["routed", "native-fwd"])
def test_conv2d_routing_autograd_graph(native_fwd, dtype, monkeypatch):
    """DF.conv2d on a C = 3 input takes _StemConvNHWC (the dispatch says so):
    y, dw (stemconv_wgrad) and the padded-path dx are exact, nothing syncs
    with the host, and replays of a captured fwd + wgrad give the eager bits.
    As routed the forward runs the padded generic kernels (stemconv_fwd
    measured slower, profiles/resnet50_mi355x.md); native-fwd forces
    stemconv_fwd through the same autograd function."""
    ext = _ext()
    from dtmx.ops import functional as DF

    if native_fwd:
        monkeypatch.setattr(DF, "_stemconv_fwd_routed", lambda *a: True)
    x64, w64, dy64, y64, dw64, stride, pad = _data(CASES[1])
    x, w, dy = _dev(x64, dtype, 1), _dev(w64, dtype, 1), _dev(dy64, dtype)
    assert DF._stemconv_in_envelope(x, w, stride, *pad)
    assert DF._conv2d_dispatch(x, w, stride, pad[0]) == "stemconv"
    with monkeypatch.context() as m:
        m.setattr(DF, "_FALLBACK", DF._FALLBACK | {"stemconv"})
        assert DF._conv2d_dispatch(x, w, stride, pad[0]) == "hip"
    x.requires_grad_(True)
    w.requires_grad_(True)

    def run(wrt):
        y = DF.conv2d(x, w, stride, pad)
        return (y.detach(),) + torch.autograd.grad(y, wrt, dy)

    torch.cuda.set_sync_debug_mode("error")
    try:
        y, dx, dw = run((x, w))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _assert_bits(y, y64, dtype)
    _assert_bits(dw, dw64, dtype)
    _assert_bits(dx, conv2d_input(x64.shape, w64, dy64, stride, pad), dtype)

    eager = run((w,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = run((w,))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
