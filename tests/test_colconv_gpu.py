"""Column convolution (colconv.hip) and its DF.conv2d routing against fp64
F.conv2d / conv2d_input / conv2d_weight on the CPU on the same 16-bit-rounded
inputs.

Integer-exact cases: |x|, |w| <= 3 and at most 7 * 72 terms keep every fp32
partial sum an exact integer: bit-equal to the fp64 result rounded once.
Random cases: |got - ref| <= K 2^-24 S + 1/2 ulp(|ref| + K 2^-24 S), K the
contraction length, S the same op on magnitudes (tests/test_gemm_conv_gpu.py).
"""
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

pytestmark = pytest.mark.gpu

DEV = "cuda"
_dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                                  ids=["bf16", "fp16"])
# (N, H, W, C, Ko): what each breaks is listed in docs/KERNELS.md
SHAPES = [(2, 3, 5, 8, 8), (1, 1, 3, 8, 8), (3, 17, 9, 72, 136),
          (1, 61, 3, 8, 8), (1, 9, 44, 8, 8)]


def _ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dtmx.ops.hip import require_ext

    return require_ext()


def _dev(t, dtype, offset=0):
    """NHWC on the device, `offset` elements into its buffer (a parameter
    that is a view of a flat bucket carries element alignment only)"""
    buf = torch.empty(t.numel() + offset, device=DEV, dtype=dtype)
    N, C, H, W = t.shape
    out = buf[offset:].view(N, H, W, C).permute(0, 3, 1, 2)
    return out.copy_(t)


def _data(seed, shape, T, dtype, ints=True):
    """x, w, dy as fp64 CPU tensors holding dtype-representable values"""
    g = torch.Generator().manual_seed(seed)
    N, H, W, C, Ko = shape
    sizes = [(N, C, H, W), (Ko, C, T, 1), (N, Ko, H, W)]
    if ints:
        return [torch.randint(-3, 4, s, generator=g).double() for s in sizes]
    return [torch.randn(s, generator=g).to(dtype).double() for s in sizes]


def _assert_bits(got, want64, dtype):
    assert got.dtype == dtype and got.shape == want64.shape
    torch.testing.assert_close(got.double().cpu(), want64.to(dtype).double(),
                               rtol=0, atol=0)


def _ulp(v, dtype):
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(v.clamp_min(2.0 ** emin))[1] - 1
    return torch.ldexp(torch.ones_like(v), e - p)


@_dtypes
@pytest.mark.parametrize("T", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_col_exact(shape, T, dtype):
    ext = _ext()
    pad = (T // 2, 0)
    x64, w64, dy64 = _data(1, shape, T, dtype)
    # the two-chunk case takes its weight 3 elements into its buffer
    x, w, dy = _dev(x64, dtype), _dev(w64, dtype, 3 * (shape[3] > 64)), _dev(dy64, dtype)
    y, dx = ext.colconv_fwd(x, w), ext.colconv_dgrad(dy, w)
    _assert_bits(y, F.conv2d(x64, w64, None, 1, pad), dtype)
    _assert_bits(dx, conv2d_input(x64.shape, w64, dy64, 1, pad), dtype)
    # double-buffer and ring state: a second run gives the same bits
    assert torch.equal(ext.colconv_fwd(x, w), y)
    assert torch.equal(ext.colconv_dgrad(dy, w), dx)


@_dtypes
@pytest.mark.parametrize("entry", ["fwd", "dgrad"])
def test_col_random(entry, dtype):
    ext = _ext()
    T, shape = 7, (2, 17, 9, 72, 136)
    N, H, W, C, Ko = shape
    pad = (T // 2, 0)
    x64, w64, dy64 = _data(2, shape, T, dtype, ints=False)
    if entry == "fwd":
        a64, K, fn = x64, T * C, ext.colconv_fwd

        def op(a, w):
            return F.conv2d(a, w, None, 1, pad)
    else:
        a64, K, fn = dy64, T * Ko, ext.colconv_dgrad

        def op(a, w):
            return conv2d_input((N, C, H, W), w, a, 1, pad)
    ref = op(a64, w64)
    slack = K * 2.0 ** -24 * op(a64.abs(), w64.abs())
    bound = slack + 0.5 * _ulp(ref.abs() + slack, dtype)
    err = (fn(_dev(a64, dtype), _dev(w64, dtype)).double().cpu() - ref).abs()
    print(f"colconv_{entry} {dtype}: max err / bound = "
          f"{(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


@_dtypes
def test_conv2d_end_to_end(dtype, monkeypatch):
    """y, dx, dw through autograd with the whole envelope routed: against
    fp64, and the same bits with colconv in DTMX_FALLBACK"""
    _ext()
    from dtmx.ops import functional as DF

    pad = (3, 0)
    x64, w64, dy64 = _data(4, (2, 17, 17, 16, 24), 7, dtype)
    x, w, dy = (_dev(t, dtype) for t in (x64, w64, dy64))
    monkeypatch.setattr(DF, "_colconv_routed", DF._colconv_in_envelope)
    assert not DF._lineconv_routed(x, w, 1, *pad)
    assert DF._colconv_routed(x, w, 1, *pad)
    x.requires_grad_(True)
    w.requires_grad_(True)

    def run():
        y = DF.conv2d(x, w, 1, pad)
        return (y.detach(),) + torch.autograd.grad(y, (x, w), dy)

    col = run()
    for got, want in zip(col, (F.conv2d(x64, w64, None, 1, pad),
                               conv2d_input(x64.shape, w64, dy64, 1, pad),
                               conv2d_weight(x64, w64.shape, dy64, 1, pad))):
        _assert_bits(got, want, dtype)
    monkeypatch.setattr(DF, "_FALLBACK", DF._FALLBACK | {"colconv"})
    for got, want in zip(run(), col):
        assert torch.equal(got, want)
