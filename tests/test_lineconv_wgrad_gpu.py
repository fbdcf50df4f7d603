"""Line-conv weight gradient (lineconv_wgrad.hip) and its DF.conv2d routing
against fp64 torch.nn.grad.conv2d_weight on the CPU, on the same
16-bit-representable inputs.

Integer cases: |x|, |dy| <= 3 and at most 1369 pixels keep every fp32 partial
sum an exact integer (< 2^24): bit-equal to the fp64 result rounded once,
whatever the slice count. Random case: |got - ref| <= K 2^-24 S +
1/2 ulp(|ref| + K 2^-24 S), K = N*H*W the contraction length, S the same op
on magnitudes (the bound of tests/test_lineconv_gpu.py).
"""
import pytest
import torch
from torch.nn.grad import conv2d_weight

pytestmark = pytest.mark.gpu

DEV = "cuda"
_dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                                  ids=["bf16", "fp16"])
_orient = pytest.mark.parametrize("vertical", [False, True], ids=["1xT", "Tx1"])
# (N, H, W, C, Ko): what each breaks is listed in docs/KERNELS.md
SHAPES = [(2, 3, 5, 8, 8), (1, 2, 2, 8, 8), (2, 9, 17, 72, 136),
          (3, 17, 9, 72, 136), (1, 37, 37, 8, 8)]


def _ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dtmx.ops.hip import require_ext

    return require_ext()


def _geom(T, vertical):
    """kernel (R, S) and padding (ph, pw) of a same-padded line conv"""
    return ((T, 1), (T // 2, 0)) if vertical else ((1, T), (0, T // 2))


def _dev(t, dtype):
    return t.to(DEV, dtype).contiguous(memory_format=torch.channels_last)


def _data(seed, shape, dtype, ints=True):
    """x, dy as fp64 CPU tensors holding dtype-representable values"""
    g = torch.Generator().manual_seed(seed)
    N, H, W, C, Ko = shape
    sizes = [(N, C, H, W), (N, Ko, H, W)]
    if ints:
        return [torch.randint(-3, 4, s, generator=g).double() for s in sizes]
    return [torch.randn(s, generator=g).to(dtype).double() for s in sizes]


def _ref(x64, dy64, T, vertical):
    rs, pad = _geom(T, vertical)
    return conv2d_weight(x64, (dy64.shape[1], x64.shape[1]) + rs, dy64, 1, pad)


def _assert_bits(got, want64, dtype):
    assert got.dtype == dtype and got.shape == want64.shape
    assert got.is_contiguous(memory_format=torch.channels_last)
    torch.testing.assert_close(got.double().cpu(), want64.to(dtype).double(),
                               rtol=0, atol=0)


@_dtypes
@_orient
@pytest.mark.parametrize("T", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_exact(shape, T, vertical, dtype):
    """the plan's slice count everywhere; on the 72 -> 136 shapes also 1, 2, 3
    slices (short last slice) and one K-tile per slice; each call twice"""
    ext = _ext()
    x64, dy64 = _data(1, shape, dtype)
    want = _ref(x64, dy64, T, vertical)
    x, dy = _dev(x64, dtype), _dev(dy64, dtype)
    ktiles = -(-shape[0] * shape[1] * shape[2] // 64)
    cls, planned = ext.lineconv_wgrad_plan(shape[4], shape[3], T, vertical, *shape[:3])
    assert 1 <= planned <= ktiles and cls in (3, 6, 10)
    for slices in [0] + ([1, 2, 3, ktiles] if shape[3] == 72 else []):
        dw = ext.lineconv_wgrad(x, dy, T, vertical, slices)
        _assert_bits(dw, want, dtype)
        assert torch.equal(dw, ext.lineconv_wgrad(x, dy, T, vertical, slices))


def test_wgrad_envelope_raises():
    ext = _ext()
    x, dy = (_dev(t, torch.bfloat16) for t in _data(1, (1, 1, 44, 8, 8), torch.bfloat16))
    with pytest.raises(RuntimeError, match="halo"):  # 7x1 at W = 44: 264 rows
        ext.lineconv_wgrad(x, dy, 7, True)
    with pytest.raises(RuntimeError, match="slices"):  # one K-tile
        ext.lineconv_wgrad(x, dy, 7, False, 2)


@_dtypes
@_orient
def test_wgrad_delta(vertical, dtype):
    """x is a delta at a corner and at an interior pixel of two images, dy is
    distinct per pixel: dw[., t, .] is the dy pixel (t - pad) steps back along
    the tap axis, zero where that leaves the image, nothing from across a
    row or image seam"""
    ext = _ext()
    T, (N, H, W, C, Ko) = 7, SHAPES[2]
    x64 = torch.zeros(N, C, H, W, dtype=torch.float64)
    x64[0, :, 0, 0] = 1
    x64[1, :, 4, 8] = 1
    i = torch.arange(N * H * W, dtype=torch.float64)  # 8 significant bits each
    dy64 = (2.0 ** (i // 128) * (1 + (i % 128) / 128)).reshape(N, 1, H, W)
    dy64 = dy64.expand(N, Ko, H, W).contiguous()
    dw = ext.lineconv_wgrad(_dev(x64, dtype), _dev(dy64, dtype), T, vertical)
    _assert_bits(dw, _ref(x64, dy64, T, vertical), dtype)
    taps = dw.double().cpu()[0, 0].flatten()
    want = torch.zeros(T, dtype=torch.float64)
    for n, h, w in ((0, 0, 0), (1, 4, 8)):
        for t in range(T):
            hh, ww = (h - (t - 3), w) if vertical else (h, w - (t - 3))
            if 0 <= hh < H and 0 <= ww < W:
                want[t] += dy64[n, 0, hh, ww]
    assert torch.equal(taps, want.to(dtype).double())


@_dtypes
@_orient
def test_wgrad_random(vertical, dtype):
    ext = _ext()
    T, shape = 7, SHAPES[2]
    K = shape[0] * shape[1] * shape[2]
    x64, dy64 = _data(2, shape, dtype, ints=False)
    ref = _ref(x64, dy64, T, vertical)
    a = K * 2.0 ** -24 * _ref(x64.abs(), dy64.abs(), T, vertical)
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp((ref.abs() + a).clamp_min(2.0 ** emin))[1] - 1
    bound = a + 0.5 * torch.ldexp(torch.ones_like(a), e - p)
    tap0 = ref.reshape(shape[4], shape[3], T).clone()
    tap0[:, :, 3] = 0
    tap0 = tap0.reshape(ref.shape)
    mutants = {"tap 3 zeroed": tap0,
               "orientation swapped": _ref(x64, dy64, T, not vertical).transpose(2, 3),
               "dy shifted one pixel": _ref(x64, dy64.roll(1, 2 if vertical else 3),
                                            T, vertical)}
    for what, m in mutants.items():
        assert bool(((m - ref).abs() > bound).any()), what
    got = ext.lineconv_wgrad(_dev(x64, dtype), _dev(dy64, dtype), T, vertical)
    err = (got.double().cpu() - ref).abs()
    print(f"lineconv_wgrad {'Tx1' if vertical else '1xT'} {dtype}: "
          f"max err / bound = {(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


@_dtypes
@_orient
def test_wgrad_routing(vertical, dtype, monkeypatch):
    """DF.conv2d backward takes the line wgrad at a routed shape and the
    generic NT kernels under DTMX_FALLBACK=linewgrad. Integer inputs give both
    the same bits (the generic split-K sums are not bit-stable on N(0,1)), so
    the line entry is taken away while the fallback is on."""
    ext = _ext()
    from dtmx.ops import functional as DF

    T = 7
    rs, pad = _geom(T, vertical)
    x64, dy64 = _data(4, (2, 17, 5, 72, 136), dtype)
    x, dy = _dev(x64, dtype), _dev(dy64, dtype)
    w = _dev(torch.ones(136, 72, *rs), dtype).requires_grad_(True)
    assert DF._lineconv_wgrad_routed(x, dy, w, 1, *pad)

    def dw():
        return torch.autograd.grad(DF.conv2d(x, w, 1, pad), w, dy)[0]

    line = ext.lineconv_wgrad(x, dy, T, vertical)
    _assert_bits(line, _ref(x64, dy64, T, vertical), dtype)
    monkeypatch.setattr(ext, "lineconv_wgrad", None)
    with pytest.raises(TypeError):  # routed: reaches for the line entry
        dw()
    monkeypatch.setattr(DF, "_FALLBACK", DF._FALLBACK | {"linewgrad"})
    assert torch.equal(dw(), ext.conv_wgrad_hw(x, dy, *rs, 1, *pad))
    monkeypatch.undo()
    assert torch.equal(dw(), line)
