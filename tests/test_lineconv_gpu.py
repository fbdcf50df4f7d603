"""Line convolution (lineconv.hip), the per-axis generic entries (conv_*_hw)
and their DF.conv2d / inception-v3 routing, against fp64 F.conv2d /
conv2d_input / conv2d_weight on the CPU on the same 16-bit-rounded inputs.

Integer-exact cases: |x|, |w| <= 3 and at most 7 * 136 terms keep every fp32
partial sum an exact integer: bit-equal to the fp64 result rounded once.
Random cases: |got - ref| <= K 2^-24 S + 1/2 ulp(|ref| + K 2^-24 S), K the
contraction length, S the same op on magnitudes (tests/test_gemm_conv_gpu.py).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

pytestmark = pytest.mark.gpu

DEV = "cuda"
_dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                                  ids=["bf16", "fp16"])
_orient = pytest.mark.parametrize("vertical", [False, True], ids=["1xT", "Tx1"])
# (N, H, W, C, Ko): what each breaks is listed in docs/KERNELS.md
SHAPES = [(2, 3, 5, 8, 8), (1, 2, 2, 8, 8), (2, 9, 17, 72, 136),
          (3, 17, 9, 72, 136), (1, 37, 37, 8, 8), (1, 1, 44, 8, 8)]


def _ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dtmx.ops.hip import require_ext

    return require_ext()


def _geom(T, vertical):
    """kernel (R, S) and padding (ph, pw) of a same-padded line conv"""
    return ((T, 1), (T // 2, 0)) if vertical else ((1, T), (0, T // 2))


def _dev(t, dtype, offset=0):
    """NHWC on the device, `offset` elements into its buffer (a parameter
    that is a view of a flat bucket carries element alignment only)"""
    buf = torch.empty(t.numel() + offset, device=DEV, dtype=dtype)
    N, C, H, W = t.shape
    out = buf[offset:].view(N, H, W, C).permute(0, 3, 1, 2)
    return out.copy_(t)


def _data(seed, shape, Ko, rs, dtype, pad, stride=1, ints=True):
    """x, w, dy as fp64 CPU tensors holding dtype-representable values"""
    g = torch.Generator().manual_seed(seed)
    N, H, W, C = shape
    P = (H + 2 * pad[0] - rs[0]) // stride + 1
    Q = (W + 2 * pad[1] - rs[1]) // stride + 1
    sizes = [(N, C, H, W), (Ko, C) + tuple(rs), (N, Ko, P, Q)]
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


def _bound(ref, S, K, dtype):
    a = K * 2.0 ** -24 * S
    return a + 0.5 * _ulp(ref.abs() + a, dtype)


@_dtypes
@_orient
@pytest.mark.parametrize("T", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_line_exact(shape, T, vertical, dtype):
    """the line kernels themselves wherever their envelope holds; the one
    shape outside it (Tx1, T = 7, W = 44: halo 264) through DF.conv2d, which
    must take the generic path and still be right"""
    ext = _ext()
    from dtmx.ops import functional as DF

    rs, pad = _geom(T, vertical)
    x64, w64, dy64 = _data(1, shape[:4], shape[4], rs, dtype, pad)
    x, w, dy = (_dev(t, dtype) for t in (x64, w64, dy64))
    line = DF._lineconv_in_envelope(x, w, 1, *pad)
    assert line == (not vertical or (T - 1) * shape[2] <= 256)
    if line:
        y, dx = ext.lineconv_fwd(x, w), ext.lineconv_dgrad(dy, w)
    else:
        with pytest.raises(RuntimeError, match="halo"):
            ext.lineconv_fwd(x, w)
        x.requires_grad_(True)
        y = DF.conv2d(x, w, 1, pad)
        dx, = torch.autograd.grad(y, x, dy)
    _assert_bits(y.detach(), F.conv2d(x64, w64, None, 1, pad), dtype)
    _assert_bits(dx, conv2d_input(x64.shape, w64, dy64, 1, pad), dtype)


@_dtypes
@_orient
def test_line_dgrad_delta(vertical, dtype):
    """dy is a delta at a corner and at an interior pixel, every tap has its
    own weight: dx is nonzero on exactly the pixels of the tap axis, in the
    right order"""
    ext = _ext()
    T, (N, H, W, C, Ko) = 7, SHAPES[2]
    rs, pad = _geom(T, vertical)
    w64 = torch.arange(1, T + 1, dtype=torch.float64).reshape(rs).expand(Ko, C, *rs).contiguous()
    dy64 = torch.zeros(N, Ko, H, W, dtype=torch.float64)
    dy64[0, :, 0, 0] = 1
    dy64[1, :, 4, 8] = 1
    dx = ext.lineconv_dgrad(_dev(dy64, dtype), _dev(w64, dtype))
    want = conv2d_input((N, C, H, W), w64, dy64, 1, pad)
    _assert_bits(dx, want, dtype)
    support = (dx != 0).any(1).cpu()
    assert support.sum().item() == (T // 2 + 1) + T
    axis = 1 if vertical else 2
    assert support.any(axis).sum().item() == 2  # one line per delta


def _random_case(entry, vertical, dtype):
    """inputs, fp64 reference, bound and the wrong references it must reject"""
    T, (N, H, W, C, Ko) = 7, SHAPES[2]
    rs, pad = _geom(T, vertical)
    x64, w64, dy64 = _data(2, (N, H, W, C), Ko, rs, dtype, pad, ints=False)
    if entry == "fwd":
        a64, K = x64, T * C

        def op(a, w, p=pad):
            return F.conv2d(a, w, None, 1, p)
    else:
        a64, K = dy64, T * Ko

        def op(a, w, p=pad):
            return conv2d_input((N, C, H, W), w, a, 1, p)
    ref = op(a64, w64)
    bound = _bound(ref, op(a64.abs(), w64.abs()), K, dtype)
    w0 = w64.clone()
    w0.view(Ko, C, T)[:, :, 3] = 0
    mutants = {"tap 3 zeroed": op(a64, w0),
               "orientation swapped": op(a64, w64.transpose(2, 3), pad[::-1]),
               "shifted one pixel": ref.roll(1, 2 if vertical else 3)}
    return a64, w64, ref, bound, mutants


@_dtypes
@_orient
@pytest.mark.parametrize("entry", ["fwd", "dgrad"])
def test_line_random(entry, vertical, dtype):
    ext = _ext()
    a64, w64, ref, bound, mutants = _random_case(entry, vertical, dtype)
    for what, m in mutants.items():
        assert bool(((m - ref).abs() > bound).any()), what
    fn = ext.lineconv_fwd if entry == "fwd" else ext.lineconv_dgrad
    # w 8-byte aligned: where a 100-class fc bias ahead in the bucket puts it
    got = fn(_dev(a64, dtype), _dev(w64, dtype, offset=4))
    err = (got.double().cpu() - ref).abs()
    print(f"lineconv_{entry} {'Tx1' if vertical else '1xT'} {dtype}: "
          f"max err / bound = {(err / bound).max().item():.4f}")
    assert bool((err <= bound).all())


@_dtypes
@pytest.mark.parametrize("rs,pad,stride", [((1, 7), (0, 3), 1), ((7, 1), (3, 0), 1),
                                           ((3, 3), (1, 0), 2), ((1, 3), (0, 0), 1)],
                         ids=["1x7", "7x1", "3x3p10s2", "1x3p00"])
def test_generic_per_axis_exact(rs, pad, stride, dtype):
    ext = _ext()
    x64, w64, dy64 = _data(3, (2, 9, 17, 24), 40, rs, dtype, pad, stride)
    x, w, dy = (_dev(t, dtype) for t in (x64, w64, dy64))
    _assert_bits(ext.conv_fwd_hw(x, w, stride, *pad),
                 F.conv2d(x64, w64, None, stride, pad), dtype)
    _assert_bits(ext.conv_dgrad_hw(dy, w, stride, *pad, 9, 17),
                 conv2d_input(x64.shape, w64, dy64, stride, pad), dtype)
    _assert_bits(ext.conv_wgrad_hw(x, dy, *rs, stride, *pad),
                 conv2d_weight(x64, w64.shape, dy64, stride, pad), dtype)


@_dtypes
@_orient
def test_conv2d_end_to_end(vertical, dtype, monkeypatch):
    """y, dx, dw through autograd: against fp64, the same bits on the generic
    per-axis path, and the same bits from replays of a captured graph.
    (2, 17, 5): two M-tiles, and a 7x1 halo of 30 rows, which is routed to
    the line kernel."""
    _ext()
    from dtmx.ops import functional as DF

    rs, pad = _geom(7, vertical)
    x64, w64, dy64 = _data(4, (2, 17, 5, 72), 136, rs, dtype, pad)
    x, w, dy = (_dev(t, dtype) for t in (x64, w64, dy64))
    assert DF._lineconv_routed(x, w, 1, *pad)
    x.requires_grad_(True)
    w.requires_grad_(True)

    def run():
        y = DF.conv2d(x, w, 1, pad)
        return (y.detach(),) + torch.autograd.grad(y, (x, w), dy)

    eager = run()
    for got, want in zip(eager, (F.conv2d(x64, w64, None, 1, pad),
                                 conv2d_input(x64.shape, w64, dy64, 1, pad),
                                 conv2d_weight(x64, w64.shape, dy64, 1, pad))):
        _assert_bits(got, want, dtype)
    monkeypatch.setattr(DF, "_FALLBACK", DF._FALLBACK | {"lineconv"})
    for got, want in zip(run(), eager):
        assert torch.equal(got, want)
    monkeypatch.undo()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # warm-up: every cached workspace exists before the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)


def test_inception_v3_factorized_step():
    import dtmx
    from dtmx.io import DataBatch
    from dtmx.models import get_symbol

    _ext()
    torch.manual_seed(0)
    shape = (2, 3, 299, 299)
    net = get_symbol("inception-v3", num_classes=100, factorized=True)
    mod = dtmx.Module(net, context=dtmx.gpu(0))
    mod.bind(data_shapes=[("data", shape)], label_shapes=[("softmax_label", (2,))],
             dtype=torch.bfloat16)
    mod.init_params()
    mod.init_optimizer(optimizer_params=(("learning_rate", 0.002), ("momentum", 0.9)))
    data = torch.randn(shape, dtype=torch.bfloat16, device="cuda:0").contiguous(
        memory_format=torch.channels_last)
    label = torch.randint(0, 100, (2,), device="cuda:0").float()
    batch = DataBatch(data=[data], label=[label])
    losses = []
    for _ in range(3):
        mod.forward_backward(batch)
        mod.update()
        losses.append(mod._loss.item())
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0] * 2.0, losses  # the zoo step test's form
