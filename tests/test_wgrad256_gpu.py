"""gemm256nt_kernel (256x256 contraction-major wgrad GEMM) reached through
ext.conv_wgrad_nt256 at the smallest shapes where each mechanism can go wrong.

Reference everywhere: torch.nn.grad.conv2d_weight in fp64 on the same inputs.
Integer inputs in [-4, 4] with N*P*Q <= 2^20 make every product and every
fp32 partial sum exact in any order (|sum| <= 16 * N*P*Q < 2^24), so the
result must be bit-equal to the 16-bit-rounded fp64 reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dtmx.ops.hip import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def _int_inputs(N, C, Ko, H, W, R, stride, pad, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    P, Q = _out_hw(H, W, R, stride, pad)
    x = _cl(torch.randint(-4, 5, (N, C, H, W), device="cuda", generator=g)
            .to(dtype))
    dy = _cl(torch.randint(-4, 5, (N, Ko, P, Q), device="cuda", generator=g)
             .to(dtype))
    return x, dy


def _ref64(x, dy, R, stride, pad):
    Ko, C = dy.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(
        x.double(), (Ko, C, R, R), dy.double(), stride=stride, padding=pad)


def _check_exact(ext, x, dy, R, stride, pad, splitk, group, ref=None):
    assert x.shape[0] * dy.shape[2] * dy.shape[3] <= 2 ** 20
    dw = ext.conv_wgrad_nt256(x, dy, R, R, stride, pad, splitk, group)
    if ref is None:
        ref = _ref64(x, dy, R, stride, pad)
    assert dw.shape == ref.shape and dw.dtype == x.dtype
    torch.testing.assert_close(dw.double(), ref.to(x.dtype).double(),
                               rtol=0, atol=0)


# (N, C, Ko, H, W, R, stride, pad) -> what it exercises
EXACT_SHAPES = {
    # one full tile, ONE K-tile: the prologue is 4 parts, not 6
    "one_ktile": (1, 256, 256, 8, 8, 1, 1, 0),
    # 98 rows: 2 K-tiles, the last with 34 rows
    "ktiles2_ragged": (2, 256, 256, 7, 7, 1, 1, 0),
    # 147 rows: 3 K-tiles (buffer parity, boundary waits)
    "ktiles3_ragged": (3, 256, 256, 7, 7, 1, 1, 0),
    # 294 rows: 5 K-tiles, the last with 38 rows
    "ktiles5_ragged": (6, 256, 256, 7, 7, 1, 1, 0),
    # RSC = 360: second n-tile has 104 columns; Ko = 264: second m-tile 8 rows
    "partial_tiles": (2, 40, 264, 7, 7, 3, 1, 1),
    # gather decode across image/row/tap boundaries with padding, H != W
    "gather_s1": (3, 32, 256, 9, 7, 3, 1, 1),
    "gather_s2": (3, 32, 256, 9, 7, 3, 2, 1),
    # 1x1 stride-2 downsample
    "downsample": (2, 256, 512, 14, 14, 1, 2, 0),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(EXACT_SHAPES))
def test_nt256_exact_on_integer_inputs(name, dtype):
    ext = _ext()
    N, C, Ko, H, W, R, stride, pad = EXACT_SHAPES[name]
    x, dy = _int_inputs(N, C, Ko, H, W, R, stride, pad, dtype, seed=1)
    _check_exact(ext, x, dy, R, stride, pad, 1, False)


_SPLITK_CASE = (16, 32, 256, 9, 7, 3, 1, 1)  # N*P*Q = 1008: 16 K-tiles
_splitk_cache = {}


def _splitk_inputs(dtype):
    """inputs + fp64 reference of the split-K shape, computed once per dtype
    and shared (read-only) by the eight (splitk, group) cases"""
    if dtype not in _splitk_cache:
        x, dy = _int_inputs(*_SPLITK_CASE, dtype, seed=2)
        R, stride, pad = _SPLITK_CASE[5:]
        _splitk_cache[dtype] = (x, dy, _ref64(x, dy, R, stride, pad))
    return _splitk_cache[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("splitk", [1, 3, 5, 16])
def test_nt256_splitk_and_grouping_exact(splitk, group, dtype):
    """1 slice, uneven slices (3 -> 6+6+4, 5 -> 4+4+4+4), one K-tile per
    slice; grouped launch with slice counts that are (16) and are not
    (1, 3, 4) a multiple of 8 — the idle slots of the last die round must
    exit before touching the workspace."""
    ext = _ext()
    x, dy, ref = _splitk_inputs(dtype)
    R, stride, pad = _SPLITK_CASE[5:]
    _check_exact(ext, x, dy, R, stride, pad, splitk, bool(group), ref=ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_nt256_workspace_rezero(dtype):
    """two calls in a row on different inputs with the same (Ko, RSC) share
    the persistent fp32 workspace: the second must be exact too"""
    ext = _ext()
    shape = (4, 32, 256, 9, 7, 3, 1, 1)
    R, stride, pad = shape[5:]
    xa, dya = _int_inputs(*shape, dtype, seed=3)
    xb, dyb = _int_inputs(*shape, dtype, seed=4)
    assert not torch.equal(xa, xb)
    _check_exact(ext, xa, dya, R, stride, pad, 2, False)
    _check_exact(ext, xb, dyb, R, stride, pad, 2, True)
    # and the workspaces are all zero again
    for ko, rsc, mx in ext.wgrad_ws_stats():
        assert mx == 0.0, (ko, rsc, mx)


def test_nt256_random_inputs_error_vs_old_kernel():
    """x ~ N(0,1), dy ~ 0.1 N(0,1), rounded to bf16 first; C = Ko = 256, 3x3,
    N = 8, 14x14 (25 K-tiles). The fp32 split-K sums of both kernels, BEFORE
    the 16-bit rounding (ext.conv_wgrad_acc32), are compared with the fp64
    reference, per element in units of sum|dy*x| * 2^-24 (sum|dy*x| from the
    same fp64 conv on |x|, |dy|): the new kernel's largest error may exceed
    the old kernel's by at most 2x (both sum fp32 partials in an unspecified
    order). The old kernel runs in-process through the binding's nt256=False
    path (the gemm_nt_kernel routing with its own split-K), whatever the
    gate says.

    Measured on MI355X (bf16), two runs (the atomic order varies): new 0.645
    and 0.618, old 0.671 and 0.509 units."""
    ext = _ext()
    g = torch.Generator(device="cuda").manual_seed(5)
    dtype = torch.bfloat16
    N, C, Ko, H = 8, 256, 256, 14
    x = _cl(torch.randn(N, C, H, H, device="cuda", generator=g).to(dtype))
    dy = _cl((0.1 * torch.randn(N, Ko, H, H, device="cuda", generator=g))
             .to(dtype))

    def flat(t):  # (Ko, C, R, S) -> [Ko][(r, s, c)]
        return t.permute(0, 2, 3, 1).reshape(Ko, -1)

    ref = flat(_ref64(x, dy, 3, 1, 1))
    unit = flat(_ref64(x.abs(), dy.abs(), 3, 1, 1)) * 2.0 ** -24
    new32 = ext.conv_wgrad_acc32(x, dy, 3, 3, 1, 1, True, 4, False)
    old32 = ext.conv_wgrad_acc32(x, dy, 3, 3, 1, 1, False, 1, False)
    assert new32.dtype == torch.float32 and old32.dtype == torch.float32
    e_new = ((new32.double() - ref).abs() / unit).max().item()
    e_old = ((old32.double() - ref).abs() / unit).max().item()
    print(f"max fp32 error in units of sum|dy*x|*2^-24: new {e_new:.3f} "
          f"old {e_old:.3f}")
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    for ko, rsc, mx in ext.wgrad_ws_stats():
        assert mx == 0.0, (ko, rsc, mx)


def test_nt256_envelope_checks():
    ext = _ext()
    bf = torch.bfloat16
    x = _cl(torch.zeros(1, 256, 8, 8, device="cuda", dtype=bf))
    dy = _cl(torch.zeros(1, 256, 8, 8, device="cuda", dtype=bf))
    with pytest.raises(RuntimeError, match=r"C % 8 == 0"):
        ext.conv_wgrad_nt256(_cl(torch.zeros(1, 12, 8, 8, device="cuda",
                                             dtype=bf)), dy, 1, 1, 1, 0, 1,
                             False)
    with pytest.raises(RuntimeError, match=r"must be CUDA tensors"):
        ext.conv_wgrad_nt256(x.cpu(), dy, 1, 1, 1, 0, 1, False)
    with pytest.raises(RuntimeError, match=r"1 <= splitk <= ceil"):
        ext.conv_wgrad_nt256(x, dy, 1, 1, 1, 0, 0, False)
    with pytest.raises(RuntimeError, match=r"1 <= splitk <= ceil"):
        ext.conv_wgrad_nt256(x, dy, 1, 1, 1, 0, 2, False)  # 1 K-tile
