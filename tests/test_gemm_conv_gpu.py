"""Dense GEMM / implicit-GEMM convolution core (gemm_conv.hip): linear_*,
conv_fwd, conv_dgrad, conv_wgrad (default routing), conv_fwd_stats and
conv_dgrad_bnfuse at the smallest shapes where each mechanism can go wrong,
in bf16 and fp16.

Reference everywhere: the same operation in fp64 on the same inputs
(F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight, @).

Every case first asserts the kernel it is meant to reach through the
read-only routing bindings (gemm_plan, smallgrid_plan, wgrad_nt_plan,
wgrad_nt256_plan): the launchers call the same host functions.

Integer-exact cases: inputs are small integers, the helper asserts
max|a| * max|b| * K < 2^24 (K the contraction length), so every product and
every fp32 partial sum is exact in any order and the result must be bit-equal
to the fp64 result rounded once to the dtype. Where the epilogue rounds twice
(acc=: round(round(gemm) + acc) in EpiBF16::store_chunk / EpiBF16Scatter /
EpiBnBwd, and the bias add of EpiBF16::store_chunk, which also works on the
already rounded tile) the reference performs the same two roundings; the
intermediate sum is an integer below 2^24, hence exact in fp32 and fp64 alike.

Random cases: N(0,1) data against the derived bound of _bound(); see there.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
KERNEL = {256: "256f", 4: "tn4", 2: "tn2"}


def _ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dtmx.ops.hip import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(g, shape, lo, hi, dtype):
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g).to(dtype)


def _randn(g, shape, dtype, scale=1.0):
    return (scale * torch.randn(shape, device=DEV, generator=g)).to(dtype)


def _ceil(a, b):
    return -(-a // b)


def _out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _assert_exact_inputs(a, b, K):
    """the bound the integer-exact cases rely on"""
    assert a.abs().max().item() * b.abs().max().item() * K < 2 ** 24


def _rnd(t64, dtype):
    return t64.to(dtype).double()


def _assert_bits(got, want64, dtype):
    """got is bit-equal to the fp64 value rounded once to dtype"""
    assert got.dtype == dtype and got.shape == want64.shape
    torch.testing.assert_close(got.double(), _rnd(want64, dtype),
                               rtol=0, atol=0)


def _rows(t):
    """(N, C, H, W) -> [N*H*W][C], the GEMM's row-major view of an NHWC map"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _slab_sums(rows64):
    """fp64 column sums over rows [128 i, min(128 i + 128, M)) -> [ceil][C]"""
    M, C = rows64.shape
    T = _ceil(M, 128)
    padded = torch.zeros(T * 128, C, dtype=torch.float64, device=rows64.device)
    padded[:M] = rows64
    return padded.reshape(T, 128, C).sum(1)


def _assert_slab_exact(rows64, unit=1.0):
    """fp32 sums of multiples of `unit` are exact in any order while the sum
    of magnitudes stays below 2^24 units — checked on the data"""
    assert _slab_sums(rows64.abs()).max().item() / unit < 2 ** 24


# ------------------------------------------------------------------ routes

def _fwd_route(ext, N, C, H, W, Ko, R, S, stride, pad):
    """(kernel, split-K slices) conv_fwd / conv_fwd_stats reach"""
    P, Q = _out_hw(H, W, R, S, stride, pad)
    M = N * P * Q
    if C % 8:  # materialised im2col, K padded to 64, never small-grid
        return KERNEL[ext.gemm_plan(M, Ko, _ceil(R * S * C, 64) * 64)[0]], 1
    K = C if (R, S, stride, pad) == (1, 1, 1, 0) else R * S * C
    small, splitk = ext.smallgrid_plan(M, Ko, K)
    if small:
        plan = ext.gemm_plan(M, Ko, K, splitk, False)
        return "smallgrid-" + KERNEL[plan[0]], plan[3]
    return KERNEL[ext.gemm_plan(M, Ko, K)[0]], 1


def _dgrad_route(ext, N, C, H, W, Ko, R, S, stride, pad, acc=False,
                 fused=False):
    """(kernel, slices) conv_dgrad / conv_dgrad_bnfuse reach; Ko is padded
    to a multiple of 8, acc= and the fused epilogue never go small-grid"""
    P, Q = _out_hw(H, W, R, S, stride, pad)
    Kop = _ceil(Ko, 8) * 8
    if R == 1 and S == 1 and pad == 0 and C % 8 == 0:
        M, K = N * P * Q, Kop
        if stride > 1:
            return "scatter-" + KERNEL[ext.gemm_plan(M, C, K)[0]], 1
    else:
        M, K = N * H * W, R * S * Kop
    if not (acc or fused):
        small, splitk = ext.smallgrid_plan(M, C, K)
        if small:
            plan = ext.gemm_plan(M, C, K, splitk, False)
            return "smallgrid-" + KERNEL[plan[0]], plan[3]
    return KERNEL[ext.gemm_plan(M, C, K)[0]], 1


# ---------------------------------------------------------------- §1 linear

# name -> (M, N, K, bias, kernel)
LINEAR_FWD = {
    # M tail of 2 rows in the second M-tile, second K-tile 8 wide, BN = 64
    "tn2_tails": (130, 40, 72, False, 2),
    # 1 row / 8 columns in the second tiles, 4 K-tiles with an 8-wide last
    "tn4_tails": (129, 136, 200, False, 4),
    # N % 8 != 0: elementwise store tail, bias not read past N
    "n100_bias": (37, 100, 64, True, 4),
    # K % 8 != 0: pad_cols8
    "k13_pad": (50, 40, 13, False, 2),
    # a single K-tile: one 16-byte piece, and a full one
    "k8": (33, 72, 8, False, 4),
    "k64": (33, 72, 64, False, 4),
    # 256f: M = 39*256 + 72; 2, 3 and 5 K-tiles (minimum, odd, buffer parity);
    # N = 1000: last N-tile 232 wide
    "f256_k128": (10056, 1000, 128, False, 256),
    "f256_k192": (10056, 1000, 192, False, 256),
    "f256_k320": (10056, 1000, 320, False, 256),
    # N % 8 != 0 tail with bias on the 256² epilogue
    "f256_n1004_bias": (10056, 1004, 192, True, 256),
}


@_dtypes
@pytest.mark.parametrize("name", list(LINEAR_FWD))
def test_linear_fwd_exact(name, dtype):
    ext = _ext()
    M, N, K, bias, kernel = LINEAR_FWD[name]
    assert ext.gemm_plan(M, N, _ceil(K, 8) * 8)[0] == kernel
    g = _gen(1)
    x, w = _ints(g, (M, K), -4, 4, dtype), _ints(g, (N, K), -4, 4, dtype)
    _assert_exact_inputs(x, w, K)
    want = x.double() @ w.double().T
    b = None
    if bias:  # added to the already rounded tile, then rounded again
        b = torch.randint(-8, 9, (N,), device=DEV, generator=g).float()
        want = _rnd(want, dtype) + b.double()
    _assert_bits(ext.linear_fwd(x, w, b), want, dtype)


# name -> (M, N, K, kernel): dx = dy @ w is the GEMM (M, K, Npad)
LINEAR_DGRAD = {
    "n100_npad": (45, 100, 72, 4),  # N padded to 104, K-tile tail 40 wide
    "tn2": (130, 72, 40, 2),
}


@_dtypes
@pytest.mark.parametrize("name", list(LINEAR_DGRAD))
def test_linear_dgrad_exact(name, dtype):
    ext = _ext()
    M, N, K, kernel = LINEAR_DGRAD[name]
    assert ext.gemm_plan(M, K, _ceil(N, 8) * 8)[0] == kernel
    g = _gen(2)
    dy, w = _ints(g, (M, N), -4, 4, dtype), _ints(g, (N, K), -4, 4, dtype)
    _assert_exact_inputs(dy, w, N)
    _assert_bits(ext.linear_dgrad(dy, w), dy.double() @ w.double(), dtype)


# name -> (M, N, K, kernel): dw = dy^T @ x is the GEMM (N, K, Mpad)
LINEAR_WGRAD = {
    "m37_mpad": (37, 72, 136, 4),  # contraction padded to 40
    "tn2": (130, 136, 40, 2),      # 3 K-tiles, the last 8 wide after padding
}


@_dtypes
@pytest.mark.parametrize("name", list(LINEAR_WGRAD))
def test_linear_wgrad_exact(name, dtype):
    ext = _ext()
    M, N, K, kernel = LINEAR_WGRAD[name]
    assert ext.gemm_plan(N, K, _ceil(M, 8) * 8)[0] == kernel
    g = _gen(3)
    dy, x = _ints(g, (M, N), -4, 4, dtype), _ints(g, (M, K), -4, 4, dtype)
    _assert_exact_inputs(dy, x, M)
    _assert_bits(ext.linear_wgrad(dy, x), dy.double().T @ x.double(), dtype)


# -------------------------------------------------------------- §1 conv fwd

# name -> ((N, C, H, W, Ko, R, S, stride, pad), route); H != W everywhere
CONV_FWD = {
    # plain LDS-staged EpiBF16 store from the gather provider (5 K-tiles):
    # decode across image, row and tap boundaries, padding, stride-2 parity
    "g3x3_s1p1": ((3, 32, 9, 7, 72, 3, 3, 1, 1), "tn4"),
    "g3x3_s2p1": ((3, 32, 9, 7, 72, 3, 3, 2, 1), "tn4"),
    # 9 K-tiles: small-grid split-K (fp32 atomics + cast)
    "g3x3_s1p1_c64": ((3, 64, 9, 7, 72, 3, 3, 1, 1), "smallgrid-tn4"),
    "g3x3_s2p1_c64": ((3, 64, 9, 7, 72, 3, 3, 2, 1), "smallgrid-tn4"),
    # C % 8 == 0, C % 64 != 0: K-tiles straddle taps
    "g3x3_c24": ((3, 24, 9, 7, 72, 3, 3, 1, 1), "tn4"),
    "g3x3_p0": ((3, 32, 9, 7, 40, 3, 3, 1, 0), "tn2"),
    # 1x1 stride 2: gather provider with R = S = 1
    "g1x1_s2": ((2, 64, 9, 7, 72, 1, 1, 2, 0), "tn4"),
    # 1x1 stride 1: dense provider
    "d1x1_ko40": ((3, 32, 9, 7, 40, 1, 1, 1, 0), "tn2"),
    "d1x1_ko136": ((3, 32, 9, 7, 136, 1, 1, 1, 0), "tn4"),
    # non-square kernels: r and s decoded separately
    "g1x3_p0": ((3, 32, 9, 7, 72, 1, 3, 1, 0), "tn4"),
    "g3x1_p0": ((3, 32, 9, 7, 72, 3, 1, 1, 0), "tn4"),
    # C % 8 != 0: materialised im2col, K padded to 64
    "stem_c3_7x7": ((2, 3, 19, 13, 64, 7, 7, 2, 3), "tn2"),
    "lenet_c1_5x5": ((2, 1, 12, 9, 20, 5, 5, 1, 0), "tn2"),
    # 256f with the gather provider: M = 79*256 + 72, 160 tiles, 9 K-tiles
    "f256_g3x3": ((2, 64, 86, 118, 512, 3, 3, 1, 1), "256f"),
}


def _fwd_inputs(g, case, dtype, xr=4, wr=4):
    N, C, H, W, Ko, R, S, stride, pad = case
    x = _cl(_ints(g, (N, C, H, W), -xr, xr, dtype))
    w = _cl(_ints(g, (Ko, C, R, S), -wr, wr, dtype))
    _assert_exact_inputs(x, w, R * S * C)
    return x, w


@_dtypes
@pytest.mark.parametrize("name", list(CONV_FWD))
def test_conv_fwd_exact(name, dtype):
    ext = _ext()
    case, route = CONV_FWD[name]
    stride, pad = case[7:]
    got_route, slices = _fwd_route(ext, *case)
    assert got_route == route
    if route.startswith("smallgrid"):
        assert slices >= 2
    x, w = _fwd_inputs(_gen(4), case, dtype)
    want = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    _assert_bits(ext.conv_fwd(x, w, stride, pad), want, dtype)


# ------------------------------------------------------------ §1 conv dgrad

# name -> ((N, C, H, W, Ko, R, S, stride, pad), route without acc)
CONV_DGRAD = {
    "g3x3_s1p1": ((3, 72, 9, 7, 32, 3, 3, 1, 1), "tn4"),
    "g3x3_s2p1": ((3, 32, 9, 7, 32, 3, 3, 2, 1), "tn2"),
    # H = 10, W = 8, stride 2, pad 0: no output reaches the last input row or
    # column — exactly 0 on the plain and on the small-grid path
    "g3x3_s2p0": ((3, 32, 10, 8, 32, 3, 3, 2, 0), "tn2"),
    "g3x3_s2p0_ko64": ((3, 32, 10, 8, 64, 3, 3, 2, 0), "smallgrid-tn2"),
    "g3x3_s1p1_ko64": ((3, 72, 9, 7, 64, 3, 3, 1, 1), "smallgrid-tn4"),
    # Ko % 8 != 0: out channels padded to 24, at::copy weight transpose
    "g3x3_ko20": ((3, 32, 9, 7, 20, 3, 3, 1, 1), "tn2"),
    "g1x3_p0": ((3, 32, 9, 7, 32, 1, 3, 1, 0), "tn2"),
    "g3x1_p0": ((3, 32, 9, 7, 32, 3, 1, 1, 0), "tn2"),
    # 1x1 stride 1: dense provider
    "d1x1": ((3, 72, 9, 7, 40, 1, 1, 1, 0), "tn4"),
    # 1x1 stride 2: EpiBF16Scatter, odd and even H, W
    "s1x1_s2_9x7": ((2, 64, 9, 7, 72, 1, 1, 2, 0), "scatter-tn2"),
    "s1x1_s2_10x8": ((2, 64, 10, 8, 72, 1, 1, 2, 0), "scatter-tn2"),
    "s1x1_s2_c136": ((2, 136, 10, 8, 72, 1, 1, 2, 0), "scatter-tn4"),
    # 256f, dense and gather provider: M = 79*256 + 72
    "f256_d1x1": ((2, 512, 86, 118, 128, 1, 1, 1, 0), "256f"),
    "f256_g3x3": ((2, 512, 86, 118, 64, 3, 3, 1, 1), "256f"),
}
# cases also run with acc= (never small-grid: the LDS-staged epilogue)
CONV_DGRAD_ACC = {
    "g3x3_s1p1": "tn4", "g3x3_s2p0_ko64": "tn2", "d1x1": "tn4",
    "s1x1_s2_9x7": "scatter-tn2", "s1x1_s2_10x8": "scatter-tn2",
    "s1x1_s2_c136": "scatter-tn4", "f256_d1x1": "256f",
}


def _dgrad_inputs(g, case, dtype, dr=4, wr=4):
    N, C, H, W, Ko, R, S, stride, pad = case
    P, Q = _out_hw(H, W, R, S, stride, pad)
    dy = _cl(_ints(g, (N, Ko, P, Q), -dr, dr, dtype))
    w = _cl(_ints(g, (Ko, C, R, S), -wr, wr, dtype))
    _assert_exact_inputs(dy, w, R * S * Ko)
    return dy, w


def _dgrad64(dy, w, case):
    N, C, H, W, Ko, R, S, stride, pad = case
    return torch.nn.grad.conv2d_input((N, C, H, W), w.double(), dy.double(),
                                      stride=stride, padding=pad)


def _unreached(case):
    """[H][W] mask of input pixels no output tap reaches"""
    N, C, H, W, Ko, R, S, stride, pad = case
    one = torch.ones(1, 1, *_out_hw(H, W, R, S, stride, pad),
                     dtype=torch.float64, device=DEV)
    k = torch.ones(1, 1, R, S, dtype=torch.float64, device=DEV)
    return torch.nn.grad.conv2d_input((1, 1, H, W), k, one, stride=stride,
                                      padding=pad)[0, 0] == 0


@_dtypes
@pytest.mark.parametrize("name", list(CONV_DGRAD))
def test_conv_dgrad_exact(name, dtype):
    ext = _ext()
    case, route = CONV_DGRAD[name]
    N, C, H, W, Ko, R, S, stride, pad = case
    got_route, slices = _dgrad_route(ext, *case)
    assert got_route == route
    if route.startswith("smallgrid"):
        assert slices >= 2
    dy, w = _dgrad_inputs(_gen(5), case, dtype)
    dx = ext.conv_dgrad(dy, w, stride, pad, H, W)
    _assert_bits(dx, _dgrad64(dy, w, case), dtype)
    hole = _unreached(case)
    if stride > 1 and pad == 0:
        assert hole.any()  # s2: odd pixels (1x1) or the far row and column
        if R == 3:
            assert hole[H - 1].all() and hole[:, W - 1].all()
    assert (dx[:, :, hole] == 0).all()


@_dtypes
@pytest.mark.parametrize("name", list(CONV_DGRAD_ACC))
def test_conv_dgrad_acc_exact(name, dtype):
    """dx = round(round(gemm) + acc), in place in acc; pixels the scatter
    does not cover keep the acc value bit for bit"""
    ext = _ext()
    case = CONV_DGRAD[name][0]
    N, C, H, W, Ko, R, S, stride, pad = case
    assert _dgrad_route(ext, *case, acc=True) == (CONV_DGRAD_ACC[name], 1)
    g = _gen(6)
    dy, w = _dgrad_inputs(g, case, dtype, dr=2, wr=1)
    acc = _cl(_ints(g, (N, C, H, W), -64, 64, dtype))
    buf = acc.clone()
    dx = ext.conv_dgrad(dy, w, stride, pad, H, W, acc=buf)
    assert dx.data_ptr() == buf.data_ptr()
    want = _rnd(_dgrad64(dy, w, case), dtype) + acc.double()
    _assert_bits(dx, want, dtype)
    hole = _unreached(case)
    assert torch.equal(dx[:, :, hole], acc[:, :, hole])


# ------------------------------------------------------------ §1 conv wgrad

# name -> ((N, C, H, W, Ko, R, S, stride, pad), route); contraction N*P*Q
# route: (wm, nj, grouped) of gemm_nt_kernel, or the gemm_tn_kernel of the
# transposed-operand path (C % 8 != 0 or Ko % 8 != 0)
CONV_WGRAD = {
    # flat 64x256 tile; N*P*Q = 252: ragged last K-tile (60 rows)
    "wm1_flat": ((4, 32, 9, 7, 64, 3, 3, 1, 1), (1, 4, False)),
    # 128x64 tile (R*S*C = 64)
    "n64_tile": ((4, 64, 9, 7, 136, 1, 1, 1, 0), (2, 2, False)),
    # 128x128 tile, 4 tiles: ungrouped
    "wm2_ungrouped": ((4, 24, 9, 7, 136, 3, 3, 1, 1), (2, 4, False)),
    "wm2_s2": ((6, 24, 9, 7, 136, 3, 3, 2, 1), (2, 4, False)),
    # 6 tiles: XCD-grouped; 4 slices, so four of the eight dies idle
    "grouped_small": ((4, 32, 9, 7, 256, 3, 3, 1, 1), (2, 4, True)),
    # 961 K-tiles, the fewest at which rounding the slice count up to a
    # multiple of 8 changes the launch (81 x 12 K-tiles -> 88 x 11)
    "grouped_ns8": ((16, 32, 62, 62, 256, 3, 3, 1, 1), (2, 4, True)),
    # transposed operands through launch_gemm + EpiAtomicF32; N*P*Q % 8 != 0
    "stem_c3": ((2, 3, 19, 13, 64, 7, 7, 2, 3), 4),
    "stem_c3_ko20": ((2, 3, 19, 13, 20, 7, 7, 2, 3), 4),  # no workspace
    "ko20": ((3, 32, 9, 7, 20, 3, 3, 1, 1), 4),
}


def _wgrad_route(ext, N, C, H, W, Ko, R, S, stride, pad):
    P, Q = _out_hw(H, W, R, S, stride, pad)
    NPQ, RSC = N * P * Q, R * S * C
    if C % 8 == 0 and Ko % 8 == 0:
        assert not ext.wgrad_nt256_plan(Ko, RSC, NPQ)[0]
        wm, nj, depth, group, slices, kt_per = ext.wgrad_nt_plan(Ko, RSC, NPQ)
        assert depth == 2
        return (wm, nj, group), slices, kt_per
    Mpad = _ceil(NPQ, 8) * 8
    splitk = max(1, min(_ceil(Mpad, 64),
                        1024 // (_ceil(Ko, 128) * _ceil(RSC, 128))))
    plan = ext.gemm_plan(Ko, RSC, Mpad, splitk, False)
    return plan[0], plan[3], plan[4]


@_dtypes
@pytest.mark.parametrize("name", list(CONV_WGRAD))
def test_conv_wgrad_exact(name, dtype):
    """twice on different inputs: the second call sees the workspace the
    first one left behind"""
    ext = _ext()
    case, route = CONV_WGRAD[name]
    N, C, H, W, Ko, R, S, stride, pad = case
    P, Q = _out_hw(H, W, R, S, stride, pad)
    assert N * P * Q <= 2 ** 20
    got_route, slices, kt_per = _wgrad_route(ext, *case)
    assert got_route == route
    if name == "grouped_small":
        assert slices % 8 != 0
    if name == "grouped_ns8":
        ktiles = _ceil(N * P * Q, 64)
        plain = _ceil(ktiles, min(ktiles, 512 // 6))
        assert (slices, kt_per) == (88, 11) and plain == 12
    if name in ("stem_c3", "stem_c3_ko20", "ko20"):
        assert (N * P * Q) % 8 != 0
    g = _gen(7)
    for _ in range(2):
        x = _cl(_ints(g, (N, C, H, W), -4, 4, dtype))
        dy = _cl(_ints(g, (N, Ko, P, Q), -4, 4, dtype))
        _assert_exact_inputs(x, dy, N * P * Q)
        want = torch.nn.grad.conv2d_weight(
            x.double(), (Ko, C, R, S), dy.double(), stride=stride, padding=pad)
        _assert_bits(ext.conv_wgrad(x, dy, R, S, stride, pad), want, dtype)
    for ko, rsc, mx in ext.wgrad_ws_stats():
        assert mx == 0.0, (ko, rsc, mx)


# --------------------------------------------------- §2 fused epilogues

# name -> ((N, C, H, W, Ko, R, S, stride, pad), route); M = N*P*Q
FWD_STATS = {
    # M = 189: last slab 61 rows
    "tn4_g3x3": ((3, 32, 9, 7, 72, 3, 3, 1, 1), "tn4"),
    "tn2_g3x3_ko40": ((3, 32, 9, 7, 40, 3, 3, 1, 1), "tn2"),
    # M = 286: last slab 30 rows
    "m286": ((2, 32, 11, 13, 72, 3, 3, 1, 1), "tn4"),
    "m286_d1x1": ((2, 32, 11, 13, 40, 1, 1, 1, 0), "tn2"),
    # M = 126: one partial slab
    "m126": ((2, 32, 9, 7, 72, 3, 3, 1, 1), "tn4"),
    # N tail: second N-tile 8 wide
    "ko136": ((3, 32, 9, 7, 136, 1, 1, 1, 0), "tn4"),
    "s2": ((3, 32, 9, 7, 72, 3, 3, 2, 1), "tn4"),
    # 256f; M % 256 = 72: the h = 1 half of the last M-tile has no slab row
    "f256_m72": ((2, 128, 86, 118, 512, 1, 1, 1, 0), "256f"),
    # M % 256 = 200: that half is partial
    "f256_m200": ((2, 128, 92, 111, 512, 1, 1, 1, 0), "256f"),
    "f256_m0": ((2, 128, 80, 128, 512, 1, 1, 1, 0), "256f"),
    # gather provider on the 256² epilogue, M % 256 = 72
    "f256_g3x3_m72": ((2, 64, 86, 118, 512, 3, 3, 1, 1), "256f"),
}


@_dtypes
@pytest.mark.parametrize("name", list(FWD_STATS))
def test_conv_fwd_stats_slabs_exact(name, dtype):
    ext = _ext()
    case, route = FWD_STATS[name]
    N, C, H, W, Ko, R, S, stride, pad = case
    assert _fwd_route(ext, *case) == (route, 1)
    P, Q = _out_hw(H, W, R, S, stride, pad)
    M = N * P * Q
    if name.startswith("f256"):
        assert M % 256 == {"m72": 72, "m200": 200, "m0": 0}[name.split("_")[-1]]
    x, w = _fwd_inputs(_gen(8), case, dtype, xr=2, wr=1)
    want = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    y, psum, psumsq = ext.conv_fwd_stats(x, w, stride, pad)
    _assert_bits(y, want, dtype)
    rows = _rows(_rnd(want, dtype))  # the slabs sum the STORED values
    _assert_slab_exact(rows)
    _assert_slab_exact(rows * rows)
    for slab, ref in ((psum, _slab_sums(rows)),
                      (psumsq, _slab_sums(rows * rows))):
        assert slab.dtype == torch.float32
        assert tuple(slab.shape) == (_ceil(M, 128), Ko)
        torch.testing.assert_close(slab.double(), ref, rtol=0, atol=0)


@_dtypes
def test_conv_fwd_stats_smallgrid_fallback(dtype):
    """a small-grid shape is not fusable: empty slabs, y as conv_fwd"""
    ext = _ext()
    case = (3, 64, 9, 7, 72, 3, 3, 1, 1)
    assert _fwd_route(ext, *case)[0] == "smallgrid-tn4"
    x, w = _fwd_inputs(_gen(9), case, dtype)
    y, psum, psumsq = ext.conv_fwd_stats(x, w, 1, 1)
    assert psum.numel() == 0 and psumsq.numel() == 0
    _assert_bits(y, F.conv2d(x.double(), w.double(), padding=1), dtype)
    assert torch.equal(y, ext.conv_fwd(x, w, 1, 1))


# name -> ((N, C, H, W, Ko, R, S, stride, pad), route); M = N*H*W, C = the
# BatchNorm channel count (the GEMM's N)
BNFUSE = {
    "tn2_d1x1": ((3, 40, 9, 7, 32, 1, 1, 1, 0), "tn2"),
    "tn4_d1x1": ((3, 72, 9, 7, 32, 1, 1, 1, 0), "tn4"),
    "tn4_g3x3": ((3, 72, 9, 7, 32, 3, 3, 1, 1), "tn4"),
    "tn2_g3x3_s2": ((3, 40, 9, 7, 32, 3, 3, 2, 1), "tn2"),
    # M = 286 (last slab 30 rows), N tail 8 wide
    "m286_c136": ((2, 136, 11, 13, 32, 3, 3, 1, 1), "tn4"),
    # 256f at the three M % 256 classes (72: the slab-overrun shape)
    "f256_m72": ((2, 512, 86, 118, 128, 1, 1, 1, 0), "256f"),
    "f256_m200": ((2, 512, 92, 111, 128, 1, 1, 1, 0), "256f"),
    "f256_m0": ((2, 512, 80, 128, 128, 1, 1, 1, 0), "256f"),
    "f256_g3x3_m72": ((2, 512, 86, 118, 64, 3, 3, 1, 1), "256f"),
}


def _pack_mask(y):
    """bit e of byte (m, n / 8) = !(y[m][n + e] <= 0)"""
    keep = ~(_rows(y).float() <= 0)
    M, C = keep.shape
    bits = keep.reshape(M, C // 8, 8).to(torch.int32)
    weights = 2 ** torch.arange(8, device=y.device, dtype=torch.int32)
    return (bits * weights).sum(-1).to(torch.uint8).contiguous()


@_dtypes
@pytest.mark.parametrize("name", list(BNFUSE))
def test_conv_dgrad_bnfuse_slabs_exact(name, dtype):
    """f = round(gemm) [+ acc], zeroed where y <= 0 (not rounded again);
    g = round(f); pdb[i] = sum f, pdg[i] = sum f * (xin - mean) * invstd over
    the rows of slab i. mean: small integers, invstd: powers of two, so every
    term is a multiple of 1/2 and the fp32 sums are exact."""
    ext = _ext()
    case, route = BNFUSE[name]
    N, C, H, W, Ko, R, S, stride, pad = case
    assert _dgrad_route(ext, *case, fused=True) == (route, 1)
    M = N * H * W
    if name.startswith("f256"):
        assert M % 256 == {"m72": 72, "m200": 200, "m0": 0}[name.split("_")[-1]]
    g = _gen(10)
    dy, w = _dgrad_inputs(g, case, dtype, dr=2, wr=1)
    acc = _cl(_ints(g, (N, C, H, W), -16, 16, dtype))
    xin = _cl(_ints(g, (N, C, H, W), -3, 3, dtype))
    y = _cl(_ints(g, (N, C, H, W), -1, 1, dtype))  # -1, 0 (exact zeros), 1
    mean = torch.randint(-2, 3, (C,), device=DEV, generator=g).float()
    invstd = 2.0 ** torch.randint(-1, 2, (C,), device=DEV, generator=g).float()
    mask = _pack_mask(y)
    gemm = _rnd(_dgrad64(dy, w, case), dtype)
    xhat = (xin.double() - mean.double().view(1, C, 1, 1)) \
        * invstd.double().view(1, C, 1, 1)
    for with_acc in (False, True):
        f = gemm + acc.double() if with_acc else gemm
        f = torch.where(y.double() <= 0, torch.zeros_like(f), f)
        db, dg = _rows(f), _rows(f * xhat)
        _assert_slab_exact(db)
        _assert_slab_exact(dg, unit=0.5)
        for packed in (False, True):
            out, pdb, pdg = ext.conv_dgrad_bnfuse(
                dy, w, stride, pad, H, W, acc.clone() if with_acc else None,
                y, xin, mean, invstd, mask if packed else None)
            _assert_bits(out, f, dtype)
            for slab, ref in ((pdb, _slab_sums(db)), (pdg, _slab_sums(dg))):
                assert slab.dtype == torch.float32
                assert tuple(slab.shape) == (_ceil(M, 128), C)
                torch.testing.assert_close(slab.double(), ref, rtol=0, atol=0)


# ------------------------------------------------- §3 random values, bound

def _ulp(v, dtype):
    """spacing of dtype at magnitude v >= 0 (fp64 tensor)"""
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(v.clamp_min(2.0 ** emin))[1] - 1  # floor(log2 v)
    return torch.ldexp(torch.ones_like(v), e - p)


def _bound(ref, S, K, dtype, first=None):
    """Any summation order with fp32 accumulation: each of the at most K
    roundings of a partial sum costs at most 2^-24 of a partial sum of
    magnitudes, so |acc32 - ref| <= a = K * 2^-24 * S with S = sum|a*b|
    (split-K atomic passes are further additions of the same sum and count
    among the K). The final rounding adds half an ulp of the dtype at the
    largest magnitude the fp32 value can have, |ref| + a.
    first: the GEMM part of a twice-rounded result (ref = first + acc): the
    half ulp of the first rounding is taken at |first| + a, and the second
    one at |ref| + everything before it."""
    a = K * 2.0 ** -24 * S
    if first is None:
        return a + 0.5 * _ulp(ref.abs() + a, dtype)
    b = a + 0.5 * _ulp(first.abs() + a, dtype)
    return b + 0.5 * _ulp(ref.abs() + b, dtype)


_ratios = {}


def _assert_within(tag, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    _ratios[tag] = ratio
    print(f"{tag}: max err / bound = {ratio:.4f}")
    assert bool((err <= bound).all()), (tag, ratio)


def _assert_rejects(ref, bound, mutants):
    """the bound is not vacuous: each wrong fp64 result lies outside it"""
    for what, m in mutants.items():
        assert m.shape == ref.shape
        assert bool(((m - ref).abs() > bound).any()), what


def _swap_hw(t):
    return t.transpose(2, 3)


def _tag(name, dtype):
    return f"{name}[{'bf16' if dtype == torch.bfloat16 else 'fp16'}]"


# name -> (entry point, (M, N, K), kernel)
RANDOM_LINEAR = {
    "linear_fwd_tn4": ("fwd", (129, 136, 200), 4),
    "linear_fwd_256f": ("fwd", (10056, 1000, 192), 256),
    "linear_dgrad_tn2": ("dgrad", (130, 72, 40), 2),
    "linear_wgrad_tn4": ("wgrad", (37, 72, 136), 4),
}


@_dtypes
@pytest.mark.parametrize("name", list(RANDOM_LINEAR))
def test_linear_random_within_bound(name, dtype):
    ext = _ext()
    op, (M, N, K), kernel = RANDOM_LINEAR[name]
    g = _gen(11)
    if op == "fwd":
        a, b, Kc = _randn(g, (M, K), dtype), _randn(g, (N, K), dtype), K
        assert ext.gemm_plan(M, N, K)[0] == kernel
        f64 = lambda a, b: a @ b.T
        got = ext.linear_fwd(a, b, None)
    elif op == "dgrad":
        a, b, Kc = _randn(g, (M, N), dtype), _randn(g, (N, K), dtype), N
        assert ext.gemm_plan(M, K, _ceil(N, 8) * 8)[0] == kernel
        f64 = lambda a, b: a @ b
        got = ext.linear_dgrad(a, b)
    else:
        a, b, Kc = _randn(g, (M, N), dtype), _randn(g, (M, K), dtype), M
        assert ext.gemm_plan(N, K, _ceil(M, 8) * 8)[0] == kernel
        f64 = lambda a, b: a.T @ b
        got = ext.linear_wgrad(a, b)
    ref = f64(a.double(), b.double())
    bound = _bound(ref, f64(a.double().abs(), b.double().abs()), Kc, dtype)
    # self-check: one contraction index dropped; rows / columns off by one
    a0 = a.double().clone()
    if op == "wgrad":
        a0[0] = 0
    else:
        a0[:, 0] = 0
    _assert_rejects(ref, bound, {
        "one k dropped": f64(a0, b.double()),
        "rows shifted": torch.roll(ref, 1, 0),
        "columns shifted": torch.roll(ref, 1, 1),
    })
    _assert_within(_tag(name, dtype), got, ref, bound)


# name -> (entry point, (N, C, H, W, Ko, R, S, stride, pad), route, w scale)
RANDOM_CONV = {
    "conv_fwd_tn4": ("fwd", (3, 32, 9, 7, 72, 3, 3, 1, 1), "tn4", 0.1),
    "conv_fwd_smallgrid": ("fwd", (3, 64, 9, 7, 72, 3, 3, 2, 1),
                           "smallgrid-tn4", 0.1),
    "conv_fwd_256f": ("fwd", (2, 64, 86, 118, 512, 3, 3, 1, 1), "256f", 0.05),
    "conv_fwd_stats_tn2": ("fwd_stats", (3, 32, 9, 7, 40, 3, 3, 1, 1), "tn2",
                           0.1),
    "conv_dgrad_tn2": ("dgrad", (3, 32, 9, 7, 32, 3, 3, 2, 1), "tn2", 0.1),
    "conv_dgrad_256f": ("dgrad", (2, 512, 86, 118, 64, 3, 3, 1, 1), "256f",
                        0.1),
    "conv_dgrad_scatter_acc": ("dgrad_acc", (2, 64, 10, 8, 72, 1, 1, 2, 0),
                               "scatter-tn2", 0.1),
    "conv_dgrad_bnfuse_tn4": ("bnfuse", (3, 72, 9, 7, 32, 3, 3, 1, 1), "tn4",
                              0.1),
    "conv_wgrad_nt_grouped": ("wgrad", (4, 32, 9, 7, 256, 3, 3, 1, 1),
                              (2, 4, True), 0.1),
    "conv_wgrad_nt_flat": ("wgrad", (4, 32, 9, 7, 64, 3, 3, 1, 1),
                           (1, 4, False), 0.1),
}


@_dtypes
@pytest.mark.parametrize("name", list(RANDOM_CONV))
def test_conv_random_within_bound(name, dtype):
    ext = _ext()
    op, case, route, wscale = RANDOM_CONV[name]
    N, C, H, W, Ko, R, S, stride, pad = case
    P, Q = _out_hw(H, W, R, S, stride, pad)
    g = _gen(12)
    first = None
    if op in ("fwd", "fwd_stats"):
        assert _fwd_route(ext, *case)[0] == route
        a = _cl(_randn(g, (N, C, H, W), dtype))
        b = _cl(_randn(g, (Ko, C, R, S), dtype, wscale))
        Kc = R * S * C
        f64 = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)
        got = (ext.conv_fwd(a, b, stride, pad) if op == "fwd"
               else ext.conv_fwd_stats(a, b, stride, pad)[0])
        b0 = b.double().clone()
        b0[:, :, 0, 0] = 0
        tap = f64(a.double(), b0)
        swapped = _swap_hw(f64(_swap_hw(a.double()), b.double()))
    elif op == "wgrad":
        assert _wgrad_route(ext, *case)[0] == route
        a = _cl(_randn(g, (N, C, H, W), dtype))
        b = _cl(_randn(g, (N, Ko, P, Q), dtype, wscale))
        Kc = N * P * Q
        f64 = lambda a, b: torch.nn.grad.conv2d_weight(
            a, (Ko, C, R, S), b, stride=stride, padding=pad)
        got = ext.conv_wgrad(a, b, R, S, stride, pad)
        tap = f64(a.double(), b.double()).clone()
        tap[:, :, 0, 0] = 0
        # x and dy both transposed: dw with r and s exchanged
        swapped = f64(_swap_hw(a.double()), _swap_hw(b.double()))
    else:
        assert _dgrad_route(ext, *case, acc=op == "dgrad_acc",
                            fused=op == "bnfuse")[0] == route
        a = _cl(_randn(g, (N, Ko, P, Q), dtype))
        b = _cl(_randn(g, (Ko, C, R, S), dtype, wscale))
        Kc = R * S * Ko
        f64 = lambda a, b, hw=(H, W): torch.nn.grad.conv2d_input(
            (N, C, *hw), b, a, stride=stride, padding=pad)
        b0 = b.double().clone()
        b0[:, :, 0, 0] = 0
        tap = f64(a.double(), b0)
        swapped = _swap_hw(f64(_swap_hw(a.double()), b.double(), (W, H)))
        if op == "dgrad":
            got = ext.conv_dgrad(a, b, stride, pad, H, W)
    ref = f64(a.double(), b.double())
    S_abs = f64(a.double().abs(), b.double().abs())
    # swapped: the same conv with H and W swapped (operands and result
    # transposed). A 1x1 conv commutes with the transpose, so there that
    # mutant IS the reference and is left out.
    mutants = {"tap (0, 0) zeroed": tap,
               "shifted by one pixel": torch.roll(ref, 1, 3)}
    if (R, S) != (1, 1):
        mutants["H and W swapped"] = swapped
    if op == "dgrad_acc":
        acc = _cl(_randn(g, (N, C, H, W), dtype))
        got = ext.conv_dgrad(a, b, stride, pad, H, W, acc=acc.clone())
        first, ref = ref, ref + acc.double()
        mutants = {k: m + acc.double() for k, m in mutants.items()}
    if op == "bnfuse":
        y = _cl(_ints(g, (N, C, H, W), -1, 1, dtype))
        xin = _cl(_randn(g, (N, C, H, W), dtype))
        mean = torch.zeros(C, device=DEV)
        invstd = torch.ones(C, device=DEV)
        got = ext.conv_dgrad_bnfuse(a, b, stride, pad, H, W, None, y, xin,
                                    mean, invstd)[0]
        keep = (y.double() > 0).double()
        ref, S_abs = ref * keep, S_abs * keep
        mutants = {k: m * keep for k, m in mutants.items()}
        assert bool((got.double()[keep == 0] == 0).all())
    bound = _bound(ref, S_abs, Kc, dtype, first=first)
    _assert_rejects(ref, bound, mutants)
    _assert_within(_tag(name, dtype), got, ref, bound)
