"""gemm_nts_kernel (streaming narrow-tile contraction-major wgrad GEMM) reached
through ext.conv_wgrad_narrow at the smallest shapes where each mechanism can
go wrong, in bf16 and fp16.

Reference everywhere: torch.nn.grad.conv2d_weight in fp64 on the CPU. Integer
inputs in [-4, 4] with N*P*Q <= 2^20 make every product and every fp32 partial
sum exact in any order (|sum| <= 16 * N*P*Q < 2^24), so the result must be
bit-equal to the fp64 reference rounded once.

The routing test at the end runs on the CPU through the plan binding only."""
import pytest
import torch

DTYPES = [torch.bfloat16, torch.float16]
_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
RING_DEPTH = 3  # K-tile buffers in the kernel's LDS ring


def _ext():
    from dtmx.ops.hip import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ceil(a, b):
    return -(-a // b)


def _out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def _ref64(x, dy, R, stride, pad):
    """fp64 on the CPU, (Ko, C, R, R)"""
    Ko, C = dy.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(
        x.double().cpu(), (Ko, C, R, R), dy.double().cpu(), stride=stride,
        padding=pad)


def _int_inputs(N, H, W, C, Ko, R, stride, pad, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    P, Q = _out_hw(H, W, R, stride, pad)
    x = _cl(torch.randint(-4, 5, (N, C, H, W), generator=g).to(dtype).cuda())
    dy = _cl(torch.randint(-4, 5, (N, Ko, P, Q), generator=g).to(dtype).cuda())
    return x, dy


# name -> ((N, H, W), C, Ko, R, stride, pad, tile class)
EXACT = {
    # one piece per operand; N*P*Q = 35 is less than one K-tile, so the
    # prologue is longer than the loop
    "one_piece": ((1, 5, 7), 8, 8, 1, 1, 0, "64x256"),
    # exactly 2 K-tiles; 64x256 tile with an R*S*C tail
    "ktiles2": ((2, 8, 8), 64, 64, 1, 1, 0, "64x256"),
    # R*S*C = 576 is 2.25 n-tiles; H != W; K tail 297 % 64; padding taps
    "l1_conv2": ((3, 9, 11), 64, 64, 3, 1, 1, "64x256"),
    # stem geometry: R*S*C = 392, stride 2, taps that cross both borders
    "stem": ((2, 13, 9), 8, 64, 7, 2, 3, "64x256"),
    # 128x256 tile; C is not a multiple of 64; stride 2
    "l2_conv2_s2": ((2, 9, 9), 72, 128, 3, 2, 1, "128x256"),
    # Ko exactly the tile width (the l1.1/2 conv1 class), K tail 315 % 64
    "l1_conv1": ((5, 7, 9), 256, 64, 1, 1, 0, "64x256"),
    # 256x128 tile with a Ko tail (520 = 2 * 256 + 8)
    "l2_conv3": ((4, 10, 10), 128, 520, 1, 1, 0, "256x128"),
    # 256x64 tile with a Ko tail
    "l1_conv3": ((4, 10, 10), 64, 264, 1, 1, 0, "256x64"),
    # ring wrap-around and the last partial K-tile
    "ring_exact": ((1, 1, RING_DEPTH * 64), 64, 64, 1, 1, 0, "64x256"),
    "ring_plus1": ((1, 1, RING_DEPTH * 64 + 1), 64, 64, 1, 1, 0, "64x256"),
    "ring_next": ((1, 1, (RING_DEPTH + 1) * 64 + 63), 64, 64, 1, 1, 0,
                  "64x256"),
}


def _splitks(ktiles):
    """1, 2 and one K-tile per slice; with 5 or more K-tiles also 3, whose
    last slice is short (5 -> 2+2+1, 7 -> 3+3+1)"""
    ks = {1, min(2, ktiles), ktiles}
    if ktiles >= 5:
        assert ktiles % _ceil(ktiles, 3) != 0
        ks.add(3)
    return sorted(ks)


@pytest.mark.gpu
@_dtypes
@pytest.mark.parametrize("name", list(EXACT))
def test_narrow_exact_on_integer_inputs(name, dtype):
    ext = _ext()
    (N, H, W), C, Ko, R, stride, pad, cls = EXACT[name]
    P, Q = _out_hw(H, W, R, stride, pad)
    NPQ = N * P * Q
    assert NPQ <= 2 ** 20
    assert ext.wgrad_narrow_plan(Ko, R * R * C, NPQ)[1] == cls
    x, dy = _int_inputs(N, H, W, C, Ko, R, stride, pad, dtype, seed=1)
    want = _ref64(x, dy, R, stride, pad).to(dtype).double()
    for splitk in _splitks(_ceil(NPQ, 64)):
        for group in (False, True):
            # twice in a row: the persistent workspace must be zero again
            for _ in range(2):
                dw = ext.conv_wgrad_narrow(x, dy, R, R, stride, pad, splitk,
                                           group)
                assert dw.shape == want.shape and dw.dtype == dtype
                torch.testing.assert_close(
                    dw.double().cpu(), want, rtol=0, atol=0,
                    msg=lambda m: f"splitk={splitk} group={group}: {m}")
    for ko, rsc, mx in ext.wgrad_ws_stats():
        assert mx == 0.0, (ko, rsc, mx)


# one random case per tile class at (2, 9, 11): (C, Ko, R, pad). 3x3 pad 1
# where the class can be reached; R*S*C <= 64 with C % 8 == 0 cannot hold a
# 3x3 window (9 * 8 = 72), so the 256x64 class runs 1x1.
RANDOM = {
    "64x256": (64, 64, 3, 1),
    "128x256": (32, 128, 3, 1),
    "256x128": (8, 264, 3, 1),
    "256x64": (64, 264, 1, 0),
}


@pytest.mark.gpu
@_dtypes
@pytest.mark.parametrize("cls", list(RANDOM))
def test_narrow_random_inputs_within_fp32_bound(cls, dtype):
    """x, dy ~ N(0,1) rounded to the 16-bit dtype. The fp32 split-K sums
    before the 16-bit rounding against fp64, per element:
        |got - ref64| <= K * 2^-24 * S + 1/2 ulp,  S = sum|dy * x|,
    K = N*P*Q additions, the ulp that of fp32 (the format of the sums) at
    |ref64| + K * 2^-24 * S. The same bound must reject the reference with
    one tap zeroed and, for the 3x3 windows, the reference of the
    H/W-swapped problem (whose taps are transposed)."""
    ext = _ext()
    C, Ko, R, pad = RANDOM[cls]
    N, H, W = 2, 9, 11
    P, Q = _out_hw(H, W, R, 1, pad)
    K = N * P * Q
    assert ext.wgrad_narrow_plan(Ko, R * R * C, K)[1] == cls
    g = torch.Generator().manual_seed(7)
    x = _cl(torch.randn(N, C, H, W, generator=g).to(dtype).cuda())
    dy = _cl(torch.randn(N, Ko, P, Q, generator=g).to(dtype).cuda())

    def flat(t):  # (Ko, C, R, S) -> [Ko][(r, s, c)]
        return t.permute(0, 2, 3, 1).reshape(Ko, -1)

    ref4 = _ref64(x, dy, R, 1, pad)
    ref = flat(ref4)
    S = flat(_ref64(x.abs(), dy.abs(), R, 1, pad))

    def bound(r):
        a = K * 2.0 ** -24 * S
        e = torch.frexp((r.abs() + a).clamp_min(2.0 ** -126))[1] - 1
        return a + 0.5 * torch.ldexp(torch.ones_like(r), e - 23)

    got = ext.conv_wgrad_narrow_acc32(x, dy, R, R, 1, pad, 2, False)
    assert got.dtype == torch.float32 and got.shape == ref.shape
    got = got.double().cpu()
    ratio = ((got - ref).abs() / bound(ref)).max().item()
    print(f"{cls} {dtype}: max err / bound = {ratio:.4f}")
    assert ((got - ref).abs() <= bound(ref)).all(), ratio
    # a dropped tap and swapped axes are outside the bound
    tap0 = ref4.clone()
    tap0[:, :, R // 2, R // 2] = 0
    tap0 = flat(tap0)
    assert not ((got - tap0).abs() <= bound(tap0)).all()
    if R > 1:  # a 1x1 window sums the same products after the swap
        swapped = flat(_ref64(x.transpose(2, 3), dy.transpose(2, 3), R, 1,
                              pad))
        assert not ((got - swapped).abs() <= bound(swapped)).all()
    for ko, rsc, mx in ext.wgrad_ws_stats():
        assert mx == 0.0, (ko, rsc, mx)


@pytest.mark.gpu
def test_narrow_envelope_checks():
    ext = _ext()
    bf = torch.bfloat16
    x = _cl(torch.zeros(1, 64, 8, 8, device="cuda", dtype=bf))
    dy = _cl(torch.zeros(1, 64, 8, 8, device="cuda", dtype=bf))
    with pytest.raises(RuntimeError, match=r"C % 8 == 0"):
        ext.conv_wgrad_narrow(_cl(torch.zeros(1, 12, 8, 8, device="cuda",
                                              dtype=bf)), dy, 1, 1, 1, 0, 1,
                              False)
    with pytest.raises(RuntimeError, match=r"must be CUDA tensors"):
        ext.conv_wgrad_narrow(x.cpu(), dy, 1, 1, 1, 0, 1, False)
    with pytest.raises(RuntimeError, match=r"1 <= splitk <= ceil"):
        ext.conv_wgrad_narrow(x, dy, 1, 1, 1, 0, 0, False)
    with pytest.raises(RuntimeError, match=r"1 <= splitk <= ceil"):
        ext.conv_wgrad_narrow(x, dy, 1, 1, 1, 0, 2, False)  # 1 K-tile
    wide = _cl(torch.zeros(1, 256, 8, 8, device="cuda", dtype=bf))
    with pytest.raises(RuntimeError, match=r"Ko <= 128 or R\*S\*C <= 128"):
        ext.conv_wgrad_narrow(wide, wide, 1, 1, 1, 0, 1, False)


# the nine wgrad shape classes of ResNet-50 that the 256x256 kernel does not
# take, at the flagship batch 4096: (Ko, R*S*C, N*P*Q) -> (routed, tile class)
_NPQ56, _NPQ28, _NPQ112 = 4096 * 56 * 56, 4096 * 28 * 28, 4096 * 112 * 112
FLAGSHIP = {
    "l1.0.c1": ((64, 64, _NPQ56), (False, "64x256")),
    "l1.x.c1": ((64, 256, _NPQ56), (True, "64x256")),
    "l1.x.c2": ((64, 576, _NPQ56), (True, "64x256")),
    "stem": ((64, 392, _NPQ112), (True, "64x256")),
    "l1.x.c3": ((256, 64, _NPQ56), (True, "256x64")),
    "l2.0.c1": ((128, 256, _NPQ56), (True, "128x256")),
    "l2.x.c1": ((128, 512, _NPQ28), (True, "128x256")),
    "l2.x.c2": ((128, 1152, _NPQ28), (True, "128x256")),
    "l2.x.c3": ((512, 128, _NPQ28), (True, "256x128")),
}


@pytest.mark.parametrize("name", list(FLAGSHIP))
def test_narrow_routing_flagship(name):
    """each flagship class is routed exactly where the per-shape A/B measured
    a win in every round (profiles/resnet50_mi355x.md)"""
    ext = _ext()
    (Ko, RSC, NPQ), (use, cls) = FLAGSHIP[name]
    plan = ext.wgrad_narrow_plan(Ko, RSC, NPQ)
    assert (plan[0], plan[1]) == (use, cls)
    assert 1 <= plan[2] <= _ceil(NPQ, 64)


def test_narrow_routing_keeps_old_plans():
    ext = _ext()
    # below the K-tile floor (2048 K-tiles): every class stays on the old kernel
    for (Ko, RSC, _), _ in FLAGSHIP.values():
        assert not ext.wgrad_narrow_plan(Ko, RSC, 2047 * 64)[0]
        assert not ext.wgrad_narrow_plan(Ko, RSC, 128 * 28 * 28)[0]
    # the 256x256 kernel's shapes are not claimed, and its plan is unchanged
    for Ko, RSC in ((192, 192), (256, 2304), (512, 256)):
        plan = ext.wgrad_narrow_plan(Ko, RSC, _NPQ28)
        assert (plan[0], plan[1]) == (False, "")
        assert ext.wgrad_nt256_plan(Ko, RSC, _NPQ28)[0]
    # C % 8 != 0 never reaches the plan: conv_wgrad takes the transposed path
    # (the stem with C = 3), whose launch the old plan binding still describes
    assert ext.gemm_plan(64, 147, _NPQ112, 8, False)[0] == 4
