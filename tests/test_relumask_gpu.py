"""Packed ReLU bitmask in BN backward (batchnorm.hip, gemm_conv.hip EpiBnBwd).

bn_fwd_train(..., want_mask=True) also returns a uint8 [rows][C/8] mask with
bit e of byte (row, cv) = !(y[row][cv*8+e] <= 0), evaluated on the stored
16-bit y. Every backward kernel that read y only for that bit takes the mask
instead. The mask carries exactly the predicate those kernels applied to y,
and nothing else in their arithmetic changes, so every comparison below is
masked call vs. the same call reading y, bit for bit (no tolerance). The one
exception is the block-level weight gradients: the wgrad split-K fp32 atomics
are unordered, so those are held to the run-to-run spread of the y path.

DTMX_BN_COL / DTMX_BN_DX_COEF pick the elementwise kernels once per process;
the strided-chunk and direct-form kernels run the same checks in fresh
children.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
# (N, H, W, C): odd row counts; one channel vector; 3 and 9 vectors (not
# powers of two); 33 vectors x 196 rows (the unrolled-pair loop and its tail)
EMIT_SHAPES = [(2, 5, 7, 8), (3, 7, 7, 24), (2, 9, 9, 72), (1, 14, 14, 264)]


def _ext():
    from dtmx.ops.hip import require_ext

    return require_ext()


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(t):
    """NHWC tensor -> [N*H*W][C] view of its memory order."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _unpack(mask):
    """uint8 [rows][C/8] -> bool [rows][C] (bit e of a byte = channel 8*cv+e)."""
    bits = np.unpackbits(mask.cpu().numpy(), axis=1, bitorder="little")
    return torch.from_numpy(bits.astype(bool))


def _pack(keep):
    """bool [rows][C] -> uint8 [rows][C/8] on the GPU (host reference packer)."""
    return torch.from_numpy(
        np.packbits(keep.cpu().numpy(), axis=1, bitorder="little")).to(DEV)


def _beq(a, b, what):
    """Bit equality (NaN == NaN): compare the raw 16/32-bit patterns."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    assert torch.equal(a.contiguous().view(it), b.contiguous().view(it)), what


def _bn_inputs(shape, dtype, residual, seed=0):
    """x with exact zeros and a few NaNs (channel 2). Channel 1 gets
    gamma = 6e-8 (stored as the smallest fp16 subnormal, 5.96e-8) and beta = 0,
    so in fp16 its outputs with 0 < xhat < 0.5 are positive in fp32 but stored
    as 0: the predicate must look at the stored value."""
    N, H, W, C = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((N, C, H, W), generator=g, device=DEV)
    x[torch.rand((N, C, H, W), generator=g, device=DEV) < 0.1] = 0.0
    x[0, 2, 0, :2] = float("nan")
    gamma = torch.randn((C,), generator=g, device=DEV)
    beta = torch.randn((C,), generator=g, device=DEV) * 0.5
    gamma[1], beta[1] = 6e-8, 0.0
    res = None
    if residual:
        res = torch.randn((N, C, H, W), generator=g, device=DEV)
        res[:, 1] = 0.0
        res[-1, 3, -1, -1] = float("nan")
        res = _cl(res.to(dtype))
    dy = _cl(torch.randn((N, C, H, W), generator=g, device=DEV).to(dtype))
    return _cl(x.to(dtype)), gamma.to(dtype), beta.to(dtype), res, dy


def _fwd(ext, x, gamma, beta, res, want_mask):
    C = x.shape[1]
    rm = torch.zeros(C, device=DEV)
    rv = torch.ones(C, device=DEV)
    if want_mask:
        return ext.bn_fwd_train(x, gamma, beta, rm, rv, 0.9, 1e-5, True, res,
                                None, None, True)
    return ext.bn_fwd_train(x, gamma, beta, rm, rv, 0.9, 1e-5, True, res, None,
                            None)


def check_emit(ext, shape, dtype, residual):
    N, H, W, C = shape
    x, gamma, beta, res, _ = _bn_inputs(shape, dtype, residual)
    y0, sm0, si0 = _fwd(ext, x, gamma, beta, res, False)
    y, sm, si, mask = _fwd(ext, x, gamma, beta, res, True)
    _beq(y, y0, "y")
    _beq(sm, sm0, "mean")
    _beq(si, si0, "invstd")
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (N * H * W, C // 8)
    assert mask.is_contiguous()
    want = ~(_rows(y).float() <= 0).cpu()
    assert torch.equal(_unpack(mask), want)
    # the inputs really produce both bit values and exact zeros
    assert want.any() and not want.all()
    if dtype == torch.float16:
        # channel 1 (no NaN, zero residual): y = 5.96e-8 * xhat in fp32, which
        # rounds to a stored 0 below half a subnormal step -> mask bit clear
        xhat = (_rows(x)[:, 1].float() - sm[1]) * si[1]
        under = ((xhat > 0.05) & (xhat < 0.45)).cpu()
        assert under.any()
        assert (_rows(y)[:, 1].cpu()[under] == 0).all()
        assert not _unpack(mask)[:, 1][under].any()


def check_bn_bwd(ext, shape, dtype, residual):
    """bn_bwd and bn_bwd_dx_presummed with the mask vs. with y; then with a
    NaN-filled y next to the mask (the mask really replaces y)."""
    N, H, W, C = shape
    rows = N * H * W
    x, gamma, beta, res, dy = _bn_inputs(shape, dtype, residual, seed=1)
    # NaN-free statistics so that the comparison is about values, not NaN
    # propagation alone
    x = torch.nan_to_num(x)
    y, sm, si, mask = _fwd(ext, x, gamma, beta, res, True)
    ynan = torch.full_like(y, float("nan"))
    ref = ext.bn_bwd(x, dy, gamma, sm, si, True, y, residual)
    for yy in (y, ynan):
        got = ext.bn_bwd(x, dy, gamma, sm, si, True, yy, residual, mask=mask)
        assert len(got) == len(ref) == (4 if residual else 3)
        for a, b, n in zip(got, ref, ("dx", "dgamma", "dbeta", "dres")):
            _beq(a, b, f"bn_bwd {n}")
    tdb = torch.randn(C, device=DEV)
    tdg = torch.randn(C, device=DEV)
    ref = ext.bn_bwd_dx_presummed(x, dy, y, sm, si, gamma, tdb, tdg, rows, True,
                                  residual)
    for yy in (y, ynan):
        got = ext.bn_bwd_dx_presummed(x, dy, yy, sm, si, gamma, tdb, tdg, rows,
                                      True, residual, mask=mask)
        assert len(got) == len(ref) == (2 if residual else 1)
        for a, b, n in zip(got, ref, ("dx", "dres")):
            _beq(a, b, f"bn_bwd_dx_presummed {n}")


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=str)
def test_mask_emit(shape, dtype, residual):
    check_emit(_ext(), shape, dtype, residual)


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "dres"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", EMIT_SHAPES, ids=str)
def test_bn_bwd_with_mask(shape, dtype, residual):
    check_bn_bwd(_ext(), shape, dtype, residual)


def test_mask_argument_checks():
    """want_mask needs fuse_relu; a mask of the wrong dtype/shape/layout is
    rejected before any launch."""
    ext = _ext()
    shape = (3, 7, 7, 24)  # 3 bytes per row: a column slice is not dense
    x, gamma, beta, _, dy = _bn_inputs(shape, torch.bfloat16, False)
    rm, rv = torch.zeros(24, device=DEV), torch.ones(24, device=DEV)
    with pytest.raises(RuntimeError, match="fuse_relu"):
        ext.bn_fwd_train(x, gamma, beta, rm, rv, 0.9, 1e-5, False, None, None,
                         None, True)
    y, sm, si, mask = _fwd(ext, x, gamma, beta, None, True)
    bad = [mask.to(torch.int8), mask[:-1], mask.cpu(),
           mask.repeat(1, 2)[:, ::2], mask.view(-1)]
    for m in bad:
        with pytest.raises(RuntimeError, match="mask"):
            ext.bn_bwd(x, dy, gamma, sm, si, True, y, False, mask=m)
        with pytest.raises(RuntimeError, match="mask"):
            ext.bn_bwd_dx_presummed(x, dy, y, sm, si, gamma, sm, si, 147, True,
                                    False, mask=m)
        w = _cl(torch.randn(16, 24, 1, 1, device=DEV).to(torch.bfloat16))
        dyo = _cl(torch.randn(3, 16, 7, 7, device=DEV).to(torch.bfloat16))
        with pytest.raises(RuntimeError, match="mask"):
            ext.conv_dgrad_bnfuse(dyo, w, 1, 0, 7, 7, None, y, x, sm, si, mask=m)
    with pytest.raises(RuntimeError, match="fuse_relu"):
        ext.bn_bwd(x, dy, gamma, sm, si, False, y, False, mask=mask)


# ----------------------------------------------------------------- epilogue

# (N, C(bn), Ko, H, W, R, stride, pad). M = N*H*W = 147 is no multiple of 128
# (two row tiles, ragged). C = 64 -> the NJ=2 (BN=64) 128-row tile, C = 128 ->
# the NJ=4 tile. The last shape meets the 256x256 routing gate of launch_gemm:
# M = 10*64*64 = 40960 >= 512, N = C = 256 >= 192, K = Ko = 128 (>= 128,
# % 64 == 0), ceil(M/256) * ceil(N/256) = 160 >= 160 tiles; the small shapes
# fail it on M < 512, so each kernel family runs. ~20 MB per tensor.
EPI_SHAPES = [
    (3, 64, 32, 7, 7, 1, 1, 0),
    (3, 128, 64, 7, 7, 1, 1, 0),
    (3, 64, 64, 7, 7, 3, 1, 1),
    (3, 128, 32, 7, 7, 3, 1, 1),
    (3, 64, 32, 7, 7, 3, 2, 1),
    (3, 128, 64, 7, 7, 3, 2, 1),
    (10, 256, 128, 64, 64, 1, 1, 0),
]


@pytest.mark.parametrize("with_acc", [False, True], ids=["noacc", "acc"])
@pytest.mark.parametrize("shape", EPI_SHAPES, ids=str)
def test_epilogue_mask_matches_y(shape, with_acc):
    ext = _ext()
    N, C, Ko, H, W, R, stride, pad = shape
    dtype = torch.bfloat16
    P = (H + 2 * pad - R) // stride + 1
    Q = (W + 2 * pad - R) // stride + 1
    g = torch.Generator(device=DEV).manual_seed(7)
    dy = _cl(torch.randn((N, Ko, P, Q), generator=g, device=DEV).to(dtype))
    w = _cl((torch.randn((Ko, C, R, R), generator=g, device=DEV) * 0.1).to(dtype))
    c = _cl(torch.randn((N, C, H, W), generator=g, device=DEV).to(dtype))
    y = torch.randn((N, C, H, W), generator=g, device=DEV)
    y = _cl(y.clamp_min(0).to(dtype))
    y[0, 0, 0, 0] = float("nan")  # NaN keeps the gradient on both paths
    acc0 = _cl(torch.randn((N, C, H, W), generator=g, device=DEV).to(dtype))
    mean = torch.randn((C,), generator=g, device=DEV) * 0.1
    invstd = torch.rand((C,), generator=g, device=DEV) + 0.5
    mask = _pack(~(_rows(y).float() <= 0))

    def run(yy, m):
        acc = acc0.clone() if with_acc else None
        return ext.conv_dgrad_bnfuse(dy, w, stride, pad, H, W, acc, yy, c, mean,
                                     invstd, mask=m)

    ref = run(y, None)
    ynan = torch.full_like(y, float("nan"))
    for yy in (y, ynan):
        got = run(yy, mask)
        for a, b, n in zip(got, ref, ("g", "pdb", "pdg")):
            _beq(a, b, n)
    # the mask was applied at all: dropped positions are exact zeros
    assert (_rows(ref[0]).float()[_rows(y).float() <= 0] == 0).all()


# -------------------------------------------------------------- block level

def _block_run(kind, down, mask_env, monkeypatch):
    from dtmx.ops import fusedblock
    from dtmx.models import resnet

    monkeypatch.setenv("DTMX_RELU_MASK", mask_env)
    monkeypatch.setenv("DTMX_FUSED_BLOCK", "1")
    for k in fusedblock.bnbwd_stats:
        fusedblock.bnbwd_stats[k] = 0
    torch.manual_seed(0)
    # two blocks of the same form in a row, so the cross-block handle (and the
    # mask it carries) is used: the second block's last dgrad epilogue masks
    # and reduces the first block's last BN
    blocks = _make_blocks(resnet, kind, down)
    blocks = blocks.to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    blocks.train()
    torch.manual_seed(1)
    cin = _BLOCK_CFG[(kind, down)][0][0]
    x = _cl(torch.randn(2, cin, 8, 8, device=DEV).to(torch.bfloat16))
    x.requires_grad_(True)
    out = blocks(x)
    torch.manual_seed(2)
    out.backward(torch.randn_like(out))
    grads = {n: p.grad.detach().clone() for n, p in blocks.named_parameters()}
    return out.detach(), x.grad.detach(), grads, dict(fusedblock.bnbwd_stats)


# (in_ch, ch) of the two chained blocks; a block has a downsample shortcut
# when in_ch != ch * expansion
_BLOCK_CFG = {
    ("bottleneck", False): [(64, 16), (64, 16)],
    ("bottleneck", True): [(32, 16), (64, 32)],
    ("basic", False): [(32, 32), (32, 32)],
    ("basic", True): [(16, 32), (32, 64)],
}


def _make_blocks(resnet, kind, down):
    cls = resnet.Bottleneck if kind == "bottleneck" else resnet.BasicBlock
    blocks = [cls(i, c, 1) for i, c in _BLOCK_CFG[(kind, down)]]
    assert all((b.downsample is not None) == down for b in blocks)
    return torch.nn.Sequential(*blocks)


@pytest.mark.parametrize("down", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_block_mask_on_off(kind, down, monkeypatch):
    out0, dx0, g0, st0 = _block_run(kind, down, "0", monkeypatch)
    out0b, dx0b, g0b, _ = _block_run(kind, down, "0", monkeypatch)
    out1, dx1, g1, st1 = _block_run(kind, down, "1", monkeypatch)
    assert st1 == st0, (st0, st1)
    assert st1["cross_emit"] == 1 and st1["cross"] == 1, st1
    _beq(out1, out0, "block output")
    _beq(dx1, dx0, "dx")
    assert set(g1) == set(g0)
    for n in g0:
        if g0[n].dim() == 1:  # BN gamma / beta gradients: no atomics
            _beq(g1[n], g0[n], n)
        else:  # conv weights: unordered split-K atomics
            spread = (g0b[n].float() - g0[n].float()).abs().max().item()
            diff = (g1[n].float() - g0[n].float()).abs().max().item()
            print(f"{kind} down={down} {n}: |mask-y| {diff:.3e} "
                  f"run-to-run {spread:.3e}")
            assert diff <= spread, (n, diff, spread)


# ------------------------------------------- env-selected elementwise kernels

def _child_main():
    ext = _ext()
    for shape in EMIT_SHAPES:
        for dtype in DTYPES:
            for residual in (False, True):
                check_emit(ext, shape, dtype, residual)
                check_bn_bwd(ext, shape, dtype, residual)
    torch.cuda.synchronize()
    print("relumask child ok")


def test_env_selected_kernels():
    """DTMX_BN_COL=0 (strided-chunk apply / dx kernels) and DTMX_BN_DX_COEF=0
    (direct-form dx) are read once per process: one fresh child per setting,
    none started after a failure."""
    for setting in ({"DTMX_BN_COL": "0"},
                    {"DTMX_BN_COL": "0", "DTMX_BN_DX_COEF": "0"}):
        env = {k: v for k, v in os.environ.items()
               if k not in ("DTMX_BN_COL", "DTMX_BN_DX_COEF")}
        env.update(setting)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"],
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (
            f"child {setting} exited {p.returncode}\n{p.stdout[-3000:]}\n"
            f"{p.stderr[-3000:]}")
        assert "relumask child ok" in p.stdout


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child_main()
