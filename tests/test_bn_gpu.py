"""BatchNorm kernels (batchnorm.hip) vs a plain fp64 reference, at the channel
counts and row counts where the stats geometry (bn_cpb / bn_grid) changes:
odd channel-vector counts, one row, fewer rows than a block's row stride,
exactly two slabs, a ragged last slab, the 256-vector cap with grid.x = 2.

Three kinds of check:

* integer-exact (zero tolerance): with inputs drawn from integers in [-4, 4]
  every partial sum is an integer below 2^24, so the fp32 sums must be
  bit-equal to the fp64 sums whatever the summation order (the GEMM trick of
  docs/KERNELS.md applied to the slab reducers);
* numeric, bf16 and fp16, against the fp64 reference below (inputs are
  rounded to the 16-bit type first, so only kernel arithmetic is compared);
* the env-selected kernels (DTMX_BN_COL=0, DTMX_BN_DX_COEF=0), which are
  chosen once per process, run the same numeric checks in fresh children.

Tolerances
----------
16-bit outputs (y, dx, dgamma, dbeta): 2 ulp of the output type,
|got - ref| <= R*|ref| + R*mean|ref| with R = 2^-7 (bf16) / 2^-10 (fp16).
dres is a copy of dy or zero, so it is compared exactly.

fp32 statistics: each deviation is normalised by the magnitude that bounds
the rounding error of the quantity (u = fp32 unit roundoff, E2 = E[x^2],
kappa = E2 / (var + eps) is the cancellation factor of the one-pass
variance E[x^2] - E[x]^2):

  save_mean      |d| / sqrt(E2)                          sum error ~ u*sum|x|
  save_invstd    |d| / invstd / (1 + kappa/2)            d(invstd)/invstd =
                                                         d(var) / 2(var+eps),
                                                         d(var) ~ u*E2
  running_mean   |d| / (m*|rm| + (1-m)*sqrt(E2))
  running_var    |d| / (m*|rv| + (1-m)*n/(n-1)*E2)
  tdb            |d| / sum|g|
  tdg            |d| / (sum|g*xhat| * (1 + kappa/2))     xhat carries invstd

The constants are 4x the largest normalised deviation from fp64 of the same
one-pass formula evaluated in float32 by torch on the CPU (`_fp32_onepass`),
over every (C, rows) of GRID plus the mean-offset case, both dtypes. The 4x
is the margin for a different summation order. Measured maxima
(`python tests/test_bn_gpu.py --measure`):

  save_mean     8.87e-08   -> K_MEAN  = 4 * 8.87e-08
  save_invstd   3.44e-07   -> K_INV   = 4 * 3.44e-07
  running_mean  2.98e-07   -> K_RMEAN = 4 * 2.98e-07
  running_var   2.69e-07   -> K_RVAR  = 4 * 2.69e-07
  tdb           2.81e-08   -> K_TDB   = 4 * 2.81e-08
  tdg           1.08e-07   -> K_TDG   = 4 * 1.08e-07

`test_torch_fp32_passes_tolerances` (CPU) confirms that torch's own fp32
batch_norm + autograd, cast to the 16-bit type, passes the 16-bit check at
every shape used here, the offset case included, with the 2-ulp bound as
stated (no widening was needed), and that the fp32 one-pass formula passes
the statistics bounds.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
MOM = 0.9  # mxnet semantics: running = running*MOM + batch*(1-MOM)

K_MEAN = 4 * 8.87e-08
K_INV = 4 * 3.44e-07
K_RMEAN = 4 * 2.98e-07
K_RVAR = 4 * 2.69e-07
K_TDB = 4 * 2.81e-08
K_TDG = 4 * 1.08e-07

R16 = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
DTYPES = [torch.bfloat16, torch.float16]
ALL_C = [8, 24, 40, 48, 56, 80, 96, 144, 2048, 4096]


# ------------------------------------------------- geometry (host-side copy)

def bn_cpb(cvecs):
    """Channel-vectors per block: largest power-of-two divisor, capped at 256."""
    return min(cvecs & -cvecs, 256)


def bn_grid(rows, C):
    """-> (grid.x, nslabs, rows_per_block), the arithmetic of bn_grid()."""
    cvecs = C // 8
    cpb = bn_cpb(cvecs)
    rstep = 256 // cpb
    rb = min(2048, max(1, rows // (rstep * 16)))
    rpb = (rows + rb - 1) // rb
    rb = (rows + rpb - 1) // rpb
    return (cvecs + cpb - 1) // cpb, rb, rpb


def two_slab_rows(C):
    """Smallest row count that gives two slabs for this C."""
    return 2 * (256 // bn_cpb(C // 8)) * 16


def _grid():
    cases = []
    for C in ALL_C:
        rows = [147, two_slab_rows(C)]
        if C in (8, 24, 80, 2048, 4096):
            rows.insert(0, 1)
        if C in (8, 24, 48, 80, 144):
            rows.append(8193)  # = 1*3*2731, never a multiple of rows_per_block
        cases += [(C, r) for r in rows]
    return cases


GRID = _grid()
OFFSET_CASE = (24, 8192)  # per-channel mean 4, std 0.5


def test_grid_reaches_every_geometry_class():
    """The shapes above must really hit the classes they were chosen for;
    a later change of bn_cpb / bn_grid must not silently empty them."""
    assert {bn_cpb(C // 8) for C in ALL_C} == {1, 2, 4, 256}
    assert bn_grid(32, 4096)[0] == 2 and bn_grid(32, 2048)[0] == 1
    for C in ALL_C:
        assert bn_grid(two_slab_rows(C), C)[1] == 2, C
        assert bn_grid(two_slab_rows(C) - 1, C)[1] == 1, C
    for C, rows in GRID:
        gx, nslabs, rpb = bn_grid(rows, C)
        if rows == 8193:
            assert nslabs >= 2 and rows % rpb != 0, (C, rows)
        if rows == 147:
            rstep = 256 // bn_cpb(C // 8)
            if bn_cpb(C // 8) == 1:  # fewer rows than the row stride
                assert rstep > rows and nslabs == 1
            # some thread runs an odd number of row steps: the tails of the
            # 2x and 4x unrolled row loops are taken
            assert rpb % (2 * rstep) != 0, (C, rpb)


# ------------------------------------------------------------ fp64 reference
# Everything is a [rows, C] matrix: NHWC BatchNorm reduces over rows.

def ref_fwd(x, gamma, beta, rm, rv, train, relu=False, res=None, count=None,
            sums=None):
    """-> y, save_mean, save_invstd, new_rm, new_rv (all float64).
    `sums` = (sum, sumsq) with `count` replaces the batch statistics."""
    x = x.double()
    gamma, beta, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
    if train:
        if sums is not None:
            n = count
            mean = sums[0].double() / n
            var = sums[1].double() / n - mean * mean
        else:
            n = x.shape[0]
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
        invstd = 1.0 / torch.sqrt(var + EPS)
        unbiased = var * n / (n - 1) if n > 1 else var
        new_rm = rm * MOM + mean * (1 - MOM)
        new_rv = rv * MOM + unbiased * (1 - MOM)
    else:
        mean, invstd = rm, 1.0 / torch.sqrt(rv + EPS)
        new_rm, new_rv = rm, rv
    y = (x - mean) * invstd * gamma + beta
    if res is not None:
        y = y + res.double()
    if relu:
        y = y.clamp_min(0)
    return y, mean, invstd, new_rm, new_rv


def ref_bwd(x, dy, gamma, mean, invstd, relu=False, y_mask=None, world=1):
    """-> dx, dgamma, dbeta, dres, tdb, tdg (float64). `y_mask` is the stored
    forward output: gradient passes where it is > 0. `world` identical ranks:
    the totals and the count are world times the local ones."""
    x, g = x.double(), dy.double()
    if relu:
        g = g * (y_mask.double() > 0)
    xhat = (x - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    m = x.shape[0] * world
    dx = gamma.double() * invstd * (g - world * dbeta / m - xhat * world * dgamma / m)
    return dx, dgamma, dbeta, g, dbeta, dgamma


# --------------------------------------- fp32 one-pass formula (CPU, torch)

def _fp32_onepass(x, rm, rv, dy):
    x = x.float()
    n = x.shape[0]
    mom = torch.tensor(MOM, dtype=torch.float32)
    s, ss = x.sum(0), (x * x).sum(0)
    mean = s / n
    var = (ss / n - mean * mean).clamp_min(0)
    invstd = torch.rsqrt(var + torch.tensor(EPS, dtype=torch.float32))
    unbiased = var * n / (n - 1) if n > 1 else var
    new_rm = rm * mom + mean * (1 - mom)
    new_rv = rv * mom + unbiased * (1 - mom)
    g = dy.float()
    tdb = g.sum(0)
    tdg = (g * ((x - mean) * invstd)).sum(0)
    return dict(mean=mean, invstd=invstd, rm=new_rm, rv=new_rv, tdb=tdb, tdg=tdg)


def _stat_devs(got, x, rm, rv, dy):
    """Normalised deviations (see module docstring) of the fp32 statistics in
    `got` (any subset of mean/invstd/rm/rv/tdb/tdg) from the fp64 reference."""
    xd = x.double()
    n = xd.shape[0]
    _, mean, invstd, nrm, nrv = ref_fwd(x, torch.ones(x.shape[1]), torch.zeros(x.shape[1]),
                                        rm, rv, True)
    e2 = (xd * xd).mean(0)
    kap = 1 + 0.5 * e2 * invstd ** 2
    g = dy.double()
    xhat = (xd - mean) * invstd
    ref = dict(mean=mean, invstd=invstd, rm=nrm, rv=nrv, tdb=g.sum(0),
               tdg=(g * xhat).sum(0))
    norm = dict(
        mean=e2.sqrt(),
        invstd=invstd * kap,
        rm=MOM * rm.double().abs() + (1 - MOM) * e2.sqrt(),
        rv=MOM * rv.double().abs() + (1 - MOM) * e2 * (n / (n - 1) if n > 1 else 1),
        tdb=g.abs().sum(0),
        tdg=(g * xhat).abs().sum(0) * kap,
    )
    out = {}
    for k, v in got.items():
        err = (v.double().cpu() - ref[k]).abs()
        # an exact value deviates by 0 even where its scale is 0 (rows = 1)
        out[k] = torch.where(err == 0, err, err / norm[k]).max().item()
    return out


K_STAT = dict(mean=K_MEAN, invstd=K_INV, rm=K_RMEAN, rv=K_RVAR, tdb=K_TDB, tdg=K_TDG)


def assert_stats(got, x, rm, rv, dy, name):
    devs = _stat_devs(got, x, rm, rv, dy)
    bad = {k: (d, K_STAT[k]) for k, d in devs.items() if not d <= K_STAT[k]}
    assert not bad, f"{name}: normalised fp32 deviation over bound: {bad}"


def assert_16(got, ref, name):
    """2 ulp of the 16-bit output type, plus the same factor of mean|ref|."""
    r = R16[got.dtype]
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs {ref.shape}"
    err = (got - ref).abs()
    bound = r * ref.abs() + r * ref.abs().mean()
    over = err > bound
    if over.any() or not torch.isfinite(got).all():
        i = (err - bound).argmax()
        raise AssertionError(
            f"{name}: {int(over.sum())} of {got.numel()} over 2 ulp; worst "
            f"got {got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r} "
            f"bound {bound.flatten()[i].item():.3e}")


def assert_exact(got, ref64, name):
    got = got.double().cpu()
    ref64 = ref64.double()
    if not torch.equal(got, ref64):
        bad = (got != ref64).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(
            f"{name}: {len(bad)} of {got.numel()} not bit-equal; first at {i}: "
            f"got {got[i].item()!r} want {ref64[i].item()!r}")


# ------------------------------------------------------------------- inputs

def make_inputs(C, rows, dtype, seed=0, offset=False):
    """Random normal inputs rounded to `dtype` (CPU, [rows, C] / [C])."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * C + rows)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(rows, C)
    if offset:
        x = x * 0.5 + 4.0
    return dict(
        x=x.to(dtype), dy=rn(rows, C).to(dtype), res=rn(rows, C).to(dtype),
        gamma=(rn(C) * 0.3 + 1.0).to(dtype), beta=(rn(C) * 0.5).to(dtype),
        rm=rn(C) * 0.5, rv=torch.rand(C, generator=g) + 0.5)


def int_mat(rows, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (rows, C), generator=g, dtype=torch.int8).to(dtype)


def dev4(m):
    """[rows, C] -> NCHW-shaped channels-last tensor on the GPU."""
    rows, C = m.shape
    n, h = (1, 3) if rows % 3 == 0 else (1, 1)
    return m.to(DEV).view(n, h, rows // h, C).permute(0, 3, 1, 2)


def mat(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _ext():
    from dtmx.ops.hip import require_ext
    return require_ext()


@pytest.fixture(scope="module", autouse=True)
def _return_gpu_memory():
    """This module allocates far larger blocks (50 MB slab-wrap inputs) than
    the rest of the suite; hand them back so that the tests that follow meet
    the caching allocator as they would without this module."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---------------------------------------------------------- numeric checks

def check_fwd_bwd(ext, C, rows, dtype, offset=False):
    """bn_fwd_train / bn_fwd_infer / bn_bwd over relu x residual."""
    d = make_inputs(C, rows, dtype, offset=offset)
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    X, DY, RES = dev4(x), dev4(dy), dev4(d["res"])
    G, B = gamma.to(DEV), beta.to(DEV)
    tag = f"C={C} rows={rows} {dtype}"
    for relu in (False, True):
        for with_res in (False, True):
            t = f"{tag} relu={relu} res={with_res}"
            res = d["res"] if with_res else None
            rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
            y, sm, si = ext.bn_fwd_train(X, G, B, rm, rv, MOM, EPS, relu,
                                         RES if with_res else None, None, None)
            ry, rmean, rinv, _, _ = ref_fwd(x, gamma, beta, d["rm"], d["rv"], True,
                                            relu, res)
            assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
            assert_16(mat(y), ry, f"fwd_train y {t}")
            assert_stats(dict(mean=sm, invstd=si, rm=rm, rv=rv), x, d["rm"], d["rv"],
                         dy, f"fwd_train {t}")

            yi = ext.bn_fwd_infer(X, G, B, d["rm"].to(DEV), d["rv"].to(DEV), EPS,
                                  relu, RES if with_res else None)
            ryi = ref_fwd(x, gamma, beta, d["rm"], d["rv"], False, relu, res)[0]
            assert_16(mat(yi), ryi, f"fwd_infer y {t}")

            # backward: fuse_relu follows relu, want_dres follows the residual;
            # the mask is the kernel's own stored y, as the kernel uses it
            out = ext.bn_bwd(X, DY, G, sm, si, relu, y, with_res)
            assert len(out) == (4 if with_res else 3)
            rdx, rdg, rdb, rdres, _, _ = ref_bwd(x, dy, gamma, rmean, rinv, relu,
                                                 mat(y).cpu())
            assert_16(mat(out[0]), rdx, f"bwd dx {t}")
            assert_16(out[1], rdg, f"bwd dgamma {t}")
            assert_16(out[2], rdb, f"bwd dbeta {t}")
            if with_res:
                assert_exact(mat(out[3]), rdres, f"bwd dres {t}")


def check_seam(ext, C, rows, dtype, world=1):
    """SyncBN seam: bn_local_sums -> bn_fwd_presummed and bn_bwd_sums ->
    bn_bwd_dx_presummed. world=2 simulates two identical ranks: doubled sums,
    count = 2*rows, checked against the reference on the doubled batch."""
    d = make_inputs(C, rows, dtype, seed=3)
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    X, DY, G, B = dev4(x), dev4(dy), gamma.to(DEV), beta.to(DEV)
    t = f"seam C={C} rows={rows} {dtype} world={world}"
    count = rows * world
    s, ss = ext.bn_local_sums(X)
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    y, sm, si = ext.bn_fwd_presummed(X, G, B, rm, rv, MOM, EPS, False, None,
                                     s * world, ss * world, count)
    x_all = torch.cat([x] * world)
    ry, rmean, rinv, _, _ = ref_fwd(x_all, gamma, beta, d["rm"], d["rv"], True)
    assert_16(mat(y), ry[:rows], f"{t} y")
    assert_stats(dict(mean=sm, invstd=si, rm=rm, rv=rv), x_all, d["rm"], d["rv"],
                 torch.cat([dy] * world), t)

    tdb, tdg = ext.bn_bwd_sums(X, DY, y, sm, si, False)
    assert_stats(dict(tdb=tdb, tdg=tdg), x, d["rm"], d["rv"], dy, t)
    (dx,) = ext.bn_bwd_dx_presummed(X, DY, y, sm, si, G, tdb * world, tdg * world,
                                    count, False, False)
    rdx = ref_bwd(x, dy, gamma, rmean, rinv, world=world)[0]
    assert_16(mat(dx), rdx, f"{t} dx")

    if world == 1:  # the all-reduce is the identity: same bits as plain BN
        rm1, rv1 = d["rm"].to(DEV), d["rv"].to(DEV)
        y1, sm1, si1 = ext.bn_fwd_train(X, G, B, rm1, rv1, MOM, EPS, False, None,
                                        None, None)
        dx1 = ext.bn_bwd(X, DY, G, sm1, si1, False, y1, False)[0]
        assert_exact(mat(y), mat(y1).double().cpu(), f"{t} y vs bn_fwd_train")
        assert_exact(sm, sm1.double().cpu(), f"{t} save_mean vs bn_fwd_train")
        assert_exact(mat(dx), mat(dx1).double().cpu(), f"{t} dx vs bn_bwd")


def _id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C,rows", GRID)
def test_fwd_bwd_vs_fp64(C, rows, dtype):
    check_fwd_bwd(_ext(), C, rows, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_mean_offset(dtype):
    """mean 4, std 0.5: where the one-pass variance and the kc*x + kb
    coefficient form of dx would show cancellation."""
    C, rows = OFFSET_CASE
    assert bn_grid(rows, C)[1] >= 2
    check_fwd_bwd(_ext(), C, rows, dtype, offset=True)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", [24, 48, 56, 80])
def test_syncbn_seam(C, dtype):
    rows = two_slab_rows(C) + 147  # two slabs, the second one ragged
    assert bn_grid(rows, C)[1] == 2
    check_seam(_ext(), C, rows, dtype)


@gpu
def test_syncbn_seam_world2():
    rows = two_slab_rows(24)
    assert bn_grid(rows, 24)[1] == 2
    check_seam(_ext(), 24, rows, torch.bfloat16, world=2)


# ----------------------------------------------------- integer-exact checks

# (C, rows): every C at two slabs, then two cases whose slab count exceeds the
# 256/ncv slab lanes of slab_reduce2_kernel, so its lane-strided loop wraps:
#   C=24: ncv 1 -> 256 lanes; rows 257*4096 -> nslabs 257
#   C=64: ncv 8 ->  32 lanes; rows  33*512  -> nslabs  33
EXACT_SUMS = [(C, two_slab_rows(C), 2) for C in ALL_C] + [
    (24, 257 * 4096, 257), (64, 33 * 512, 33)]


@gpu
@pytest.mark.parametrize("C,rows,nslabs", EXACT_SUMS)
def test_local_and_bwd_sums_exact(C, rows, nslabs):
    ext = _ext()
    assert bn_grid(rows, C)[1] == nslabs and nslabs >= 2
    ncv = min(bn_cpb(C // 8), 8)
    if nslabs > 2:
        assert nslabs > 256 // ncv
    x = int_mat(rows, C, torch.bfloat16, 11)
    dy = int_mat(rows, C, torch.bfloat16, 12)
    xd, gd = x.double(), dy.double()
    assert (xd * xd).sum(0).max() < 2 ** 24
    X, DY = dev4(x), dev4(dy)
    s, ss = ext.bn_local_sums(X)
    assert s.dtype == torch.float32 and s.shape == (C,)
    assert_exact(s, xd.sum(0), f"sum C={C} nslabs={nslabs}")
    assert_exact(ss, (xd * xd).sum(0), f"sumsq C={C} nslabs={nslabs}")
    # mean 0, invstd 1: xhat = x, so sum(dy*xhat) is integer-exact as well
    zero, one = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    tdb, tdg = ext.bn_bwd_sums(X, DY, X, zero, one, False)
    assert_exact(tdb, gd.sum(0), f"tdb C={C} nslabs={nslabs}")
    assert_exact(tdg, (gd * xd).sum(0), f"tdg C={C} nslabs={nslabs}")


SLAB_COUNTS = [1, 1024, 1025, 1500]  # both sides of the > 1024 pre-reduce


def _int_slabs(nslabs, C, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (nslabs, C), generator=g).float()


@gpu
@pytest.mark.parametrize("C", [24, 64, 80])
@pytest.mark.parametrize("nslabs", SLAB_COUNTS)
def test_fwd_train_presummed_slabs_exact(nslabs, C):
    """bn_fwd_train with hand-made integer slabs in place of its own stats."""
    ext = _ext()
    rows, dtype = 147, torch.bfloat16
    d = make_inputs(C, rows, dtype, seed=5)
    psum = _int_slabs(nslabs, C, -4, 4, 21)
    psumsq = _int_slabs(nslabs, C, 40, 80, 22)  # keeps sumsq/n - mean^2 > 0
    s64, ss64 = psum.double().sum(0), psumsq.double().sum(0)
    assert ss64.max() < 2 ** 24
    assert (ss64 / rows - (s64 / rows) ** 2).min() > 0.1
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    y, sm, si = ext.bn_fwd_train(dev4(d["x"]), d["gamma"].to(DEV), d["beta"].to(DEV),
                                 rm, rv, MOM, EPS, False, None, psum.to(DEV),
                                 psumsq.to(DEV))
    want_mean = s64.numpy().astype(np.float32) / np.float32(rows)
    assert_exact(sm, torch.from_numpy(want_mean), f"save_mean nslabs={nslabs} C={C}")
    ry, _, rinv, nrm, nrv = ref_fwd(d["x"], d["gamma"], d["beta"], d["rm"], d["rv"],
                                    True, count=rows, sums=(s64, ss64))
    # scale and shift show through y
    assert_16(mat(y), ry, f"y nslabs={nslabs} C={C}")
    e2 = ss64 / rows
    kap = 1 + 0.5 * e2 * rinv ** 2
    assert ((si.double().cpu() - rinv).abs() <= K_INV * rinv * kap).all()
    assert ((rm.double().cpu() - nrm).abs()
            <= K_RMEAN * (MOM * d["rm"].abs() + (1 - MOM) * e2.sqrt())).all()
    assert ((rv.double().cpu() - nrv).abs()
            <= K_RVAR * (MOM * d["rv"].abs() + (1 - MOM) * e2 * rows / (rows - 1))).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("C", [24, 64, 80])
@pytest.mark.parametrize("nslabs", SLAB_COUNTS)
def test_bwd_finalize_slabs_exact(nslabs, C, dtype):
    ext = _ext()
    pdb = _int_slabs(nslabs, C, -4, 4, 31)
    pdg = _int_slabs(nslabs, C, -4, 4, 32)
    like = torch.empty(1, dtype=dtype, device=DEV)
    dgamma, dbeta, tdb, tdg = ext.bn_bwd_finalize_slabs(pdb.to(DEV), pdg.to(DEV), like)
    db64, dg64 = pdb.double().sum(0), pdg.double().sum(0)
    t = f"nslabs={nslabs} C={C}"
    assert_exact(tdb, db64, f"tdb {t}")
    assert_exact(tdg, dg64, f"tdg {t}")
    assert dgamma.dtype == dtype and dbeta.dtype == dtype
    assert_exact(dgamma, dg64.float().to(dtype), f"dgamma {t}")
    assert_exact(dbeta, db64.float().to(dtype), f"dbeta {t}")


# ----------------------------------------------------- entry-point checks

def _bad_calls(ext, x, dy, y, C):
    v = torch.ones(C, device=DEV)
    g = torch.ones(C, dtype=x.dtype, device=DEV)
    return {
        "bn_fwd_presummed": lambda: ext.bn_fwd_presummed(
            x, g, g, v.clone(), v.clone(), MOM, EPS, False, None, v, v, 4),
        "bn_bwd_sums": lambda: ext.bn_bwd_sums(x, dy, y, v, v, True),
        "bn_bwd_dx_presummed": lambda: ext.bn_bwd_dx_presummed(
            x, dy, y, v, v, g, v, v, 4, True, False),
        "bn_bwd": lambda: ext.bn_bwd(x, dy, g, v, v, True, y, False),
    }


@gpu
def test_entry_points_reject_bad_arguments():
    """The checks run before any launch, so nothing reaches the device."""
    ext = _ext()
    cl = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV).contiguous(
        memory_format=torch.channels_last)
    x12 = cl(1, 12, 2, 2)
    for name, call in _bad_calls(ext, x12, x12, x12, 12).items():
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call()
    x = cl(2, 16, 3, 3)
    nchw = torch.zeros(2, 16, 3, 3, dtype=torch.bfloat16, device=DEV)
    small = cl(1, 16, 3, 3)
    for name, call in _bad_calls(ext, nchw, x, x, 16).items():
        with pytest.raises(RuntimeError, match="NHWC"):
            call()
    for bad in (nchw, small):
        for name, call in _bad_calls(ext, x, bad, x, 16).items():
            if name != "bn_fwd_presummed":  # takes no dy
                with pytest.raises(RuntimeError, match="bn: dy"):
                    call()
        for name, call in _bad_calls(ext, x, x, bad, 16).items():
            if name != "bn_fwd_presummed":
                with pytest.raises(RuntimeError, match="bn: y"):
                    call()


# ------------------------------------------------- env-selected kernels

CHILD_CASES = [(24, 147), (24, 8193), (64, 147), (64, 1024), (4096, 32), (4096, 147)]


def _child_main():
    """Numeric fwd/bwd + seam checks at small shapes; the env decides which
    elementwise kernels the extension dispatches to."""
    ext = _ext()
    for C, rows in CHILD_CASES:
        for dtype in DTYPES:
            check_fwd_bwd(ext, C, rows, dtype)
            check_seam(ext, C, rows, dtype)
    torch.cuda.synchronize()
    print("bn child ok:", {k: os.environ.get(k) for k in ("DTMX_BN_COL", "DTMX_BN_DX_COEF")})


@gpu
def test_env_selected_kernels():
    """DTMX_BN_COL=0 (strided-chunk apply / dx) and DTMX_BN_DX_COEF=0
    (direct-form dx) are read once per process: one fresh child per setting,
    one after the other, none started after a failure."""
    for setting in ({"DTMX_BN_COL": "0"}, {"DTMX_BN_DX_COEF": "0"},
                    {"DTMX_BN_COL": "0", "DTMX_BN_DX_COEF": "0"}):
        env = {k: v for k, v in os.environ.items()
               if k not in ("DTMX_BN_COL", "DTMX_BN_DX_COEF")}
        env.update(setting)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"],
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (
            f"child {setting} exited {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}")
        assert "bn child ok" in p.stdout


# ------------------------------------------------------------- CPU tests

def _torch_f64(x, dy, gamma, beta, rm, rv, relu, res):
    """torch.nn.functional.batch_norm in float64 with autograd."""
    leaf = lambda t: t.double().clone().requires_grad_(True)
    xl, gl, bl = leaf(x), leaf(gamma), leaf(beta)
    rl = leaf(res) if res is not None else None
    trm, trv = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xl, trm, trv, gl, bl, True, 1 - MOM, EPS)
    if rl is not None:
        y = y + rl
    if relu:
        y = F.relu(y)
    y.backward(dy.double())
    return y.detach(), trm, trv, xl.grad, gl.grad, bl.grad, (rl.grad if rl is not None else None)


@pytest.mark.parametrize("C,rows", [(8, 2), (24, 147), (40, 1000)])
def test_reference_matches_torch_float64(C, rows):
    d = make_inputs(C, rows, torch.bfloat16, seed=9)
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    close = lambda a, b, n: torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10, msg=n)
    for relu in (False, True):
        for res in (None, d["res"]):
            y, mean, invstd, nrm, nrv = ref_fwd(x, gamma, beta, d["rm"], d["rv"], True,
                                                relu, res)
            ty, trm, trv, tdx, tdg, tdb, tdres = _torch_f64(
                x, dy, gamma, beta, d["rm"], d["rv"], relu, res)
            close(y, ty, "y")
            close(nrm, trm, "running_mean")
            close(nrv, trv, "running_var")
            xd = x.double()
            close(mean, xd.mean(0), "save_mean")
            close(invstd, 1 / torch.sqrt(xd.var(0, unbiased=False) + EPS), "save_invstd")
            dx, dgamma, dbeta, dres, _, _ = ref_bwd(x, dy, gamma, mean, invstd, relu, y)
            close(dx, tdx, "dx")
            close(dgamma, tdg, "dgamma")
            close(dbeta, tdb, "dbeta")
            if res is not None:
                close(dres, tdres, "dres")
            # inference uses the running stats as given
            yi = ref_fwd(x, gamma, beta, d["rm"], d["rv"], False, relu, res)[0]
            ti = F.batch_norm(xd, d["rm"].double(), d["rv"].double(), gamma.double(),
                              beta.double(), False, 0.0, EPS)
            ti = ti + res.double() if res is not None else ti
            close(yi, F.relu(ti) if relu else ti, "infer y")
    # count == 1: the unbiased variance falls back to the biased one
    one = ref_fwd(x[:1], gamma, beta, d["rm"], d["rv"], True)
    close(one[4], d["rv"].double() * MOM, "running_var rows=1")
    # presummed statistics with a world-2 count equal the doubled batch
    xd = x.double()
    two = ref_fwd(x, gamma, beta, d["rm"], d["rv"], True, count=2 * rows,
                  sums=(2 * xd.sum(0), 2 * (xd * xd).sum(0)))
    dbl = ref_fwd(torch.cat([x, x]), gamma, beta, d["rm"], d["rv"], True)
    for a, b in zip(two[1:], dbl[1:]):
        close(a, b, "world=2 stats")
    close(ref_bwd(x, dy, gamma, dbl[1], dbl[2], world=2)[0],
          ref_bwd(torch.cat([x, x]), torch.cat([dy, dy]), gamma, dbl[1], dbl[2])[0][:rows],
          "world=2 dx")


def _measure_case(C, rows, dtype, offset=False):
    """-> stat deviations of the fp32 one-pass formula; asserts that torch's
    fp32 batch_norm + autograd, cast to dtype, passes the 16-bit check."""
    d = make_inputs(C, rows, dtype, offset=offset)
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    t = f"torch fp32 C={C} rows={rows} {dtype}"
    for relu in (False, True):
        for res in (None, d["res"]):
            leaf = lambda v: v.float().clone().requires_grad_(True)
            xl, gl, bl = leaf(x), leaf(gamma), leaf(beta)
            rl = leaf(res) if res is not None else None
            # torch.batch_norm: F.batch_norm refuses one value per channel
            y = torch.batch_norm(xl, gl, bl, None, None, True, 1 - MOM, EPS, False)
            y = y + rl if rl is not None else y
            y = F.relu(y) if relu else y
            y16 = y.detach().to(dtype)
            y.backward(dy.float())
            ry, mean, invstd, _, _ = ref_fwd(x, gamma, beta, d["rm"], d["rv"], True,
                                             relu, res)
            assert_16(y16, ry, f"{t} y")
            rdx, rdg, rdb, _, _, _ = ref_bwd(x, dy, gamma, mean, invstd, relu, y.detach())
            assert_16(xl.grad.to(dtype), rdx, f"{t} dx")
            assert_16(gl.grad.to(dtype), rdg, f"{t} dgamma")
            assert_16(bl.grad.to(dtype), rdb, f"{t} dbeta")
            yi = F.batch_norm(x.float(), d["rm"], d["rv"], gamma.float(), beta.float(),
                              False, 0.0, EPS)
            yi = yi + res.float() if res is not None else yi
            yi = F.relu(yi) if relu else yi
            assert_16(yi.to(dtype), ref_fwd(x, gamma, beta, d["rm"], d["rv"], False,
                                            relu, res)[0], f"{t} infer y")
    return _stat_devs(_fp32_onepass(x, d["rm"], d["rv"], dy), x, d["rm"], d["rv"], dy)


def test_torch_fp32_passes_tolerances():
    """The tolerance must never be what fails: torch's own fp32 BN passes the
    16-bit bound, and the fp32 one-pass formula passes the statistics bounds,
    at every shape the GPU tests use."""
    worst = {}
    for dtype in DTYPES:
        for C, rows in GRID + CHILD_CASES:
            for k, v in _measure_case(C, rows, dtype).items():
                worst[k] = max(worst.get(k, 0.0), v)
        for k, v in _measure_case(*OFFSET_CASE, dtype, offset=True).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("fp32 one-pass normalised deviations:", worst)
    for k, v in worst.items():
        assert v <= K_STAT[k], (k, v, K_STAT[k])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if "--child" in sys.argv:
        _child_main()
    elif "--measure" in sys.argv:
        worst = {}
        for dtype in DTYPES:
            cases = [(c, r, False) for c, r in GRID] + [(*OFFSET_CASE, True)]
            for C, rows, off in cases:
                for k, v in _measure_case(C, rows, dtype, off).items():
                    worst[k] = max(worst.get(k, 0.0), v)
        for k, v in worst.items():
            print(f"{k:8s} {v:.3e}")
