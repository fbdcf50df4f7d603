"""Fused flat-bucket LBSGD / NAG steps (dtmx/csrc/optimizer.hip) against fp64
references, from the kernels up to Module.

Conventions of test_elem_gpu.py: inputs are rounded to the 16-bit dtype first,
the reference is fp64 on those rounded values on the CPU (hyperparameters
rounded to fp32, the format the kernels take them in), every case runs in bf16
and fp16, and each test prints its figures before asserting. The flats of the
kernel-level tests start at an odd element offset of their allocation, so no
segment is 4-byte aligned by accident.
"""
import math
import pickle

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
both_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])

from dtmx.parallel.bucketer import OPT_CHUNK as CHUNK  # noqa: E402

SIZES = [1, 7, 8, 9, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]

# Largest relative error of seg_lr against the fp64 rule measured on an MI355X
# over test_random_norms_and_seg_lr's cases (docs/KERNELS.md, "Optimizer");
# the test bound is twice that.
SEG_LR_MEASURED = 8.989e-8
SEG_LR_BOUND = 2 * SEG_LR_MEASURED
# A chunk sums CHUNK/256 terms serially, then an 8-level tree, in fp32; chunks
# are summed in fp64. Above this on sq is a bug, not rounding.
SQ_SANITY = 32 * 2.0 ** -24


def ext():
    from dtmx.ops.hip import require_ext
    return require_ext()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(n, seed, scale=1.0):
    return torch.randn((n,), generator=gen(seed)) * scale


def f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def odd(t):
    """Copy of the 1-D CPU tensor t on the GPU, one element into its buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t)
    return buf[1:]


def tables(sizes):
    from dtmx.parallel.bucketer import SegmentTables
    return SegmentTables(sizes, torch.device(DEV))


def ulp(dtype, ref):
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(ref.double().abs())[1] - 1
    e = torch.where(ref == 0, torch.full_like(e, emin), e).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - mant).double())


def check_ulp(got, ref, dtype, n, name):
    e = ((got.double().cpu() - ref).abs() / ulp(dtype, ref)).max().item()
    print(f"{name}: max error {e:.3f} ulp (bound {n})")
    assert got.dtype == dtype and e <= n, f"{name}: {e:.3f} ulp > {n}"


def assert_close(got, want, rtol, atol, name):
    torch.testing.assert_close(got.double().cpu(), want.double(), rtol=rtol,
                               atol=atol, msg=lambda m: f"{name}: {m}")


def check_update(w, m, v, master_ref, mom_ref, dtype, name):
    """The criteria of test_elem_sgd_mom_mp."""
    assert_close(m, master_ref, 1e-5, 1e-6, name + " master")
    assert_close(v, mom_ref, 1e-5, 1e-6, name + " mom")
    check_ulp(w, master_ref, dtype, 1, name + " w")
    assert torch.equal(w, m.to(dtype))          # w is the rounded master


def pre_g(g16, rs, clip):
    gv = g16.double() * f32(rs)
    if clip > 0:
        gv = gv.clamp(-f32(clip), f32(clip))
    return gv


def sq_ref(g16, master, seg_off, rs, clip):
    gv, m = pre_g(g16, rs, clip), master.double()
    return torch.stack([torch.stack([(m[a:b] ** 2).sum(), (gv[a:b] ** 2).sum()])
                        for a, b in zip(seg_off, seg_off[1:])])


def seg_lr_rule(sq, lr, wd, eta):
    """The rule of LBSGD.update, in fp64."""
    out = []
    for sw, sg in sq.tolist():
        wn, gn, r = math.sqrt(sw), math.sqrt(sg), f32(lr)
        if wn > 0 and gn > 0:
            r = min(f32(lr) * (f32(eta) * wn / (gn + f32(wd) * wn + 1e-12)), f32(lr))
        out.append(r)
    return torch.tensor(out, dtype=torch.float64)


def lbsgd_rule(g16, master, mom, seg_off, seg_lr, mu, wd, rs, clip):
    """fp64 LBSGD update with the given per-segment learning rates."""
    lr = torch.cat([torch.full((b - a,), float(seg_lr[s]), dtype=torch.float64)
                    for s, (a, b) in enumerate(zip(seg_off, seg_off[1:]))])
    gv = pre_g(g16, rs, clip) + f32(wd) * master.double()
    mom_ref = f32(mu) * mom.double() - lr * gv
    return master.double() + mom_ref, mom_ref


def nag_rule(g16, master, mom, lr, mu, wd, rs, clip):
    gv = pre_g(g16, rs, clip) + f32(wd) * master.double()
    mom_ref = f32(mu) * mom.double() + gv
    return master.double() - f32(lr) * (gv + f32(mu) * mom_ref), mom_ref


def run_sqnorm(t, g, m, lr, wd, rs, clip, eta, hyper=None):
    ext().seg_sqnorm(g, m, t.chunk_start, t.chunk_len, t.seg_chunk_off, t.seg_off,
                     t.part, t.sq, t.seg_lr, lr, wd, rs, clip, eta, hyper)
    return t.sq.cpu().clone(), t.seg_lr.cpu().clone()


def run_lbsgd(t, w, g, m, v, lr, mu, wd, rs, clip, eta, hyper=None):
    run_sqnorm(t, g, m, lr, wd, rs, clip, eta, hyper)
    if hyper is None:
        ext().lbsgd_mom_mp(w, g, m, v, t.chunk_seg, t.chunk_start, t.chunk_len,
                           t.seg_lr, t.seg_off, mu, wd, rs, clip)
    else:
        ext().lbsgd_mom_mp_dev(w, g, m, v, t.chunk_seg, t.chunk_start,
                               t.chunk_len, t.seg_lr, t.seg_off, hyper)


# ================================================== 4. integer-exact norms ==

@both_dtypes
def test_integer_exact_norms(dtype):
    sizes = SIZES + [2 ** 20]
    t = tables(sizes)
    n = sum(sizes)
    m = torch.randint(-4, 5, (n,), generator=gen(10)).float()
    g = torch.randint(-4, 5, (n,), generator=gen(11)).float().to(dtype)
    want = sq_ref(g, m, t.seg_off.tolist(), 1.0, 0.0)
    assert want.max().item() <= 2 ** 24
    t.part.fill_(float("nan"))                  # the workspace needs no zero fill
    sq, _ = run_sqnorm(t, odd(g), odd(m), 0.1, 0.0, 1.0, 0.0, 0.001)
    bad = (sq != want).sum().item()
    print(f"integer norms: {bad} of {want.numel()} sums differ")
    assert sq.dtype == torch.float64 and torch.equal(sq, want)


# ============================================ 5. random norms and seg_lr ==

NORM_SIZES = [1, 7, 257, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5, 1000, 1000, 5000,
              9, 256, CHUNK, 70 * CHUNK + 3]
ZERO_W, ZERO_G = 6, 7              # all-zero weights / all-zero gradients
BIG_G = [0, 2, 4, 8, 10, 12]       # gradients x1000: trust ratio below 1


@both_dtypes
@pytest.mark.parametrize("clip_on", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_random_norms_and_seg_lr(wd, clip_on, dtype):
    """N(0,1) weights and N(0,1e-3) gradients at rescale 1/256 give a trust
    ratio of 256 (wd 0) or about 9.6 (wd 1e-4) at eta 1e-3, capped at lr;
    segments whose gradients are scaled by 1000 give about 0.25, below 1."""
    lr, eta, rs = 0.1, 1e-3, 1.0 / 256
    t = tables(NORM_SIZES)
    off = t.seg_off.tolist()
    n = off[-1]
    m, g = randn(n, 20), randn(n, 21, 1e-3)
    m[off[ZERO_W]:off[ZERO_W + 1]] = 0
    g[off[ZERO_G]:off[ZERO_G + 1]] = 0
    for s in BIG_G:
        g[off[s]:off[s + 1]] *= 1000
    g = g.to(dtype)
    clip = 0.5 * (g.double() * f32(rs)).abs().max().item() if clip_on else 0.0
    want_sq = sq_ref(g, m, off, rs, clip)
    want_lr = seg_lr_rule(want_sq, lr, wd, eta)
    ratio = want_lr / f32(lr)
    capped = [s for s in range(len(NORM_SIZES)) if s not in BIG_G]
    assert (ratio[BIG_G] < 0.6).all() and (ratio[capped] == 1).all()

    sq, seg_lr = run_sqnorm(t, odd(g), odd(m), lr, wd, rs, clip, eta)
    nz = want_sq > 0
    e_sq = ((sq - want_sq).abs()[nz] / want_sq[nz]).max().item()
    e_lr = ((seg_lr.double() - want_lr).abs() / want_lr).max().item()
    print(f"sq: max rel error {e_sq:.3e} (sanity {SQ_SANITY:.3e}); "
          f"seg_lr: max rel error {e_lr:.3e} (bound {SEG_LR_BOUND:.3e})")
    assert torch.equal(sq[~nz], want_sq[~nz])           # zero stays zero
    assert e_sq <= SQ_SANITY
    assert seg_lr.dtype == torch.float32
    # capped segments, all-zero weights and all-zero gradients: lr exactly
    assert torch.equal(seg_lr[capped], torch.full((len(capped),), lr).float())
    assert e_lr <= SEG_LR_BOUND

    # device hyperparameters: bit-equal
    hyper = torch.tensor([lr, 0.9, wd, rs, clip, eta], dtype=torch.float32, device=DEV)
    sq2, seg_lr2 = run_sqnorm(t, odd(g), odd(m), 0, 0, 0, 0, 0, hyper)
    assert torch.equal(sq2, sq) and torch.equal(seg_lr2, seg_lr)


# =============================================================== 6. update ==

UPD = dict(lr=0.1, mu=0.9, wd=1e-4, rs=0.5)


def _update_inputs(n, dtype):
    """The inputs of test_elem_sgd_mom_mp: no update cancels its weight."""
    master = randn(n, 700)
    master = torch.where(master < 0, master - 1, master + 1)
    mom = randn(n, 701, 0.1)
    g = (randn(n, 702, 2.0) + (3.0 if n == 1 else 0.0)).to(dtype)
    return master, mom, g


@both_dtypes
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_lbsgd_update(clip, dtype):
    h, eta = UPD, (0.2 if clip else 0.5)    # trust ratios 0.8 .. 1 (capped)
    t = tables(SIZES)
    off = t.seg_off.tolist()
    master, mom, g = _update_inputs(off[-1], dtype)
    w, m, v, gd = odd(master.to(dtype)), odd(master), odd(mom), odd(g)
    run_lbsgd(t, w, gd, m, v, h["lr"], h["mu"], h["wd"], h["rs"], clip, eta)
    seg_lr = t.seg_lr.cpu()
    want_lr = seg_lr_rule(sq_ref(g, master, off, h["rs"], clip), h["lr"], h["wd"], eta)
    r = (seg_lr.double() / f32(h["lr"])).tolist()
    print("seg_lr / lr:", ["%.3f" % x for x in r])
    assert min(r) < 1 and max(r) == 1
    e_lr = ((seg_lr.double() - want_lr).abs() / want_lr).max().item()
    print(f"seg_lr: max rel error {e_lr:.3e} (sanity {SQ_SANITY:.3e})")
    assert e_lr <= SQ_SANITY
    master_ref, mom_ref = lbsgd_rule(g, master, mom, off, seg_lr, h["mu"], h["wd"],
                                     h["rs"], clip)
    check_update(w, m, v, master_ref, mom_ref, dtype, "lbsgd")

    w2, m2, v2 = odd(master.to(dtype)), odd(master), odd(mom)
    hyper = torch.tensor([h["lr"], h["mu"], h["wd"], h["rs"], clip, eta],
                         dtype=torch.float32, device=DEV)
    run_lbsgd(t, w2, gd, m2, v2, 0, 0, 0, 0, 0, 0, hyper)
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(v2, v)


@both_dtypes
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_lbsgd_capped_is_sgd(clip, dtype):
    """One segment whose trust ratio is >= 1 runs at lr: bit-equal to
    sgd_mom_mp on the same inputs."""
    h, n = UPD, 2 ** 20 + 5
    t = tables([n])
    master, mom, g = _update_inputs(n, dtype)
    w, m, v, gd = odd(master.to(dtype)), odd(master), odd(mom), odd(g)
    run_lbsgd(t, w, gd, m, v, h["lr"], h["mu"], h["wd"], h["rs"], clip, 100.0)
    assert t.seg_lr.cpu().item() == f32(h["lr"])
    w2, m2, v2 = odd(master.to(dtype)), odd(master), odd(mom)
    ext().sgd_mom_mp(w2, gd, m2, v2, h["lr"], h["mu"], h["wd"], h["rs"], clip)
    assert torch.equal(w, w2) and torch.equal(m, m2) and torch.equal(v, v2)


# ================================================================== 7. NAG ==

@both_dtypes
@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("mu", [0.0, 0.9])
@pytest.mark.parametrize("n", [1, 1000, 2 ** 20 + 5])
def test_nag_mom_mp(n, mu, clip, dtype):
    h = UPD
    master, mom, g = _update_inputs(n, dtype)
    master_ref, mom_ref = nag_rule(g, master, mom, h["lr"], mu, h["wd"], h["rs"], clip)
    if mu == 0:      # plain master -= lr * g
        gv = pre_g(g, h["rs"], clip) + f32(h["wd"]) * master.double()
        assert torch.equal(master_ref, master.double() - f32(h["lr"]) * gv)
    w, m, v, gd = odd(master.to(dtype)), odd(master), odd(mom), odd(g)
    ext().nag_mom_mp(w, gd, m, v, h["lr"], mu, h["wd"], h["rs"], clip)
    check_update(w, m, v, master_ref, mom_ref, dtype, "nag")

    w2, m2, v2 = odd(master.to(dtype)), odd(master), odd(mom)
    hyper = torch.tensor([h["lr"], mu, h["wd"], h["rs"], clip],
                         dtype=torch.float32, device=DEV)
    ext().nag_mom_mp_dev(w2, gd, m2, v2, hyper)
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(v2, v)


# ===================================================== binding refusals ==

def test_binding_checks():
    t = tables([5, 3])
    g = torch.zeros(8, dtype=torch.bfloat16, device=DEV)
    m = torch.zeros(8, device=DEV)
    args = lambda **k: dict(dict(
        grad=g, master=m, chunk_start=t.chunk_start, chunk_len=t.chunk_len,
        seg_chunk_off=t.seg_chunk_off, seg_off=t.seg_off, part=t.part, sq=t.sq,
        seg_lr=t.seg_lr, lr=0.1, wd=0.0, rescale=1.0, clip=0.0, eta=0.001), **k)
    ext().seg_sqnorm(**args())
    for bad, msg in [
        (dict(grad=g.float()), "bfloat16/float16"),
        (dict(master=m[:7]), "differ in length"),
        (dict(chunk_start=t.chunk_start.long()), "chunk_start must be int32"),
        (dict(chunk_len=t.chunk_len.cpu()), "device of the flats"),
        (dict(seg_off=torch.tensor([0, 6, 5, 8], dtype=torch.int32)), "non-decreasing"),
        (dict(seg_off=torch.tensor([0, 5, 7], dtype=torch.int32)), "end at numel"),
    ]:
        with pytest.raises(RuntimeError, match=msg):
            ext().seg_sqnorm(**args(**bad))
    with pytest.raises(RuntimeError, match="differ in length"):
        ext().nag_mom_mp(g, g[:7], m, m.clone(), 0.1, 0.9, 0.0, 1.0, 0.0)


# ========================== 8. placement invariance and determinism ==

PLACE_SHAPES = [(1,), (7,), (257,), (CHUNK + 1,), (3 * CHUNK + 5,), (16, 8, 3, 3),
                (33, 65), (9,)]


def _bucketer_run(bucket_mb, dtype=torch.bfloat16):
    from dtmx.parallel.bucketer import GradBucketer

    params = [torch.nn.Parameter(randn(math.prod(s), 800 + i).view(s).to(dtype).to(DEV))
              for i, s in enumerate(PLACE_SHAPES)]
    b = GradBucketer(params, bucket_mb=bucket_mb, flatten_params=True)
    for step in range(2):
        for i, p in enumerate(params):
            with torch.no_grad():
                p.grad.copy_(randn(p.numel(), 900 + 10 * step + i, 0.3)
                             .view(p.shape).to(dtype))
        b.fused_lbsgd_step(0.1, 0.9, 1e-4, 0.5, 0.25, 0.02)
    out = {}
    for bi, bucket in enumerate(b.buckets):
        off = 0
        for si, p in enumerate(bucket):
            i = next(k for k, q in enumerate(params) if q is p)
            out[i] = (b.flat_master[bi][off:off + p.numel()].cpu().clone(),
                      b.segment_tables()[bi].seg_lr.cpu()[si].item())
            off += p.numel()
    b.detach()
    return len(b.buckets), out


def test_placement_invariance_and_determinism():
    n_small, small = _bucketer_run(1e-3)
    n_big, big = _bucketer_run(64)
    print(f"buckets: {n_small} vs {n_big}")
    assert n_small >= 4 and n_big == 1
    lrs = [big[i][1] for i in range(len(PLACE_SHAPES))]
    assert min(lrs) < f32(0.1)                  # the trust ratio is in play
    for i in range(len(PLACE_SHAPES)):
        assert small[i][1] == big[i][1], i
        assert torch.equal(small[i][0], big[i][0]), i
    _, again = _bucketer_run(64)
    for i in range(len(PLACE_SHAPES)):
        assert torch.equal(again[i][0], big[i][0]), i


# ================================== 9. no host sync, capturable ==

def test_no_host_sync_and_graph_capture():
    from dtmx.parallel.bucketer import GradBucketer

    dtype = torch.bfloat16
    params = [torch.nn.Parameter(randn(math.prod(s), 820 + i).view(s).to(dtype).to(DEV))
              for i, s in enumerate(PLACE_SHAPES)]
    b = GradBucketer(params, bucket_mb=0.02, flatten_params=True)
    assert len(b.buckets) > 1
    with torch.no_grad():
        for i, p in enumerate(params):
            p.grad.copy_(randn(p.numel(), 920 + i, 0.3).view(p.shape).to(dtype))
    hp = [0.1, 0.9, 1e-4, 0.5, 0.25, 0.02]
    hyper = torch.tensor(hp, dtype=torch.float32, device=DEV)
    lr1 = torch.tensor(hp, dtype=torch.float32, device=DEV)
    lr2 = lr1.clone()
    lr1[0], lr2[0] = 0.05, 0.2
    b.segment_tables()                           # tables are uploaded once
    torch.cuda.synchronize()

    torch.cuda.set_sync_debug_mode("error")
    try:
        b.fused_lbsgd_step(*hp, hyper=hyper)
        b.fused_lbsgd_step(*hp)
    finally:
        torch.cuda.set_sync_debug_mode("default")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            b.fused_lbsgd_step(*hp, hyper=hyper)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    saved = [t.clone() for t in b.state_tensors()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.fused_lbsgd_step(*hp, hyper=hyper)
    hyper.copy_(lr1)
    graph.replay()
    hyper.copy_(lr2)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in b.state_tensors()]

    with torch.no_grad():
        for dst, src in zip(b.state_tensors(), saved):
            dst.copy_(src)
    b.fused_lbsgd_step(0.05, *hp[1:])
    b.fused_lbsgd_step(0.2, *hp[1:])
    torch.cuda.synchronize()
    for got, want, old in zip(replayed, b.state_tensors(), saved):
        assert torch.equal(got, want)
        assert not torch.equal(got, old)
    b.detach()


# ============================ 10. agreement with the per-tensor classes ==

AGREE_SIZES = [1, 257, CHUNK + 1, 3 * CHUNK + 5]


@both_dtypes
@pytest.mark.parametrize("kind", ["lbsgd", "nag"])
def test_agrees_with_per_tensor_class(kind, dtype):
    """Two steps of the per-tensor class (CPU, fp32 master) and of the fused
    GPU step from the same start, each against the fp64 rule. One step of an
    fp32 master is good to rtol 1e-5 / atol 1e-6 of the fp64 rule (the
    criterion of test_elem_sgd_mom_mp), two steps to twice that; the two
    paths then differ by at most the sum of their bounds."""
    from dtmx.optimizer.optimizer import LBSGD, NAG

    lr, mu, wd, rs, clip, eta = 0.1, 0.9, 1e-4, 0.5, 0.5, 0.2   # trust ratio ~0.85
    common = dict(momentum=mu, learning_rate=lr, wd=wd, rescale_grad=rs,
                  clip_gradient=clip, multi_precision=True)
    if kind == "lbsgd":
        opt = LBSGD(eta=eta, warmup_strategy="linear", warmup_epochs=1,
                    updates_per_epoch=4, **common)
    else:
        opt = NAG(**common)
    t = tables(AGREE_SIZES)
    off = t.seg_off.tolist()
    n = off[-1]
    master0 = _update_inputs(n, dtype)[0].to(dtype).float()   # master = w exactly
    grads = [randn(n, 710 + s, 2.0).to(dtype) for s in range(2)]

    # per-tensor class on the CPU
    ws = [master0[a:b].to(dtype).clone() for a, b in zip(off, off[1:])]
    states = [opt.create_state_multi_precision(i, w) for i, w in enumerate(ws)]
    for g in grads:
        for i, (a, b) in enumerate(zip(off, off[1:])):
            opt.update_multi_precision(i, ws[i], g[a:b], states[i])
    pt_master = torch.cat([s[0] for s in states])
    assert opt.num_update == 2

    # fused step on the GPU, lr as Module.update derives it
    w, m, v = odd(master0.to(dtype)), odd(master0), odd(torch.zeros(n))
    for step, g in enumerate(grads, 1):
        if kind == "lbsgd":
            run_lbsgd(t, w, odd(g), m, v, opt.warmup_lr(lr, step), mu, wd, rs, clip, eta)
        else:
            ext().nag_mom_mp(w, odd(g), m, v, lr, mu, wd, rs, clip)

    # fp64 rule
    rm, rv = master0.double(), torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(grads, 1):
        if kind == "lbsgd":
            step_lr = opt.warmup_lr(lr, step)
            seg = seg_lr_rule(sq_ref(g, rm, off, rs, clip), step_lr, wd, eta)
            rm, rv = lbsgd_rule(g, rm, rv, off, seg, mu, wd, rs, clip)
        else:
            rm, rv = nag_rule(g, rm, rv, lr, mu, wd, rs, clip)

    tol = 2 * (1e-5 * rm.abs() + 1e-6)
    d_fused = (m.double().cpu() - rm).abs()
    d_pt = (pt_master.double() - rm).abs()
    d_both = (m.double().cpu() - pt_master.double()).abs()
    print(f"{kind}: fused-fp64 {(d_fused / tol).max():.4f}, per-tensor-fp64 "
          f"{(d_pt / tol).max():.4f}, fused-per-tensor {(d_both / (2 * tol)).max():.4f} "
          f"of the bound; max |fused - per-tensor| {d_both.max():.3e}")
    assert (d_fused <= tol).all() and (d_pt <= tol).all()
    assert (d_both <= 2 * tol).all()
    assert torch.equal(w, m.to(dtype))


# ===================================================== 11. Module level ==

def _gpu_mlp(optimizer, lr_mult=None, **params):
    import dtmx
    from dtmx.io import DataBatch
    from dtmx.models import get_symbol
    from dtmx.optimizer import create as opt_create

    torch.manual_seed(0)
    net = get_symbol("mlp", num_classes=10, input_dim=64)
    mod = dtmx.Module(net, context=dtmx.gpu(0))
    mod.bind(data_shapes=[("data", (8, 64))], label_shapes=[("softmax_label", (8,))],
             dtype=torch.bfloat16)
    mod.init_params()
    p = dict(learning_rate=0.1, momentum=0.9, wd=1e-4)
    p.update(params)
    if lr_mult is not None:
        opt = opt_create(optimizer, rescale_grad=1.0 / 8, multi_precision=True, **p)
        opt.lr_mult = lr_mult
        mod.init_optimizer(optimizer=opt)
    else:
        mod.init_optimizer(optimizer=optimizer, optimizer_params=tuple(p.items()))
    g = gen(3)
    data = torch.randn(8, 64, generator=g).to(torch.bfloat16).to(DEV)
    label = torch.randint(0, 10, (8,), generator=g).float().to(DEV)
    return mod, DataBatch(data=[data], label=[label])


def _segments(b):
    return [[0] + torch.tensor([p.numel() for p in bucket]).cumsum(0).tolist()
            for bucket in b.buckets]


@pytest.mark.parametrize("kind", ["lbsgd", "nag"])
def test_module_fused_step_matches_rule(kind):
    mod, batch = _gpu_mlp(kind, eta=0.05, clip_gradient=0.05, warmup_epochs=1,
                          updates_per_epoch=4) if kind == "lbsgd" else \
        _gpu_mlp(kind, clip_gradient=0.05)
    assert mod._use_fused_sgd and mod._fused_kind == kind
    opt, b = mod._optimizer, mod._bucketer
    for step in (1, 2):
        mod.forward_backward(batch)
        snap = [(g.cpu().clone(), m.cpu().clone(), v.cpu().clone())
                for g, m, v in zip(b.flat, b.flat_master, b.flat_mom)]
        mod.update()
        lr = opt.warmup_lr(0.1, step) if kind == "lbsgd" else 0.1
        for bi, (g, m, v) in enumerate(snap):
            off = _segments(b)[bi]
            if kind == "lbsgd":
                seg = seg_lr_rule(sq_ref(g, m, off, 1 / 8, 0.05), lr, 1e-4, 0.05)
                got = b.segment_tables()[bi].seg_lr.cpu().double()
                e_lr = ((got - seg).abs() / seg).max().item()
                print(f"seg_lr: max rel error {e_lr:.3e} (sanity {SQ_SANITY:.3e})")
                assert e_lr <= SQ_SANITY
                rm, rv = lbsgd_rule(g, m, v, off, seg, 0.9, 1e-4, 1 / 8, 0.05)
            else:
                rm, rv = nag_rule(g, m, v, lr, 0.9, 1e-4, 1 / 8, 0.05)
            for a, e in zip(off, off[1:]):      # per parameter
                check_update(b.flat_w[bi][a:e], b.flat_master[bi][a:e],
                             b.flat_mom[bi][a:e], rm[a:e], rv[a:e],
                             torch.bfloat16, f"{kind} step {step} bucket {bi}")
    assert opt.num_update == 2
    assert any(g.abs().max().item() > 0 for g, _, _ in snap)


@pytest.mark.parametrize("kind", ["lbsgd", "nag"])
@pytest.mark.parametrize("why", ["env", "lr_mult"])
def test_module_falls_back_to_per_tensor(kind, why, monkeypatch):
    if why == "env":
        monkeypatch.setenv("DTMX_FUSED_OPT", "0")
        mod, batch = _gpu_mlp(kind)
    else:
        mod, batch = _gpu_mlp(kind, lr_mult={"fc1_weight": 0.5})
    assert mod._use_fused_sgd is False and mod._fused_kind is None
    assert not mod._bucketer.flatten_params
    before = [p.detach().clone() for p in mod.symbol.parameters()]
    losses = []
    for _ in range(3):
        mod.forward_backward(batch)
        mod.update()
        losses.append(mod._loss.item())
    assert all(math.isfinite(v) for v in losses)
    assert any(not torch.equal(a, c) for a, c in zip(before, mod.symbol.parameters()))


def test_module_env_knob_leaves_sgd_alone(monkeypatch):
    monkeypatch.setenv("DTMX_FUSED_OPT", "0")
    mod, _ = _gpu_mlp("sgd")
    assert mod._use_fused_sgd and mod._fused_kind == "sgd"


def test_module_states_roundtrip_and_kind(tmp_path):
    mod, batch = _gpu_mlp("lbsgd", eta=0.05)
    for _ in range(2):
        mod.forward_backward(batch)
        mod.update()
    b = mod._bucketer
    fname = str(tmp_path / "lbsgd.states")
    mod.save_optimizer_states(fname)
    with open(fname, "rb") as f:
        payload = pickle.load(f)
    assert payload["fused"] is True and payload["kind"] == "lbsgd"
    assert set(payload) == {"fused", "kind", "master", "mom", "num_update"}
    want = [t.clone() for t in b.flat_master + b.flat_mom]

    mod2, _ = _gpu_mlp("lbsgd", eta=0.05)
    mod2.load_optimizer_states(fname)
    b2 = mod2._bucketer
    assert mod2._optimizer.num_update == 2
    for got, ref in zip(b2.flat_master + b2.flat_mom, want):
        assert torch.equal(got, ref)
    for wb, mb in zip(b2.flat_w, b2.flat_master):
        assert torch.equal(wb, mb.to(wb.dtype))

    sgd, batch = _gpu_mlp("sgd")
    sgd.forward_backward(batch)
    sgd.update()
    sgd_name = str(tmp_path / "sgd.states")
    sgd.save_optimizer_states(sgd_name)
    with pytest.raises(ValueError, match="'sgd'.*'lbsgd'"):
        mod2.load_optimizer_states(sgd_name)
    # a payload from before the key existed is SGD's
    with open(sgd_name, "rb") as f:
        old = pickle.load(f)
    assert old.pop("kind") == "sgd"
    old_name = str(tmp_path / "old.states")
    with open(old_name, "wb") as f:
        pickle.dump(old, f)
    sgd.load_optimizer_states(old_name)
    with pytest.raises(ValueError, match="'sgd'.*'lbsgd'"):
        mod2.load_optimizer_states(old_name)


def test_module_sgd_calls_unchanged():
    mod, batch = _gpu_mlp("sgd", clip_gradient=0.5)
    assert mod._fused_kind == "sgd"
    b, calls = mod._bucketer, []
    orig = b.fused_sgd_step
    b.fused_sgd_step = lambda *a, **k: calls.append((a, k)) or orig(*a, **k)
    b.fused_lbsgd_step = b.fused_nag_step = None
    mod.forward_backward(batch)
    mod.update()
    assert calls == [((0.1, 0.9, 1e-4, 1.0 / 8, 0.5), {"hyper": None})]
    assert b._seg_tables is None                # nothing built for plain SGD
