#!/usr/bin/env python3
"""Grouped 3x3 microbenchmark: the seven distinct ResNeXt-50 (32x4d) conv2
shapes, fwd / dgrad / wgrad, hand HIP kernels (gconv.hip) against the parent
path — bf16 channels_last F.conv2d(groups=32) and its autograd, what
GroupedConv2dNHWC did before — timed alternately in one process.

Prints ms for both paths (median, [min .. max] over the rounds) and the new
kernel's effective bandwidth: the minimal bytes the pass must move (fwd: read
x + write y; dgrad: read dy + write dx; wgrad: read x + read dy; the weight
is at most 0.6 MB) over its time. A refcheck against the fp32 reference runs
first; timings are refused if it fails.

    python tools/bench_gconv.py [--batch 256] [--rounds 5] [--iters 20]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

DEV = "cuda:0"

# (C, H=W, stride): ResNeXt-50 conv2 layers, cardinality 32, pad 1
SHAPES = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1),
          (1024, 14, 2), (1024, 7, 1)]
GROUPS = 32
PAD = 1


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def make(N, C, H, stride, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = (H + 2 * PAD - 3) // stride + 1
    x = nhwc(torch.randn(N, C, H, H, generator=g).bfloat16())
    dy = nhwc(torch.randn(N, C, P, P, generator=g).bfloat16())
    # the weight as Module.bind leaves it: channels_last
    w = nhwc((torch.randn(C, C // GROUPS, 3, 3, generator=g) * 0.2).bfloat16())
    return x, dy, w, P


def passes(ext, x, dy, w, stride):
    """{pass: (new, parent)} closures. The parent's dgrad/wgrad are its own
    autograd: one F.conv2d graph per pass, backward for that input only."""
    H = x.shape[2]
    xr = x.detach().requires_grad_(True)
    yx = F.conv2d(xr, w, None, stride, PAD, 1, GROUPS)
    wr = w.detach().requires_grad_(True)
    yw = F.conv2d(x, wr, None, stride, PAD, 1, GROUPS)
    return {
        "fwd": (lambda: ext.gconv_fwd(x, w, stride, PAD, GROUPS),
                lambda: F.conv2d(x, w, None, stride, PAD, 1, GROUPS)),
        "dgrad": (lambda: ext.gconv_dgrad(dy, w, stride, PAD, GROUPS, H, H),
                  lambda: torch.autograd.grad(yx, xr, dy, retain_graph=True)[0]),
        "wgrad": (lambda: ext.gconv_wgrad(x, dy, stride, PAD, GROUPS, True),
                  lambda: torch.autograd.grad(yw, wr, dy, retain_graph=True)[0]),
    }


def min_bytes(name, x, dy):
    nx, ny = x.numel() * 2, dy.numel() * 2
    return {"fwd": nx + ny, "dgrad": ny + nx, "wgrad": nx + ny}[name]


def close(got, want):
    got, want = got.float(), want.float()
    atol = 0.02 * want.abs().mean().item() + 1e-3
    return bool(((got - want).abs() <= atol + 0.02 * want.abs()).all().item())


def refcheck(ext):
    """The new path against fp32 on a small batch of every shape."""
    ok = True
    for C, H, stride in SHAPES:
        x, dy, w, _ = make(2, C, H, stride, seed=1)
        xf = x.float().requires_grad_(True)
        wf = w.float().requires_grad_(True)
        yf = F.conv2d(xf, wf, None, stride, PAD, 1, GROUPS)
        dxf, dwf = torch.autograd.grad(yf, (xf, wf), dy.float())
        ref = {"fwd": yf.detach(), "dgrad": dxf, "wgrad": dwf}
        for name, (new, _old) in passes(ext, x, dy, w, stride).items():
            good = close(new(), ref[name])
            ok &= good
            if not good:
                print(f"refcheck FAILED: {name} C={C} H={H} s={stride}")
    return ok


def time_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def stats_ok(y, ps, pss, y_plain):
    """At the timed shape: y equals the plain entry's bits and the slab
    column totals are the fp64 sums over y within n * 2^-24 * sum|v|."""
    v = y.double().permute(1, 0, 2, 3).reshape(y.shape[1], -1)
    u = v.shape[1] * 2.0 ** -24
    return bool(torch.equal(y, y_plain)
                and ((ps.double().sum(0) - v.sum(1)).abs() <= u * v.abs().sum(1)).all()
                and ((pss.double().sum(0) - (v * v).sum(1)).abs()
                     <= u * (v * v).sum(1)).all())


def bench_stats(ext, args):
    """Forward + the following training BatchNorm (fused ReLU, packed mask):
    gconv_fwd_stats feeding bn_fwd_train its slabs, against the parent's
    gconv_fwd and the BatchNorm's own statistics pass. Also the two conv
    kernels alone, and the fused kernel's GB/s over x + y + both slabs."""
    print(f"batch {args.batch}, bf16 NHWC, groups {GROUPS}, pad 1; median "
          f"[min .. max] of {args.rounds} alternating rounds x {args.iters} calls")
    print("| C | H=W | s | fwd ms | fwd_stats ms | stats GB/s | slab rows | "
          "fwd + BN ms | fwd_stats + BN ms | parent/new |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for C, H, stride in SHAPES:
        x, _, w, _ = make(args.batch, C, H, stride)
        g, b = torch.ones(C, device=DEV).bfloat16(), torch.zeros(C, device=DEV).bfloat16()
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)

        def bn(y, ps=None, pss=None):
            return ext.bn_fwd_train(y, g, b, rm, rv, 0.9, 1e-5, True, None, ps, pss, True)

        fns = {
            "fwd": lambda: ext.gconv_fwd(x, w, stride, PAD, GROUPS),
            "fwd_stats": lambda: ext.gconv_fwd_stats(x, w, stride, PAD, GROUPS),
            "old": lambda: bn(ext.gconv_fwd(x, w, stride, PAD, GROUPS)),
            "new": lambda: bn(*ext.gconv_fwd_stats(x, w, stride, PAD, GROUPS)),
        }
        y, ps, pss = fns["fwd_stats"]()
        if not stats_ok(y, ps, pss, fns["fwd"]()):
            sys.exit(f"bench_gconv: stats check failed C={C} H={H} s={stride}")
        nbytes = (x.numel() + y.numel()) * 2 + 2 * ps.numel() * 4
        for _ in range(3):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, f in fns.items():
                t[k].append(time_ms(f, args.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = lambda k: f"{med[k]:.4f} [{min(t[k]):.4f} .. {max(t[k]):.4f}]"
        print(f"| {C} | {H} | {stride} | {cell('fwd')} | {cell('fwd_stats')} | "
              f"{nbytes / (med['fwd_stats'] * 1e-3) / 1e9:.0f} | {ps.shape[0]} | "
              f"{cell('old')} | {cell('new')} | {med['old'] / med['new']:.3f}x |",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stats", action="store_true",
                    help="time the fused BN-statistics forward instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gconv: needs a GPU")
    from dtmx.ops.hip import require_ext
    ext = require_ext()
    if args.stats:
        return bench_stats(ext, args)

    if not refcheck(ext):
        sys.exit("bench_gconv: refcheck failed, no timings")
    print(f"refcheck ok ({len(SHAPES)} shapes x fwd/dgrad/wgrad vs fp32)")
    print(f"batch {args.batch}, bf16 NHWC, groups {GROUPS}, pad 1; median of "
          f"{args.rounds} alternating rounds x {args.iters} calls [min .. max]")
    print("| C | Cg | H=W | s | pass | new ms | parent ms | parent/new | new TB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for C, H, stride in SHAPES:
        x, dy, w, _ = make(args.batch, C, H, stride)
        for name, (new, old) in passes(ext, x, dy, w, stride).items():
            for _ in range(3):  # warm both paths on this shape
                new()
                old()
            torch.cuda.synchronize()
            tn, to = [], []
            for _ in range(args.rounds):
                tn.append(time_ms(new, args.iters))
                to.append(time_ms(old, args.iters))
            mn, mo = statistics.median(tn), statistics.median(to)
            tbs = min_bytes(name, x, dy) / (mn * 1e-3) / 1e12
            print(f"| {C} | {C // GROUPS} | {H} | {stride} | {name} | "
                  f"{mn:.4f} [{min(tn):.4f} .. {max(tn):.4f}] | "
                  f"{mo:.4f} [{min(to):.4f} .. {max(to):.4f}] | {mo / mn:.2f}x | "
                  f"{tbs:.2f} |", flush=True)


if __name__ == "__main__":
    main()
