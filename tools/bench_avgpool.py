#!/usr/bin/env python3
"""Windowed average pool microbenchmark: the distinct 3x3 stride-1 pad-1
average-pool shapes of the four Inception families at their training
resolutions (inception-bn 224, the others 299), each with its model's
count_include_pad, fwd / bwd, hand HIP kernels (avgpool.hip) against the
parent path — bf16 channels_last F.avg_pool2d and its autograd, what the
models called before — timed alternately in one process.

Prints ms for both paths and the new kernel's effective bandwidth: the
minimal bytes the pass must move (read one tensor, write one of the same
size) over its time. A refcheck of the new kernels against the fp32 CPU
reference runs first; timings are refused if it fails.

    python tools/bench_avgpool.py [--batch 128] [--rounds 5] [--iters 20]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

DEV = "cuda:0"

# (C, H=W, count_include_pad, where)
SHAPES = [
    (192, 28, True, "bn 3a"), (256, 28, True, "bn 3b"),
    (576, 14, True, "bn 4a-4c"), (608, 14, True, "bn 4d"),
    (1056, 7, True, "bn 5a"),
    (192, 35, False, "v3 A1, irv2 stem"), (256, 35, False, "v3 A2"),
    (288, 35, False, "v3 A3"), (768, 17, False, "v3 C1-C4"),
    (1280, 8, False, "v3 E1"), (2048, 8, False, "v3 E2"),
    (384, 35, False, "v4 A"), (1024, 17, False, "v4 B"),
    (1536, 8, False, "v4 C"),
]
K, STRIDE, PAD = 3, 1, 1


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def make(N, C, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = nhwc(torch.randn(N, C, H, H, generator=g).bfloat16())
    dy = nhwc(torch.randn(N, C, H, H, generator=g).bfloat16())
    return x, dy


def passes(ext, x, dy, cip):
    """{pass: (new, parent)} closures. The parent's bwd is its own autograd
    over one F.avg_pool2d graph."""
    H = x.shape[2]
    xr = x.detach().requires_grad_(True)
    yr = F.avg_pool2d(xr, K, STRIDE, PAD, False, cip)
    return {
        "fwd": (lambda: ext.avgpool_fwd(x, K, STRIDE, PAD, cip),
                lambda: F.avg_pool2d(x, K, STRIDE, PAD, False, cip)),
        "bwd": (lambda: ext.avgpool_bwd(dy, H, H, K, STRIDE, PAD, cip),
                lambda: torch.autograd.grad(yr, xr, dy, retain_graph=True)[0]),
    }


def close(got, want):
    got, want = got.float(), want.float()
    atol = 0.02 * want.abs().mean().item() + 1e-3
    return bool(((got - want).abs() <= atol + 0.02 * want.abs()).all().item())


def refcheck(ext):
    """The new kernels against fp32 F.avg_pool2d and its autograd on the CPU,
    on a small batch of every shape. The parent path's largest error against
    the same reference is printed for information; it does not gate."""
    ok = True
    for C, H, cip, _ in SHAPES:
        x, dy = make(2, C, H, seed=1)
        xf = x.float().cpu().requires_grad_(True)
        yf = F.avg_pool2d(xf, K, STRIDE, PAD, False, cip)
        (dxf,) = torch.autograd.grad(yf, xf, dy.float().cpu())
        ref = {"fwd": yf.detach(), "bwd": dxf}
        for name, (new, old) in passes(ext, x, dy, cip).items():
            if not close(new().cpu(), ref[name]):
                ok = False
                print(f"refcheck FAILED: {name} C={C} H={H} count_include_pad={cip}")
            got = old().cpu()
            if not close(got, ref[name]):
                err = (got.float() - ref[name]).abs().max().item()
                print(f"note: parent {name} C={C} H={H} count_include_pad={cip} "
                      f"is outside tolerance of the fp32 CPU reference "
                      f"(max abs err {err:.3g})")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_avgpool: needs a GPU")
    from dtmx.ops.hip import require_ext
    ext = require_ext()

    if not refcheck(ext):
        sys.exit("bench_avgpool: refcheck failed, no timings")
    print(f"refcheck ok ({len(SHAPES)} shapes x fwd/bwd, new kernels vs fp32 CPU)")
    print(f"batch {args.batch}, bf16 NHWC, 3x3 s1 p1; median of {args.rounds} "
          f"alternating rounds x {args.iters} calls (min in brackets)")
    print("| C | H=W | incl. pad | where | pass | new ms | parent ms | "
          "parent/new | new TB/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    slower = []
    for C, H, cip, where in SHAPES:
        x, dy = make(args.batch, C, H)
        for name, (new, old) in passes(ext, x, dy, cip).items():
            for _ in range(3):  # warm both paths on this shape
                new()
                old()
            torch.cuda.synchronize()
            tn, to = [], []
            for _ in range(args.rounds):
                tn.append(time_ms(new, args.iters))
                to.append(time_ms(old, args.iters))
            mn, mo = statistics.median(tn), statistics.median(to)
            tbs = 2 * x.numel() * 2 / (mn * 1e-3) / 1e12
            if mn > mo:
                slower.append((C, H, name))
            print(f"| {C} | {H} | {cip} | {where} | {name} | "
                  f"{mn:.4f} [{min(tn):.4f}] | {mo:.4f} [{min(to):.4f}] | "
                  f"{mo / mn:.2f}x | {tbs:.2f} |", flush=True)
    print("native slower than parent on: " + (str(slower) if slower else "none"))


if __name__ == "__main__":
    main()
