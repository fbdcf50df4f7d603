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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gconv: needs a GPU")
    from dtmx.ops.hip import require_ext
    ext = require_ext()

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
