#!/usr/bin/env python3
"""Stem-conv microbenchmark: the first layers of the zoo (3 input channels),
fwd and wgrad in bf16, the stem kernels (stemconv.hip) against the parent path
(x and w zero-padded to 8 channels with F.pad, the generic conv_fwd_stats /
conv_wgrad kernels, dw sliced back to 3 channels) on the same inputs, timed
alternately in one process. The parent's time includes its F.pad passes and
the dw slice: that is what a training step pays.

Prints ms for both paths (median, [min .. max] over the rounds) and the spread
of the repeated identical rounds (max / min - 1, the larger of the two paths).
A bit-for-bit check of the two paths on integer inputs runs first; timings are
refused if it fails.

    python tools/bench_stemconv.py [--batch 256] [--rounds 7] [--iters 50]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

DEV = "cuda:0"

# (name, H = W, Ko, R = S, stride, pad)
SHAPES = [("resnet 7x7 s2 p3", 224, 64, 7, 2, 3),
          ("inception 3x3 s2 p0", 299, 32, 3, 2, 0),
          ("mobilenet 3x3 s2 p1", 224, 32, 3, 2, 1),
          ("vgg 3x3 s1 p1", 224, 64, 3, 1, 1),
          ("cifar 3x3 s1 p1", 32, 64, 3, 1, 1)]
C = 3


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def make(N, H, Ko, R, stride, pad, ints=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = (H + 2 * pad - R) // stride + 1

    def draw(shape, scale=1.0):
        if ints:
            return torch.randint(-3, 4, shape, generator=g).bfloat16()
        return (torch.randn(shape, generator=g) * scale).bfloat16()

    return (nhwc(draw((N, C, H, H))), nhwc(draw((N, Ko, P, P))),
            nhwc(draw((Ko, C, R, R), 0.05)))


def passes(ext, x, dy, w, R, stride, pad):
    """{pass: (stem, parent)} closures; fwd with the fused BN statistics both
    ways, as Conv2dNHWC asks for them in training"""

    def pad8(t):
        return F.pad(t, (0, 0, 0, 0, 0, 8 - C)).contiguous(
            memory_format=torch.channels_last)

    def parent_wgrad():
        dw8 = ext.conv_wgrad(pad8(x), dy, R, R, stride, pad)
        return dw8[:, :C].contiguous(memory_format=torch.channels_last)

    return {
        "fwd": (lambda: ext.stemconv_fwd(x, w, stride, pad, pad, True)[0],
                lambda: ext.conv_fwd_stats(pad8(x), pad8(w), stride, pad)[0]),
        "wgrad": (lambda: ext.stemconv_wgrad(x, dy, R, R, stride, pad, pad, True),
                  parent_wgrad),
    }


def bitcheck(ext):
    """Integer inputs: both paths round the same exact fp32 sums once."""
    ok = True
    for name, H, Ko, R, stride, pad in SHAPES:
        x, dy, w = make(2, min(H, 64), Ko, R, stride, pad, ints=True, seed=1)
        for pname, (stem, parent) in passes(ext, x, dy, w, R, stride, pad).items():
            good = torch.equal(stem(), parent())
            ok &= good
            if not good:
                print(f"bitcheck FAILED: {pname} {name}")
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stemconv: needs a GPU")
    from dtmx.ops.hip import require_ext
    ext = require_ext()

    if not bitcheck(ext):
        sys.exit("bench_stemconv: bitcheck failed, no timings")
    print(f"bitcheck ok ({len(SHAPES)} shapes x fwd/wgrad, stem == parent)")
    print(f"batch {args.batch}, bf16 NHWC, C = {C}; median of {args.rounds} "
          f"alternating rounds x {args.iters} calls [min .. max]")
    print("| stem | HxW | Ko | pass | stem ms | parent ms | parent/stem | spread |")
    print("|---|---|---|---|---|---|---|---|")
    for name, H, Ko, R, stride, pad in SHAPES:
        x, dy, w = make(args.batch, H, Ko, R, stride, pad)
        for pname, (stem, parent) in passes(ext, x, dy, w, R, stride, pad).items():
            for _ in range(3):  # warm both paths on this shape
                stem()
                parent()
            torch.cuda.synchronize()
            ts, tp = [], []
            for _ in range(args.rounds):
                ts.append(time_ms(stem, args.iters))
                tp.append(time_ms(parent, args.iters))
            ms, mp = statistics.median(ts), statistics.median(tp)
            spread = max(max(ts) / min(ts), max(tp) / min(tp)) - 1
            print(f"| {name} | {H}x{H} | {Ko} | {pname} | "
                  f"{ms:.4f} [{min(ts):.4f} .. {max(ts):.4f}] | "
                  f"{mp:.4f} [{min(tp):.4f} .. {max(tp):.4f}] | {mp / ms:.2f}x | "
                  f"{100 * spread:.1f}% |", flush=True)


if __name__ == "__main__":
    main()
