#!/usr/bin/env python3
"""Line-conv microbenchmark: the factorised Inception-v3 layers (17x17 1x7 /
7x1 at C = Ko in {128, 160, 192}; 8x8 1x3 / 3x1 at 384 -> 384 and 448 -> 384),
fwd, dgrad and wgrad, line kernels (lineconv.hip, lineconv_wgrad.hip) against
the generic per-axis path (conv_fwd_hw / conv_dgrad_hw / conv_wgrad_hw) on the
same inputs, timed alternately in one process. wgrad rows also carry the slice
count of the line kernel's plan.

Prints ms for both paths (median, [min .. max] over the rounds), the spread of
the repeated identical rounds (max / min - 1, the larger of the two paths),
and achieved TF/s counted from the shape: 2 N H W T C Ko per pass, border
taps included. A bit-for-bit check of the two paths on integer inputs runs
first; timings are refused if it fails.

    python tools/bench_lineconv.py [--batch 128] [--rounds 7] [--iters 200]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"

# (H = W, C, Ko, T)
SHAPES = [(17, 128, 128, 7), (17, 160, 160, 7), (17, 192, 192, 7),
          (8, 384, 384, 3), (8, 448, 384, 3)]


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def make(N, H, C, Ko, T, vertical, ints=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    rs = (T, 1) if vertical else (1, T)

    def draw(shape, scale=1.0):
        if ints:
            return torch.randint(-3, 4, shape, generator=g).bfloat16()
        return (torch.randn(shape, generator=g) * scale).bfloat16()

    return (nhwc(draw((N, C, H, H))), nhwc(draw((N, Ko, H, H))),
            nhwc(draw((Ko, C) + rs, 0.05)))


def passes(ext, x, dy, w, T, vertical):
    """{pass: (line, generic)} closures"""
    H = x.shape[2]
    ph, pw = (T // 2, 0) if vertical else (0, T // 2)
    rs = (T, 1) if vertical else (1, T)
    return {
        "fwd": (lambda: ext.lineconv_fwd(x, w),
                lambda: ext.conv_fwd_hw(x, w, 1, ph, pw)),
        "dgrad": (lambda: ext.lineconv_dgrad(dy, w),
                  lambda: ext.conv_dgrad_hw(dy, w, 1, ph, pw, H, H)),
        "wgrad": (lambda: ext.lineconv_wgrad(x, dy, T, vertical),
                  lambda: ext.conv_wgrad_hw(x, dy, *rs, 1, ph, pw)),
    }


def bitcheck(ext):
    """Integer inputs: both paths round the same exact fp32 sums once."""
    ok = True
    for H, C, Ko, T in SHAPES:
        for vertical in (False, True):
            x, dy, w = make(2, H, C, Ko, T, vertical, ints=True, seed=1)
            for name, (line, generic) in passes(ext, x, dy, w, T, vertical).items():
                good = torch.equal(line(), generic())
                ok &= good
                if not good:
                    print(f"bitcheck FAILED: {name} H={H} C={C} Ko={Ko} T={T} "
                          f"vertical={vertical}")
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lineconv: needs a GPU")
    from dtmx.ops.hip import require_ext
    ext = require_ext()

    if not bitcheck(ext):
        sys.exit("bench_lineconv: bitcheck failed, no timings")
    print(f"bitcheck ok ({len(SHAPES)} shapes x 2 orientations x fwd/dgrad/wgrad, "
          "line == generic)")
    print(f"batch {args.batch}, bf16 NHWC, stride 1; median of {args.rounds} "
          f"alternating rounds x {args.iters} calls [min .. max]")
    print("| HxW | C | Ko | kernel | pass | line ms | generic ms | generic/line "
          "| spread | line TF/s | generic TF/s | slices |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for H, C, Ko, T in SHAPES:
        for vertical in (False, True):
            x, dy, w = make(args.batch, H, C, Ko, T, vertical)
            flop = 2.0 * args.batch * H * H * T * C * Ko
            kern = f"{T}x1" if vertical else f"1x{T}"
            slices = ext.lineconv_wgrad_plan(Ko, C, T, vertical, args.batch, H, H)[1]
            for name, (line, generic) in passes(ext, x, dy, w, T, vertical).items():
                for _ in range(5):  # warm both paths on this shape
                    line()
                    generic()
                torch.cuda.synchronize()
                tl, tg = [], []
                for _ in range(args.rounds):
                    tl.append(time_ms(line, args.iters))
                    tg.append(time_ms(generic, args.iters))
                ml, mg = statistics.median(tl), statistics.median(tg)
                spread = max(max(tl) / min(tl), max(tg) / min(tg)) - 1
                print(f"| {H}x{H} | {C} | {Ko} | {kern} | {name} | "
                      f"{ml:.4f} [{min(tl):.4f} .. {max(tl):.4f}] | "
                      f"{mg:.4f} [{min(tg):.4f} .. {max(tg):.4f}] | {mg / ml:.2f}x | "
                      f"{100 * spread:.1f}% | {flop / ml * 1e-9:.1f} | "
                      f"{flop / mg * 1e-9:.1f} | {slices if name == 'wgrad' else ''} |",
                      flush=True)


if __name__ == "__main__":
    main()
