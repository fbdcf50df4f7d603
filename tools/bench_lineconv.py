#!/usr/bin/env python3
"""Line-conv microbenchmark: the factorised Inception-v3 layers (17x17 1x7 /
7x1 at C = Ko in {128, 160, 192}; 8x8 1x3 / 3x1 at 384 -> 384 and 448 -> 384),
fwd, dgrad and wgrad, line kernels (lineconv.hip, lineconv_wgrad.hip) against
the generic per-axis path (conv_fwd_hw / conv_dgrad_hw / conv_wgrad_hw) on the
same inputs, timed alternately in one process. wgrad rows also carry the slice
count of the line kernel's plan. Tx1 rows time the column strip kernel
(colconv.hip, fwd and dgrad) as a third path, and two Tx1-only shapes add a
tall image (35x35, two bands) and one outside the line kernels' envelope
(8x44, halo 264), where the line columns stay empty.

Prints ms for the paths (median, [min .. max] over the rounds), the spread of
the repeated identical rounds (max / min - 1, the largest of the paths),
and achieved TF/s counted from the shape: 2 N H W T C Ko per pass, border
taps included. A bit-for-bit check of the paths on integer inputs runs
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

# (H, W, C, Ko, T, orientations: vertical False = 1xT, True = Tx1)
SHAPES = [(17, 17, 128, 128, 7, (False, True)), (17, 17, 160, 160, 7, (False, True)),
          (17, 17, 192, 192, 7, (False, True)), (8, 8, 384, 384, 3, (False, True)),
          (8, 8, 448, 384, 3, (False, True)), (35, 35, 192, 192, 7, (True,)),
          (8, 44, 128, 128, 7, (True,))]


def nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def make(N, H, W, C, Ko, T, vertical, ints=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    rs = (T, 1) if vertical else (1, T)

    def draw(shape, scale=1.0):
        if ints:
            return torch.randint(-3, 4, shape, generator=g).bfloat16()
        return (torch.randn(shape, generator=g) * scale).bfloat16()

    return (nhwc(draw((N, C, H, W))), nhwc(draw((N, Ko, H, W))),
            nhwc(draw((Ko, C) + rs, 0.05)))


def passes(ext, x, dy, w, T, vertical):
    """{pass: {path: closure}}; a path that does not serve the shape is absent"""
    H, W = x.shape[2:]
    ph, pw = (T // 2, 0) if vertical else (0, T // 2)
    rs = (T, 1) if vertical else (1, T)
    out = {"fwd": {"generic": lambda: ext.conv_fwd_hw(x, w, 1, ph, pw)},
           "dgrad": {"generic": lambda: ext.conv_dgrad_hw(dy, w, 1, ph, pw, H, W)},
           "wgrad": {"generic": lambda: ext.conv_wgrad_hw(x, dy, *rs, 1, ph, pw)}}
    if not vertical or (T - 1) * W <= 256:  # the line kernels' envelope
        out["fwd"]["line"] = lambda: ext.lineconv_fwd(x, w)
        out["dgrad"]["line"] = lambda: ext.lineconv_dgrad(dy, w)
        out["wgrad"]["line"] = lambda: ext.lineconv_wgrad(x, dy, T, vertical)
    if vertical:
        out["fwd"]["col"] = lambda: ext.colconv_fwd(x, w)
        out["dgrad"]["col"] = lambda: ext.colconv_dgrad(dy, w)
    return out


def bitcheck(ext):
    """Integer inputs: every path rounds the same exact fp32 sums once."""
    ok, n = True, 0
    for H, W, C, Ko, T, orients in SHAPES:
        for vertical in orients:
            x, dy, w = make(2, H, W, C, Ko, T, vertical, ints=True, seed=1)
            for name, paths in passes(ext, x, dy, w, T, vertical).items():
                want = paths.pop("generic")()
                for path, fn in paths.items():
                    good = torch.equal(fn(), want)
                    ok &= good
                    n += 1
                    if not good:
                        print(f"bitcheck FAILED: {path} {name} {H}x{W} C={C} "
                              f"Ko={Ko} T={T} vertical={vertical}")
    return ok, n


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

    ok, n = bitcheck(ext)
    if not ok:
        sys.exit("bench_lineconv: bitcheck failed, no timings")
    print(f"bitcheck ok ({n} line / column results == generic)")
    print(f"batch {args.batch}, bf16 NHWC, stride 1; median of {args.rounds} "
          f"alternating rounds x {args.iters} calls [min .. max]")
    print("| HxW | C | Ko | kernel | pass | line ms | generic ms | generic/line "
          "| spread | line TF/s | generic TF/s | slices | col ms | generic/col "
          "| line/col | col TF/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for H, W, C, Ko, T, orients in SHAPES:
        for vertical in orients:
            x, dy, w = make(args.batch, H, W, C, Ko, T, vertical)
            flop = 2.0 * args.batch * H * W * T * C * Ko
            kern = f"{T}x1" if vertical else f"1x{T}"
            for name, paths in passes(ext, x, dy, w, T, vertical).items():
                for _ in range(5):  # warm every path on this shape
                    for fn in paths.values():
                        fn()
                torch.cuda.synchronize()
                ts = {p: [] for p in paths}
                for _ in range(args.rounds):
                    for p, fn in paths.items():
                        ts[p].append(time_ms(fn, args.iters))
                med = {p: statistics.median(v) for p, v in ts.items()}
                spread = max(max(v) / min(v) for v in ts.values()) - 1

                def ms(p):
                    return (f"{med[p]:.4f} [{min(ts[p]):.4f} .. {max(ts[p]):.4f}]"
                            if p in med else "")

                def ratio(p, q):
                    return f"{med[p] / med[q]:.2f}x" if p in med and q in med else ""

                def tf(p):
                    return f"{flop / med[p] * 1e-9:.1f}" if p in med else ""

                slices = (ext.lineconv_wgrad_plan(Ko, C, T, vertical, args.batch, H, W)[1]
                          if name == "wgrad" and "line" in med else "")
                print(f"| {H}x{W} | {C} | {Ko} | {kern} | {name} | {ms('line')} | "
                      f"{ms('generic')} | {ratio('generic', 'line')} | "
                      f"{100 * spread:.1f}% | {tf('line')} | {tf('generic')} | "
                      f"{slices} | {ms('col')} | {ratio('generic', 'col')} | "
                      f"{ratio('line', 'col')} | {tf('col')} |", flush=True)


if __name__ == "__main__":
    main()
