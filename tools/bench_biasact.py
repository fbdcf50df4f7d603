#!/usr/bin/env python3
"""Fused bias + ReLU microbenchmark: the bias convs and hidden FCs of VGG-16,
AlexNet and GoogLeNet (3a, 5b), forward and backward, the fused path
(DF.conv2d_bias_act / DF.linear(relu=True): conv_fwd_act, bias_act_bwd) against
the three-op sequence it replaces (conv -> broadcast add -> relu and their
autograd, what DTMX_FALLBACK=biasact runs), timed alternately in one process
after a warm-up of each.

Prints ms for both paths (median, [min .. max] over the rounds). The backward
column is the whole backward of the layer (mask + bias gradient, dgrad,
wgrad); dgrad and wgrad are the same kernels on both sides. Timings are
refused if the fused forward is not bit-equal to the unfused one on
integer-valued operands of the timed shape (exact sums: the split-K routes add
with fp32 atomics, whose order changes the last bit of a random sum on either
path).

    python tools/bench_biasact.py [--batch 128] [--rounds 5] [--iters 10]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"

# (name, C, Ko, kernel, stride, pad, H=W); kernel 0: FC with C -> Ko features
LAYERS = [
    ("vgg 224", 64, 64, 3, 1, 1, 224), ("vgg 112", 128, 128, 3, 1, 1, 112),
    ("vgg 56", 256, 256, 3, 1, 1, 56), ("vgg 28", 512, 512, 3, 1, 1, 28),
    ("vgg 14", 512, 512, 3, 1, 1, 14),
    ("alex 1", 3, 64, 11, 4, 2, 224), ("alex 2", 64, 192, 5, 1, 2, 27),
    ("alex 3", 192, 384, 3, 1, 1, 13), ("alex 4", 384, 256, 3, 1, 1, 13),
    ("alex 5", 256, 256, 3, 1, 1, 13),
    ("3a 1x1", 192, 64, 1, 1, 0, 28), ("3a 3x3r", 192, 96, 1, 1, 0, 28),
    ("3a 3x3", 96, 128, 3, 1, 1, 28), ("3a 5x5r", 192, 16, 1, 1, 0, 28),
    ("3a 5x5", 16, 32, 5, 1, 2, 28), ("3a proj", 192, 32, 1, 1, 0, 28),
    ("5b 1x1", 832, 384, 1, 1, 0, 7), ("5b 3x3r", 832, 192, 1, 1, 0, 7),
    ("5b 3x3", 192, 384, 3, 1, 1, 7), ("5b 5x5r", 832, 48, 1, 1, 0, 7),
    ("5b 5x5", 48, 128, 5, 1, 2, 7), ("5b proj", 832, 128, 1, 1, 0, 7),
    ("fc 25088", 25088, 4096, 0, 0, 0, 0), ("fc 4096", 4096, 4096, 0, 0, 0, 0),
]


def make(layer, N, integer=False):
    """(fused, unfused) forward closures over shared leaves, and the leaves
    whose gradient the layer's backward computes. integer: operands in
    [-2, 2], so every sum is exact whatever the order of the split-K atomics."""
    from dtmx.ops import functional as DF
    _, C, Ko, k, stride, pad, H = layer
    g = torch.Generator().manual_seed(0)

    def leaf(shape, scale):
        t = (torch.randint(-2, 3, shape, generator=g) if integer
             else torch.randn(shape, generator=g) * scale).bfloat16().to(DEV)
        return t.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else t

    b = leaf((Ko,), 1.0).requires_grad_()
    if k == 0:
        x, w = leaf((N, C), 1.0).requires_grad_(), leaf((Ko, C), 0.01).requires_grad_()
        return (lambda: DF.linear(x, w, b, relu=True),
                lambda: DF.relu(DF.linear(x, w, b)), (x, w, b))
    x = leaf((N, C, H, H), 1.0).requires_grad_(C % 8 == 0)  # the image needs none
    w = leaf((Ko, C, k, k), (C * k * k) ** -0.5).requires_grad_()
    return (lambda: DF.conv2d_bias_act(x, w, b, True, stride, pad),
            lambda: DF.relu(DF.conv2d(x, w, stride, pad) + b.reshape(1, -1, 1, 1)),
            tuple(t for t in (x, w, b) if t.requires_grad))


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--routed", action="store_true",
                    help="the fused side as DF routes it (its forward gate on); "
                         "default: the fused forward on every layer")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_biasact: needs a GPU")
    from dtmx.ops import functional as DF
    if "biasact" in DF._FALLBACK:
        sys.exit("bench_biasact: DTMX_FALLBACK=biasact leaves nothing to compare")
    if not args.routed:
        DF._biasact_fwd_routed = lambda *a: True
    print(f"batch {args.batch}, bf16 NHWC, fused forward "
          f"{'as routed' if args.routed else 'on every layer'}; "
          f"median [min .. max] of {args.rounds} "
          f"alternating rounds x {args.iters} calls")
    print("| layer | C | Ko | k | H=W | pass | fused ms | unfused ms | unfused/fused |")
    print("|---|---|---|---|---|---|---|---|---|")
    for layer in LAYERS:
        fused, unfused, _ = make(layer, args.batch, integer=True)
        if not torch.equal(fused(), unfused()):
            sys.exit(f"bench_biasact: fused forward differs from unfused on {layer}")
        fused, unfused, leaves = make(layer, args.batch)
        yf, yu = fused(), unfused()
        dy = torch.randn_like(yf)
        fns = {"fwd": (fused, unfused),
               "bwd": tuple((lambda y=y: torch.autograd.grad(y, leaves, dy,
                                                             retain_graph=True))
                            for y in (yf, yu))}
        for name, (new, old) in fns.items():
            for _ in range(3):  # warm both paths on this shape
                new()
                old()
            torch.cuda.synchronize()
            tn, to = [], []
            for _ in range(args.rounds):
                tn.append(time_ms(new, args.iters))
                to.append(time_ms(old, args.iters))
            mn, mo = statistics.median(tn), statistics.median(to)
            print(f"| {layer[0]} | {layer[1]} | {layer[2]} | {layer[3] or 'fc'} | "
                  f"{layer[6] or '-'} | {name} | "
                  f"{mn:.4f} [{min(tn):.4f} .. {max(tn):.4f}] | "
                  f"{mo:.4f} [{min(to):.4f} .. {max(to):.4f}] | {mo / mn:.3f}x |",
                  flush=True)
        del fused, unfused, leaves, yf, yu, dy, fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
