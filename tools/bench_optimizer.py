#!/usr/bin/env python3
"""Optimizer-step microbenchmark on the ResNet-50 parameter list (161
parameters, 25.6 M elements; sizes only, no model run): the fused flat-bucket
steps — SGD (softmax_opt.hip), NAG and LBSGD (optimizer.hip), LBSGD also split
into its norm stage 1, norm stage 2 and update launches — and the per-tensor
`NAG` / `LBSGD` loops of dtmx/optimizer/optimizer.py (what Module ran for them
before the fused path), all over bf16 parameters with fp32 masters and momenta
in one process, timed in alternating rounds.

Prints ms per step, the ratio to fused SGD measured in the same run, and the
effective bandwidth of the fused steps from the byte model: per element SGD
and NAG read g 2 B + master 4 B + mom 4 B and write mom 4 B + master 4 B +
w 2 B = 20 B; LBSGD's norm pass re-reads g and master, 26 B.

    python tools/bench_optimizer.py [--rounds 7] [--iters 50] [--loop-iters 5]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

DEV = "cuda:0"
HYP = dict(lr=1e-3, momentum=0.9, wd=1e-4, rescale=1.0 / 256, clip=0.0, eta=1e-3)


def resnet50_shapes():
    """Parameter shapes of ResNet-50 v1 (1000 classes) in definition order."""
    def bn(c):
        return [(c,), (c,)]
    shapes = [(64, 3, 7, 7)] + bn(64)
    cin = 64
    for mid, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        out = 4 * mid
        for b in range(blocks):
            shapes += [(mid, cin, 1, 1)] + bn(mid)
            shapes += [(mid, mid, 3, 3)] + bn(mid)
            shapes += [(out, mid, 1, 1)] + bn(out)
            if b == 0:
                shapes += [(out, cin, 1, 1)] + bn(out)
            cin = out
    return shapes + [(1000, 2048), (1000,)]


def make_params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in shapes:
        fan = 1
        for d in s[1:]:
            fan *= d
        w = torch.randn(s, generator=g) * (1.0 / max(fan, 1)) ** 0.5 + (1.0 if len(s) == 1 else 0.0)
        out.append(torch.nn.Parameter(w.bfloat16().to(DEV)))
    return out


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loop-iters", type=int, default=5,
                    help="steps per round of the per-tensor loops")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optimizer: needs a GPU")
    from dtmx.ops.hip import require_ext
    from dtmx.optimizer.optimizer import LBSGD, NAG, Updater
    from dtmx.parallel.bucketer import GradBucketer

    ext = require_ext()
    shapes = resnet50_shapes()
    params = make_params(shapes, 0)
    n = sum(p.numel() for p in params)
    b = GradBucketer(params, flatten_params=True)
    gg = torch.Generator().manual_seed(1)
    for buf in b.flat:
        buf.copy_((torch.randn(buf.numel(), generator=gg) * 2.0).bfloat16())
    tabs = b.segment_tables()
    h = HYP
    args5 = (h["lr"], h["momentum"], h["wd"], h["rescale"], h["clip"])

    def norm(stages):
        def run():
            for bi, t in enumerate(tabs):
                ext.seg_sqnorm(b.flat[bi], b.flat_master[bi], t.chunk_start,
                               t.chunk_len, t.seg_chunk_off, t.seg_off, t.part,
                               t.sq, t.seg_lr, h["lr"], h["wd"], h["rescale"],
                               h["clip"], h["eta"], None, stages)
        return run

    def lbsgd_update():
        for bi, t in enumerate(tabs):
            ext.lbsgd_mom_mp(b.flat_w[bi], b.flat[bi], b.flat_master[bi],
                             b.flat_mom[bi], t.chunk_seg, t.chunk_start,
                             t.chunk_len, t.seg_lr, t.seg_off, h["momentum"],
                             h["wd"], h["rescale"], h["clip"])

    # per-tensor loops on their own copies of the parameters
    def loop(opt):
        ws = [p.detach().clone() for p in make_params(shapes, 0)]
        gs = [torch.randn(w.shape, device=DEV).mul_(2.0).to(w.dtype) for w in ws]
        upd = Updater(opt)

        def run():
            for i, (w, g) in enumerate(zip(ws, gs)):
                upd(i, g, w)
        return run

    common = dict(momentum=h["momentum"], learning_rate=h["lr"], wd=h["wd"],
                  rescale_grad=h["rescale"], multi_precision=True)
    cases = [
        ("fused SGD", lambda: b.fused_sgd_step(*args5), args.iters, 20),
        ("fused NAG", lambda: b.fused_nag_step(*args5), args.iters, 20),
        ("fused LBSGD (norms + update)",
         lambda: b.fused_lbsgd_step(*args5, h["eta"]), args.iters, 26),
        ("  LBSGD norm stage 1", norm(1), args.iters, 6),
        ("  LBSGD norm stage 2", norm(2), args.iters, None),
        ("  LBSGD update", lbsgd_update, args.iters, 20),
        ("per-tensor NAG loop", loop(NAG(**common)), args.loop_iters, None),
        ("per-tensor LBSGD loop", loop(LBSGD(eta=h["eta"], **common)),
         args.loop_iters, None),
    ]
    for _, fn, _, _ in cases:                    # warm every path
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in cases}
    for _ in range(args.rounds):
        for name, fn, iters, _ in cases:
            times[name].append(time_ms(fn, iters))
    for t in b.flat_master:
        assert torch.isfinite(t).all()

    print(f"ResNet-50 parameter list: {len(shapes)} parameters, {n} elements, "
          f"{len(b.flat)} bucket(s), {sum(t.nchunks for t in tabs)} chunks of "
          f"<= {ext.opt_chunk()}; bf16 + fp32 master/momentum; median of "
          f"{args.rounds} alternating rounds x {args.iters} steps "
          f"({args.loop_iters} for the per-tensor loops), min in brackets")
    print("| step | ms | vs fused SGD | B/elem | TB/s |")
    print("|---|---|---|---|---|")
    sgd = statistics.median(times["fused SGD"])
    for name, _, _, bpe in cases:
        med, lo = statistics.median(times[name]), min(times[name])
        bw = f"{bpe * n / (med * 1e-3) / 1e12:.2f}" if bpe else "-"
        print(f"| {name} | {med:.4f} [{lo:.4f}] | {med / sgd:.2f}x | "
              f"{bpe or '-'} | {bw} |", flush=True)
    fused = statistics.median(times["fused LBSGD (norms + update)"])
    print(f"fused LBSGD / fused SGD = {fused / sgd:.2f} (byte model 1.30); "
          f"per-tensor LBSGD loop / fused LBSGD = "
          f"{statistics.median(times['per-tensor LBSGD loop']) / fused:.1f}; "
          f"per-tensor NAG loop / fused NAG = "
          f"{statistics.median(times['per-tensor NAG loop']) / statistics.median(times['fused NAG']):.1f}")


if __name__ == "__main__":
    main()
