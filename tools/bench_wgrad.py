#!/usr/bin/env python3
"""Wgrad NT per-shape micro: TF/s + implied HBM traffic, for the roofline
question 'is the 20%-of-step wgrad family bandwidth-bound or schedule-bound?'
Run under rocprofv3 --pmc FETCH_SIZE,WRITE_SIZE to get true fetched bytes."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from dtmx.ops.hip import require_ext

ext = require_ext()
DEV = "cuda:0"


def timeit(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main(bs=1024):
    torch.manual_seed(0)
    # (C_in, K_out, H, stride, pad) resnet50 3x3 representatives + stem-adjacent
    shapes = [(128, 128, 28, 1, 1), (256, 256, 14, 1, 1), (512, 512, 7, 1, 1),
              (64, 64, 56, 1, 1)]
    for (C, Ko, H, st, pa) in shapes:
        x = torch.randn(bs, C, H, H, dtype=torch.bfloat16, device=DEV).contiguous(
            memory_format=torch.channels_last)
        dy = torch.randn(bs, Ko, H, H, dtype=torch.bfloat16, device=DEV).contiguous(
            memory_format=torch.channels_last)
        s = timeit(lambda: ext.conv_wgrad(x, dy, 3, 3, st, pa))
        fl = 2.0 * bs * H * H * Ko * C * 9
        # minimum HBM traffic: dy once, x once, dw out (tiny)
        min_gb = (dy.numel() + x.numel()) * 2 / 1e9
        print(f"wgrad3x3 bs{bs} {C}->{Ko} {H}^2: {fl/s/1e12:7.1f} TF  "
              f"{s*1e3:7.3f} ms  min-traffic {min_gb:5.2f} GB -> "
              f"{min_gb/s/1e3:5.2f} TB/s floor", flush=True)


# ResNet-50 (v1.5) wgrad shapes with Ko >= 256 and R*S*C >= 256: all of
# layer3 / layer4 and the 1x1 downsample convs at the head of layer2-4.
# (name, C_in, K_out, H_in, R, stride, pad)
NT256_SHAPES = [
    ("l2.ds   1x1s2", 256, 512, 56, 1, 2, 0),
    ("l3.0.c1 1x1", 512, 256, 28, 1, 1, 0),
    ("l3.0.c2 3x3s2", 256, 256, 28, 3, 2, 1),
    ("l3.ds   1x1s2", 512, 1024, 28, 1, 2, 0),
    ("l3.x.c1 1x1", 1024, 256, 14, 1, 1, 0),
    ("l3.x.c2 3x3", 256, 256, 14, 3, 1, 1),
    ("l3.x.c3 1x1", 256, 1024, 14, 1, 1, 0),
    ("l4.0.c1 1x1", 1024, 512, 14, 1, 1, 0),
    ("l4.0.c2 3x3s2", 512, 512, 14, 3, 2, 1),
    ("l4.ds   1x1s2", 1024, 2048, 14, 1, 2, 0),
    ("l4.x.c1 1x1", 2048, 512, 7, 1, 1, 0),
    ("l4.x.c2 3x3", 512, 512, 7, 3, 1, 1),
    ("l4.x.c3 1x1", 512, 2048, 7, 1, 1, 0),
]


def _cdiv(a, b):
    return (a + b - 1) // b


def nt256(bs, new, sweep, rounds=3):
    """Per-shape old-vs-new wgrad in ONE process, alternating. ext.conv_wgrad
    runs the old routing (the caller set DTMX_DISABLE_NT256=1 before the
    extension's first call); the new kernel runs through
    ext.conv_wgrad_nt256 with the split-K / grouping the routing plans for
    the shape (ext.wgrad_nt256_plan). Implied traffic = dy re-read once per
    n-tile + the im2col view of x once per m-tile, for each path's tile."""
    torch.manual_seed(0)
    for (name, C, Ko, H, R, st, pa) in NT256_SHAPES:
        P = (H + 2 * pa - R) // st + 1
        x = torch.randn(bs, C, H, H, dtype=torch.bfloat16, device=DEV).contiguous(
            memory_format=torch.channels_last)
        dy = torch.randn(bs, Ko, P, P, dtype=torch.bfloat16, device=DEV).contiguous(
            memory_format=torch.channels_last)
        npq, rsc = bs * P * P, R * R * C
        fl = 2.0 * npq * Ko * rsc
        ktiles = _cdiv(npq, 64)

        def gb(tile):
            return (npq * Ko * 2 * _cdiv(rsc, tile) +
                    npq * rsc * 2 * _cdiv(Ko, tile)) / 1e9

        use, sk, grp = ext.wgrad_nt256_plan(Ko, rsc, npq)
        tiles = _cdiv(Ko, 256) * _cdiv(rsc, 256)
        cfgs = [("plan", sk, grp)] if new else []
        if new and sweep:
            for tgt in (128, 256, 512):
                k = max(1, min(ktiles, tgt // tiles))
                cfgs.append((f"t{tgt}", k, False))
                # grouped: slices a multiple of 8
                k8 = max(8, (k // 8) * 8)
                cfgs.append((f"t{tgt}g", min(ktiles, k8), True))
        res = {"old": []}
        for _ in range(rounds):
            res["old"].append(timeit(lambda: ext.conv_wgrad(x, dy, R, R, st, pa)))
            for (cn, k, g) in cfgs:
                res.setdefault((cn, k, g), []).append(timeit(
                    lambda: ext.conv_wgrad_nt256(x, dy, R, R, st, pa, k, g)))
        so = sorted(res["old"])[len(res["old"]) // 2]
        print(f"{name} bs{bs} {C}->{Ko} {H}^2 tiles256={tiles} routed={int(use)}: "
              f"old {fl/so/1e12:6.1f} TF {so*1e3:7.3f} ms "
              f"implied {gb(128)/so/1e3:5.2f} TB/s", flush=True)
        for key, v in res.items():
            if key == "old":
                continue
            s = sorted(v)[len(v) // 2]
            print(f"    nt256 {key[0]:6s} splitk={key[1]:4d} group={int(key[2])}: "
                  f"{fl/s/1e12:6.1f} TF {s*1e3:7.3f} ms "
                  f"implied {gb(256)/s/1e3:5.2f} TB/s  x{so/s:5.3f} vs old",
                  flush=True)
        del x, dy


def triad():
    """bf16 RW-mix ceilings for the BN elementwise kernels: what does THIS
    box sustain on d=a+b (2R+1W, the bn_bwd_dx mix) and b=a*s (1R+1W, the
    bn_apply mix)? Quantifies how close 4.9-5.0 TB/s is to attainable."""
    n = 1024 * 256 * 56 * 56  # the bn micro shape's element count
    a = torch.randn(n, dtype=torch.bfloat16, device=DEV)
    b = torch.randn_like(a)
    d = torch.empty_like(a)
    s = timeit(lambda: torch.add(a, b, out=d), iters=20)
    print(f"triad d=a+b  (2R+1W): {3 * n * 2 / s / 1e12:5.2f} TB/s")
    s = timeit(lambda: torch.mul(a, 1.5, out=d), iters=20)
    print(f"scale b=a*s  (1R+1W): {2 * n * 2 / s / 1e12:5.2f} TB/s")


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default=None,
                    help="'triad', or the batch size of the 3x3 micro")
    ap.add_argument("--nt256", type=int, choices=[0, 1], default=None,
                    help="layer3/4 + downsample shapes: 0 = old routing only, "
                         "1 = old and the 256^2 kernel alternating")
    ap.add_argument("--sweep", action="store_true",
                    help="with --nt256 1: also sweep split-K targets "
                         "128/256/512 with and without XCD grouping")
    ap.add_argument("--bs", type=int, default=4096,
                    help="per-GPU batch for --nt256 (flagship: 4096)")
    args = ap.parse_args()
    if args.nt256 is not None:
        # conv_wgrad reads the flag once, at its first call
        os.environ["DTMX_DISABLE_NT256"] = "1"
        nt256(args.bs, bool(args.nt256), args.sweep)
    elif args.what == "triad":
        triad()
    else:
        main(int(args.what) if args.what else 1024)
