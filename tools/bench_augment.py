#!/usr/bin/env python3
"""Device-side augmentation benchmark (augment.hip, ImageRecordIter).

kernel   augment_batch at B=256, 500x375 sources to 224x224, bf16 out: a
         random-resized-crop + mirror plan per image, without and with
         contrast (the gmean pre-pass). Prints ms per call and the effective
         bandwidth: the bytes the pass must move (the source pixels inside
         each crop once + the output once) over its time. A refcheck against
         the torch CPU path runs first; timings are refused if it fails.
iter     img/s of ImageRecordIter on a synthetic JPEG .rec (500x375, q90) at
         --threads workers: the fp32 CPU path (resize, random crop, mirror)
         against the staged path with the same flags and with the full
         augmenter set, alternating, each consumer ending in a device batch
         in bf16 channels_last (the first path through the Module's copy,
         cast and re-layout).

    python tools/bench_augment.py [--mode kernel|iter|both] [--batch 256]
"""
import argparse
import os
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

DEV = "cuda:0"
SH, SW, TH, TW = 375, 500, 224, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_batch(ext, B, contrast, seed=0):
    rng = np.random.RandomState(seed)
    src = torch.from_numpy(rng.randint(0, 256, B * SH * SW * 3, dtype=np.uint8))
    geom = torch.tensor([[i * SH * SW * 3, SH, SW] for i in range(B)])
    cfg = dict(th=TH, tw=TW, random_resized_crop=True, min_random_area=0.08,
               max_random_area=1.0, min_aspect_ratio=0.75, max_aspect_ratio=1.333,
               rand_mirror=True, brightness=0.4, saturation=0.4, pca_noise=0.1)
    if contrast:
        cfg["contrast"] = 0.4
    par = torch.stack([ext.aug_plan(cfg, seed, 1, i, SH, SW) for i in range(B)])
    crop = ((par[:, 7] - par[:, 6] + 1) * (par[:, 9] - par[:, 8] + 1)).sum().item()
    nbytes = crop * 3 + B * TH * TW * 3 * 2
    return src, geom, par, nbytes


def time_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def bench_kernel(ext, args):
    from dtmx.io.augment import augment_batch

    for contrast in (False, True):  # refcheck at a small batch
        src, geom, par, _ = make_batch(ext, 4, contrast, seed=1)
        want = augment_batch(src, geom, par, MEAN, STD, TH, TW, torch.float32)
        got = augment_batch(src.to(DEV), geom, par, MEAN, STD, TH, TW,
                            torch.float32).cpu()
        err = (got - want).abs().max().item() * 255 * min(STD)
        if not err < 0.05:
            sys.exit(f"bench_augment: refcheck failed (contrast={contrast}, "
                     f"max err {err:.3g} level), no timings")
    print("refcheck ok (kernel vs torch CPU path, both plans)")
    print(f"B={args.batch}, {SW}x{SH} -> {TW}x{TH}, bf16 NHWC out; median of "
          f"{args.rounds} rounds x {args.iters} calls (min in brackets)")
    print("| contrast | ms | GB/s effective | Mpix/s out |")
    print("|---|---|---|---|")
    for contrast in (False, True):
        src, geom, par, nbytes = make_batch(ext, args.batch, contrast)
        d = [t.to(DEV) for t in (src, geom, par)]

        def run():
            return augment_batch(d[0], d[1], d[2], MEAN, STD, TH, TW,
                                 torch.bfloat16, geom_host=geom, par_host=par)

        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ts = [time_ms(run, args.iters) for _ in range(args.rounds)]
        m = statistics.median(ts)
        print(f"| {contrast} | {m:.4f} [{min(ts):.4f}] | "
              f"{nbytes / (m * 1e-3) / 1e9:.1f} | "
              f"{args.batch * TH * TW / (m * 1e-3) / 1e6:.0f} |", flush=True)


def write_jpeg_rec(ext, path, n):
    rng = np.random.RandomState(0)
    ys, xs = np.mgrid[0:SH, 0:SW]
    recs = []
    for i in range(n):  # smooth gradients plus noise: photo-like JPEG sizes
        im = np.stack([(ys + i * 7) % 256, (xs + i * 11) % 256,
                       ((ys + xs) // 2 + i * 5) % 256], -1)
        im = np.clip(im + rng.randint(-12, 13, im.shape), 0, 255).astype(np.uint8)
        recs.append(struct.pack("<IfQQ", 0, float(i % 1000), i, 0)
                    + ext.encode_jpeg(im.tobytes(), SH, SW, 3, 90))
    ext.write_recordio(path, recs)


def bench_iter(ext, args):
    from dtmx.io import ImageRecordIter

    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "bench.rec")
    n = args.records
    write_jpeg_rec(ext, path, n)
    common = dict(preprocess_threads=args.threads, rand_mirror=True, resize=256,
                  mean_r=MEAN[0], mean_g=MEAN[1], mean_b=MEAN[2], std_r=STD[0],
                  std_g=STD[1], std_b=STD[2])
    full = dict(common, random_resized_crop=True, min_random_area=0.08,
                max_aspect_ratio=0.25, brightness=0.4, contrast=0.4,
                saturation=0.4, pca_noise=0.1)
    full.pop("resize")
    paths = {
        "cpu fp32 path (resize, crop, mirror)": dict(common, rand_crop=True),
        "staged, same flags": dict(common, rand_crop=True, device=DEV),
        "staged, full augmenter set": dict(full, device=DEV),
    }

    def epoch(kw):
        it = ImageRecordIter(path, (3, TH, TW), args.batch, **kw)
        it.next()  # workers are up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seen = 0
        for b in it:
            x = b.data[0].to(DEV, non_blocking=True).to(torch.bfloat16) \
                .contiguous(memory_format=torch.channels_last)
            seen += x.shape[0]
        torch.cuda.synchronize()
        return seen / (time.perf_counter() - t0)

    print(f"{n} JPEG records {SW}x{SH} q90, batch {args.batch}, "
          f"{args.threads} threads; img/s, median of {args.rounds} alternating "
          f"epochs (min..max)")
    rates = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, kw in paths.items():
            rates[k].append(epoch(kw))
    print("| path | img/s |")
    print("|---|---|")
    for k, r in rates.items():
        print(f"| {k} | {statistics.median(r):.0f} ({min(r):.0f}..{max(r):.0f}) |")
    os.remove(path)
    os.rmdir(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "iter", "both"), default="both")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--records", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment: needs a GPU")
    from dtmx.ops.hip import require_ext

    ext = require_ext()
    if args.mode in ("kernel", "both"):
        bench_kernel(ext, args)
    if args.mode in ("iter", "both"):
        bench_iter(ext, args)


if __name__ == "__main__":
    main()
