"""fp64 reference and shared cases for the augment_batch tests (CPU and GPU).

`ref_augment` is the chain dtmx/io/augment.py documents, written as a plain
per-pixel loop in float64. Two deliberately wrong variants exist so the tests
can show their bound rejects them: `centre=False` drops the half-pixel centre
and `swap=True` exchanges the first two colour stages."""
import math

import numpy as np
import torch

ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
INF = float("inf")


def _gray(v):
    return 0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2]


def ref_augment(case, centre=True, swap=False):
    src = case["src"].numpy()
    mean = np.asarray(case["mean"], np.float64)
    std = np.asarray(case["std"], np.float64)
    TH, TW = case["TH"], case["TW"]
    geom = case["geom"].tolist()
    par = case["par"].double().tolist()
    out = np.zeros((len(geom), TH, TW, 3), np.float64)
    h = 0.5 if centre else 0.0
    for i, ((off, H, W), p) in enumerate(zip(geom, par)):
        img = src[off:off + H * W * 3].reshape(H, W, 3).astype(np.float64)

        def tap(xi, yi):
            if 0 <= xi < W and 0 <= yi < H:
                return img[yi, xi]
            return np.full(3, p[10])

        v = np.zeros((TH, TW, 3))
        for y in range(TH):
            for x in range(TW):
                fx = p[0] * (x + h) + p[1] * (y + h) + p[2] - h
                fy = p[3] * (x + h) + p[4] * (y + h) + p[5] - h
                fx = min(max(fx, p[6]), p[7])
                fy = min(max(fy, p[8]), p[9])
                x0, y0 = math.floor(fx), math.floor(fy)
                wx, wy = fx - x0, fy - y0
                top = tap(x0, y0) * (1 - wx) + tap(x0 + 1, y0) * wx
                bot = tap(x0, y0 + 1) * (1 - wx) + tap(x0 + 1, y0 + 1) * wx
                v[y, x] = top * (1 - wy) + bot * wy
        v = np.clip(v, 0, 255)
        order = list(ORDERS[int(p[14])])
        if swap:
            order[0], order[1] = order[1], order[0]
        for st in order:
            if st == 0:
                v = v * p[11]
            elif st == 1:
                v = p[12] * v + (1 - p[12]) * _gray(v).mean()
            else:
                v = p[13] * v + (1 - p[13]) * _gray(v)[..., None]
            v = np.clip(v, 0, 255)
        v = np.clip(v + np.asarray(p[15:18]), 0, 255)
        out[i] = (v / 255.0 - mean) / std
    return out


def plan(a=(1, 0, 0, 0, 1, 0), box=(-INF, INF, -INF, INF), fill=0.0,
         alphas=(1, 1, 1), order=0, pca=(0, 0, 0)):
    return list(a) + list(box) + [fill] + list(alphas) + [order] + list(pca) + [0, 0]


def pack(images, gap=1):
    """Back to back with `gap` junk bytes in front of each: odd offsets."""
    chunks, geom, pos = [], [], 0
    for im in images:
        chunks.append(np.full(gap, 0xAB, np.uint8))
        pos += gap
        geom.append([pos, im.shape[0], im.shape[1]])
        chunks.append(im.reshape(-1))
        pos += im.size
    return (torch.from_numpy(np.concatenate(chunks)),
            torch.tensor(geom, dtype=torch.int64))


def _case(images, plans, TH, TW, mean=(0, 0, 0), std=(1, 1, 1)):
    src, geom = pack(images)
    return dict(src=src, geom=geom,
                par=torch.tensor(plans, dtype=torch.float32), TH=TH, TW=TW,
                mean=tuple(float(m) for m in mean),
                std=tuple(float(s) for s in std))


SIZES = ((1, 1), (7, 5), (16, 16), (33, 20), (64, 48))  # (H, W)


def _images(seed, sizes=SIZES):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _fit(H, W, TH, TW, **kw):
    """Whole image resized to the target, edges replicated."""
    return plan((W / TW, 0, 0, 0, H / TH, 0), (0, W - 1, 0, H - 1), **kw)


def numeric_cases():
    """name -> case. Up- and down-scaling, a rotated map with fill, an active
    clamp box, every colour stage alone at a saturating alpha, all six
    orders, PCA and mean/std, on five packed images, to 8x8 and 12x10 and to
    an odd 7x5 target (TH*TW no multiple of the kernel's strip)."""
    cases = {}
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for TH, TW in ((8, 8), (12, 10), (7, 5)):
        ims = _images(TH)
        t = f"{TH}x{TW}"
        cases[f"scale_{t}"] = _case(
            ims, [_fit(h, w, TH, TW) for h, w in SIZES], TH, TW)
        c, s = math.cos(0.4), math.sin(0.4)
        rot = []
        for h, w in SIZES:  # rotate about the centre, scaled to the target
            k = max(h / TH, w / TW)
            rot.append(plan((c * k, -s * k, w / 2 - k * (c * TW - s * TH) / 2,
                             s * k, c * k, h / 2 - k * (s * TW + c * TH) / 2),
                            fill=200.0))
        cases[f"rotate_fill_{t}"] = _case(ims, rot, TH, TW, mean, std)
        box = []
        for h, w in SIZES:  # crop the central half, mirrored, clamped to it
            cw, ch = max(1, w // 2), max(1, h // 2)
            cx, cy = (w - cw) // 2, (h - ch) // 2
            box.append(plan((-cw / TW, 0, cx + cw, 0, ch / TH, cy),
                            (cx, cx + cw - 1, cy, cy + ch - 1), fill=255.0))
        cases[f"clamp_box_{t}"] = _case(ims, box, TH, TW)
        jit = [_fit(h, w, TH, TW, alphas=(1.3, 0.6, 1.4), order=i % 6,
                    pca=(9.5, -7.25, 3.0)) for i, (h, w) in enumerate(SIZES)]
        cases[f"jitter_{t}"] = _case(ims, jit, TH, TW, mean, std)
    ims = _images(3, SIZES[2:])
    for name, al in (("brightness", (1.8, 1, 1)), ("contrast", (1, 1.9, 1)),
                     ("saturation", (1, 1, 1.9)), ("darken", (0.3, 0.2, 0.0))):
        cases[name] = _case(ims, [_fit(h, w, 8, 8, alphas=al)
                                  for h, w in SIZES[2:]], 8, 8)
    six = _images(4, [(16, 16)] * 6)
    cases["orders"] = _case(six, [_fit(16, 16, 8, 8, alphas=(1.7, 1.6, 1.8),
                                       order=k) for k in range(6)], 8, 8)
    cases["pca"] = _case(ims, [_fit(h, w, 8, 8, pca=(40.0, -30.0, 12.5))
                               for h, w in SIZES[2:]], 8, 8)
    cases["mean_std"] = _case(ims, [_fit(h, w, 8, 8) for h, w in SIZES[2:]],
                              8, 8, mean, (0.229, -0.5, 2.0))
    return cases


def multiblock_case():
    """40x36 target at B=3: an image spans two 1024-output chunks, the second
    one partly empty."""
    sizes = ((50, 41), (36, 40), (23, 61))
    ims = _images(7, sizes)
    plans = [_fit(h, w, 40, 36, alphas=(1.2, 0.7, 1.3), order=3 + i,
                  pca=(3.0, -2.0, 1.0)) for i, (h, w) in enumerate(sizes)]
    return _case(ims, plans, 40, 36, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def exact_cases():
    """name -> (case, expected uint8 (B,TH,TW,3) selection)."""
    rng = np.random.RandomState(11)
    out = {}
    ims = [rng.randint(0, 256, (8, 8, 3), dtype=np.uint8) for _ in range(3)]
    out["identity"] = (_case(ims, [plan(box=(0, 7, 0, 7))] * 3, 8, 8),
                       np.stack(ims))
    big = [rng.randint(0, 256, (20, 17, 3), dtype=np.uint8) for _ in range(2)]
    cy, cx, TH, TW = 5, 3, 12, 10
    crop = plan((1, 0, cx, 0, 1, cy), (cx, cx + TW - 1, cy, cy + TH - 1))
    mirr = plan((-1, 0, cx + TW, 0, 1, cy), (cx, cx + TW - 1, cy, cy + TH - 1))
    out["crop_mirror"] = (
        _case(big, [crop, mirr], TH, TW),
        np.stack([big[0][cy:cy + TH, cx:cx + TW],
                  big[1][cy:cy + TH, cx:cx + TW][:, ::-1]]))
    return out


def run(case, dtype=torch.float32, device="cpu", **kw):
    from dtmx.io.augment import augment_batch

    src, geom, par = case["src"], case["geom"], case["par"]
    if device != "cpu":
        kw.update(geom_host=geom, par_host=par)
        src, geom, par = src.to(device), geom.to(device), par.to(device)
    return augment_batch(src, geom, par, case["mean"], case["std"], case["TH"],
                         case["TW"], dtype, **kw)


def nhwc(out):
    return out.permute(0, 2, 3, 1).double().cpu().numpy()


def level_tol(case, level):
    """`level` grey levels in output units, per channel."""
    return level / 255.0 / np.abs(np.asarray(case["std"], np.float64))


def ulp16(v, dtype):
    """Spacing of `dtype` at |v| (v an fp64 array)."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin)))
    return 2.0 ** (e - mant)
