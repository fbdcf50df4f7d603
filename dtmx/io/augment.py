"""Batch image augmentation: decoded uint8 records -> normalised NHWC batch.

`augment_batch` is the one per-pixel stage of the staged `ImageRecordIter`
path: a single bilinear resampling through a per-image affine map, colour
jitter, PCA lighting and mean/std normalisation (reference
src/io/image_aug_default.cc, composed into one pass). GPU inputs run the HIP
kernel (dtmx/csrc/augment.hip); CPU inputs — and `DTMX_FALLBACK=augment` —
run the vectorised torch implementation below, which is the documented
meaning of the kernel.

Inputs
  src   uint8[bytes]: the batch's RGB images back to back, HWC
  geom  int64[B][3]:  {byte offset, H_i, W_i}
  par   float32[B][20], the per-image plan:
          0-5   affine map output -> source, u = a00(x+.5) + a01(y+.5) + a02,
                v = a10(x+.5) + a11(y+.5) + a12; taps at fx = u-.5, fy = v-.5
          6-9   clamp box fx_lo, fx_hi, fy_lo, fy_hi on (fx, fy); +-inf = off
          10    fill, read by taps outside [0,W-1] x [0,H-1]
          11-13 alpha_b, alpha_c, alpha_s (1 = off)
          14    order of (brightness, contrast, saturation), index into ORDERS
          15-17 PCA add for R, G, B in levels
          18-19 spare
  mean, std  3 floats in [0,1] units (the mean_r / std_r convention)

Chain per pixel, fp32 on [0,255], a clamp to [0,255] after every stage and
no rounding to integers in between: bilinear; the three colour stages in the
plan's order (v*ab; ac*v + (1-ac)*gmean; as*v + (1-as)*gray, gray = .299R +
.587G + .114B, gmean = mean of gray over the image's outputs as they stand
when contrast is reached); + pca; (v*(1/255) - mean) / std; one convert.
"""
from __future__ import annotations

import os

import torch

PAR_LEN = 20
# stage codes: 0 brightness, 1 contrast, 2 saturation
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))

_FALLBACK = "augment" in os.environ.get("DTMX_FALLBACK", "").split(",")


def _gray(v):
    return 0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2]


def _augment_image(img, p, ys, xs):
    """One image (H,W,3 float32) through sampling and the colour stages;
    p is its plan row as python floats. Returns (TH,TW,3) float32."""
    H, W = img.shape[:2]
    fx = p[0] * xs + p[1] * ys + p[2] - 0.5
    fy = p[3] * xs + p[4] * ys + p[5] - 0.5
    fx = fx.clamp(p[6], p[7]).clamp(-2.0, W + 1.0)
    fy = fy.clamp(p[8], p[9]).clamp(-2.0, H + 1.0)
    x0f, y0f = fx.floor(), fy.floor()
    wx, wy = (fx - x0f)[..., None], (fy - y0f)[..., None]
    x0, y0 = x0f.long(), y0f.long()
    fill = torch.tensor(p[10], dtype=torch.float32)

    def tap(xi, yi):
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        t = img[yi.clamp(0, H - 1), xi.clamp(0, W - 1)]
        return torch.where(inside[..., None], t, fill)

    t00, t01 = tap(x0, y0), tap(x0 + 1, y0)
    t10, t11 = tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    top = t00 + wx * (t01 - t00)
    bot = t10 + wx * (t11 - t10)
    v = (top + wy * (bot - top)).clamp(0.0, 255.0)
    ab, ac, as_ = p[11], p[12], p[13]
    for st in ORDERS[min(max(int(p[14]), 0), 5)]:
        if st == 0:
            v = (v * ab).clamp(0.0, 255.0)
        elif st == 1:
            gmean = _gray(v).mean() if ac != 1.0 else 0.0
            v = (ac * v + (1.0 - ac) * gmean).clamp(0.0, 255.0)
        else:
            v = (as_ * v + ((1.0 - as_) * _gray(v))[..., None]).clamp(0.0, 255.0)
    return v


def _augment_torch(src, geom, par, mean, std, TH, TW, out_dtype):
    B = geom.shape[0]
    ys, xs = torch.meshgrid(torch.arange(TH, dtype=torch.float32) + 0.5,
                            torch.arange(TW, dtype=torch.float32) + 0.5,
                            indexing="ij")
    out = torch.empty((B, TH, TW, 3), dtype=torch.float32)
    rows = par.tolist()
    for i, (off, H, W) in enumerate(geom.tolist()):
        img = src[off:off + H * W * 3].reshape(H, W, 3).float()
        v = _augment_image(img, rows[i], ys, xs)
        pca = torch.tensor(rows[i][15:18], dtype=torch.float32)
        out[i] = ((v + pca).clamp(0.0, 255.0) * (1.0 / 255.0) - mean) / std
    return out.permute(0, 3, 1, 2).to(out_dtype)  # logical NCHW, NHWC memory


def _check(src, geom, par, mean, std, TH, TW, out_dtype):
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise ValueError("augment_batch: src must be a 1-D uint8 tensor")
    if geom.dtype != torch.int64 or geom.dim() != 2 or geom.shape[1] != 3 \
            or geom.shape[0] < 1:
        raise ValueError("augment_batch: geom must be int64 of shape (B, 3), B >= 1")
    if par.dtype != torch.float32 or tuple(par.shape) != (geom.shape[0], PAR_LEN):
        raise ValueError(f"augment_batch: par must be float32 of shape (B, {PAR_LEN})")
    if TH < 1 or TW < 1:
        raise ValueError("augment_batch: TH and TW must be >= 1")
    if out_dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise ValueError("augment_batch: out_dtype must be bfloat16, float16 or float32")
    if mean.numel() != 3 or std.numel() != 3:
        raise ValueError("augment_batch: mean and std must have 3 elements")
    if bool((std == 0).any()):
        raise ValueError("augment_batch: std must be != 0")


def _check_geom(geom_host, nbytes):
    for i, (off, H, W) in enumerate(geom_host.tolist()):
        if H < 1 or W < 1:
            raise ValueError(f"augment_batch: image {i} must have H, W >= 1")
        if off < 0 or off + H * W * 3 > nbytes:
            raise ValueError(f"augment_batch: image {i} must lie inside src")


def augment_batch(src, geom, par, mean, std, TH, TW, out_dtype=torch.float32,
                  geom_host=None, par_host=None):
    """-> (B,3,TH,TW) tensor of `out_dtype` in channels_last memory, on src's
    device. `mean` / `std` are 3-element CPU tensors or sequences. For a GPU
    `src`, `geom` / `par` may be CPU tensors (uploaded here) or device tensors
    with their CPU copies passed as `geom_host` / `par_host`: image bounds are
    checked on the host, so the call never waits for the device."""
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(3)
    std = torch.as_tensor(std, dtype=torch.float32).reshape(3)
    if mean.is_cuda or std.is_cuda:
        raise ValueError("augment_batch: mean and std must be CPU tensors")
    if geom_host is None and not geom.is_cuda:
        geom_host = geom
    if par_host is None and not par.is_cuda:
        par_host = par
    if geom_host is None or par_host is None:
        raise ValueError("augment_batch: device geom / par need geom_host / "
                         "par_host, their CPU copies")
    _check(src, geom_host, par_host, mean, std, TH, TW, out_dtype)
    if src.is_cuda and not _FALLBACK:
        from dtmx.ops.hip import require_ext

        if not geom.is_cuda:
            geom = geom.to(src.device, non_blocking=True)
        if not par.is_cuda:
            par = par.to(src.device, non_blocking=True)
        return require_ext().augment_batch(src, geom, par, mean, std, TH, TW,
                                           out_dtype, geom_host, par_host)
    _check_geom(geom_host, src.numel())
    out = _augment_torch(src.cpu(), geom_host, par_host, mean, std, TH, TW, out_dtype)
    return out.to(src.device) if src.is_cuda else out
