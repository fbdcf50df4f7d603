"""Augmentation planner, the torch path of io.augment.augment_batch against
the fp64 reference, and the staged ImageRecordIter's flag handling."""
import functools
import logging
import struct

import numpy as np
import pytest
import torch

import augment_ref as R
from dtmx.ops.hip import get_ext

pytestmark = pytest.mark.skipif(get_ext() is None, reason="ext not built")

# fp32 against fp64, in grey levels. Tap coordinates reach 64 and come from
# three fp32 roundings (about 3 * 64 * 2^-24 = 1.1e-5 px, times at most 255
# levels per pixel = 3e-3 level); each of the three colour stages can scale
# that by its alpha (< 2) and adds roundings of its own at 255 * 2^-24 =
# 1.5e-5 level. 0.02 level covers the product 3e-3 * 1.8^3 and stays below the
# 0.05-level ceiling above which a real error could hide.
CPU_BOUND_LEVEL = 0.02

RRC = dict(th=8, tw=8, random_resized_crop=True, min_random_area=0.08,
           max_random_area=1.0, min_aspect_ratio=0.75, max_aspect_ratio=1.333,
           rand_mirror=True, brightness=0.4, contrast=0.3, saturation=0.2,
           pca_noise=0.1)


@functools.lru_cache(maxsize=None)
def _cases():
    return R.numeric_cases()


@functools.lru_cache(maxsize=None)
def _ref(name, centre=True, swap=False):
    return R.ref_augment(_cases()[name], centre, swap)


def _within_one_ulp_of_pix_over_255(got, pix):
    """fp32 output (B,3,H,W) against correctly rounded pix/255 (B,H,W,3)."""
    exact = (pix.astype(np.float64) / 255.0).astype(np.float32)
    got = got.permute(0, 2, 3, 1).numpy()
    return bool((np.abs(got - exact) <= np.spacing(exact)).all())


# ------------------------------------------------------------------ planner

def test_plan_is_a_function_of_seed_epoch_record():
    ext = get_ext()
    a = ext.aug_plan(RRC, 3, 1, 17, 30, 40)
    assert a.shape == (20,) and a.dtype == torch.float32
    assert torch.equal(a, ext.aug_plan(RRC, 3, 1, 17, 30, 40))
    assert not torch.equal(a, ext.aug_plan(RRC, 3, 2, 17, 30, 40))
    assert not torch.equal(a, ext.aug_plan(RRC, 3, 1, 18, 30, 40))
    assert not torch.equal(a, ext.aug_plan(RRC, 4, 1, 17, 30, 40))


def test_plan_invariants_over_2000_draws():
    ext = get_ext()
    H, W, TH, TW = 30, 40, 8, 8
    rows = torch.stack([ext.aug_plan(RRC, 1, 1, r, H, W) for r in range(2000)])
    rows = rows.double().numpy()
    # no resize, no pad: the clamp box is the crop rectangle's pixel centres
    cx, cy = rows[:, 6], rows[:, 8]
    cw, ch = rows[:, 7] - cx + 1, rows[:, 9] - cy + 1
    for v in (cx, cy, cw, ch):
        assert np.array_equal(v, np.round(v))
    assert (cx >= 0).all() and (cy >= 0).all()
    assert (cx + cw <= W).all() and (cy + ch <= H).all()
    assert (cw >= 1).all() and (ch >= 1).all()
    # w, h are roundings of sqrt(area * ratio), sqrt(area / ratio)
    A = H * W
    assert ((cw + .5) * (ch + .5) >= 0.08 * A).all()
    assert ((cw - .5) * (ch - .5) <= 1.0 * A).all()
    lo, hi = 0.75, 1.333

    def aspect_ok(w, h):
        return ((w + .5) / (h - .5) >= lo) & ((w - .5) / (h + .5) <= hi)

    assert (aspect_ok(cw, ch) | aspect_ok(ch, cw)).all()
    # the map is that rectangle, mirrored or not
    mirrored = rows[:, 0] < 0
    assert 600 < mirrored.sum() < 1400
    assert np.allclose(np.abs(rows[:, 0]), cw / TW, rtol=1e-6)
    assert np.allclose(rows[:, 4], ch / TH, rtol=1e-6)
    assert np.allclose(rows[:, 2], np.where(mirrored, cx + cw, cx), rtol=1e-6)
    assert np.array_equal(rows[:, 5], cy)
    assert set(rows[:, 14].astype(int)) == set(range(6))
    for col, p in ((11, 0.4), (12, 0.3), (13, 0.2)):
        assert (np.abs(rows[:, col] - 1) <= p + 1e-6).all()
        assert np.abs(rows[:, col] - 1).max() > 0.9 * p
    # undo eigenvalue * eigenvector: three N(0, pca_noise) draws per row
    M = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140],
                  [-0.5836, -0.6948, 0.4203]]) * np.array([55.46, 4.794, 1.148])
    alpha = np.linalg.solve(M, rows[:, 15:18].T).ravel()
    sigma = 0.1
    assert abs(alpha.std(ddof=1) - sigma) <= 5 * sigma / np.sqrt(2 * alpha.size)
    assert abs(alpha.mean()) <= 5 * sigma / np.sqrt(alpha.size)


def test_impossible_resized_crop_falls_back_to_fixed_window():
    ext = get_ext()
    cfg = dict(th=8, tw=8, random_resized_crop=True, min_random_area=0.9,
               max_random_area=1.0, min_aspect_ratio=0.75, max_aspect_ratio=1.333)
    for rec in range(20):
        p = ext.aug_plan(cfg, 0, 1, rec, 4, 100).tolist()
        # 4x100 scaled up to 8x200, aspect kept, then the central 8x8 window
        assert p[0] == 0.5 and p[4] == 0.5
        assert p[2] == (200 - 8) // 2 * 0.5 and p[5] == 0.0


def test_plan_defaults_are_the_identity_and_max_aspect_alone_is_symmetric():
    ext = get_ext()
    p = ext.aug_plan(dict(th=8, tw=8), 0, 1, 0, 8, 8).tolist()
    assert p[:6] == [1, 0, 0, 0, 1, 0] and p[6:10] == [0, 7, 0, 7]
    assert p[11:15] == [1, 1, 1, 0] and p[15:18] == [0, 0, 0]
    cfg = dict(th=8, tw=8, random_resized_crop=True, min_random_area=0.25,
               max_random_area=0.5, max_aspect_ratio=0.25)
    rows = np.array([ext.aug_plan(cfg, 0, 1, r, 64, 64).tolist() for r in range(300)])
    cw, ch = rows[:, 7] - rows[:, 6] + 1, rows[:, 9] - rows[:, 8] + 1
    def aspect_ok(w, h):  # the swap coin exchanges w and h
        return ((w + .5) / (h - .5) >= 0.75) & ((w - .5) / (h + .5) <= 1.25)

    assert (aspect_ok(cw, ch) | aspect_ok(ch, cw)).all()
    assert (cw != ch).any() and (np.maximum(cw, ch) / np.minimum(cw, ch)).max() < 1.4


def test_pad_reads_fill_and_crop_size_is_square():
    ext = get_ext()
    p = ext.aug_plan(dict(th=8, tw=8, pad=2, fill_value=7), 0, 1, 0, 4, 4).tolist()
    # 4x4 padded to 8x8: the window is the canvas, shifted by the pad
    assert p[:6] == [1, 0, -2, 0, 1, -2] and p[10] == 7
    assert p[6:10] == [-2, 5, -2, 5]
    cfg = dict(th=8, tw=8, min_crop_size=10, max_crop_size=20, rand_crop=True)
    rows = np.array([ext.aug_plan(cfg, 0, 1, r, 30, 40).tolist() for r in range(200)])
    cw, ch = rows[:, 7] - rows[:, 6] + 1, rows[:, 9] - rows[:, 8] + 1
    assert np.array_equal(cw, ch) and cw.min() == 10 and cw.max() == 20
    assert (rows[:, 6] + cw <= 40).all() and (rows[:, 8] + ch <= 30).all()


# --------------------------------------------------- torch path vs reference

@pytest.mark.parametrize("name", sorted(R.numeric_cases()))
def test_cpu_matches_fp64_reference(name):
    case = _cases()[name]
    got = R.nhwc(R.run(case))
    tol = R.level_tol(case, CPU_BOUND_LEVEL)
    err = np.abs(got - _ref(name))
    print(f"{name}: max err {(err / R.level_tol(case, 1.0)).max():.3g} level")
    assert (err <= tol).all()


def test_bound_rejects_wrong_variants():
    """The same bound must fail the reference without the half-pixel centre
    and the reference with two colour stages swapped."""
    case = _cases()["scale_12x10"]
    got = R.nhwc(R.run(case))
    assert not (np.abs(got - _ref("scale_12x10", centre=False))
                <= R.level_tol(case, CPU_BOUND_LEVEL)).all()
    case = _cases()["orders"]
    got = R.nhwc(R.run(case))
    assert not (np.abs(got - _ref("orders", swap=True))
                <= R.level_tol(case, CPU_BOUND_LEVEL)).all()


@pytest.mark.parametrize("name", sorted(R.exact_cases()))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_cpu_exact_selection(name, dtype):
    case, want = R.exact_cases()[name]
    got = R.run(case, dtype)
    assert got.dtype == dtype and got.shape == (len(want), 3, case["TH"], case["TW"])
    assert got.is_contiguous(memory_format=torch.channels_last)
    # the loader's convention: pix * fp32(1/255), within one fp32 ulp of pix/255
    exp = (torch.from_numpy(want).float() * (1.0 / 255.0)).to(dtype)
    assert torch.equal(got.permute(0, 2, 3, 1), exp)
    if dtype == torch.float32:
        assert _within_one_ulp_of_pix_over_255(got, want)


def test_host_checks():
    case = dict(_cases()["pca"])
    bad = dict(case, geom=case["geom"].clone())
    bad["geom"][1, 0] = case["src"].numel() - 5
    with pytest.raises(ValueError, match="inside src"):
        R.run(bad)
    with pytest.raises(ValueError, match="std"):
        R.run(dict(case, std=(1.0, 0.0, 1.0)))
    with pytest.raises(ValueError, match="out_dtype"):
        R.run(case, torch.float64)


# ----------------------------------------------------------------- iterator

def _write_raw(tmp_path, n=16, h=8, w=8, sized=False, seed=0):
    """Raw records; with `sized` the header's id2 carries (H << 32) | W."""
    ext = get_ext()
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 256, (n, h, w, 3), dtype=np.uint8)
    recs = [struct.pack("<IfQQ", 0, float(i % 5), i, (h << 32 | w) if sized else 0)
            + x[i].tobytes() for i in range(n)]
    path = str(tmp_path / f"raw_{h}x{w}.rec")
    ext.write_recordio(path, recs)
    return path, x


def test_staged_identity_equals_legacy_iterator(tmp_path):
    from dtmx.io import ImageRecordIter

    path, x = _write_raw(tmp_path)
    kw = dict(mean_r=0.5, mean_g=0.25, std_r=2.0, std_b=4.0)
    for extra in ({}, kw):
        old = list(ImageRecordIter(path, (3, 8, 8), 8, **extra))
        new = list(ImageRecordIter(path, (3, 8, 8), 8, device="cpu", **extra))
        assert len(old) == len(new) == 2
        for a, b in zip(old, new):
            assert b.data[0].dtype == torch.float32
            assert b.data[0].is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(a.data[0], b.data[0])
            assert torch.equal(a.label[0], b.label[0])
    first = next(ImageRecordIter(path, (3, 8, 8), 8, device="cpu")).data[0]
    assert _within_one_ulp_of_pix_over_255(first, x[:8])
    # dtype exists on the staged path alone: this pins the path taken
    it = ImageRecordIter(path, (3, 8, 8), 8, device="cpu", dtype=torch.float16)
    assert it.provide_data[0].dtype == torch.float16
    half = next(it).data[0]
    assert half.dtype == torch.float16 and torch.equal(half, first.half())


def test_staged_batches_do_not_depend_on_thread_count(tmp_path):
    from dtmx.io import ImageRecordIter

    path, _ = _write_raw(tmp_path, n=32, h=20, w=17, sized=True)
    flags = dict(random_resized_crop=True, min_random_area=0.3,
                 max_aspect_ratio=0.25, rand_mirror=True, brightness=0.4,
                 contrast=0.4, saturation=0.4, pca_noise=0.1, shuffle=True, seed=9,
                 dtype=torch.float16)  # a staged-path argument: pins the path

    def epoch(threads):
        return list(ImageRecordIter(path, (3, 8, 8), 8,
                                    preprocess_threads=threads, **flags))

    one, four = epoch(1), epoch(4)
    assert len(one) == len(four) == 4
    for a, b in zip(one, four):
        assert a.data[0].dtype == torch.float16
        assert torch.equal(a.data[0], b.data[0])
        assert torch.equal(a.label[0], b.label[0])
    assert not torch.equal(one[0].data[0], one[1].data[0])


def test_staged_iterator_follows_the_plan(tmp_path):
    """A batch is augment_batch of the records under aug_plan's rows (first
    epoch = 1), whatever the batch position."""
    from dtmx.io import ImageRecordIter

    ext = get_ext()
    path, x = _write_raw(tmp_path, n=8, h=20, w=17, sized=True)
    flags = dict(rand_crop=True, rand_mirror=True, pad=2, fill_value=9,
                 brightness=0.3)
    batches = list(ImageRecordIter(path, (3, 12, 10), 4, seed=5, **flags))
    cfg = dict(th=12, tw=10, rand_crop=True, rand_mirror=True, pad=2,
               fill_value=9.0, brightness=0.3)
    rows = torch.stack([ext.aug_plan(cfg, 5, 1, r, 20, 17) for r in range(8)])
    src, geom = R.pack(list(x), gap=3)
    case = dict(src=src, geom=geom, par=rows, TH=12, TW=10, mean=(0, 0, 0),
                std=(1, 1, 1))
    want = R.run(case)
    assert torch.equal(torch.cat([b.data[0] for b in batches]), want)


def test_rejected_flags_and_conflicts_name_the_flag(tmp_path):
    from dtmx.io import ImageRecordIter

    path, _ = _write_raw(tmp_path)
    for flag, value in (("max_rotate_angle", 10), ("rotate", 90),
                        ("max_shear_ratio", 0.1), ("min_random_scale", 0.5),
                        ("max_random_scale", 1.5), ("min_img_size", 32),
                        ("max_img_size", 64), ("random_h", 36), ("random_s", 50),
                        ("random_l", 50), ("inter_method", 2)):
        with pytest.raises(ValueError, match=flag):
            ImageRecordIter(path, (3, 8, 8), 8, **{flag: value})
    # the reference's defaults for them pass
    ImageRecordIter(path, (3, 8, 8), 8, max_random_scale=1, inter_method=1)
    for flag, value in (("rand_crop", True), ("min_crop_size", 4),
                        ("max_crop_size", 6)):
        with pytest.raises(ValueError, match=flag):
            ImageRecordIter(path, (3, 8, 8), 8, random_resized_crop=True,
                            **{flag: value})
    with pytest.raises(ValueError, match="data_shape"):
        ImageRecordIter(path, (1, 8, 8), 8, brightness=0.1)
    with pytest.raises(ValueError, match="crop_size"):
        ImageRecordIter(path, (3, 8, 8), 8, max_crop_size=6)
    with pytest.raises(ValueError, match="std"):
        ImageRecordIter(path, (3, 8, 8), 8, device="cpu", std_g=0.0)


def test_unknown_kwarg_warns_once(tmp_path, caplog):
    from dtmx.io import ImageRecordIter

    path, _ = _write_raw(tmp_path)
    with caplog.at_level(logging.WARNING):
        ImageRecordIter(path, (3, 8, 8), 8, no_such_augmenter=1)
        ImageRecordIter(path, (3, 8, 8), 8, no_such_augmenter=1)
    hits = [r for r in caplog.records if "no_such_augmenter" in r.getMessage()]
    assert len(hits) == 1 and hits[0].levelno == logging.WARNING


def test_example_trainer_takes_the_reference_flag_names(tmp_path):
    """examples/train_imagenet.py reaches the staged path through the
    reference's flag names (CPU context: the torch path of augment_batch)."""
    import os
    import subprocess
    import sys

    ext = get_ext()
    ys, xs = np.mgrid[0:24, 0:24]
    recs = []
    for i in range(32):
        im = np.stack([(ys * 2 + i * 7) % 256, (xs * 3 + i * 11) % 256,
                       ((ys + xs) * 2 + i * 5) % 256], -1).astype(np.uint8)
        recs.append(struct.pack("<IfQQ", 0, float(i % 4), i, 0)
                    + ext.encode_jpeg(im.tobytes(), 24, 24, 3, 95))
    rec = str(tmp_path / "ex.rec")
    ext.write_recordio(rec, recs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "examples", "train_imagenet.py"),
           "--network", "lenet", "--num-classes", "4", "--num-examples", "32",
           "--image-shape", "3,16,16", "--batch-size", "8", "--num-epochs", "1",
           "--data-train", rec, "--dtype", "float32", "--kv-store", "local",
           "--random-resized-crop", "1", "--min-random-area", "0.3",
           "--max-random-aspect-ratio", "0.25", "--brightness", "0.4",
           "--contrast", "0.4", "--saturation", "0.4", "--pca-noise", "0.1",
           "--rgb-mean", "123.68,116.779,103.939", "--rgb-std", "58.393,57.12,57.375"]
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, capture_output=True, timeout=240, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"Epoch[0]" in r.stderr or b"Epoch[0]" in r.stdout


def test_id2_counts_as_a_size_only_when_it_matches_the_payload(tmp_path):
    from dtmx.io import ImageRecordIter

    ext = get_ext()
    x = np.random.RandomState(2).randint(0, 256, (8, 8, 8, 3), dtype=np.uint8)
    # id2 in use for something else: huge, or a size the payload does not have
    recs = [struct.pack("<IfQQ", 0, 0.0, i, (1 << 63 | 7) if i % 2 else (4 << 32 | 4))
            + x[i].tobytes() for i in range(8)]
    path = str(tmp_path / "id2.rec")
    ext.write_recordio(path, recs)
    got = next(ImageRecordIter(path, (3, 8, 8), 8, device="cpu")).data[0]
    want = torch.from_numpy(x).float() * (1.0 / 255.0)
    assert torch.equal(got.permute(0, 2, 3, 1), want)
