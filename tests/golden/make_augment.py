"""Generates tests/golden/aug_transform.npz: the reference's own training augmentation (transform.py:10-28) on small volumes.

Run in the build container only (needs the reference, imported through tools/ref_shim.py):  python tests/golden/make_augment.py

Per case: the input (images (4, D, H, W) fp32, labels (D, H, W) uint8; the reference gets them as GBMset builds them,
(4, 1, D, H, W) fp32 and (1, D, H, W) fp64), the configuration, the parameters the reference drew under the seeded np.random
(the alphas, the three flip uniforms, the crop origins) and its outputs (x (4, d, h, w) fp32, mask (3, d, h, w) uint8).
The parameters are recorded by wrapping np.random.uniform / randint around the reference's own calls.  The maker refuses to
write unless a numpy restatement that uses only the recorded parameters reproduces the reference's outputs exactly."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_shim  # noqa: E402

RT = ref_shim.load_transform()
NAN = float("nan")


def volume(seed, shape, zero_channel=None, one_voxel_channel=None):
    """A brain-like volume: fp32 intensities in (0, 255] inside an ellipsoid, 0 outside; labels 0..4 inside a smaller one."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[(np.arange(s) - (s - 1) / 2) / (s / 2) for s in shape], indexing="ij")
    r2 = sum(a * a for a in g)
    img = np.zeros((4,) + shape, np.float32)
    for c in range(4):
        v = rng.uniform(0.0, 255.0, shape).astype(np.float32) * (0.5 + 0.25 * c)
        img[c] = np.where(r2 < 0.8 + 0.05 * c, np.maximum(v, np.float32(0.5)), 0)
    lab = np.where(r2 < 0.35, rng.integers(0, 5, shape), 0).astype(np.uint8)
    if zero_channel is not None:
        img[zero_channel] = 0
    if one_voxel_channel is not None:
        img[one_voxel_channel] = 0
        img[one_voxel_channel][tuple(s // 3 for s in shape)] = 77.25
    return img, lab


def run_reference(img, lab, cfg, seed):
    """transforms(**cfg) of the reference on GBMset's layout, under np.random.seed(seed); returns outputs + recorded draws."""
    calls = []
    uni, rint = np.random.uniform, np.random.randint

    def uniform(*a, **k):
        v = uni(*a, **k)
        calls.append(("uniform", float(v)))
        return v

    def randint(*a, **k):
        v = rint(*a, **k)
        calls.append(("randint", int(v)))
        return v

    np.random.seed(seed)
    np.random.uniform, np.random.randint = uniform, randint
    try:
        t = RT.transforms(**cfg)
        x, m = t((img[:, None].copy(), lab[None].astype(np.float64)))
    finally:
        np.random.uniform, np.random.randint = uni, rint
    assert x.dtype == np.float32 and m.dtype == np.uint8 and m.shape[1] == 1
    if x.ndim == 5:                       # without Random_Crop_3D the image keeps GBMset's singleton axis (4, 1, D, H, W)
        assert x.shape[1] == 1
        x = x[:, 0]
    return np.ascontiguousarray(x), np.ascontiguousarray(m[:, 0]), calls


def parse(calls, cfg, shape):
    it = iter(calls)
    a_scale = next(it)[1] if cfg.get("scale") is not None else NAN
    a_shift = next(it)[1] if cfg.get("shift") is not None else NAN
    flip_u = [next(it)[1] for _ in range(3)] if cfg.get("flip_prob") is not None else [NAN] * 3
    origin = [0, 0, 0]
    crop = cfg.get("random_crop")
    if crop is not None:
        crop = list(crop) if isinstance(crop, (list, tuple)) else [crop] * 3
        for a in range(3):
            if crop[a] < shape[a]:
                kind, v = next(it)
                assert kind == "randint"
                origin[a] = v
    assert next(it, None) is None, "unparsed draws"
    return a_scale, a_shift, flip_u, origin, crop


def restate(img, lab, cfg, a_scale, a_shift, flip_u, origin, crop):
    """The reference's arithmetic from the recorded parameters alone (numpy 2 promotion: a Python float is weak)."""
    x = img.copy()
    if cfg.get("scale") is not None:
        x = x * a_scale
    if cfg.get("shift") is not None:
        ch = []
        for c in range(4):
            nz = x[c] != 0
            s = np.std(x[c][nz]) if nz.any() else np.float32(0)
            ch.append(np.where(nz, x[c] + s * a_shift, 0))
        x = np.stack(ch, 0)
    m = lab.astype(np.float64)
    if cfg.get("flip_prob") is not None:
        for ax in (1, 2):                                   # draw 0 flips the singleton axis of the reference's arrays
            if flip_u[ax] > cfg["flip_prob"]:
                x, m = np.flip(x, ax), np.flip(m, ax - 1)
    if crop is not None:
        sl = tuple(slice(o, o + c) for o, c in zip(origin, crop))
        x, m = x[(slice(None),) + sl], m[sl]
    if cfg.get("normalize", True):
        x = x / 255.0
    mask = np.stack([(m > 0), (m == 1) | (m == 2) | (m == 3), (m == 1)]).astype(np.uint8)
    return np.ascontiguousarray(x), mask


TRAIN = dict(shift=0.1, flip_prob=0.5)


def cases():
    # the training configuration under several seeds: each flip axis (D, H) is seen both ways
    seen = set()
    for seed in range(1, 40):
        img, lab = volume(100 + seed, (14, 16, 12))
        yield f"train_s{seed}", img, lab, dict(TRAIN, random_crop=(8, 10, 6)), seed
        _, _, calls = run_reference(img, lab, dict(TRAIN, random_crop=(8, 10, 6)), seed)
        u = [c[1] for c in calls[1:4]]
        seen |= {(1, u[1] > 0.5), (2, u[2] > 0.5)}
        if len(seen) == 4 and seed >= 4:
            break
    img, lab = volume(7, (14, 16, 12))
    yield "val_crop", img, lab, dict(random_crop=8), 7                                   # the validation configuration
    img, lab = volume(8, (10, 12, 14))
    yield "scale_shift", img, lab, dict(scale=0.1, shift=0.1), 8
    img, lab = volume(9, (16, 20, 14))
    yield "crop_eq_h", img, lab, dict(TRAIN, random_crop=(10, 20, 8)), 9                  # crop == size on H
    img, lab = volume(10, (14, 16, 12), zero_channel=2)
    yield "zero_channel", img, lab, dict(TRAIN, random_crop=(8, 10, 6)), 10
    img, lab = volume(11, (14, 16, 12), one_voxel_channel=1)
    yield "one_voxel", img, lab, dict(scale=0.2, shift=0.1, flip_prob=0.5, random_crop=(12, 14, 10)), 11
    img, lab = volume(12, (12, 14, 10))
    lab[:] = np.arange(lab.size).reshape(lab.shape) % 5                                 # every label 0..4, everywhere
    yield "labels_0to4", img, lab, dict(TRAIN, random_crop=(9, 11, 7)), 12
    img, lab = volume(13, (13, 17, 11))
    yield "odd_13x17x11", img, lab, dict(TRAIN, random_crop=(7, 9, 5)), 13
    img, lab = volume(14, (3, 5, 300))
    yield "wide_w300", img, lab, dict(TRAIN, random_crop=(2, 4, 281)), 14               # rows of 281 > 256: several workgroups


def main():
    out = {}
    names = []
    for name, img, lab, cfg, seed in cases():
        x, m, calls = run_reference(img, lab, cfg, seed)
        a_scale, a_shift, flip_u, origin, crop = parse(calls, cfg, img.shape[1:])
        rx, rm = restate(img, lab, cfg, a_scale, a_shift, flip_u, origin, crop)
        if not (rx.dtype == x.dtype and np.array_equal(rx, x) and np.array_equal(rm, m)):
            raise SystemExit(f"{name}: the numpy restatement does not reproduce the reference; not writing")
        names.append(name)
        out[f"{name}__img"], out[f"{name}__lab"] = img, lab
        out[f"{name}__cfg"] = np.array([cfg.get("scale", NAN) if cfg.get("scale") is not None else NAN,
                                        cfg.get("shift") if cfg.get("shift") is not None else NAN,
                                        cfg.get("flip_prob") if cfg.get("flip_prob") is not None else NAN,
                                        float(cfg.get("normalize", True))])
        out[f"{name}__crop"] = np.array(crop if crop is not None else [-1, -1, -1], np.int64)
        out[f"{name}__alpha"] = np.array([a_scale, a_shift])
        out[f"{name}__flip_u"] = np.array(flip_u)
        out[f"{name}__origin"] = np.array(origin, np.int64)
        out[f"{name}__x"], out[f"{name}__mask"] = x, m
        out[f"{name}__seed"] = np.array(seed)
        print(f"{name:14s} in {img.shape} -> {x.shape}  alpha {a_scale:.4f} {a_shift:+.4f}  flip_u {np.round(flip_u, 3)}  "
              f"origin {origin}")
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "aug_transform.npz"), **out)


if __name__ == "__main__":
    main()
