"""Generates tests/golden/metric_hd95.npz: HD95 of the three sigmoid regions computed by the REAL reference (metrics.py).

Run in the build container only (needs the reference, imported through tools/ref_shim.py):  python tests/golden/make_hd95.py

Per case: the binary prediction and target masks (3, D, H, W) = (WT, TC, EC), bit-packed; the spacing; the expected HD95 per
region and the six surface sizes.  The expected values use getHausdorff's channel map (WT / TC / EC = channels 0 / 1 / 2, the
map of DiceRegion and SegToMask) with the reference's own get_surface_points and the KDTree hausdorff_distance_95 of
getHausdorff_KD; where the surfaces are small enough, getHausdorff's own __call__ (dense cdist) must give the same number.
The prediction given to the reference is the probability map 0.1 + 0.8 * mask (thresholded at 0.5 by the reference)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_shim  # noqa: E402
from synth_blobs import blob_case  # noqa: E402

torch.set_num_threads(8)
RM = ref_shim.load_reference().metrics
CDIST_MAX = 6000               # getHausdorff's dense cdist is |S(a)| x |S(b)| doubles: only for small surfaces


def grid(shape):
    return np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")


def ball(shape, c, r, aniso=(1.0, 1.0, 1.0)):
    g = grid(shape)
    return sum(((g[i] - c[i]) / aniso[i]) ** 2 for i in range(3)) < r * r


def perturb(mask, seed, shift=(1, 0, -1), p=0.002):
    """A prediction near the target: shifted by `shift` and with a sparse sprinkle of flipped voxels."""
    rng = np.random.default_rng(seed)
    out = np.roll(mask, shift, axis=(1, 2, 3))
    return out ^ (rng.random(mask.shape) < p)


def cases():
    for seed, S in ((11, 64), (12, 128)):
        _, m = blob_case(seed, 1, S)
        t = m[0].numpy() > 0.5
        yield f"blob{S}", perturb(t, seed), t, (1.0, 1.0, 1.0)
    sh = (37, 41, 29)
    t = np.stack([ball(sh, (18, 20, 14), 12, (1.0, 1.2, 0.8)), ball(sh, (17, 22, 13), 7), ball(sh, (19, 19, 15), 3)])
    p = np.stack([ball(sh, (20, 19, 13), 11), ball(sh, (16, 23, 12), 8), ball(sh, (25, 15, 20), 2)])
    yield "odd_37x41x29", p, t, (1.0, 1.0, 1.0)
    sh = (20, 24, 18)
    t = np.zeros((3,) + sh, bool)
    p = np.zeros((3,) + sh, bool)
    t[0, 5, 7, 9] = p[0, 12, 3, 15] = True                                # one voxel each
    t[1, 0, 0, 0] = p[1, 19, 23, 17] = True                               # opposite corners
    t[2, 10, 12, 9] = p[2, 10, 12, 9] = True                              # the same voxel
    yield "single_voxel", p, t, (1.0, 1.0, 1.0)
    sh = (30, 26, 34)
    g = grid(sh)
    t = np.stack([~ball(sh, (15, 13, 17), 9), (g[0] < 4) | (g[0] > 25) | (g[1] < 3) | (g[1] > 22) | (g[2] < 5) | (g[2] > 28),
                  np.ones(sh, bool)])
    p = np.stack([~ball(sh, (14, 12, 18), 10), (np.abs(g[0] - 15) < 3) | (np.abs(g[1] - 13) < 3) | (np.abs(g[2] - 17) < 3),
                  (g[0] + g[1] + g[2]) % 7 != 0])
    yield "touch_faces", p, t, (1.0, 1.0, 1.0)
    sh = (16, 20, 24)
    yield "all_ones", np.ones((3,) + sh, bool), np.ones((3,) + sh, bool), (1.0, 1.0, 1.0)
    sh = (24, 28, 20)
    b = np.stack([ball(sh, (12, 14, 10), 8), ball(sh, (12, 14, 10), 5), ball(sh, (11, 13, 9), 2)])
    z = np.zeros_like(b)
    yield "empty_pred", z, b, (1.0, 1.0, 1.0)
    yield "empty_target", b, z, (1.0, 1.0, 1.0)
    yield "empty_both", z, z.copy(), (1.0, 1.0, 1.0)
    _, m = blob_case(13, 1, 48)
    t = m[0].numpy() > 0.5
    yield "aniso_48", perturb(t, 13, shift=(0, 1, 1), p=0.001), t, (1.0, 1.0, 2.5)
    sh = (240, 240, 155)
    t = np.stack([ball(sh, (120, 120, 77), 40), ball(sh, (118, 122, 75), 25), ball(sh, (121, 119, 78), 12)])
    p = np.stack([ball(sh, (123, 118, 77), 38, (1.0, 1.1, 0.9)), ball(sh, (118, 125, 75), 27), ball(sh, (125, 119, 80), 10)])
    yield "brats_240x240x155", p, t, (1.0, 1.0, 1.0)


def expected(p, t, spacing):
    """HD95 per region and the six surface sizes, by the reference's own functions."""
    kd = RM.getHausdorff_KD(spacing=spacing)
    prob = torch.from_numpy(0.1 + 0.8 * p.astype(np.float32))[None]
    tgt = torch.from_numpy(t.astype(np.float32))[None]
    hd, counts = [], []
    for r, region in enumerate(("WT", "TC", "EC")):
        sa = kd.get_surface_points((prob[:, r] > 0.5).float())
        sb = kd.get_surface_points(tgt[:, r].float())
        counts += [len(sa), len(sb)]
        v = 0.0 if sa.size == 0 or sb.size == 0 else float(kd.hausdorff_distance_95(sa, sb))
        if len(sa) * len(sb) and max(len(sa), len(sb)) <= CDIST_MAX:
            dense = float(RM.getHausdorff(spacing=spacing)(prob, tgt, region=region))
            assert dense == v, (region, dense, v)
        hd.append(v)
    return np.array(hd, np.float64), np.array(counts, np.int64)


def main():
    arrs, names = {}, []
    for name, p, t, spacing in cases():
        p, t = np.ascontiguousarray(p, bool), np.ascontiguousarray(t, bool)
        hd, counts = expected(p, t, spacing)
        print(f"  {name:20s} {p.shape[1:]} spacing={spacing} hd95={hd} surfaces={counts.tolist()}")
        names.append(name)
        arrs[f"{name}__shape"] = np.array(p.shape[1:], np.int64)
        arrs[f"{name}__pred"] = np.packbits(p.ravel())
        arrs[f"{name}__target"] = np.packbits(t.ravel())
        arrs[f"{name}__spacing"] = np.array(spacing, np.float64)
        arrs[f"{name}__hd95"] = hd
        arrs[f"{name}__counts"] = counts
    np.savez_compressed(os.path.join(HERE, "metric_hd95.npz"), names=np.array(names), **arrs)


if __name__ == "__main__":
    main()
