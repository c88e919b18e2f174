"""Times the training augmentation of csrc/augment.hip on BraTS-shaped 4 x 240 x 240 x 155 volumes: the apply launch at the
training crop 1 x 4 x 128 x 192 x 128 (bf16 x, fp32 mask; int16 and fp32 sources), the draw launch, the moments pass done
once per registered volume, and a numpy restatement of the host transform (transform.py: shift + flip + crop + /255 +
SegToMask) on the same input.  Prints one JSON line (device times by CUDA events; bytes = what the kernel must move).
Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py` for the per-kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xlstm_hved_amd as X  # noqa: E402
from xlstm_hved_amd import augment as A  # noqa: E402

SHAPE, CROP = (240, 240, 155), (128, 192, 128)
HBM_PEAK = 8.0e12


def volume(dtype, seed, dev="cuda"):
    g = torch.Generator(device=dev).manual_seed(seed)
    img = torch.rand((4,) + SHAPE, generator=g, device=dev) * 255
    img[img < 60] = 0                                     # about a quarter background, as in a skull-stripped scan
    lab = (torch.rand(SHAPE, generator=g, device=dev) * 5).to(torch.uint8)
    return (img.round().to(torch.int16) if dtype == torch.int16 else img), lab


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters              # us


def host_transform(img, lab, a_shift, flip, origin):
    """transform.py's numpy arithmetic for shift + flip + crop + Normalize + SegToMask on one (4, D, H, W) fp32 volume."""
    x = np.stack([np.where(img[c] != 0, img[c] + np.std(img[c][img[c] != 0]) * a_shift, 0) for c in range(4)])
    m = lab
    for ax in (1, 2):
        if flip[ax - 1]:
            x, m = np.stack([np.flip(x[c], ax - 1) for c in range(4)]), np.flip(m, ax - 1)
    sl = tuple(slice(o, o + c) for o, c in zip(origin, CROP))
    x, m = x[(slice(None),) + sl] / 255.0, m[sl]
    return x, np.stack([m > 0, (m == 1) | (m == 2) | (m == 3), m == 1]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=3)
    a = ap.parse_args()
    bank = A.VolumeBank(capacity=4)
    vols = {"int16": volume(torch.int16, 1), "fp32": volume(torch.float32, 2)}
    ids = {k: bank.register(*v) for k, v in vols.items()}
    torch.cuda.synchronize()
    t = A.transforms(shift=0.1, flip_prob=0.5, random_crop=CROP).seed(0)
    dhw = CROP[0] * CROP[1] * CROP[2]
    x = torch.empty((1, 4) + CROP, dtype=torch.bfloat16, device="cuda")
    m = torch.empty((1, 3) + CROP, dtype=torch.float32, device="cuda")
    out = {"crop": list(CROP), "volume": list(SHAPE), "x_dtype": "bf16", "mask_dtype": "fp32", "hbm_peak_GBps": HBM_PEAK / 1e9}
    for name, src_bytes in (("int16", 2), ("fp32", 4)):
        idx = torch.tensor([ids[name]], dtype=torch.int32, device="cuda")
        params = t.draw(bank, idx)
        us = timed(lambda: X.ops.aug_apply(bank.table, bank.capacity, bank.moments, idx, params, t.flags, x, m), a.iters, a.warmup)
        nbytes = dhw * (4 * src_bytes + 1 + 4 * 2 + 3 * 4)
        out[f"apply_{name}"] = {"us_per_sample": us, "bytes": nbytes, "GBps": nbytes / us / 1e3, "frac_of_hbm_peak": nbytes / (us * 1e-6) / HBM_PEAK}
    idx = torch.tensor([ids["int16"]], dtype=torch.int32, device="cuda")
    out["draw_us"] = timed(lambda: t.draw(bank, idx), a.iters, a.warmup)
    out["draw_apply_us"] = timed(lambda: t(bank, idx, out=(x, m)), a.iters, a.warmup)
    for name, src_bytes in (("int16", 2), ("fp32", 4)):
        img, lab = vols[name]
        desc = X._lib.AugVolume(img.data_ptr(), lab.data_ptr(), *SHAPE, X._lib.XH_F32 if name == "fp32" else X._lib.XH_I16)
        row = torch.empty(4, 4, dtype=torch.float64, device="cuda")
        us = timed(lambda: X.ops.aug_moments(desc, row), 20, 3)
        nbytes = 4 * SHAPE[0] * SHAPE[1] * SHAPE[2] * src_bytes
        out[f"moments_{name}"] = {"us_per_volume": us, "bytes": nbytes, "GBps": nbytes / us / 1e3}
    # the host transform the reference runs per sample, on the same fp32 volume
    img, lab = (v.cpu().numpy() for v in vols["fp32"])
    rng = np.random.default_rng(0)
    ts = []
    for _ in range(a.host_iters):
        t0 = time.perf_counter()
        host_transform(img, lab, rng.uniform(-0.1, 0.1), rng.uniform(size=2) > 0.5,
                       [int(rng.integers(0, s - c)) for s, c in zip(SHAPE, CROP)])
        ts.append(time.perf_counter() - t0)
    out["host_numpy_ms_per_sample"] = 1e3 * float(np.median(ts))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
