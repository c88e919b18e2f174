"""Times ops.hd95 (all three regions of one volume, csrc/hd95.hip) on a BraTS-shaped 240 x 240 x 155 volume with nested
spheres, after a warm-up.  Prints one JSON line (ms per call by CUDA events).  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_hd95.py` for the per-kernel times."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xlstm_hved_amd as X  # noqa: E402


def volume(shape=(240, 240, 155), dev="cuda"):
    g = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device=dev) for s in shape], indexing="ij"))

    def ball(c, r):
        return ((g - torch.tensor(c, device=dev).view(3, 1, 1, 1)) ** 2).sum(0) < r * r

    t = torch.stack([ball((120., 120., 77.), 40), ball((118., 122., 75.), 25), ball((121., 119., 78.), 12)])[None]
    p = torch.stack([ball((123., 118., 77.), 38), ball((118., 125., 75.), 27), ball((125., 119., 80.), 10)])[None]
    return (0.9 * p.float()).contiguous(), t.to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0))
    a = ap.parse_args()
    prob, tgt = volume()
    for _ in range(a.warmup):
        out = X.ops.hd95(prob, tgt, tuple(a.spacing))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = X.ops.hd95(prob, tgt, tuple(a.spacing))
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"shape": [240, 240, 155], "spacing": list(a.spacing), "ms_per_volume": e0.elapsed_time(e1) / a.iters,
                      "hd95": out.cpu().tolist()}))


if __name__ == "__main__":
    main()
