"""-m gpu: the HD95 region metric on the device (csrc/hd95.hip via losses.getHausdorff / hd95_regions) against the reference's
own numbers (tests/golden/metric_hd95.npz, from metrics.py: Sobel surfaces + KDTree + np.percentile) and against an in-test
brute-force restatement (Sobel by conv3d, all-pairs distances by chunked torch.cdist); storage dtypes; one call vs three;
graph capture; and the per-volume evaluation row of inference.eval_overlap_metrics."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import load

pytestmark = pytest.mark.gpu

import xlstm_hved_amd as X  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_hd95.npz")
REGIONS = ("WT", "TC", "EC")


def _golden_cases():
    z = np.load(GOLDEN)
    out = {}
    for n in (str(v) for v in z["names"]):
        d, h, w = (int(v) for v in z[f"{n}__shape"])
        unpack = lambda k: torch.from_numpy(np.unpackbits(z[k])[:3 * d * h * w].reshape(1, 3, d, h, w).astype(bool))  # noqa: E731
        out[n] = (unpack(f"{n}__pred"), unpack(f"{n}__target"), tuple(float(s) for s in z[f"{n}__spacing"]),
                  torch.from_numpy(z[f"{n}__hd95"]), torch.from_numpy(z[f"{n}__counts"]))
    return out


GOLD = _golden_cases()


def _prob(mask, dtype=torch.float32):
    return (0.1 + 0.8 * mask.float()).to(DEV, dtype)


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300) if b != 0 else abs(a)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_golden_replay(name):
    p, t, spacing, want, want_counts = GOLD[name]
    got, counts = X.ops.hd95(_prob(p), t.to(DEV, torch.uint8), spacing, counts=True)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == want_counts.tolist(), "surface sizes differ from the reference's"
    tol = 1e-12 if spacing == (1.0, 1.0, 1.0) else 1e-6
    for r in range(3):
        assert _rel(got[r].item(), want[r].item()) <= tol, (name, REGIONS[r], got[r].item(), want[r].item())


# ---------------------------------------------------------------------------------------------- brute-force restatement
def _sobel():
    s = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    dv = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64)
    one = torch.ones(3, dtype=torch.float64)
    kx = torch.einsum("a,b,c->abc", s, s, dv)       # metrics.py:277-279 (d, h, w kernel axes)
    ky = torch.einsum("a,b,c->abc", one, dv, s)     # :281-283
    kz = torch.einsum("a,b,c->abc", dv, one, one)   # :285-287
    return torch.stack([kx, ky, kz])[:, None]


def _surface(m):
    r = F.conv3d(m.double()[None, None], _sobel(), padding=1)[0]
    return (r != 0).any(0).nonzero().double()


def _directed(q, s, spacing):
    sp = torch.tensor(spacing, dtype=torch.float64)
    q, s = q * sp, s * sp
    out = torch.empty(len(q), dtype=torch.float64)
    for i in range(0, len(q), 2048):
        out[i:i + 2048] = torch.cdist(q[i:i + 2048], s).min(1).values
    return out.numpy()


def brute_hd95(pmask, tmask, spacing=(1.0, 1.0, 1.0)):
    res = []
    for r in range(3):
        sa, sb = _surface(pmask[0, r]), _surface(tmask[0, r])
        if len(sa) == 0 or len(sb) == 0:
            res.append(0.0)
            continue
        res.append(max(np.percentile(_directed(sb, sa, spacing), 95), np.percentile(_directed(sa, sb, spacing), 95)))
    return res, [len(_surface(m[0, r])) for r in range(3) for m in (pmask, tmask)]


def _random_masks(seed, shape):
    g = torch.Generator().manual_seed(seed)
    grid = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32) for s in shape], indexing="ij"))

    def blobs(k):
        m = torch.zeros(shape, dtype=torch.bool)
        for _ in range(k):
            c = torch.rand(3, generator=g) * torch.tensor(shape, dtype=torch.float32)
            rad = 2 + torch.rand(1, generator=g).item() * min(shape) / 3
            ax = 0.6 + 0.8 * torch.rand(3, generator=g)
            m |= ((((grid - c.view(3, 1, 1, 1)) / ax.view(3, 1, 1, 1)) ** 2).sum(0) < rad * rad)
        return m

    t = torch.stack([blobs(3), blobs(2), blobs(1)])[None]
    p = torch.stack([blobs(3), blobs(2), blobs(1)])[None]
    p ^= torch.rand(p.shape, generator=g) < 0.001                          # scattered single voxels
    if seed % 5 == 0:
        p[0, 2] = False                                                    # an empty prediction region now and then
    return p, t


FUZZ = [(s, (24 + (7 * s) % 25, 24 + (11 * s) % 25, 24 + (5 * s) % 25)) for s in range(20)]
# W past one 64-bit ballot word (the W pass's cross-word bit scans): 65, two full words, and tails past 128 and 192
FUZZ += [(20, (20, 24, 65)), (21, (18, 22, 128)), (22, (16, 21, 131)), (23, (17, 19, 200))]


@pytest.mark.parametrize("seed,shape", FUZZ, ids=[f"{s}-{'x'.join(map(str, sh))}" for s, sh in FUZZ])
def test_fuzz_against_brute_force(seed, shape):
    p, t = _random_masks(seed, shape)
    want, want_counts = brute_hd95(p, t)
    got, counts = X.ops.hd95(_prob(p), t.to(DEV), counts=True)
    assert counts.cpu().tolist() == want_counts
    for r in range(3):
        assert _rel(got[r].item(), want[r]) <= 1e-12, (REGIONS[r], got[r].item(), want[r])


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 2.5), (0.8, 1.3, 1.0)])
def test_anisotropic_against_brute_force(spacing):
    p, t = _random_masks(101, (31, 36, 27))
    want, _ = brute_hd95(p, t, spacing)
    got = X.hd95_regions(_prob(p), t.to(DEV), spacing)
    for r in range(3):
        assert _rel(got[r].item(), want[r]) <= 1e-6, (REGIONS[r], got[r].item(), want[r])


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("t_dtype", [torch.uint8, torch.bool, torch.float32])
def test_storage_dtypes(in_dtype, t_dtype):
    p, t, _, want, _ = GOLD["odd_37x41x29"]
    got = X.hd95_regions(_prob(p, in_dtype), t.to(DEV, t_dtype))
    assert got.dtype == torch.float64 and got.shape == (3,) and got.device.type == "cuda"
    for r in range(3):
        assert _rel(got[r].item(), want[r].item()) <= 1e-12


def test_threshold_is_strict_in_storage_dtype():
    p, t, _, _, _ = GOLD["blob64"]
    prob = torch.where(p, torch.tensor(0.5 + 2 ** -8), torch.tensor(0.5)).to(DEV, torch.bfloat16)   # 0.5 itself is background
    a = X.hd95_regions(prob, t.to(DEV))
    b = X.hd95_regions(_prob(p), t.to(DEV))
    assert torch.equal(a, b)


def test_regions_equal_single_calls_and_names():
    p, t, _, _, _ = GOLD["blob64"]
    prob, tgt = _prob(p), t.to(DEV, torch.float32)
    all3 = X.hd95_regions(prob, tgt)
    for r, name in enumerate(REGIONS):
        one = X.getHausdorff()(prob, tgt, region=name)
        assert one.dim() == 0 and one.dtype == torch.float64
        assert one.item() == all3[r].item()
    assert X.getHausdorff()(prob, tgt, region="ET").item() == all3[2].item()
    assert X.getHausdorff_KD()(prob, tgt, region="EC").item() == all3[2].item()


def test_graph_capture_replays_eager_result():
    p1, t1, _, want1, _ = GOLD["odd_37x41x29"]
    p2, t2 = _random_masks(7, (37, 41, 29))
    prob, tgt = _prob(p1), t1.to(DEV)
    eager = X.hd95_regions(prob, tgt).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        X.hd95_regions(prob, tgt)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = X.hd95_regions(prob, tgt)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert all(_rel(out[r].item(), want1[r].item()) <= 1e-12 for r in range(3))
    prob.copy_(_prob(p2))                                   # new data through the same captured launches
    tgt.copy_(t2.to(DEV, tgt.dtype))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, X.hd95_regions(prob, tgt))


def test_eval_overlap_metrics_row():
    m = X.XLSTM_HVED(1, 3, **X.TRAIN_KWARGS)
    m.load_state_dict(load("weights_seed1"), strict=True)
    m = m.to(DEV).eval()
    torch.manual_seed(5)
    x = torch.rand(1, 4, 48, 40, 36, device=DEV)
    grid = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32) for s in (48, 40, 36)], indexing="ij"))
    r = ((grid - torch.tensor([24.0, 20.0, 18.0]).view(3, 1, 1, 1)) ** 2).sum(0).sqrt()
    mask = torch.stack([r < 14, r < 9, r < 4])[None].float().to(DEV)
    kw = dict(patch_size=(32, 32, 32), overlap_stepsize=(16, 16, 16))
    row = X.eval_overlap_metrics(m, x, mask, subset_idx=14, **kw)
    assert row.shape == (2, 3) and row.dtype == torch.float64 and row.device.type == "cuda"
    prob = X.eval_overlap_volume(m, x, subset_idx=14, **kw)
    dice = X.DiceRegion()
    for i, name in enumerate(REGIONS):
        assert row[0, i].item() == float(dice(prob, mask, region=name))
        assert row[1, i].item() == X.getHausdorff()(prob, mask, region=name).item()
    want, _ = brute_hd95((prob > 0.5).cpu(), mask.cpu().bool())
    for i in range(3):
        assert _rel(row[1, i].item(), want[i]) <= 1e-12
