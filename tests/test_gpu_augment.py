"""-m gpu: training-time augmentation on the device (csrc/augment.hip via xlstm_hved_amd.augment) against the reference's own
outputs (tests/golden/aug_transform.npz, from transform.py), the documented word -> parameter mapping (restated on
oracle/philox_ref.py), the distributions of the draws, determinism and the generator state, mixed-shape / mixed-storage
batches at the training crop, graph capture, and TrainStep.replay_augmented."""
import os

import numpy as np
import pytest
import torch

from philox_ref import philox4x32_10

pytestmark = pytest.mark.gpu

import xlstm_hved_amd as X  # noqa: E402
from xlstm_hved_amd import augment as A  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aug_transform.npz")
STREAM = X._lib.XH_AUG_RNG_STREAM


def _golden():
    z = np.load(GOLDEN)
    return z, [str(n) for n in z["names"]]


Z, NAMES = _golden()


def _opt(v):
    return None if np.isnan(v) else float(v)


def _golden_transform(n):
    s_scale, s_shift, p, norm = Z[f"{n}__cfg"]
    crop = Z[f"{n}__crop"]
    t = A.transforms(scale=_opt(s_scale), shift=_opt(s_shift), flip_prob=_opt(p),
                     random_crop=None if crop[0] < 0 else tuple(int(c) for c in crop), normalize=bool(norm))
    a_scale, a_shift = Z[f"{n}__alpha"]
    u = Z[f"{n}__flip_u"]
    flip = (False, False) if np.isnan(p) else (bool(u[1] > p), bool(u[2] > p))
    params = A.pack_params(scale=1.0 if np.isnan(a_scale) else a_scale, shift=0.0 if np.isnan(a_shift) else a_shift,
                           origin=Z[f"{n}__origin"], flip=flip)
    return t, params


@pytest.fixture(scope="module")
def golden_bank():
    bank = A.VolumeBank(capacity=64)
    idx = {n: bank.register(torch.from_numpy(Z[f"{n}__img"]), torch.from_numpy(Z[f"{n}__lab"])) for n in NAMES}
    return bank, idx


@pytest.mark.parametrize("name", NAMES)
def test_golden_replay(golden_bank, name):
    bank, idx = golden_bank
    t, params = _golden_transform(name)
    x, m = t.apply(bank, [idx[name]], params)
    torch.cuda.synchronize()
    want_x, want_m = torch.from_numpy(Z[f"{name}__x"]), torch.from_numpy(Z[f"{name}__mask"])
    got_x, got_m = x[0].cpu(), m[0].cpu()
    assert torch.equal(got_m, want_m.float()), "masks are bit-exact"
    assert not torch.isnan(got_x).any()
    zero = want_x == 0
    assert torch.equal(got_x[zero], want_x[zero]) and not (got_x[~zero] == 0).any(), "zeros stay exactly zero"
    err = (got_x - want_x).abs().max().item()
    assert err <= 1e-6 * want_x.abs().max().item(), f"max|d| {err:.3e}"
    for dt in (torch.bfloat16, torch.float16):      # 16-bit storage = the fp32 result rounded to nearest-even
        xh, mh = t.apply(bank, [idx[name]], params, dtype=dt, mask_dtype=dt)
        assert torch.equal(xh[0].cpu(), x[0].cpu().to(dt)) and torch.equal(mh[0].float().cpu(), got_m)


def test_moments_fp64_and_deterministic(golden_bank):
    bank, idx = golden_bank
    for n in ("train_s1", "zero_channel", "one_voxel", "wide_w300"):
        img = Z[f"{n}__img"].astype(np.float64)
        got = bank.stats(idx[n])
        for c in range(4):
            v = img[c][img[c] != 0]
            assert got[c, 0] == v.size
            if v.size:
                assert abs(got[c, 1] - v.mean()) <= 1e-12 * abs(v.mean())
                assert abs(got[c, 2] - v.std()) <= 1e-10 * max(v.std(), 1.0)
            else:
                assert got[c, 1] == 0 and got[c, 2] == 0
    # bit-identical from run to run: the same volume registered again
    j = bank.register(torch.from_numpy(Z["wide_w300__img"]), torch.from_numpy(Z["wide_w300__lab"]))
    assert torch.equal(bank.moments[j], bank.moments[idx["wide_w300"]])


# ------------------------------------------------------------------------------------------------ the draws
def _u53(a, b):
    return float(((int(a) << 32) | int(b)) >> 11) * 2.0 ** -53


def _ranged(a, b, r):
    return (((int(a) << 32) | int(b)) * r) >> 64


def restate_draw(seed, counter, n, shapes, crop, s_scale, s_shift, p):
    """include/xlstm_hved.h xh_aug_draw, restated on philox_ref: sample k takes counter blocks i = 4 k + j, j = 0..3."""
    i = np.arange(4 * n, dtype=np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    c = np.stack([i & mask, (i >> np.uint64(32)) | np.uint64(STREAM << 24), np.full(4 * n, counter & 0xFFFFFFFF, np.uint64),
                  np.full(4 * n, (counter >> 32) & 0xFFFFFFFF, np.uint64)], -1)
    w = philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(n, 4, 4)
    out = []
    for k in range(n):
        B = w[k]
        sc = (1.0 - s_scale) + (2.0 * s_scale) * _u53(B[0, 0], B[0, 1]) if s_scale is not None else 1.0
        sh = (-s_shift) + (2.0 * s_shift) * _u53(B[0, 2], B[0, 3]) if s_shift is not None else 0.0
        D, H, W = shapes[k]
        o = [_ranged(B[1, 0], B[1, 1], D - crop[0]), _ranged(B[1, 2], B[1, 3], H - crop[1]), _ranged(B[2, 0], B[2, 1], W - crop[2])]
        f = [False, False] if p is None else [_u53(B[2, 2], B[2, 3]) > p, _u53(B[3, 0], B[3, 1]) > p]
        out.append((sc, sh, o, f))
    return out


def _vol(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((4,) + tuple(shape), generator=g) * 255
    img[img < 25] = 0
    lab = torch.randint(0, 5, tuple(shape), generator=g, dtype=torch.uint8)
    return (img.round().to(dtype) if dtype == torch.int16 else img), lab


@pytest.fixture(scope="module")
def draw_bank():
    bank = A.VolumeBank(capacity=8)
    shapes = [(20, 30, 40), (17, 33, 45)]
    for k, s in enumerate(shapes):
        bank.register(*_vol(s, 50 + k))
    return bank, shapes


def test_draws_are_the_documented_mapping(draw_bank):
    bank, shapes = draw_bank
    crop = (10, 20, 33)
    t = A.transforms(scale=0.1, shift=0.1, flip_prob=0.5, random_crop=crop)
    seed, c0 = 0x1234_5678_9ABC_DEF1, 2 ** 33 + 5
    t.set_state((seed, c0))
    idx = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1] * 9, dtype=torch.int32, device=DEV)
    n = idx.numel()
    for step in range(3):
        got = A.unpack_params(t.draw(bank, idx))
        want = restate_draw(seed, c0 + step, n, [shapes[v] for v in idx.tolist()], crop, 0.1, 0.1, 0.5)
        for k, (sc, sh, o, f) in enumerate(want):
            assert got["scale"][k] == sc and got["shift"][k] == sh, (step, k)
            assert got["origin"][k].tolist() == o and got["flip"][k].tolist() == f, (step, k)
    assert t.state() == (seed, c0 + 3)
    # the flags leave every other parameter's words alone: shift + flip + crop draws the same flips / origins / shift
    t2 = A.transforms(shift=0.1, flip_prob=0.5, random_crop=crop).set_state((seed, c0))
    got2 = A.unpack_params(t2.draw(bank, idx))
    want = restate_draw(seed, c0, n, [shapes[v] for v in idx.tolist()], crop, None, 0.1, 0.5)
    assert (got2["scale"] == 1.0).all() and got2["shift"].tolist() == [w[1] for w in want]
    assert got2["origin"].tolist() == [w[2] for w in want]


def test_distributions(draw_bank):
    from scipy import stats
    bank, shapes = draw_bank
    crop, p, N = (10, 20, 33), 0.3, 16384
    t = A.transforms(scale=0.2, shift=0.1, flip_prob=p, random_crop=crop).seed(77)
    idx = torch.zeros(N, dtype=torch.int32, device=DEV)
    q = A.unpack_params(t.draw(bank, idx))
    raw = t.last_params.cpu().numpy().view(A.PARAMS_DTYPE).reshape(-1)
    assert ((raw["flip"] & ~3) == 0).all(), "only D and H can flip"
    sigma = (p * (1 - p) / N) ** 0.5
    for ax in range(2):
        rate = q["flip"][:, ax].mean()
        assert abs(rate - (1 - p)) <= 5 * sigma, (ax, rate)          # flips when u > p
    for a in range(3):
        r = shapes[0][a] - crop[a]
        o = q["origin"][:, a]
        assert o.min() == 0 and o.max() == r - 1, "origins cover [0, size - crop - 1]; the bound is never drawn"
        counts = np.bincount(o, minlength=r)
        assert stats.chisquare(counts).pvalue > 1e-4, (a, counts)
    assert (q["scale"] >= 0.8).all() and (q["scale"] < 1.2).all()
    assert (q["shift"] >= -0.1).all() and (q["shift"] < 0.1).all()
    for v, lo, hi in ((q["scale"], 0.8, 1.2), (q["shift"], -0.1, 0.1)):
        assert stats.kstest(v, stats.uniform(lo, hi - lo).cdf).pvalue > 1e-4
    # W never flips on the voxels either: a volume whose value is 1 + w stays increasing along W
    wb = A.VolumeBank(capacity=1)
    ramp = (torch.arange(40, dtype=torch.float32) + 1).expand(4, 12, 14, 40).contiguous()
    wb.register(ramp, torch.zeros(12, 14, 40, dtype=torch.uint8))
    x, _ = A.transforms(flip_prob=0.0, random_crop=(6, 7, 40), normalize=False).seed(3)(wb, torch.zeros(64, dtype=torch.int32, device=DEV))
    assert torch.equal(x.cpu(), ramp[:, :6, :7].expand(64, 4, 6, 7, 40).cpu())


def test_determinism_seeds_and_state(draw_bank):
    bank, _ = draw_bank
    idx = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    t = A.transforms(scale=0.1, shift=0.1, flip_prob=0.5, random_crop=(10, 20, 33))
    t.seed(9)
    xa, ma = t(bank, idx)
    pa = t.last_params.clone()
    t.seed(9)
    xb, mb = t(bank, idx)
    assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(pa, t.last_params)
    t.seed(10)
    t(bank, idx)
    assert not torch.equal(pa, t.last_params), "different seeds, different draws"
    t.seed(9)
    t(bank, idx)
    mid = t.state()
    assert mid == (9, 1)
    after = [t.draw(bank, idx).clone() for _ in range(2)]
    t.set_state(mid)                                                     # a checkpoint resumes the stream
    again = [t.draw(bank, idx).clone() for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(after, again))
    # ranks: base seed + rank draw independent streams
    r0 = A.transforms(shift=0.1, flip_prob=0.5, random_crop=(10, 20, 33)).seed(100)
    r1 = A.transforms(shift=0.1, flip_prob=0.5, random_crop=(10, 20, 33)).seed(101)
    assert not torch.equal(r0.draw(bank, idx), r1.draw(bank, idx))


# ------------------------------------------------------------------------------------------------ batches and graphs
def test_mixed_batch_at_the_training_crop():
    """N = 3 from volumes of different shapes stored as fp32 and int16, crop 128 x 192 x 128: each sample equals its
    single-sample result, and int16 storage gives what fp32 storage of the same values gives."""
    bank = A.VolumeBank(capacity=4)
    img0, lab0 = _vol((140, 200, 150), 1)
    img1, lab1 = _vol((131, 197, 129), 2, torch.int16)
    img2, lab2 = _vol((128, 240, 155), 3)
    for im, lb in ((img0, lab0), (img1, lab1), (img2, lab2)):
        bank.register(im, lb)
    i1f = bank.register(img1.float(), lab1)
    t = A.transforms(shift=0.1, flip_prob=0.5, random_crop=(128, 192, 128)).seed(5)
    idx = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    x, m = t(bank, idx, dtype=torch.bfloat16)
    params = t.last_params.clone()
    assert not torch.isnan(x.float()).any()
    q = A.unpack_params(params)
    assert q["origin"][2, 0] == 0                                     # crop == size on D
    for k in range(3):
        xs, ms = t.apply(bank, [k], params[k:k + 1], dtype=torch.bfloat16)
        assert torch.equal(xs[0], x[k]) and torch.equal(ms[0], m[k]), k
    xf, mf = t.apply(bank, [i1f], params[1:2], dtype=torch.bfloat16)
    assert torch.equal(xf[0], x[1]) and torch.equal(mf[0], m[1])
    # against a host restatement of sample 0 (fp32 output)
    x0, m0 = t.apply(bank, [0], params[0:1])
    im = img0.double().numpy()
    o, f, sh = q["origin"][0], q["flip"][0], q["shift"][0]
    ref = []
    for c in range(4):
        v = im[c][im[c] != 0]
        ch = np.where(im[c] != 0, im[c] + np.float32(v.std()) * np.float32(sh), 0)
        if f[0]:
            ch = ch[::-1]
        if f[1]:
            ch = ch[:, ::-1]
        ref.append(ch[o[0]:o[0] + 128, o[1]:o[1] + 192, o[2]:o[2] + 128] / 255.0)
    ref = torch.from_numpy(np.stack(ref))
    assert (x0[0].double().cpu() - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()


def test_graph_capture(draw_bank):
    bank, shapes = draw_bank
    crop = (10, 20, 33)
    t = A.transforms(scale=0.1, shift=0.1, flip_prob=0.5, random_crop=crop).seed(21)
    idx = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=DEV)
    x = torch.empty((4, 4) + crop, device=DEV)
    m = torch.empty((4, 3) + crop, device=DEV)
    t(bank, idx, out=(x, m))                                 # warm-up (and the generator words on the device)
    torch.cuda.synchronize()
    seed, c0 = t.state()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t(bank, idx, out=(x, m))
    params = t.last_params
    assert t.state() == (seed, c0), "capturing draws nothing"
    for r in range(3):
        g.replay()
        got = A.unpack_params(params)
        want = restate_draw(seed, c0 + r, 4, [shapes[v] for v in idx.tolist()], crop, 0.1, 0.1, 0.5)
        for k, (sc, sh, o, f) in enumerate(want):
            assert got["scale"][k] == sc and got["shift"][k] == sh and got["origin"][k].tolist() == o and got["flip"][k].tolist() == f
        xe, me = t.apply(bank, idx, params)
        assert torch.equal(xe, x) and torch.equal(me, m), r
    assert t.state() == (seed, c0 + 3)


def test_trainstep_replay_augmented():
    """A captured TrainStep fed by replay_augmented gives the parts replay() gives on the batch built eagerly from the same
    parameters."""
    from gpu_common import load
    import disc_common as DC
    from xlstm_hved_amd.train_step import TrainStep
    S = 32
    torch.manual_seed(7)
    eps = [[torch.randn(1, 2 ** l, S >> (l + 1), S >> (l + 1), S >> (l + 1)).to(DEV) for l in range(4)] for _ in range(2)]
    model = X.XLSTM_HVED(1, 3, **X.TRAIN_KWARGS)
    model.load_state_dict(load("weights_seed1"), strict=True)
    model = model.to(DEV).train()
    d = X.Discriminator(in_channels=7, ks=4, strides=[1, 2, 2, 2])
    d.load_state_dict(DC.seeded_disc_state(4), strict=True)
    ts = TrainStep(model, d.to(DEV), alpha=0.1, beta=0.2, storage=torch.bfloat16)
    ts.capture(torch.zeros(1, 4, S, S, S, device=DEV), torch.zeros(1, 3, S, S, S, device=DEV), eps_lists=eps)
    bank = A.VolumeBank(capacity=2)
    bank.register(*_vol((40, 36, 34), 11))
    bank.register(*_vol((33, 45, 32), 12, torch.int16))
    t = A.transforms(shift=0.1, flip_prob=0.5, random_crop=S).seed(4)
    for k, subset in ((0, [3]), (1, [12])):
        idx = torch.tensor([k], dtype=torch.int32, device=DEV)
        got = ts.replay_augmented(bank, idx, subset, t, update=False)
        got = {n: got[n].clone() for n in ("dice", "m_dice", "recon", "kld", "g_gan", "loss", "loss_d")}
        xe, me = t.apply(bank, idx, t.last_params)
        assert torch.equal(xe, ts._sx) and torch.equal(me, ts._smask)
        want = ts.replay(xe, me, subset, eps_lists=eps, update=False)
        torch.cuda.synchronize()
        for n, v in got.items():
            a, b = v.item(), want[n].item()
            assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (k, n, a, b)
