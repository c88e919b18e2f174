"""HD95 region metric (losses.getHausdorff / hd95_regions, xh_hd95): argument validation that needs no GPU, and the golden
fixture tests/golden/metric_hd95.npz (made by tests/golden/make_hd95.py from the reference's metrics.py)."""
import os

import numpy as np
import pytest
import torch

import xlstm_hved_amd as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_hd95.npz")


def _pair(n=1, c=3, s=(6, 7, 8), tdtype=torch.uint8):
    return torch.rand((n, c) + s), (torch.rand((n, c) + s) > 0.5).to(tdtype)


def test_exports():
    assert X.getHausdorff_KD is X.getHausdorff
    assert callable(X.hd95_regions) and callable(X.eval_overlap_metrics)
    assert X.losses.getHausdorff is X.getHausdorff


def test_abi_entries_declared():
    lib = X._lib.SIGNATURES
    assert "xh_hd95" in lib and "xh_hd95_workspace_bytes" in lib
    assert len(lib["xh_hd95"][1]) == 17


@pytest.mark.parametrize("region", ["XX", "wt", "NCR", 0])
def test_unknown_region_raises(region):
    p, t = _pair()
    with pytest.raises(ValueError):
        X.getHausdorff()(p, t, region=region)


def test_softmax_mode_not_implemented():
    p, t = _pair()
    with pytest.raises(NotImplementedError):
        X.getHausdorff()(p, t, region="WT", mode="softmax")


def test_batch_of_two_raises():
    p, t = _pair(n=2)
    with pytest.raises(ValueError, match="N == 1"):
        X.getHausdorff()(p, t)
    with pytest.raises(ValueError):
        X.hd95_regions(p, t)


def test_shape_mismatch_raises():
    p, _ = _pair()
    _, t = _pair(s=(6, 7, 9))
    with pytest.raises(ValueError):
        X.getHausdorff()(p, t, region="TC")
    with pytest.raises(ValueError):
        X.hd95_regions(p[:, :, :, :, :4], t)
    with pytest.raises(ValueError):
        X.hd95_regions(p[0], t[0])                       # 4D


def test_too_few_channels_raises():
    p, t = _pair(c=2)
    with pytest.raises(ValueError):
        X.hd95_regions(p, t)


def test_bad_spacing_raises():
    p, t = _pair()
    for sp in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0)):
        with pytest.raises(ValueError):
            X.hd95_regions(p, t, sp)


@pytest.mark.parametrize("region", ["WT", "TC", "EC", "ET"])
@pytest.mark.parametrize("tdtype", [torch.uint8, torch.bool, torch.float32])
def test_host_tensors_raise_device_error(region, tdtype):
    p, t = _pair(tdtype=tdtype)
    with pytest.raises(RuntimeError, match="device tensors"):
        X.getHausdorff()(p, t, region=region)
    with pytest.raises(RuntimeError, match="device tensors"):
        X.getHausdorff_KD(spacing=(1.0, 1.0, 2.5))(p, t, region=region)


def test_unsupported_target_dtype_raises():
    p, _ = _pair()
    t = torch.zeros(p.shape, dtype=torch.int64)
    with pytest.raises(TypeError):
        X.hd95_regions(p, t)


def _golden():
    z = np.load(GOLDEN)
    return z, [str(n) for n in z["names"]]


def test_golden_loads_and_covers_the_cases():
    z, names = _golden()
    shapes = {n: tuple(int(v) for v in z[f"{n}__shape"]) for n in names}
    for n in names:
        d, h, w = shapes[n]
        for side in ("pred", "target"):
            bits = np.unpackbits(z[f"{n}__{side}"])[:3 * d * h * w]
            assert bits.size == 3 * d * h * w
        assert z[f"{n}__hd95"].shape == (3,) and z[f"{n}__hd95"].dtype == np.float64
        assert z[f"{n}__counts"].shape == (6,)
        assert np.all(z[f"{n}__hd95"] >= 0)
    assert shapes["blob64"] == (64, 64, 64) and shapes["blob128"] == (128, 128, 128)
    assert any(all(s % 2 for s in shapes[n]) and len(set(shapes[n])) == 3 for n in names)          # odd sizes
    assert shapes["brats_240x240x155"] == (240, 240, 155)
    for n in ("single_voxel", "touch_faces", "all_ones", "empty_pred", "empty_target", "empty_both"):
        assert n in names
    counts = {n: z[f"{n}__counts"] for n in names}
    assert (counts["empty_pred"][0::2] == 0).all() and (counts["empty_pred"][1::2] > 0).all()
    assert (counts["empty_target"][1::2] == 0).all() and (counts["empty_target"][0::2] > 0).all()
    assert (counts["empty_both"] == 0).all()
    assert all((z[f"{n}__hd95"] == 0).all() for n in ("empty_pred", "empty_target", "empty_both", "all_ones"))
    aniso = [n for n in names if tuple(z[f"{n}__spacing"]) != (1.0, 1.0, 1.0)]
    assert aniso and all((z[f"{n}__hd95"] > 0).all() for n in aniso)
    # the masks touch every face of the volume in touch_faces
    d, h, w = shapes["touch_faces"]
    t = np.unpackbits(z["touch_faces__target"])[:3 * d * h * w].reshape(3, d, h, w)
    for ax in range(1, 4):
        assert t.take(0, axis=ax).any() and t.take(-1, axis=ax).any()
