"""Training-time augmentation (xlstm_hved_amd.augment, csrc/augment.hip): argument validation that needs no GPU, the host
parameter packing, and the golden fixture tests/golden/aug_transform.npz (made by tests/golden/make_augment.py from the
reference's transform.py): which cases it covers, and that its outputs follow from its recorded parameters."""
import os

import numpy as np
import pytest
import torch

import xlstm_hved_amd as X
from xlstm_hved_amd import augment as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aug_transform.npz")


class _Shapes:
    """What Transform.out_shape reads of a VolumeBank."""

    def __init__(self, *shapes):
        self.shapes = list(shapes)

    def __len__(self):
        return len(self.shapes)


def test_abi_entries_declared():
    sig = X._lib.SIGNATURES
    for n in ("xh_aug_moments_workspace_bytes", "xh_aug_moments", "xh_aug_draw", "xh_aug_apply"):
        assert n in sig
    assert len(sig["xh_aug_draw"][1]) == 12 and len(sig["xh_aug_apply"][1]) == 15
    assert A.PARAMS_DTYPE.itemsize == X._lib.AUG_PARAMS_BYTES == 32


def test_angle_rejected():
    with pytest.raises(NotImplementedError, match="RandomRotate.*Scale"):
        A.transforms(angle=10)


@pytest.mark.parametrize("crop, axis, name", [((241, 10, 10), 0, "z"), ((10, 250, 10), 1, "y"), ((10, 10, 156), 2, "x")])
def test_crop_too_large_message(crop, axis, name):
    t = A.transforms(shift=0.1, flip_prob=0.5, random_crop=crop)
    with pytest.raises(ValueError, match=rf"crop_size\[{axis}\] must be smaller or equal to the images {name} dimension"):
        t.out_shape(_Shapes((240, 240, 155)))


def test_crop_sizes():
    assert A.transforms(random_crop=64).crop == [64, 64, 64]                     # transform.py:220-221
    assert A.transforms(random_crop=(128, 192, 128)).out_shape(_Shapes((240, 240, 155), (130, 200, 128))) == (128, 192, 128)
    assert A.transforms(random_crop=[240, 240, 155]).out_shape(_Shapes((240, 240, 155))) == (240, 240, 155)
    # every registered volume counts when the indices live on the device; only the batch's volumes when they are given
    t = A.transforms(random_crop=(128, 192, 128))
    with pytest.raises(ValueError, match=r"crop_size\[0\]"):
        t.out_shape(_Shapes((240, 240, 155), (100, 240, 155)))
    assert t.out_shape(_Shapes((240, 240, 155), (100, 240, 155)), host=[0]) == (128, 192, 128)
    with pytest.raises(ValueError, match="same shape"):
        A.transforms(shift=0.1).out_shape(_Shapes((240, 240, 155), (200, 240, 155)))
    assert A.transforms(shift=0.1).out_shape(_Shapes((20, 30, 40))) == (20, 30, 40)


def test_flags():
    L = X._lib
    assert A.transforms().flags == L.XH_AUG_NORMALIZE
    assert A.transforms(shift=0.1, flip_prob=0.5, random_crop=8).flags == L.XH_AUG_SHIFT | L.XH_AUG_FLIP | L.XH_AUG_NORMALIZE
    assert A.transforms(scale=0.1, normalize=False).flags == L.XH_AUG_SCALE


def test_generator_state_on_host():
    t = A.transforms(shift=0.1).seed(2 ** 64 - 3)
    assert t.state() == (2 ** 64 - 3, 0)
    t.set_state((5, 2 ** 40 + 1))
    assert t.state() == (5, 2 ** 40 + 1)


def test_pack_unpack_params():
    p = A.pack_params(scale=[1.05, 0.93], shift=[-0.02, 0.07], origin=[[1, 2, 3], [4, 5, 6]], flip=[[True, False], [False, True]])
    assert p.dtype.itemsize == 32 and p.shape == (2,)
    q = A.unpack_params(p)
    assert q["scale"].tolist() == [1.05, 0.93] and q["shift"].tolist() == [-0.02, 0.07]
    assert q["origin"].tolist() == [[1, 2, 3], [4, 5, 6]] and q["flip"].tolist() == [[True, False], [False, True]]
    assert A.pack_params(n=3)["scale"].tolist() == [1.0, 1.0, 1.0]
    raw = torch.from_numpy(p.view(np.uint8).reshape(2, 32).copy())
    assert A.unpack_params(raw)["origin"].tolist() == [[1, 2, 3], [4, 5, 6]]


def test_bank_needs_gpu_device():
    with pytest.raises(ValueError):
        A.VolumeBank(capacity=4, device="cpu")


# ------------------------------------------------------------------------------------------------ golden fixture
def _golden():
    z = np.load(GOLDEN)
    return z, [str(n) for n in z["names"]]


def test_golden_covers_the_cases():
    z, names = _golden()
    train = [n for n in names if n.startswith("train_s")]
    assert len(train) >= 3
    for n in train:                                                         # shift + flip + crop: train.py:121
        cfg = z[f"{n}__cfg"]
        assert np.isnan(cfg[0]) and cfg[1] == 0.1 and cfg[2] == 0.5
    flips = {(ax, bool(z[f"{n}__flip_u"][ax] > 0.5)) for n in train for ax in (1, 2)}
    assert flips == {(1, False), (1, True), (2, False), (2, True)}, "each flip axis both ways"
    assert np.isnan(z["val_crop__cfg"][:3]).all()                           # crop only: the validation configuration
    cfg = z["scale_shift__cfg"]
    assert cfg[0] == 0.1 and cfg[1] == 0.1 and (z["scale_shift__crop"] == -1).all()
    crop, shape = z["crop_eq_h__crop"], z["crop_eq_h__img"].shape[1:]
    assert crop[1] == shape[1] and crop[0] < shape[0] and crop[2] < shape[2]
    img = z["zero_channel__img"]
    assert not img[2].any() and all(img[c].any() for c in (0, 1, 3))
    assert np.count_nonzero(z["one_voxel__img"][1]) == 1
    assert set(np.unique(z["labels_0to4__lab"]).tolist()) == {0, 1, 2, 3, 4}
    assert all(s % 2 == 1 for s in z["odd_13x17x11__img"].shape[1:]) and len(set(z["odd_13x17x11__img"].shape[1:])) == 3
    assert z["wide_w300__img"].shape[3] > 256 and z["wide_w300__crop"][2] > 256


def test_golden_follows_from_its_parameters():
    """Each case's outputs are the reference's arithmetic applied with the recorded parameters (fp32, numpy's promotion),
    and every recorded draw lies in the reference's ranges: flips only of D and H, origins in [0, size - crop - 1]."""
    z, names = _golden()
    for n in names:
        img, lab = z[f"{n}__img"], z[f"{n}__lab"]
        s_scale, s_shift, p, norm = z[f"{n}__cfg"]
        a_scale, a_shift = z[f"{n}__alpha"]
        u, o, crop = z[f"{n}__flip_u"], z[f"{n}__origin"], z[f"{n}__crop"]
        x = img.copy()
        if not np.isnan(s_scale):
            assert 1 - s_scale <= a_scale < 1 + s_scale
            x = x * float(a_scale)
        if not np.isnan(s_shift):
            assert -s_shift <= a_shift < s_shift
            x = np.stack([np.where(x[c] != 0, x[c] + (np.std(x[c][x[c] != 0]) if x[c].any() else np.float32(0)) * float(a_shift), 0)
                          for c in range(4)])
        m = lab
        if not np.isnan(p):
            for ax in (1, 2):
                if u[ax] > p:
                    x, m = np.flip(x, ax), np.flip(m, ax - 1)
        if crop[0] > 0:
            for a in range(3):
                size = img.shape[1 + a]
                assert (o[a] == 0) if crop[a] == size else (0 <= o[a] <= size - crop[a] - 1)
            sl = tuple(slice(int(oo), int(oo + c)) for oo, c in zip(o, crop))
            x, m = x[(slice(None),) + sl], m[sl]
        if norm:
            x = x / 255.0
        mask = np.stack([m > 0, (m >= 1) & (m <= 3), m == 1]).astype(np.uint8)
        assert x.dtype == np.float32 and np.array_equal(x, z[f"{n}__x"]), n
        assert np.array_equal(mask, z[f"{n}__mask"]), n
