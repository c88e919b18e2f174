"""Training-time augmentation on the GPU: transform.py:10-28 (`transforms(shift=0.1, flip_prob=0.5, random_crop=crop_size)`,
train.py:121) applied to volumes that live on the device (csrc/augment.hip, include/xlstm_hved.h "Training-time augmentation").

    bank = VolumeBank()                                   # device-resident volumes, one row per subject
    i = bank.register(images, labels)                     # (4, D, H, W) fp32 | int16, (D, H, W) labels; moments computed once
    t = transforms(shift=0.1, flip_prob=0.5, random_crop=(128, 192, 128))
    x, mask = t(bank, indices)                            # (N, 4, d, h, w), (N, 3, d, h, w): one draw + one gather launch

It replaces what GBMset.__getitem__ (BraTSdataset.py:389-390) does with the tensors: the reference's order is kept
(IntensityScale, IntensityShift, RandomFlip, Random_Crop_3D, Normalize, SegToMask) and so are its quirks:
  * RandomFlip acts on (1, D, H, W) arrays, so its first draw flips the singleton axis (nothing), D and H can flip and W never
    does; an axis flips when its uniform is > flip_prob;
  * Random_Crop_3D draws each origin with np.random.randint(0, size - crop): the last origin is never drawn;
  * SegToMask: WT = label > 0, TC = label in {1, 2, 3}, ET = label == 1 (label 4 counts for WT only);
  * IntensityShift adds std * alpha to the nonzero voxels only, the std (ddof 0) taken over the nonzero voxels of the whole
    pre-crop channel; one alpha for all channels.
The parameters come from a device-resident Philox4x32-10 counter (one draw per launch), so a captured graph draws afresh on
every replay; `seed()`, `state()` and `set_state()` manage it.  RandomRotate / Scale (scipy interpolation, not used by
train.py) are not provided."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops

PARAMS_DTYPE = np.dtype([("scale", "<f8"), ("shift", "<f8"), ("origin", "<i4", (3,)), ("flip", "<i4")])
assert PARAMS_DTYPE.itemsize == L.AUG_PARAMS_BYTES
_DESC_BYTES = C.sizeof(L.AugVolume)
_AXES = ("z", "y", "x")


class VolumeBank:
    """Device-resident training volumes.  The descriptor table and the moments have a fixed capacity, so their addresses never
    change: a graph captured over the bank keeps working as volumes are added."""

    def __init__(self, capacity=2048, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("VolumeBank lives on the GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = int(capacity)
        self.table = torch.zeros(self.capacity * _DESC_BYTES, dtype=torch.uint8, device=self.device)
        self.moments = torch.zeros(self.capacity, 4, 4, dtype=torch.float64, device=self.device)
        self.shapes = []
        self._keep = []

    def __len__(self):
        return len(self.shapes)

    def register(self, images, labels):
        """images (4, D, H, W) fp32 or int16 (or (4, 1, D, H, W) as GBMset stacks them); labels (D, H, W) (or (1, D, H, W)),
        integer label values 0..255.  Uploads both, computes the nonzero moments of each channel once and returns the index."""
        if len(self.shapes) >= self.capacity:
            raise RuntimeError(f"VolumeBank is full ({self.capacity} volumes)")
        img = torch.as_tensor(images)
        lab = torch.as_tensor(labels)
        if img.dim() == 5 and img.shape[1] == 1:
            img = img[:, 0]
        if lab.dim() == 4 and lab.shape[0] == 1:
            lab = lab[0]
        if img.dim() != 4 or img.shape[0] != 4:
            raise ValueError(f"images must be (4, D, H, W), got {tuple(img.shape)}")
        if tuple(lab.shape) != tuple(img.shape[1:]):
            raise ValueError(f"labels must be (D, H, W) = {tuple(img.shape[1:])}, got {tuple(lab.shape)}")
        if img.dtype == torch.float32:
            dt = L.XH_F32
        elif img.dtype == torch.int16:
            dt = L.XH_I16
        else:
            raise ValueError(f"images must be fp32 or int16, got {img.dtype}")
        img = img.to(self.device).contiguous()
        lab = lab.to(self.device).to(torch.uint8).contiguous() if lab.dtype != torch.uint8 else lab.to(self.device).contiguous()
        d, h, w = (int(s) for s in img.shape[1:])
        desc = L.AugVolume(img.data_ptr(), lab.data_ptr(), d, h, w, dt)
        i = len(self.shapes)
        row = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8)
        self.table[i * _DESC_BYTES:(i + 1) * _DESC_BYTES].copy_(row)
        ops.aug_moments(desc, self.moments[i])
        self._keep.append((img, lab))
        self.shapes.append((d, h, w))
        return i

    def stats(self, i):
        """(4, 3) fp64 host array {count, mean, std} of the nonzero voxels of volume i's channels."""
        return self.moments[i, :, :3].cpu().numpy()


def pack_params(scale=1.0, shift=0.0, origin=(0, 0, 0), flip=(False, False), n=None):
    """Host parameter rows (PARAMS_DTYPE) for `Transform.apply`.  Arguments broadcast over n samples; flip = (flip D, flip H)."""
    scale, shift = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    origin, flip = np.asarray(origin, np.int64).reshape(-1, 3), np.asarray(flip, bool).reshape(-1, 2)
    if n is None:
        n = max(scale.size, shift.size, origin.shape[0], flip.shape[0])
    p = np.zeros(n, PARAMS_DTYPE)
    p["scale"], p["shift"] = np.broadcast_to(scale.reshape(-1), (n,)), np.broadcast_to(shift.reshape(-1), (n,))
    p["origin"] = np.broadcast_to(origin, (n, 3))
    p["flip"] = np.broadcast_to(flip[:, 0].astype(np.int32) | (flip[:, 1].astype(np.int32) << 1), (n,))
    return p


def unpack_params(params):
    """Device (N, 32) uint8 parameter rows (or host PARAMS_DTYPE rows) -> dict of host arrays: scale, shift (N,) fp64,
    origin (N, 3) int, flip (N, 2) bool.  Synchronises."""
    p = params.cpu().numpy().view(PARAMS_DTYPE).reshape(-1) if torch.is_tensor(params) else np.asarray(params, PARAMS_DTYPE)
    return dict(scale=p["scale"].copy(), shift=p["shift"].copy(), origin=p["origin"].astype(np.int64),
                flip=np.stack([(p["flip"] & 1) != 0, (p["flip"] & 2) != 0], -1))


def _crop3(random_crop):
    if random_crop is None:
        return None
    c = list(random_crop) if type(random_crop) in (tuple, list) else [random_crop] * 3      # transform.py:220-221
    if len(c) != 3:
        raise ValueError(f"random_crop must be one size or three, got {random_crop}")
    return [int(v) for v in c]


class Transform:
    """The callable `transforms(...)` returns.  t(bank, indices) draws the parameters on the device and builds the batch;
    t.apply(bank, indices, params) builds it from given parameters."""

    def __init__(self, scale=None, shift=None, flip_prob=None, random_crop=None, normalize=True):
        self.scale, self.shift, self.flip_prob = scale, shift, flip_prob
        self.crop = _crop3(random_crop)
        self.normalize = bool(normalize)
        self.flags = ((L.XH_AUG_SCALE if scale is not None else 0) | (L.XH_AUG_SHIFT if shift is not None else 0)
                      | (L.XH_AUG_FLIP if flip_prob is not None else 0) | (L.XH_AUG_NORMALIZE if normalize else 0))
        self._state = (torch.initial_seed() & (2 ** 64 - 1), 0)
        self._rng = None
        self.last_params = None

    # -------------------------------------------------------------------------------------------- generator state
    @staticmethod
    def _signed(v):
        v &= 2 ** 64 - 1
        return v - 2 ** 64 if v >= 2 ** 63 else v

    def _rng_on(self, device):
        if self._rng is None or self._rng.device != device:
            s, c = self.state()
            self._rng = torch.tensor([self._signed(s), self._signed(c)], dtype=torch.int64, device=device)
        return self._rng

    def seed(self, s):
        """Restarts the stream at draw 0 of seed s (per rank: base seed + rank)."""
        self.set_state((int(s), 0))
        return self

    def state(self):
        """(seed, draw counter) as unsigned ints: the next launch draws with this counter.  Synchronises when on the device."""
        if self._rng is None:
            return self._state
        s, c = (int(v) & (2 ** 64 - 1) for v in self._rng.cpu().tolist())
        return s, c

    def set_state(self, state):
        s, c = (int(v) & (2 ** 64 - 1) for v in state)
        self._state = (s, c)
        if self._rng is not None:
            self._rng.copy_(torch.tensor([self._signed(s), self._signed(c)], dtype=torch.int64))
        return self

    # -------------------------------------------------------------------------------------------- shapes and checks
    def _indices(self, bank, indices):
        """(device int32 indices, host list of the indices or None when they already live on the device)."""
        if torch.is_tensor(indices) and indices.is_cuda:
            if indices.dim() != 1 or indices.numel() == 0 or indices.dtype not in (torch.int32, torch.int64):
                raise ValueError("indices: a non-empty 1-D int32 / int64 tensor")
            return indices.to(torch.int32).contiguous(), None
        host = [int(v) for v in (indices.tolist() if torch.is_tensor(indices) else np.asarray(indices).reshape(-1).tolist())]
        if not host:
            raise ValueError("indices: at least one sample")
        for v in host:
            if not 0 <= v < len(bank):
                raise IndexError(f"volume index {v} outside the bank (0..{len(bank) - 1})")
        return torch.tensor(host, dtype=torch.int32).to(bank.device), host

    def out_shape(self, bank, host=None):
        """(d, h, w) of the batch; raises the reference's ValueError when the crop exceeds a volume (the volumes of `host`,
        or every registered volume when the indices live on the device)."""
        if len(bank) == 0:
            raise ValueError("the VolumeBank is empty")
        shapes = [bank.shapes[v] for v in host] if host is not None else bank.shapes
        if self.crop is None:
            if len(set(shapes)) != 1:
                raise ValueError("without random_crop every volume of the batch must have the same shape")
            return shapes[0]
        for a in range(3):
            if any(self.crop[a] > s[a] for s in shapes):           # transform.py:231-249
                raise ValueError(f"crop_size[{a}] must be smaller or equal to the images {_AXES[a]} dimension")
        return tuple(self.crop)

    def _outputs(self, n, shape, device, out, dtype, mask_dtype):
        if out is None:
            return (torch.empty((n, 4) + tuple(shape), dtype=dtype, device=device),
                    torch.empty((n, 3) + tuple(shape), dtype=mask_dtype, device=device))
        x, m = out
        if tuple(x.shape) != (n, 4) + tuple(shape) or tuple(m.shape) != (n, 3) + tuple(shape):
            raise ValueError(f"out must be ({n}, 4, *{shape}) and ({n}, 3, *{shape}), got {tuple(x.shape)} and {tuple(m.shape)}")
        return x, m

    # -------------------------------------------------------------------------------------------- launches
    def draw(self, bank, indices):
        """Draws the parameters of a batch on the device ((N, 32) uint8 rows of xh_aug_params) and advances the generator."""
        idx, host = self._indices(bank, indices)
        shape = self.out_shape(bank, host)
        return self._draw(bank, idx, shape)

    def _draw(self, bank, idx, shape):
        params = torch.empty(idx.numel(), L.AUG_PARAMS_BYTES, dtype=torch.uint8, device=bank.device)
        ops.aug_draw(bank.table, bank.capacity, idx, shape, self.flags, self.scale or 0.0, self.shift or 0.0,
                     self.flip_prob if self.flip_prob is not None else 1.0, self._rng_on(bank.device), params)
        self.last_params = params
        return params

    def __call__(self, bank, indices, out=None, dtype=torch.float32, mask_dtype=torch.float32):
        """(x (N, 4, d, h, w), mask (N, 3, d, h, w)) of volumes bank[indices] with freshly drawn parameters (kept in
        `last_params`).  indices: a list / host tensor (checked here) or a device tensor (no host synchronisation; capturable).
        out: optional (x, mask) to write into."""
        idx, host = self._indices(bank, indices)
        shape = self.out_shape(bank, host)
        x, m = self._outputs(idx.numel(), shape, bank.device, out, dtype, mask_dtype)
        params = self._draw(bank, idx, shape)
        return ops.aug_apply(bank.table, bank.capacity, bank.moments, idx, params, self.flags, x, m)

    def apply(self, bank, indices, params, out=None, dtype=torch.float32, mask_dtype=torch.float32):
        """The batch for given parameters: `params` = device rows from draw() / last_params, or host rows (pack_params,
        checked against the volumes' extents here)."""
        idx, host = self._indices(bank, indices)
        shape = self.out_shape(bank, host)
        if not torch.is_tensor(params):
            p = np.asarray(params, PARAMS_DTYPE).reshape(-1)
            if host is not None:
                for k, v in enumerate(host):
                    for a in range(3):
                        if not 0 <= p["origin"][k, a] <= bank.shapes[v][a] - shape[a]:
                            raise ValueError(f"sample {k}: origin {tuple(p['origin'][k])} outside volume {bank.shapes[v]}")
            params = torch.from_numpy(p.view(np.uint8).reshape(-1, L.AUG_PARAMS_BYTES).copy()).to(bank.device)
        if params.dtype != torch.uint8 or params.dim() != 2 or params.shape[1] != L.AUG_PARAMS_BYTES or not params.is_cuda:
            raise ValueError("params: (N, 32) uint8 device rows")
        x, m = self._outputs(idx.numel(), shape, bank.device, out, dtype, mask_dtype)
        return ops.aug_apply(bank.table, bank.capacity, bank.moments, idx, params.contiguous(), self.flags, x, m)


def transforms(scale=None, angle=None, shift=None, flip_prob=None, random_crop=None, normalize=True):
    """transform.py:10-28 with the reference's signature; returns a Transform (see the module docstring)."""
    if angle is not None:
        raise NotImplementedError("RandomRotate (angle=...) is not provided on the GPU: like Scale it is scipy interpolation, "
                                  "which train.py does not use")
    return Transform(scale=scale, shift=shift, flip_prob=flip_prob, random_crop=random_crop, normalize=normalize)
