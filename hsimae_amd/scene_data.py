"""Fine-tuning data that stays in the scene (Utils/Preprocessing.py:189-273 `get_data_set_dual`, Model_Finetuning.py:28-63
`HSIdataset`): the reference builds one symmetric-padded 9 x 9 x C window per pixel on the host (`data_cubes`, 81 copies of
the scene) and the non-overlapping tiles of the unpadded scene (`data_cubes_2`), and indexes them by pixel.  Here the scene
is the only array: a labeled, validation or unlabeled set is a table of pixel indices (+ labels) next to the one
HBM-resident [H, W, C] scene, and a batch (windows, flips, labels) is one `hsimae_scene_batch` launch (csrc/scene.hip).

  tile_origins / unlabeled_pixels   where `data_cubes_2`'s tiles sit, as the centre pixels of the equivalent padded windows
  split_labeled                     get_data_set_dual's train / test split (same np.random consumption, same order)
  get_scene_set_dual                get_data_set_dual without the cubes: (train_index, train_labels, scene, test_gt, gt_raw)
  SceneCubes                        HSIdataset over (scene, pixels, labels); works with hsimae_amd.data.DeviceLoader
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .data import draw_flips
from .scene_pass import PATCH, as_scene, batch_params, window_buffer


def tile_origins(length: int, size: int = PATCH) -> np.ndarray:
    """Origins of the tiles `splitHSI(.., stride 1)` cuts along an axis of `length` (get_inital_seq(length, size, 1)):
    0, size, 2 size, ... for every whole tile, one more tile if a remainder is left, and the LAST origin replaced by
    length - size so that the last tile ends at the axis' end (it overlaps its neighbour; negative when length < size)."""
    length, size = int(length), int(size)
    whole, rest = divmod(length, size)
    seq = np.arange(whole + (1 if rest else 0), dtype=np.int64) * size
    seq[-1] = length - size
    return seq


def unlabeled_pixels(H: int, W: int) -> np.ndarray:
    """int64 centre pixels (r + 4) * W + (c + 4) of `data_cubes_2`'s tiles, rows outer, columns inner: the unpadded tile at
    (r, c) is the padded window of that pixel, and it never touches the pad."""
    if H < PATCH or W < PATCH:
        raise ValueError(f"a {H} x {W} scene is smaller than one {PATCH} x {PATCH} tile: it has no unlabeled set")
    r, c = tile_origins(H) + PATCH // 2, tile_origins(W) + PATCH // 2
    return (r[:, None] * int(W) + c[None, :]).reshape(-1)


def split_labeled(gt, percent=None, num=None, mask=None):
    """The train / test split of get_data_set_dual (Utils/Preprocessing.py:219-273) -> (train_index, train_labels, test_gt).
    `mask` (same size as gt): its non-zero pixels are the training set, in pixel order; np.random is not touched.
    Otherwise ONE np.random.permutation(H * W); walking the pixels in that order, a labeled pixel joins the training set while
    its class has not reached its quota: ceil(count * percent), or `num` — and num - 5 for a class that has exactly `num`
    pixels, as the reference does.  test_gt is gt with the training pixels set to 0."""
    gt_raw = np.asarray(gt)
    flat = gt_raw.reshape(-1)
    n_classes = len(np.unique(flat))
    assert n_classes == flat.max() + 1, "the label map must use every class 0 .. max"
    test_gt = flat.copy()
    if mask is not None:
        m = np.asarray(mask).reshape(-1)
        assert len(m) == len(flat), "mask and gt differ in size"
        train_index = np.flatnonzero(m != 0).astype(np.int64)
    else:
        if not percent and not num:
            raise ValueError("give percent, num or mask")
        shuffled = np.random.permutation(np.arange(flat.shape[0]))
        labels = flat[shuffled]
        count = np.bincount(labels, minlength=n_classes)
        if percent:
            quota = np.ceil(count * percent)
        else:
            quota = np.where(count == num, num - 5, num).astype(np.float64)
        # rank of every pixel inside its class, in shuffled order (1-based)
        order = np.argsort(labels, kind="stable")
        first = np.concatenate([[0], np.cumsum(count)[:-1]])
        rank = np.empty(len(labels), dtype=np.int64)
        rank[order] = np.arange(len(labels)) - first[labels[order]] + 1
        train_index = shuffled[(labels != 0) & (rank <= quota[labels])].astype(np.int64)
    test_gt[train_index] = 0
    return train_index, flat[train_index], test_gt.reshape(gt_raw.shape)


def _load(a):
    return np.load(a) if isinstance(a, (str, bytes)) or hasattr(a, "__fspath__") else a


def _minmax(s: torch.Tensor) -> torch.Tensor:
    """(x - min) / (max - min) as numpy computes it in the scene's dtype.  fp32 goes through fp64 with a rounding to fp32
    after each operation: a correctly rounded fp32 result (53 >= 2 * 24 + 2 bits), whatever the device's fp32 division does."""
    mn, mx = s.min(), s.max()
    if s.dtype == torch.float64:
        return (s - mn) / (mx - mn)
    d = (s.double() - mn.double()).float()
    r = (mx.double() - mn.double()).float()
    return (d.double() / r.double()).float()


def get_scene_set_dual(data, gt, patch_size=9, percent=None, num=None, mask=None, norm=False, GWPCA=True, device="cuda:0"):
    """`get_data_set_dual` (Utils/Preprocessing.py:189-273) without `data_cubes` / `data_cubes_2`: the processed scene stays
    one [H, W, C] device tensor.  data / gt / mask: arrays or .npy paths.
    -> (train_index, train_labels, scene, test_gt, gt_raw); feed them to dual_branch_finetuning_scene / test_model_scene."""
    if patch_size != PATCH:
        raise NotImplementedError(f"patch_size={patch_size}: the window kernels cut {PATCH} x {PATCH} windows")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("hsimae_amd runs on MI355X only (no CPU fallback): get_scene_set_dual needs a GPU")
    raw = _load(data)
    gt_raw = np.asarray(_load(gt))
    if GWPCA:
        from .gwpca import GWPCA as _GWPCA
        scene = _GWPCA(32, 4, True).fit_transform(raw, device=device)
    else:
        from .gwpca import _as_scene
        scene = _as_scene(raw).to(device).contiguous()
    if norm:
        scene = _minmax(scene)
    if tuple(scene.shape[:2]) != tuple(gt_raw.shape):
        raise ValueError(f"scene is {tuple(scene.shape[:2])} pixels, the label map {tuple(gt_raw.shape)}")
    train_index, train_labels, test_gt = split_labeled(gt_raw, percent, num, None if mask is None else _load(mask))
    return train_index, train_labels, scene, test_gt, gt_raw


def _resident(s: torch.Tensor, device) -> torch.Tensor:
    if s.device.type != "cuda":
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("hsimae_amd.scene_data is device-resident: it needs a GPU (no CPU fallback)")
        s = s.to(device)
    return s.contiguous()


def device_scene(scene, device="cuda:0") -> torch.Tensor:
    """The [H, W, C] fp32 / fp64 scene as a contiguous device tensor: a contiguous device tensor is used as it is (shared, not
    copied, whatever `device` says); anything else is uploaded to `device` once."""
    return _resident(as_scene(scene), device)


class SceneCubes:
    """The fine-tuning `HSIdataset` (Model_Finetuning.py:28-63) over a scene: item i is the padded window of pixel
    `pixels[i]` (default: pixel i, the reference's `data_cubes[i]`) and, with `gt`, its label `gt[i]`.  A device tensor
    `scene` is shared, never copied: the labeled, validation and unlabeled sets of a run hold the same one.  The tables are
    checked on the host and uploaded once; every batch is one hsimae_scene_batch launch."""

    def __init__(self, scene, pixels=None, gt=None, train=False, device="cuda:0"):
        s = as_scene(scene)
        H, W, Cb = (int(v) for v in s.shape)
        pix = None
        if pixels is not None:
            pix = np.asarray(pixels)
            if pix.ndim != 1 or pix.dtype.kind not in "iu":
                raise ValueError("pixels must be a 1-D array of integer pixel indices (r * W + c)")
            pix = np.ascontiguousarray(pix.astype(np.int64))
            if pix.size and (pix.min() < 0 or pix.max() >= H * W):
                raise ValueError(f"pixel index out of range [0, {H * W}): min {int(pix.min())}, max {int(pix.max())}")
        n = H * W if pix is None else int(pix.size)
        lab = None
        if gt is not None:
            lab = np.asarray(gt)
            if lab.ndim != 1 or lab.dtype.kind not in "iu":
                raise ValueError("gt must be a 1-D array of integer labels")
            if lab.size != n:
                raise ValueError(f"{lab.size} labels for {n} items")
            lab = np.ascontiguousarray(lab.astype(np.int64))
        self.scene = _resident(s, device)
        self.device = self.scene.device
        self.train = train
        self.H, self.W, self.bands, self._n = H, W, Cb, n
        self.gt = lab
        self._pix = None if pix is None else torch.from_numpy(pix).to(self.device)
        self._y = None if lab is None else torch.from_numpy(lab).to(self.device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def __len__(self):
        return self._n

    def gather(self, indices, flips=None):
        """x [n, 1, C, 9, 9] fp32 (band-fastest: a permuted view of [n, 9, 9, C], the reference's own memory order) of the
        given items, and with labels (x, y).  `flips`: uint8 per sample (data.draw_flips), default none."""
        n = len(indices)
        idx = torch.as_tensor(np.asarray(indices, dtype=np.int64)).to(self.device)
        fl = None if flips is None else torch.as_tensor(np.asarray(flips, dtype=np.uint8)).to(self.device)
        if fl is not None and fl.numel() != n:
            raise ValueError(f"{fl.numel()} flip bytes for {n} items")
        out = window_buffer(n, self.bands, self.device)
        y = None if self._y is None else torch.empty(n, dtype=torch.int64, device=self.device)
        p = batch_params(self.scene, out, idx.data_ptr(), n, self._n, self._bad, flips=fl, pixels=self._pix, labels=self._y, y=y)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.load().hsimae_scene_batch(C.byref(p), stream), "hsimae_scene_batch")
        return out if y is None else (out, y)

    def batch(self, indices):
        """The batch a DataLoader(num_workers=0) would collate for these items (draws the flips now: two python-`random`
        draws per training sample, horizontal first; none in eval)."""
        return self.gather(indices, draw_flips(len(indices), self.train))

    def __getitem__(self, index):
        b = self.batch([index])
        return b[0] if self._y is None else (b[0][0], b[1][0])

    def check(self):
        """Raise if an item asked for since the last check() was outside the tables (one small copy from the device)."""
        if int(self._bad.item()):
            self._bad.zero_()
            raise RuntimeError(f"SceneCubes: an item index was outside [0, {self._n}) (its window was written as zeros, its label as -1)")
