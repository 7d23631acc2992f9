"""Group-wise PCA of a raw scene on the device (Utils/GroupWisePCA.py `applyGWPCA`): `GWPCA` and `apply_gwpca`.

The raw [H, W, bands] array is min-max normalised over the whole scene, the band axis is halved `group // 2` times into
contiguous groups, and each group gets a (whitened) PCA with `nc // group` components; the groups' components are
concatenated into [H, W, nc].  All arithmetic is fp64 on the GPU (hsimae_gwpca_fit / hsimae_gwpca_apply, csrc/gwpca.hip): the
scene is uploaded once and the result stays on the device, so it can go straight into `predict_scene`.

Stated deviations from the reference: an fp32 scene is widened to fp64 (the reference would stay in fp32); the covariance is
accumulated centred, in two passes; and the PCA is the exact one of scikit-learn >= 1.5 (`covariance_eigh` / `full`), not the
randomized approximation that the scikit-learn 1.3 the reference pins picks for a large scene.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_GROUP_WIDTH = 128            # the eigen-solver keeps a group's w x w matrix in LDS


def group_offsets(bands: int, group: int = 4) -> list[int]:
    """Band offsets of the reference's `split_data`: every range is halved (c -> c // 2, c - c // 2), `group // 2` times.
    -> group + 1 offsets; 103 bands, group 4 -> [0, 25, 51, 77, 103]."""
    off = [0, int(bands)]
    for _ in range(group // 2):
        nxt = []
        for a, e in zip(off[:-1], off[1:]):
            nxt += [a, a + (e - a) // 2]
        off = nxt + [int(bands)]
    return off


def _check_args(nc, group, whiten):
    for name, v in (("nc", nc), ("group", group)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v).__name__}")
    if group not in (1, 2, 4):
        raise ValueError(f"group must be 1, 2 or 4, got {group}")
    if nc < 1 or nc % group:
        raise ValueError(f"nc must be a positive multiple of group={group}, got {nc}")
    return int(nc), int(group), bool(whiten)


def _as_scene(X, what="scene"):
    if isinstance(X, torch.Tensor):
        s = X.detach()
    elif isinstance(X, np.ndarray):
        if X.dtype not in (np.float32, np.float64):
            raise TypeError(f"{what} must be float32 or float64, got {X.dtype}")
        s = torch.from_numpy(np.ascontiguousarray(X))
    else:
        raise TypeError(f"{what} must be a numpy array or a torch tensor, got {type(X).__name__}")
    if s.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what} must be float32 or float64, got {s.dtype}")
    if s.dim() != 3:
        raise ValueError(f"{what} must be [H, W, bands], got shape {tuple(s.shape)}")
    return s


class GWPCA:
    """`applyGWPCA` as an estimator: fit(raw) learns min / max, the band means and each group's eigenpairs on the device;
    transform(raw2) projects any scene with the same band count; fit_transform(raw) does both.  Every result is a device
    tensor, enqueued on the current stream; nothing inside waits for the host."""

    def __init__(self, nc=32, group=4, whiten=True):
        self.nc, self.group, self.whiten = _check_args(nc, group, whiten)
        self._model = None
        self._bands = None

    # ---- fitted attributes (read-only device tensors) ----
    def _fitted(self):
        if self._model is None:
            raise RuntimeError("this GWPCA has not been fitted: call fit() or fit_transform() first")
        return self._model

    @property
    def min_(self):
        return self._fitted()["minmax"][0]

    @property
    def max_(self):
        return self._fitted()["minmax"][1]

    @property
    def mean_(self):
        """fp64 [bands]: the mean of every normalised band."""
        return self._fitted()["mean"]

    @property
    def explained_variance_(self):
        """fp64 [bands]: ALL eigenvalues of each group's covariance, descending inside the group, at the group's band offsets
        (`group_offsets_`); the first nc // group of a group are the retained ones."""
        return self._fitted()["lambda"]

    @property
    def group_offsets_(self):
        self._fitted()
        return group_offsets(self._bands, self.group)

    @property
    def components_(self):
        """One fp64 [nc // group, w_g] tensor per group: the signed unit eigenvectors (sklearn's `components_`).  With `whiten`
        they are recovered from the projection matrix, which holds them divided by max(sqrt(lambda), eps)."""
        m = self._fitted()
        k = self.nc // self.group
        out = []
        for a, e in zip(self.group_offsets_[:-1], self.group_offsets_[1:]):
            comp = m["proj"][a:e].t()
            if self.whiten:
                comp = comp * m["lambda"][a:a + k].sqrt().clamp_min(float(np.finfo(np.float64).eps))[:, None]
            out.append(comp)
        return out

    # ---- work ----
    def _params(self, s, model):
        H, W, Cb = (int(v) for v in s.shape)
        return _lib.GwpcaParams(scene=s.data_ptr(), scene_f64=int(s.dtype == torch.float64), H=H, W=W, C=Cb, nc=self.nc,
                                group=self.group, whiten=int(self.whiten), minmax=model["minmax"].data_ptr(),
                                mean=model["mean"].data_ptr(), lambda_=model["lambda"].data_ptr(), proj=model["proj"].data_ptr(),
                                group_off=model["group_off"].data_ptr())

    def _upload(self, X, device):
        s = _as_scene(X)
        H, W, Cb = (int(v) for v in s.shape)
        if H * W < 2:
            raise ValueError(f"a PCA needs at least 2 pixels, got scene shape {tuple(s.shape)}")
        off = group_offsets(Cb, self.group)
        widths = [e - a for a, e in zip(off[:-1], off[1:])]
        k = self.nc // self.group
        if max(widths) > MAX_GROUP_WIDTH:
            raise ValueError(f"scene shape {tuple(s.shape)}: {Cb} bands in {self.group} groups give a group of {max(widths)} bands, "
                             f"the eigen-solver serves at most {MAX_GROUP_WIDTH}")
        if k > min(widths) or k > H * W:
            raise ValueError(f"scene shape {tuple(s.shape)}: nc // group = {k} components need groups of at least {k} bands "
                             f"(narrowest: {min(widths)}) and at least {k} pixels")
        if device is None:
            device = s.device if s.device.type == "cuda" else (torch.device("cuda", torch.cuda.current_device())
                                                               if torch.cuda.is_available() else None)
        if device is None or torch.device(device).type != "cuda":
            raise RuntimeError("hsimae_amd runs on MI355X only (no CPU fallback): GWPCA needs a GPU")
        return s.to(device).contiguous()

    def fit(self, X, device=None):
        s = self._upload(X, device)
        dev, Cb = s.device, int(s.shape[2])
        k = self.nc // self.group
        lib = _lib.load()
        with torch.cuda.device(dev):
            f64 = dict(dtype=torch.float64, device=dev)
            model = {"minmax": torch.empty(2, **f64), "mean": torch.empty(Cb, **f64), "lambda": torch.empty(Cb, **f64),
                     "proj": torch.empty(Cb, k, **f64), "group_off": torch.empty(5, dtype=torch.int32, device=dev)}
            p = self._params(s, model)
            nbytes = lib.hsimae_gwpca_workspace_bytes(C.byref(p))
            if nbytes < 0:
                _lib.check(int(nbytes), "hsimae_gwpca_workspace_bytes")
            ws = torch.empty(nbytes // 8, **f64)
            _lib.check(lib.hsimae_gwpca_fit(C.byref(p), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "hsimae_gwpca_fit")
        self._model, self._bands = model, Cb
        return self

    def transform(self, X, dtype=torch.float64, device=None):
        """-> [H, W, nc] device tensor, fp64 or (dtype=torch.float32) the fp64 result rounded to nearest even."""
        model = self._fitted()
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        s = self._upload(X, model["mean"].device if device is None else device)
        if int(s.shape[2]) != self._bands:
            raise ValueError(f"scene has {int(s.shape[2])} bands (shape {tuple(s.shape)}), this GWPCA was fitted on {self._bands}")
        if s.device != model["mean"].device:
            raise ValueError(f"scene is on {s.device}, this GWPCA was fitted on {model['mean'].device}")
        dev = s.device
        with torch.cuda.device(dev):
            out = torch.empty(int(s.shape[0]), int(s.shape[1]), self.nc, dtype=dtype, device=dev)
            p = self._params(s, model)
            _lib.check(_lib.load().hsimae_gwpca_apply(C.byref(p), out.data_ptr(), int(dtype == torch.float64),
                                                      torch.cuda.current_stream(dev).cuda_stream), "hsimae_gwpca_apply")
        return out

    def fit_transform(self, X, dtype=torch.float64, device=None):
        s = self._upload(X, device)
        return self.fit(s).transform(s, dtype=dtype)


def apply_gwpca(X, nc=32, group=4, whiten=True):
    """The reference's `applyGWPCA(X, nc=32, group=4, whiten=True)`: raw [H, W, bands] in, numpy fp64 [H, W, nc] out (host)."""
    return GWPCA(nc=nc, group=group, whiten=whiten).fit_transform(X).cpu().numpy()
