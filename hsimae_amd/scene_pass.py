"""What the whole-scene entry points share (DualViT.predict_scene / classify_scene / scene_features / knn_scene / cluster_scene,
recon.reconstruct_scene, scene_data.SceneCubes): the checks of a scene and of a pixel list, the chunk that fits the workspace
budget, and `ScenePass`.  An entry point adds the outputs it allocates and the kernels that follow the encoder.
Imports only _lib, numpy and torch: finetune.py, recon.py and scene_data.py all import it.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

PATCH = 9


def as_scene(scene) -> torch.Tensor:
    """A numpy array or tensor as the [H, W, C] fp32 / fp64 tensor it must be (a tensor keeps its storage)."""
    if isinstance(scene, torch.Tensor):
        s = scene.detach()
    else:
        s = torch.from_numpy(np.ascontiguousarray(np.asarray(scene)))
    if s.dim() != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(s.shape)}")
    if s.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"scene must be float32 or float64, got {s.dtype}")
    if min(s.shape) <= 0:
        raise ValueError(f"empty scene {tuple(s.shape)}")
    return s


def pixel_indices(p, n_pixels, what="pixels", allow_empty=True) -> torch.Tensor:
    """Row-major pixel indices r * W + c of a scene of `n_pixels` pixels, checked on the host -> contiguous int64 CPU tensor."""
    if isinstance(p, (list, tuple)) and not p:
        p = torch.empty(0, dtype=torch.int64)             # (an empty list has no dtype: torch would call it float)
    p = torch.as_tensor(p).detach().cpu()
    if p.dim() != 1 or p.dtype.is_floating_point or p.dtype == torch.bool or not (allow_empty or p.numel()):
        raise ValueError(f"{what} must be a {'' if allow_empty else 'non-empty '}1-D array of integer pixel indices (r * W + c)")
    p = p.to(torch.int64).contiguous()
    if p.numel() and (int(p.min()) < 0 or int(p.max()) >= n_pixels):
        raise ValueError(f"{what}: pixel index out of range [0, {n_pixels}): min {int(p.min())}, max {int(p.max())}")
    return p


def largest_chunk(lib, cfg, grids, batch_size, budget, cap=None) -> int:
    """The largest n <= min(batch_size, cap) whose hsimae_workspace_bytes(cfg, n, len_t, len_l) lies in [0, budget] for every
    token grid (len_t, len_l) of `grids`; never less than 1."""
    best = max(1, int(batch_size) if cap is None else min(int(batch_size), int(cap)))
    for len_t, len_l in grids:
        lo, hi = 1, best
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if 0 <= lib.hsimae_workspace_bytes(C.byref(cfg), mid, len_t, len_l) <= budget:
                lo = mid
            else:
                hi = mid - 1
        best = lo
    return best


def gpu_of(model) -> torch.device:
    """The device of the model's parameters; the last of an entry point's checks."""
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("hsimae_amd runs on MI355X only (no CPU fallback): move the model to a GPU")
    return dev


def to_host(out, on_device):
    """An entry point's results (a list; None entries stay None): as they are with on_device, else copied to the CPU."""
    return out if on_device else [None if t is None else t.cpu() for t in out]


def window_buffer(n, bands, dev) -> torch.Tensor:
    """The encoder's input of n windows, band-fastest as the reference's HSIdataset yields it: [n, 9, 9, C] viewed [n, 1, C, 9, 9]."""
    return torch.empty(n, PATCH, PATCH, bands, dtype=torch.float32, device=dev).permute(0, 3, 1, 2).unsqueeze(1)


def _window_fields(scene, out):
    """The fields hsimae_scene_windows' and hsimae_scene_batch's params share: the scene and the strides of the window buffer."""
    H, W, Cb = (int(v) for v in scene.shape)
    return dict(scene=scene.data_ptr(), scene_f64=int(scene.dtype == torch.float64), H=H, W=W, C=Cb, out=out.data_ptr(),
                sn=out.stride(0), sb=out.stride(2), sh=out.stride(3), sw=out.stride(4))


def batch_params(scene, out, items, n, n_items, bad, flips=None, pixels=None, labels=None, y=None) -> _lib.SceneBatchParams:
    """hsimae_scene_batch's params: the windows of `n` items at the device address `items` (int64) into `out`; the tables
    (`pixels`, `labels` -> `y`) are SceneCubes', without them an item is a pixel index below `n_items`."""
    return _lib.SceneBatchParams(items=items, N=n, n_items=n_items, pixels=_lib.ptr(pixels), labels=_lib.ptr(labels),
                                 flips=_lib.ptr(flips), y=_lib.ptr(y), bad=bad.data_ptr(), **_window_fields(scene, out))


class ScenePass:
    """One pass over `items` (device int64 pixel indices; None: every pixel, by its p0) of the checked `scene`, at most `chunk` per
    step.  Holds the contiguous device scene (a contiguous device tensor is used as it is), H, W, C, the window buffer `win`, the
    current stream, the `bad` flag and, from the first encode(), the identity noise."""

    def __init__(self, model, scene, items, chunk):
        self.model, self.dev = model, gpu_of(model)
        self.scene = scene.to(self.dev).contiguous()
        self.H, self.W, self.C = (int(v) for v in scene.shape)
        self.items = None if items is None else items.to(self.dev)
        self.n_total = self.H * self.W if items is None else int(items.numel())
        self.chunk = max(1, min(int(chunk), self.n_total))
        self.T, self.L = model.input_size[0], model.input_size[1] ** 2
        self.win = window_buffer(self.chunk, self.C, self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        # int32 [1], set by hsimae_scene_batch when an item was outside the scene (a pass by p0 never cuts with it)
        self.bad = None if items is None else torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._noise = None                                # the identity noise, made by the first encode()

    def chunks(self, start=0, stop=None):
        """(k0, n) of every step over the items start .. stop (default: all); the last may be short."""
        stop = self.n_total if stop is None else stop
        for k0 in range(start, stop, self.chunk):
            yield k0, min(self.chunk, stop - k0)

    def window_params(self, k0, n) -> _lib.SceneParams:
        """What hsimae_scene_windows and hsimae_class_argmax take for the items k0 .. k0 + n: a range from p0, or the index list."""
        by_p0 = self.items is None
        return _lib.SceneParams(p0=k0 if by_p0 else 0, pixels=None if by_p0 else self.items.data_ptr() + 8 * k0, N=n,
                                **_window_fields(self.scene, self.win))

    def cut(self, k0, n, flips=None):
        """hsimae_scene_batch: the windows of the items k0 .. k0 + n, flipped by `flips` (uint8 per window) -> win[:n]."""
        bp = batch_params(self.scene, self.win, self.items.data_ptr() + 8 * k0, n, self.H * self.W, self.bad, flips)
        _lib.check(_lib.load().hsimae_scene_batch(C.byref(bp), self.stream), "hsimae_scene_batch")
        return self.win[:n]

    def encode(self, n):
        """The unmasked encoder on win[:n] (increasing noise keeps every token in its place) -> the state; the caller releases it."""
        if self._noise is None:
            self._noise = tuple(torch.arange(k, dtype=torch.float32, device=self.dev).expand(self.chunk, k).contiguous()
                                for k in (self.T, self.L))
        n1, n2 = self._noise
        return self.model._run_forward(self.win[:n], 0.0, (n1[:n], n2[:n]), (self.T, self.L), want_latent=True, encoder_only=True)[3]

    def pooled_into(self, out, n):
        """encode, and the AGG pooling written into `out` (fp32 [n, T * D], contiguous rows).  The head GEMM is not run."""
        st = self.encode(n)
        lat = st["latent"].contiguous()
        _lib.check(_lib.load().hsimae_agg_pool(lat.data_ptr(), out.data_ptr(), n, self.T, self.L, self.model.dim, self.stream),
                   "hsimae_agg_pool")
        st.release()
