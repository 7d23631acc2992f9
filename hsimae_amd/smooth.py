"""Edge-preserving smoothing of a scene's class-probability maps before the argmax: `EdgeFilter`, `scene_guide`,
`smooth_classification`.

Every whole-scene classifier here decides each pixel alone (classify_scene, knn_scene, probe_scene).  The hyperspectral
literature's standard repair of the salt-and-pepper maps this gives is EPF (Kang, Li and Benediktsson, "Spectral-Spatial
Hyperspectral Image Classification With Edge-Preserving Filtering", IEEE TGRS 2014): every class's probability map is filtered
with an edge-preserving filter whose guide image is taken from the scene (its first principal components), and the label is
the argmax of the filtered probabilities.  This is its joint-bilateral form; one launch of hsimae_prob_filter (csrc/smooth.hip)
filters all class planes and writes the label, confidence and margin maps.  The reference has no such step: every default
leaves it off.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .finetune import SceneClassification
from .gwpca import GWPCA, MAX_GROUP_WIDTH
from .scene_pass import as_scene, to_host

MAX_RADIUS = 8
MAX_GUIDE = 4
LOG2E = math.log2(math.e)


def _gpu(device):
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("hsimae_amd runs on MI355X only (no CPU fallback): the probability filter needs a GPU")
    return torch.device(device)


def guide_scale(guide: torch.Tensor) -> torch.Tensor:
    """fp32 [G] on the guide's device: 1 / (max - min) of every channel of a [H, W, G] guide, 0 for a constant channel.  One
    device-side min / max; nothing waits for the host."""
    flat = guide.reshape(-1, guide.shape[-1])
    span = flat.amax(0) - flat.amin(0)
    return torch.where(span > 0, 1.0 / span, torch.zeros_like(span)).to(torch.float32).contiguous()


def as_guide(guide, device=None):
    """An explicit guide image, any fp32 [H, W, G] array with 1 <= G <= 4 (chosen bands, an index map, ..) -> (guide fp32
    [H, W, G], scale fp32 [G]) on the device, scaled as scene_guide scales its own.  A (guide, scale) pair passes through."""
    if isinstance(guide, tuple):
        g, scale = guide
        if not (isinstance(g, torch.Tensor) and isinstance(scale, torch.Tensor) and g.is_cuda and scale.device == g.device and
                g.dtype == scale.dtype == torch.float32 and g.dim() == 3 and tuple(scale.shape) == (g.shape[2],)):
            raise ValueError("a guide pair must be (fp32 [H, W, G], fp32 [G]) tensors on one GPU, as scene_guide returns them")
        if not 1 <= g.shape[2] <= MAX_GUIDE:
            raise ValueError(f"a guide has 1 to {MAX_GUIDE} channels, got {g.shape[2]}")
        return g.contiguous(), scale.contiguous()
    g = as_scene(guide)
    if g.dtype != torch.float32:
        raise ValueError(f"an explicit guide must be float32, got {g.dtype}")
    if not 1 <= g.shape[2] <= MAX_GUIDE:
        raise ValueError(f"a guide has 1 to {MAX_GUIDE} channels, got shape {tuple(g.shape)}")
    g = g.to(g.device if g.is_cuda and device is None else _gpu(device)).contiguous()
    return g, guide_scale(g)


def scene_guide(scene, channels=1, device=None):
    """The guide image EPF takes from the scene itself: its first `channels` principal components (GWPCA(nc=channels, group=1,
    whiten=False), fp64 on the device, rounded to fp32) -> (guide fp32 [H, W, channels], scale fp32 [channels]), both on the
    device; scale = 1 / (max - min) per channel, so that sigma_r is in units of the guide's range.  Nothing waits for the host."""
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or not 1 <= channels <= MAX_GUIDE:
        raise ValueError(f"channels must be an int in 1 .. {MAX_GUIDE}, got {channels!r}")
    s = as_scene(scene)
    if s.shape[2] > MAX_GROUP_WIDTH:
        raise ValueError(f"scene shape {tuple(s.shape)}: the principal components of more than {MAX_GROUP_WIDTH} bands are not "
                         "served here; pass an explicit guide instead (as_guide: chosen bands, or components computed elsewhere)")
    g = GWPCA(nc=int(channels), group=1, whiten=False).fit_transform(s, dtype=torch.float32, device=device)
    return g, guide_scale(g)


class EdgeFilter:
    """The joint bilateral filter of EPF over the class-probability maps of a scene.  A tap at offset (dy, dx) of a pixel weighs
    exp(-(dy^2 + dx^2) / (2 sigma_s^2)) * exp(-|I_j - I_i|^2 / (2 sigma_r^2)) with I the guide scaled to [0, 1] per channel;
    taps outside the scene or at pixels that were not classified are left out (no reflection).  radius=3, sigma_s=3.0,
    sigma_r=0.2 are Kang et al.'s EPF-B settings; they are not tuned here.  sigma_r=None switches the range term off: a plain
    Gaussian smoothing, which needs no guide."""

    def __init__(self, radius=3, sigma_s=3.0, sigma_r=0.2):
        if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
            raise ValueError(f"radius must be an int in 1 .. {MAX_RADIUS}, got {radius!r}")
        for name, v in (("sigma_s", sigma_s), ("sigma_r", sigma_r)):
            if v is None and name == "sigma_r":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v <= 0:
                raise ValueError(f"{name} must be a positive finite number{' or None' if name == 'sigma_r' else ''}, got {v!r}")
            with np.errstate(over="ignore"):
                a = float(np.float32(LOG2E / (2.0 * float(v) ** 2)))
            if not math.isfinite(a):
                raise ValueError(f"{name}={v!r} is too small: log2(e) / (2 {name}^2) is not a finite float32")
        self.radius, self.sigma_s, self.sigma_r = int(radius), float(sigma_s), None if sigma_r is None else float(sigma_r)

    @property
    def a_s(self) -> float:
        """fp32(log2 e / (2 sigma_s^2)), formed in fp64 and rounded once: what the kernel is given."""
        return float(np.float32(LOG2E / (2.0 * self.sigma_s ** 2)))

    @property
    def a_r(self) -> float:
        """fp32(log2 e / (2 sigma_r^2)); 0 without the range term."""
        return 0.0 if self.sigma_r is None else float(np.float32(LOG2E / (2.0 * self.sigma_r ** 2)))

    def __repr__(self):
        return f"EdgeFilter(radius={self.radius}, sigma_s={self.sigma_s}, sigma_r={self.sigma_r})"

    def apply(self, probs, H, W, guide, pixels=None, first=1, return_probs=False):
        """Filter `probs`, fp32 [n, num_class] on the device (the columns below `first` are not classes: they are never read and
        come out 0), the probabilities of the pixels `pixels` (int64 row-major indices on the device, distinct; None: all H * W
        pixels in order) of an H x W scene.  `guide`: scene_guide's (guide, scale) pair, or a bare fp32 [H, W, G] device tensor
        (scaled here, as_guide); None is allowed with sigma_r=None.
        -> SceneClassification(labels int64 [H, W], confidence fp32 [H, W], margin fp32 [H, W], probs fp32 [n, num_class] in the
        input's row order with return_probs=True, else None), all on the device: label = argmax of the filtered probabilities,
        confidence = its value, margin = its lead over the runner-up; pixels that are not in `pixels` keep 0.  One device-side
        scatter (with `pixels`), one launch on the current stream; nothing waits for the host."""
        if not isinstance(probs, torch.Tensor) or not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 2:
            raise ValueError("probs must be a float32 [n, num_class] tensor on the GPU (no CPU fallback)")
        H, W, first = int(H), int(W), int(first)
        n, nc = (int(v) for v in probs.shape)
        if H <= 0 or W <= 0 or H * W >= 2 ** 31:
            raise ValueError(f"bad scene size {H} x {W}")
        if nc < 2 or not 0 <= first < nc:
            raise ValueError(f"probs has {nc} columns and first={first}: at least two columns, first in [0, {nc})")
        dev = probs.device
        probs = probs.contiguous()
        if self.sigma_r is None and guide is None:
            g = scale = None
        else:
            if guide is None:
                raise ValueError("a filter with a range term (sigma_r) needs a guide: scene_guide(scene), or an explicit fp32 [H, W, G] image")
            g, scale = as_guide(guide, dev)
            if tuple(g.shape[:2]) != (H, W) or g.device != dev:
                raise ValueError(f"the guide is {tuple(g.shape)} on {g.device}, the scene {H} x {W} on {dev}")
        with torch.no_grad(), torch.cuda.device(dev):
            if pixels is None:
                if n != H * W:
                    raise ValueError(f"{n} rows of probabilities for {H * W} pixels: pass the `pixels` they belong to")
                row_of = None
            else:
                if not isinstance(pixels, torch.Tensor) or pixels.dtype != torch.int64 or pixels.dim() != 1 or pixels.device != dev:
                    raise ValueError("pixels must be a 1-D int64 tensor of row-major pixel indices on the probabilities' device")
                if pixels.numel() != n:
                    raise ValueError(f"{pixels.numel()} pixels for {n} rows of probabilities")
                row_of = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
                row_of[pixels] = torch.arange(n, dtype=torch.int32, device=dev)
            labels = torch.zeros(H * W, dtype=torch.int64, device=dev)
            conf = torch.zeros(H * W, dtype=torch.float32, device=dev)
            margin = torch.zeros(H * W, dtype=torch.float32, device=dev)
            out = torch.zeros(n, nc, dtype=torch.float32, device=dev) if return_probs else None
            p = _lib.ProbFilterParams(probs=probs.data_ptr(), ldp=nc, n=n, C=nc, first=first, H=H, W=W, row_of=_lib.ptr(row_of),
                                      guide=_lib.ptr(g), G=1 if g is None else int(g.shape[2]), guide_scale=_lib.ptr(scale),
                                      radius=self.radius, a_s=self.a_s, a_r=self.a_r if g is not None else 0.0,
                                      out_probs=_lib.ptr(out), ldo=nc, label_map=labels.data_ptr(), conf_map=conf.data_ptr(),
                                      margin_map=margin.data_ptr())
            _lib.check(_lib.load().hsimae_prob_filter(C.byref(p), torch.cuda.current_stream(dev).cuda_stream), "hsimae_prob_filter")
        return SceneClassification(labels.view(H, W), conf.view(H, W), margin.view(H, W), out)


def edge_filter_of(smooth):
    """The `smooth` argument of the evaluation entry points: None -> None, True -> the default EdgeFilter, an EdgeFilter -> itself."""
    if smooth is None or isinstance(smooth, EdgeFilter):
        return smooth
    if smooth is True:
        return EdgeFilter()
    raise TypeError(f"smooth must be None, True or an EdgeFilter, got {smooth!r}")


def smooth_classification(result, guide, pixels=None, filt=None, return_probs=False, on_device=False):
    """A SceneClassification that carries its probabilities (classify_scene / knn_scene / probe_scene with return_probs=True)
    -> a new one from the filtered probabilities (EdgeFilter.apply; class 0 is "unlabelled" as in those entry points).
    `guide`: scene_guide(scene)'s pair or an explicit fp32 [H, W, G] image (None with a filter without range term); `pixels`: the
    list the result was computed for (None: the whole scene); `filt`: an EdgeFilter, None = EdgeFilter().  The input result is
    not modified.  A result on the CPU is uploaded to the guide's device (the current one without a guide).
    -> on the CPU after one wait for the copies; on_device=True: everything stays on the device and nothing waits for the host."""
    filt = EdgeFilter() if filt is None else filt
    if not isinstance(filt, EdgeFilter):
        raise TypeError(f"filt must be an EdgeFilter, got {type(filt).__name__}")
    if getattr(result, "probs", None) is None:
        raise ValueError("this result carries no probabilities: classify the scene with return_probs=True")
    H, W = (int(v) for v in result.labels.shape)
    probs = result.probs
    if probs.is_cuda:
        dev = probs.device
    elif isinstance(guide, tuple) and isinstance(guide[0], torch.Tensor) and guide[0].is_cuda:
        dev = guide[0].device
    elif isinstance(guide, torch.Tensor) and guide.is_cuda:
        dev = guide.device
    else:
        dev = _gpu(None)
    if pixels is not None:
        pixels = torch.as_tensor(np.asarray(pixels) if not isinstance(pixels, torch.Tensor) else pixels)
        if pixels.dim() != 1 or pixels.dtype.is_floating_point or pixels.dtype == torch.bool:
            raise ValueError("pixels must be a 1-D array of integer pixel indices (r * W + c)")
        pixels = pixels.to(device=dev, dtype=torch.int64)
    out = filt.apply(probs.to(dev), H, W, guide, pixels=pixels, first=1, return_probs=return_probs)
    return SceneClassification(*to_host(list(out), on_device))
