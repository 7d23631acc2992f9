"""Superpixel segmentation of a scene and object-level class maps: `Superpixels`, `SceneSegments`, `scene_segments`,
`segment_classification`.

The object-based spatial step of hyperspectral classification: segment the scene into superpixels with SLIC (Achanta et al.,
"SLIC Superpixels Compared to State-of-the-Art Superpixel Methods", TPAMI 2012; on a GPU gSLIC, Ren and Reid 2011), then let
every superpixel decide as a unit, by the mean of its pixels' class probabilities or by the majority of their labels.  Two entry
points of csrc/slic.hip do the work, hsimae_slic and hsimae_segment_vote.  The reference has no such step: every default leaves
it off.

The definition (restated in fp64 in tests/slic_ref.py).  Inputs: a guide pair as scene_guide / as_guide return it (guide fp32
[H, W, G], 1 <= G <= 4, and scale fp32 [G]), `size` S in 2 .. 32, `compactness` m > 0 in units of the guide's range, and
`max_iter` >= 0.
  Grid      ny = ceil(H / S), nx = ceil(W / S), K = ny nx centres, centre k = i nx + j.  The home cell of pixel (y, x) is
            (y ny // H, x nx // W).
  Start     centre (i, j) sits at pixel y = (2 i + 1) H // (2 ny), x = (2 j + 1) W // (2 nx) with that pixel's scaled guide
            value.  There is NO gradient perturbation of the seeds (SLIC moves each to the lowest gradient of a 3 x 3
            neighbourhood; this does not).
  Distance  d = sum_g (scale_g I_g(p) - c_g)^2 + w ((y - c_y)^2 + (x - c_x)^2) in fp32, w = fp32(m^2 / S^2) formed in fp64 and
            rounded once.
  Assign    a pixel compares only the centres of the 3 x 3 cells around its home cell (gSLIC's form; cells outside the grid are
            left out).  The smallest d wins, ties go to the lower centre index, a NaN distance loses to every number, and if
            all are NaN the home cell's centre wins.
  Update    a centre becomes the mean (G features, y, x) of the pixels assigned to it: fp64 sums, one ascending-x chain per
            scene row, then the row partials in ascending y; divided once, rounded to fp32 once.  A centre with no pixel keeps
            its bits.
  Fit       exactly max_iter rounds of assign and update, then one final assign; the label of a pixel is its centre's k.
CONNECTIVITY IS NOT ENFORCED: a segment may have stray fragments (SLIC's last step relabels them; voting does not need it).
Every label is one of the nine cells around its pixel's home cell, so all pixels of segment k lie in the 3 x 3 cells around
cell k: both kernels rest on that, and it is why segment_classification takes a SceneSegments and not an arbitrary label map.
size=8, compactness=0.1, max_iter=10 are not tuned here, and the effect on a real labelled scene is not measured.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .finetune import SceneClassification
from .scene_pass import to_host
from .smooth import EdgeFilter, _gpu, as_guide, edge_filter_of, scene_guide

MIN_SIZE, MAX_SIZE = 2, 32
MODES = {"mean": 0, "vote": 1}


class SceneSegments(collections.namedtuple("SceneSegments", ["labels", "centres", "counts", "grid", "size"])):
    """labels int32 [H, W] (the centre index k of every pixel), centres fp32 [K, G + 2] (G features, y, x), counts int32 [K]
    (the pixels that carry label k; 0 for an empty segment), all on the device; grid = (ny, nx), K = ny nx; size = S."""
    __slots__ = ()

    def check(self):
        """Host-side validation (for tests: it waits for the device): every label lies in the 3 x 3 cells around its pixel's home
        cell, and the counts are the counts of the labels.  -> self."""
        lab = self.labels.cpu().numpy().astype(np.int64)
        H, W = lab.shape
        ny, nx = self.grid
        if (ny, nx) != (-(-H // self.size), -(-W // self.size)) or tuple(self.centres.shape[:1]) != (ny * nx,):
            raise ValueError(f"grid {self.grid} does not belong to a {H} x {W} scene at size {self.size}")
        hi = (np.arange(H, dtype=np.int64) * ny // H)[:, None]
        hj = (np.arange(W, dtype=np.int64) * nx // W)[None, :]
        if lab.min() < 0 or lab.max() >= ny * nx or np.abs(lab // nx - hi).max() > 1 or np.abs(lab % nx - hj).max() > 1:
            raise ValueError("a label lies outside the 3 x 3 cells around its pixel's home cell")
        if not np.array_equal(np.bincount(lab.reshape(-1), minlength=ny * nx), self.counts.cpu().numpy()):
            raise ValueError("counts are not the counts of the labels")
        return self


class Superpixels:
    """SLIC superpixels of a guide image (the module docstring has the definition).  size: the grid interval S in pixels;
    compactness: m, in units of the guide's range (larger = more rigid, squarer segments); max_iter: rounds of assign + update.
    The defaults are not tuned here."""

    def __init__(self, size=8, compactness=0.1, max_iter=10):
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not MIN_SIZE <= size <= MAX_SIZE:
            raise ValueError(f"size must be an int in {MIN_SIZE} .. {MAX_SIZE}, got {size!r}")
        if isinstance(compactness, bool) or not isinstance(compactness, (int, float, np.integer, np.floating)) or \
                not math.isfinite(compactness) or compactness <= 0:
            raise ValueError(f"compactness must be a positive finite number, got {compactness!r}")
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
            raise ValueError(f"max_iter must be an int >= 0, got {max_iter!r}")
        with np.errstate(over="ignore"):
            if not math.isfinite(float(np.float32(float(compactness) ** 2 / int(size) ** 2))):
                raise ValueError(f"compactness={compactness!r} is too large: compactness^2 / size^2 is not a finite float32")
        self.size, self.compactness, self.max_iter = int(size), float(compactness), int(max_iter)

    @property
    def w(self) -> float:
        """fp32(compactness^2 / size^2), formed in fp64 and rounded once: what the kernel is given."""
        return float(np.float32(self.compactness ** 2 / self.size ** 2))

    def __repr__(self):
        return f"Superpixels(size={self.size}, compactness={self.compactness}, max_iter={self.max_iter})"

    def fit(self, guide, H=None, W=None) -> SceneSegments:
        """`guide`: scene_guide's (guide, scale) pair, or a bare fp32 [H, W, G] image (scaled here, as_guide); H, W: the scene
        size the guide must have, if given.  -> SceneSegments on the device.  max_iter + 2 launches on the current stream;
        nothing waits for the host."""
        g, scale = as_guide(guide)
        dev = _gpu(g.device)
        gh, gw, G = (int(v) for v in g.shape)
        if (H is not None and int(H) != gh) or (W is not None and int(W) != gw):
            raise ValueError(f"the guide is {gh} x {gw}, the scene {H} x {W}")
        if gh * gw >= 2 ** 31:
            raise ValueError(f"bad scene size {gh} x {gw}")
        ny, nx = -(-gh // self.size), -(-gw // self.size)
        K = ny * nx
        with torch.no_grad(), torch.cuda.device(dev):
            centres = torch.empty(K, 8, dtype=torch.float32, device=dev)
            tmp = torch.empty(K, 8, dtype=torch.float32, device=dev)
            counts = torch.empty(K, dtype=torch.int32, device=dev)
            labels = torch.empty(gh, gw, dtype=torch.int32, device=dev)
            p = _lib.SlicParams(guide=g.data_ptr(), guide_scale=scale.data_ptr(), G=G, H=gh, W=gw, size=self.size, w=self.w, init=1,
                                rounds=self.max_iter, centres=centres.data_ptr(), centres_tmp=tmp.data_ptr(),
                                counts=counts.data_ptr(), labels=labels.data_ptr(), dist=None)
            _lib.check(_lib.load().hsimae_slic(C.byref(p), torch.cuda.current_stream(dev).cuda_stream), "hsimae_slic")
        return SceneSegments(labels, centres[:, :G + 2], counts, (ny, nx), self.size)


def scene_segments(scene, size=8, compactness=0.1, max_iter=10, channels=3) -> SceneSegments:
    """Superpixels of a scene from its own first `channels` principal components: scene_guide(scene, channels), then
    Superpixels(size, compactness, max_iter).fit.  Everything on the device; nothing waits for the host."""
    return Superpixels(size, compactness, max_iter).fit(scene_guide(scene, channels))


def segment_vote(probs, segments, pixels=None, first=1, mode="mean", fill=False, return_probs=False):
    """One launch of hsimae_segment_vote.  `probs`: fp32 [n, num_class] on the device (columns below `first` are not classes),
    the probabilities of the pixels `pixels` (int64 row-major indices on the device, distinct; None: all H W pixels in order).
    -> SceneClassification on the device: labels int64 [H, W] / confidence / margin fp32 [H, W] = every classified pixel carries
    the label, value and lead of its segment's vector (mode "mean": the mean of its classified pixels' probabilities; "vote": the
    share of them whose own argmax is each class); fill=True writes them to the segment's unclassified pixels too; pixels of
    segments without a classified pixel, and without `fill` all unclassified ones, keep 0.  probs (return_probs=True): fp32
    [n, num_class], the segment vector of each input row.  Nothing waits for the host."""
    if mode not in MODES:
        raise ValueError(f'mode must be "mean" or "vote", got {mode!r}')
    if not isinstance(segments, SceneSegments):
        raise TypeError(f"segments must be a SceneSegments (Superpixels.fit, scene_segments), got {type(segments).__name__}")
    if not isinstance(probs, torch.Tensor) or not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 2:
        raise ValueError("probs must be a float32 [n, num_class] tensor on the GPU (no CPU fallback)")
    H, W = (int(v) for v in segments.labels.shape)
    n, nc = (int(v) for v in probs.shape)
    first = int(first)
    if nc < 2 or not 0 <= first < nc:
        raise ValueError(f"probs has {nc} columns and first={first}: at least two columns, first in [0, {nc})")
    dev = probs.device
    if segments.labels.device != dev:
        raise ValueError(f"the segments are on {segments.labels.device}, the probabilities on {dev}")
    probs, seg = probs.contiguous(), segments.labels.contiguous()
    K = segments.grid[0] * segments.grid[1]
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
        vec = torch.zeros(K, nc, dtype=torch.float32, device=dev) if return_probs else None
        p = _lib.SegmentVoteParams(probs=probs.data_ptr(), ldp=nc, n=n, C=nc, first=first, row_of=_lib.ptr(row_of),
                                   labels=seg.data_ptr(), H=H, W=W, size=segments.size, mode=MODES[mode], fill=int(bool(fill)),
                                   out_probs=_lib.ptr(vec), ldo=nc, seg_count=None, label_map=labels.data_ptr(),
                                   conf_map=conf.data_ptr(), margin_map=margin.data_ptr())
        _lib.check(_lib.load().hsimae_segment_vote(C.byref(p), torch.cuda.current_stream(dev).cuda_stream), "hsimae_segment_vote")
        out = None
        if return_probs:
            of_row = seg.view(-1) if pixels is None else seg.view(-1).index_select(0, pixels)
            out = vec.index_select(0, of_row.to(torch.int64))
    return SceneClassification(labels.view(H, W), conf.view(H, W), margin.view(H, W), out)


def segment_classification(result, segments, pixels=None, mode="mean", fill=False, return_probs=False, on_device=False):
    """A SceneClassification that carries its probabilities (classify_scene / knn_scene / probe_scene with return_probs=True)
    -> a new one decided superpixel by superpixel (segment_vote; class 0 is "unlabelled" as in those entry points).
    `segments`: Superpixels.fit's / scene_segments' SceneSegments of the same scene; `pixels`: the list the result was computed
    for (None: the whole scene); fill=True carries each segment's decision to its pixels outside `pixels` (object-based inference
    from a sparse set).  The input result is not modified; a result on the CPU is uploaded to the segments' device.
    -> on the CPU after one wait for the copies; on_device=True: everything stays on the device and nothing waits for the host."""
    if not isinstance(segments, SceneSegments):
        raise TypeError(f"segments must be a SceneSegments (Superpixels.fit, scene_segments), got {type(segments).__name__}")
    if getattr(result, "probs", None) is None:
        raise ValueError("this result carries no probabilities: classify the scene with return_probs=True")
    if tuple(result.labels.shape) != tuple(segments.labels.shape):
        raise ValueError(f"the result is {tuple(result.labels.shape)}, the segments {tuple(segments.labels.shape)}")
    dev = segments.labels.device
    if pixels is not None:
        pixels = torch.as_tensor(np.asarray(pixels) if not isinstance(pixels, torch.Tensor) else pixels)
        if pixels.dim() != 1 or pixels.dtype.is_floating_point or pixels.dtype == torch.bool:
            raise ValueError("pixels must be a 1-D array of integer pixel indices (r * W + c)")
        pixels = pixels.to(device=dev, dtype=torch.int64)
    out = segment_vote(result.probs.to(dev), segments, pixels=pixels, first=1, mode=mode, fill=fill, return_probs=return_probs)
    return SceneClassification(*to_host(list(out), on_device))


def spatial_step_of(smooth):
    """The `smooth` argument of the evaluation entry points: a Superpixels -> itself; None, True or an EdgeFilter -> what
    smooth.edge_filter_of makes of it; anything else raises TypeError."""
    if isinstance(smooth, Superpixels):
        return smooth
    if smooth is None or smooth is True or isinstance(smooth, EdgeFilter):
        return edge_filter_of(smooth)
    raise TypeError(f"smooth must be None, True, an EdgeFilter or a Superpixels, got {smooth!r}")


def spatial_labels(step, res, scene):
    """The label map of a whole-scene result (on the device, with its probabilities) after the spatial step: an EdgeFilter
    guided by the first principal component of the device-resident `scene`, or a Superpixels on scene_guide(scene, 3) deciding
    by the mean probabilities of each segment."""
    H, W = (int(v) for v in res.labels.shape)
    if isinstance(step, Superpixels):
        return segment_vote(res.probs, step.fit(scene_guide(scene, 3)), first=1, mode="mean").labels
    guide = None if step.sigma_r is None else scene_guide(scene)
    return step.apply(res.probs, H, W, guide, first=1).labels
