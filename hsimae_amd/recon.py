"""Masked reconstruction of a whole scene on the device (csrc/recon.hip): `reconstruct_scene`, `recon_eval_scene`.

A masked autoencoder's own evidence of quality, and it needs no labels: windows on a grid of scene pixels are masked and
reconstructed (hsimae_scene_batch -> hsimae_forward with want_recons), the reconstructed voxels are averaged back into the scene
(hsimae_recon_accumulate, one launch per chunk), and one hsimae_recon_finish gives the reconstructed cube, per-pixel RMSE and
spectral-angle maps and the sums behind MSE / PSNR / mean SAM, in the scene's units.  Only masked voxels are reconstructed: a
voxel that was visible in every window that held it keeps the scene's value and counts nowhere.
Nothing here waits for the host except the final copies (on_device=False).
"""
from __future__ import annotations

import collections
import ctypes as C
import random

import numpy as np
import torch

from . import _lib
from .checkpoint import load_matching
from .finetune import DualViT, scene_array
from .scene_pass import ScenePass, gpu_of, largest_chunk, to_host

SceneReconstruction = collections.namedtuple(
    "SceneReconstruction", ["recon", "count", "cover", "rmse", "sam", "loss", "mse", "psnr", "mean_sam", "coverage"])


def window_centres(length, stride):
    """Centres of the 9-wide windows along an axis of `length` pixels: min(4, length - 1), then every `stride`-th pixel while inside
    the axis, and the last pixel appended when the last window would not reach it.  Every pixel lies un-reflected in at least
    one window for 1 <= stride <= 9; with stride 9 the interior windows are scene_data.unlabeled_pixels' tiles."""
    length, stride = int(length), int(stride)
    if length < 1:
        raise ValueError(f"axis of length {length}")
    if not 1 <= stride <= 9:
        raise ValueError(f"stride between 1 and 9 is served, got {stride}")
    c = list(range(min(4, length - 1), length, stride))
    if c[-1] + 4 < length - 1:
        c.append(length - 1)
    return np.asarray(c, dtype=np.int32)


def _centres_on(dev, length, stride, count):
    """window_centres as an int32 device tensor, built there (no copy from the host, so nothing waits)."""
    c = torch.arange(min(4, length - 1), length, stride, dtype=torch.int32, device=dev)
    if c.numel() < count:
        c = torch.cat([c, torch.full((1,), length - 1, dtype=torch.int32, device=dev)])
    return c


def _recon_chunk(model, mask_ratio, batch_size, n_windows):
    """The largest n <= min(batch_size, n_windows) whose workspace fits DualViT.SCENE_WORKSPACE_BUDGET at every grid the pass may draw."""
    grids = model.grid_candidates(model.input_size[0], model.input_size[1] ** 2, mask_ratio)
    return largest_chunk(_lib.load(), model._config(), grids, batch_size, DualViT.SCENE_WORKSPACE_BUDGET, cap=n_windows)


def reconstruct_scene(model, scene, mask_ratio=0.75, stride=9, passes=1, generator=None, batch_size=4096, return_recon=True,
                      on_device=False):
    """Mask and reconstruct `scene` [H, W, C] (fp32 / fp64, numpy or tensor; checked as predict_scene checks it) with `model`, an
    HSIMAE or a DualViT / HSIViT that has its decoder.  Windows sit on the grid window_centres(H, stride) x window_centres(W,
    stride); every pass draws one token grid through model.get_dim_patches (python `random`, as forward does) and, per chunk of
    windows, the masking noise n1 = rand(n, T) then n2 = rand(n, 9) from `generator` (default: the device's), so that a seeded
    caller can replay a chunk with HSIMAE.forward(model, win, mask_ratio, noise=, grid=).  Runs without autograd and without
    DropPath; `model.want_recons` is forced on for the call.  The chunk is the largest n <= batch_size whose workspace fits
    DualViT.SCENE_WORKSPACE_BUDGET.
    -> SceneReconstruction(
         recon    fp32 [H, W, C]: the mean of a voxel's masked reconstructions, the scene's value where it was never masked
                  (None with return_recon=False),
         count    int32 [H, W, C]: how many reconstructions a voxel got,   cover int32 [H, W]: bands of the pixel with count > 0,
         rmse, sam fp32 [H, W]: over the pixel's reconstructed bands (0 where cover is 0; sam in radians),
         loss     the windows-weighted mean of the chunks' own masked loss (normalised pixels when the model was built so),
         mse, psnr, mean_sam, coverage: 0-d fp64: mean squared error over the reconstructed voxels, 10 log10(peak^2 / mse) with
                  peak = scene.max() - scene.min(), the mean angle over the pixels with cover > 0, reconstructed voxels / all).
    On the CPU after one wait for the copies; on_device=True: everything stays on the model's device and nothing waits."""
    passes = int(passes)
    if passes < 1:
        raise ValueError(f"passes must be >= 1, got {passes}")
    if not 0.0 <= float(mask_ratio) < 1.0:
        raise ValueError(f"mask_ratio must lie in [0, 1), got {mask_ratio}")
    if not getattr(model, "decoder_blocks", None):
        raise ValueError("reconstruct_scene needs a model with a decoder")
    s, H, W, Cb = scene_array(scene, model.patch_embed.bands, batch_size)
    rows, cols = window_centres(H, stride), window_centres(W, stride)
    dev = gpu_of(model)
    lib = _lib.load()
    T, L = model.input_size[0], model.input_size[1] ** 2
    nrows, ncols = len(rows), len(cols)
    n_win = nrows * ncols
    was = model.want_recons
    model.want_recons = True
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            rows_d, cols_d = _centres_on(dev, H, stride, nrows), _centres_on(dev, W, stride, ncols)
            items = (rows_d.to(torch.int64)[:, None] * W + cols_d.to(torch.int64)[None, :]).reshape(-1).contiguous()
            sp = ScenePass(model, s, items, _recon_chunk(model, mask_ratio, batch_size, n_win))
            s, stream = sp.scene, sp.stream
            acc = torch.zeros(H, W, Cb, dtype=torch.float32, device=dev)
            cnt = torch.zeros(H, W, Cb, dtype=torch.int32, device=dev)
            loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
            for _ in range(passes):
                grid = model.get_dim_patches(T, L, mask_ratio)
                for w0, n in sp.chunks():
                    win = sp.cut(w0, n)
                    n1 = torch.rand(n, T, device=dev, generator=generator)
                    n2 = torch.rand(n, L, device=dev, generator=generator)
                    loss, pred_img, mask_img, st = model._run_forward(win, mask_ratio, (n1, n2), grid, want_latent=False)
                    st.release()
                    ap = _lib.ReconAccumulateParams(pred_img=pred_img.data_ptr(), mask_img=mask_img.data_ptr(), n=n, w0=w0,
                                                    rows=rows_d.data_ptr(), nrows=nrows, cols=cols_d.data_ptr(), ncols=ncols,
                                                    H=H, W=W, C=Cb, sum=acc.data_ptr(), cnt=cnt.data_ptr())
                    _lib.check(lib.hsimae_recon_accumulate(C.byref(ap), stream), "hsimae_recon_accumulate")
                    loss_sum += loss.double() * n
            recon = torch.empty(H, W, Cb, dtype=torch.float32, device=dev) if return_recon else None
            cover = torch.empty(H, W, dtype=torch.int32, device=dev)
            rmse = torch.empty(H, W, dtype=torch.float32, device=dev)
            sam = torch.empty(H, W, dtype=torch.float32, device=dev)
            partials = torch.empty(4 * _lib.RECON_GRID, dtype=torch.float64, device=dev)
            stats = torch.empty(4, dtype=torch.float64, device=dev)
            fp = _lib.ReconFinishParams(scene=s.data_ptr(), scene_f64=int(s.dtype == torch.float64), H=H, W=W, C=Cb,
                                        sum=acc.data_ptr(), cnt=cnt.data_ptr(), recon=_lib.ptr(recon), cover=cover.data_ptr(),
                                        rmse=rmse.data_ptr(), sam=sam.data_ptr(), partials=partials.data_ptr(),
                                        stats=stats.data_ptr())
            _lib.check(lib.hsimae_recon_finish(C.byref(fp), stream), "hsimae_recon_finish")
            out = to_host([recon, cnt, cover, rmse, sam, (loss_sum / (passes * n_win)).float()] + scene_scalars(stats, s, H * W * Cb),
                          on_device)
    finally:
        model.want_recons = was
    return SceneReconstruction(*out)


def scene_scalars(stats, scene, n_voxels):
    """[mse, psnr, mean_sam, coverage] as 0-d fp64 tensors on stats' device, from hsimae_recon_finish's stats = (sum of squared
    errors, reconstructed voxels, sum of angles, pixels with a reconstructed band) and the scene's own range."""
    peak = (scene.max() - scene.min()).double()
    mse = stats[0] / stats[1]
    return [mse, 10.0 * torch.log10(peak * peak / mse), stats[2] / stats[3], stats[1] / float(n_voxels)]


def recon_eval_scene(scene, pretrained, depth=12, dim=64, s_depth=6, dec_depth=2, dec_dim=48, mask_ratio=0.75, stride=9, passes=1,
                     seed=0, device="cuda:0", batch_size=4096):
    """The label-free evaluation of a checkpoint: reconstruct_scene of `scene` [H, W, C] with the model built from these widths
    (mask_pretraining's defaults) and the state dict at `pretrained` loaded key-filtered, as knn_eval_scene loads it: a
    pretraining checkpoint (HSIMAE) and a fine-tuned one (DualViT, whose head is dropped) both work.  `seed` seeds python
    `random` (the token grids) and a generator on the device (the masking noise).  -> SceneReconstruction on the CPU."""
    from .model import HSIMAE
    device = torch.device(device)
    if len(scene.shape) != 3:
        raise ValueError(f"scene must be [H, W, C], got shape {tuple(scene.shape)}")
    model = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=int(scene.shape[2]), b_patch_size=8, embed_dim=dim, depth=depth,
                   num_heads=dim // 16, s_depth=s_depth, decoder_embed_dim=dec_dim, decoder_depth=dec_depth,
                   decoder_num_heads=dec_dim // 8, norm_pix_loss=True, trunc_init=True).to(device)
    load_matching(model, pretrained, device, match_shapes=True)
    random.seed(seed)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    return reconstruct_scene(model, scene, mask_ratio=mask_ratio, stride=stride, passes=passes, generator=gen,
                             batch_size=batch_size)
