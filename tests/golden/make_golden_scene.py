#!/usr/bin/env python3
"""Golden fixture for whole-scene inference (hsimae_scene_windows) from the REFERENCE implementation.

Runs only in the build container (needs /root/reference).  Two seeded synthetic scenes are written to a temporary directory
and loaded by the reference's `Utils.Preprocessing.get_data_set_dual`, which pads the processed scene symmetrically and
cuts one 9 x 9 window per pixel (`data_cubes`); the windows are then taken through the reference's fine-tuning
`HSIdataset` (Model_Finetuning.py:26-63, eval mode), whose items are what `test_model` feeds the network.
  A: 10 x 7 pixels, 64 raw bands, GWPCA=True  -> fp64 scene of 32 bands
  B:  3 x 5 pixels,  8 bands fp32, GWPCA=False -> smaller than the 4-pixel pad
`get_data_set_dual` does not return the processed scene; it is recorded from the window centres, data_cubes[:, 4, 4].
Only arrays are recorded.  `Model_Finetuning` imports timm's CosineLRScheduler at module scope; timm is not in this image,
so an empty placeholder module is registered (nothing on the dataset path touches it).

    python tests/golden/make_golden_scene.py        ->  tests/golden/scene_windows.npz
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
if "timm" not in sys.modules:
    timm = types.ModuleType("timm")
    sched = types.ModuleType("timm.scheduler")
    sched.CosineLRScheduler = None
    timm.scheduler = sched
    sys.modules["timm"], sys.modules["timm.scheduler"] = timm, sched
with contextlib.redirect_stdout(io.StringIO()):
    import Model_Finetuning as MF  # noqa: E402
    from Utils.Preprocessing import get_data_set_dual  # noqa: E402


def one_scene(tmp, tag, raw, gt, gwpca):
    dp, gp = os.path.join(tmp, tag + "_data.npy"), os.path.join(tmp, tag + "_gt.npy")
    np.save(dp, raw)
    np.save(gp, gt)
    np.random.seed(0)                                   # get_data_set_dual's train / test split draws a permutation
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        _, _, _, data_cubes, _, gt_raw = get_data_set_dual(dp, gp, patch_size=9, num=1, GWPCA=gwpca)
    H, W = gt.shape
    scene = np.ascontiguousarray(data_cubes[:, 4, 4].reshape(H, W, -1))
    ds = MF.HSIdataset(data_cubes)
    items = np.stack([ds[i].numpy() for i in range(len(ds))])          # [H*W, 1, C, 9, 9] fp32
    print(tag, "data_cubes", data_cubes.shape, data_cubes.dtype, "items", items.shape)
    return {f"{tag}_scene": scene, f"{tag}_gt": np.asarray(gt_raw), f"{tag}_items": items}


def main():
    rng = np.random.default_rng(21)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        raw_a = rng.standard_normal((10, 7, 64))                        # fp64, as the reference's .npy scenes usually are
        gt_a = np.arange(70).reshape(10, 7) % 5                         # every class 0..4 present (get_data_set_dual asserts it)
        out.update(one_scene(tmp, "A", raw_a, gt_a, True))
        raw_b = rng.standard_normal((3, 5, 8)).astype(np.float32)
        gt_b = np.arange(15).reshape(3, 5) % 3
        out.update(one_scene(tmp, "B", raw_b, gt_b, False))
    assert out["A_scene"].dtype == np.float64 and out["A_scene"].shape == (10, 7, 32)
    assert out["B_scene"].dtype == np.float32 and out["B_scene"].shape == (3, 5, 8)
    path = os.path.join(HERE, "scene_windows.npz")
    np.savez_compressed(path, **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
