"""Whole-scene classification throughput: the existing flow (host windowing as Utils/Preprocessing.py:208-213 does it, then
test_model's HSIdataset upload + batch-256 loop) against DualViT.predict_scene at its default chunk, on a seeded synthetic
Pavia-sized scene (610 x 340 x 32 fp64) with HSIViT Base (128 / 12 / 9) and Large (256 / 12 / 9) as in
Model_Finetuning.py:__main__.  Both legs run in one process, alternating, each warmed up first.

Reports per model: pixels/s of each leg (the existing one with and without the host windowing), peak device memory of each
leg, the host windowing time, and the number of pixels whose labels differ between the two flows.  One JSON line per model.

    python scripts/scene_throughput.py [--models base,large] [--reps 3] [--out FILE]
    python scripts/scene_throughput.py --profile     # predict_scene only (Base): run under rocprofv3 --kernel-trace --stats
    python scripts/scene_throughput.py --views flips # predict_scene against classify_scene with one view and with these views
                                                     # (a comma list of flip codes, or "flips"); with --profile: classify_scene
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hsimae_amd import HSIViT  # noqa: E402
from hsimae_amd.data import DeviceLoader  # noqa: E402
from hsimae_amd.finetune_train import HSIdataset  # noqa: E402

MODELS = {"base": (128, 8), "large": (256, 16)}      # embed_dim, heads; depth 12, s_depth 9
H, W, BANDS, CLASSES = 610, 340, 32, 10              # Pavia University after GWPCA; 9 classes + "unlabelled"


def make_model(name):
    dim, heads = MODELS[name]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIViT(img_size=9, patch_size=3, in_chans=1, bands=BANDS, b_patch_size=8, num_class=CLASSES, embed_dim=dim, depth=12,
                   num_heads=heads, s_depth=9, trunc_init=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                             # a head that separates classes (the init's is ~0)
        m.cls_head.weight.copy_(0.05 * torch.randn(m.cls_head.weight.shape, generator=g))
    return m.cuda().eval()


def host_windows(scene):
    """get_data_set_dual's windowing: np.pad 'symmetric' by 4, one 9 x 9 x C slice per pixel, np.array of the list."""
    pad = np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")
    return np.array([pad[r:r + 9, c:c + 9] for r in range(scene.shape[0]) for c in range(scene.shape[1])])


def existing_flow(model, data_cubes):
    """test_model's body (Model_Finetuning.py:268-283): cubes uploaded, batches of 256, 1 + argmax(logits[:, 1:])."""
    ds = HSIdataset(data_cubes, device="cuda")
    preds = []
    with torch.no_grad():
        for x in DeviceLoader(ds, batch_size=256, shuffle=False):
            preds.append(model(x)[:, 1:].argmax(1))
    return (torch.cat(preds).cpu().numpy() + 1).reshape(H, W)


def new_flow(model, scene):
    return model.predict_scene(scene).numpy()


def parse_views(text):
    return "flips" if text == "flips" else tuple(int(v) for v in text.split(","))


def views_flow(models, scene, views, reps, out):
    """predict_scene, classify_scene(views=(0,)) and classify_scene(views) in one process, alternating, each warmed up first."""
    rows = []
    for name in models:
        m = make_model(name)
        legs = {"predict_scene": lambda: m.predict_scene(scene).numpy(),
                "classify_one_view": lambda: m.classify_scene(scene).labels.numpy(),
                "classify_views": lambda: m.classify_scene(scene, views=views).labels.numpy()}
        secs = {k: [] for k in legs}
        first = {}
        for k, fn in legs.items():
            release(m)
            first[k] = fn()
        for _ in range(reps):
            for k, fn in legs.items():
                release(m)
                pred, s, _ = timed(fn)
                secs[k].append(s)
                assert np.array_equal(pred, first[k]), f"{k}: labels changed between runs"
        row = {"model": name, "scene": [H, W, BANDS], "pixels": H * W, "reps": reps, "views": views, "chunk": m._scene_chunk(8192),
               "one_view_labels_differ": int((first["predict_scene"] != first["classify_one_view"]).sum()),
               "views_labels_differ": int((first["predict_scene"] != first["classify_views"]).sum())}
        for k in legs:
            row[k + "_s"] = [round(v, 4) for v in secs[k]]
            row[k + "_px_per_s"] = round(H * W / float(np.median(secs[k])))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del m
        torch.cuda.empty_cache()
    if out:
        with open(out, "w") as fh:
            json.dump(rows, fh, indent=1)


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, torch.cuda.max_memory_allocated()


def release(model):
    model._pool.free.clear()                         # workspace arenas kept by the model between calls
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="base,large")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--views", default=None)
    a = ap.parse_args()
    scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
    if a.profile:
        m = make_model("base")
        views = None if a.views is None else parse_views(a.views)
        for _ in range(2):
            new_flow(m, scene) if views is None else m.classify_scene(scene, views=views)
            torch.cuda.synchronize()
        print(f"profiled {'predict_scene' if views is None else f'classify_scene(views={views})'} (base) x2")
        return
    if a.views is not None:
        views_flow(a.models.split(","), scene, parse_views(a.views), a.reps, a.out)
        return
    t0 = time.perf_counter()
    data_cubes = host_windows(scene)
    t_win = time.perf_counter() - t0
    rows = []
    for name in a.models.split(","):
        m = make_model(name)
        legs = {"existing": lambda: existing_flow(m, data_cubes), "new": lambda: new_flow(m, scene)}
        res = {k: {"s": [], "peak": 0, "pred": None} for k in legs}
        for k, fn in legs.items():                  # warm-up: code objects, arenas, packed weights
            release(m)
            res[k]["pred"] = fn()
        for _ in range(a.reps):
            for k, fn in legs.items():
                release(m)
                pred, s, peak = timed(fn)
                res[k]["s"].append(s)
                res[k]["peak"] = max(res[k]["peak"], peak)
                assert np.array_equal(pred, res[k]["pred"]), f"{k}: labels changed between runs"
        t_old, t_new = np.median(res["existing"]["s"]), np.median(res["new"]["s"])
        row = {"model": name, "scene": [H, W, BANDS], "pixels": H * W, "reps": a.reps,
               "existing_s": [round(v, 4) for v in res["existing"]["s"]], "new_s": [round(v, 4) for v in res["new"]["s"]],
               "existing_px_per_s": round(H * W / t_old), "existing_with_windowing_px_per_s": round(H * W / (t_old + t_win)),
               "new_px_per_s": round(H * W / t_new), "speedup": round(t_old / t_new, 2),
               "speedup_with_windowing": round((t_old + t_win) / t_new, 2), "host_windowing_s": round(t_win, 3),
               "existing_peak_mib": round(res["existing"]["peak"] / 2**20), "new_peak_mib": round(res["new"]["peak"] / 2**20),
               "new_chunk": m._scene_chunk(8192),
               "labels_differ": int((res["existing"]["pred"] != res["new"]["pred"]).sum())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del m
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
