"""Group-wise PCA throughput: GWPCA.fit_transform on the device against the fp64 restatement (tests/gwpca_ref.py) on the host's
CPUs, on a seeded synthetic Pavia-sized raw scene (610 x 340 x 103 fp64) and on a batch of 128 x 128 x 224 scenes (HySpecNet
tiles).  The scene is resident on the device for the kernel timings: HIP events around fit_transform (fit + transform: three
reads of the scene and one write of the output), warm-up first, then the median of --reps repetitions.

Reports per workload, one JSON line: ms per scene (median, min, max); the bytes the kernels must move (3 reads + 1 write) and
the rate that is as a share of the 4.9 TB/s that plain streaming kernels with three read and one write stream reach on this
chip (scripts/micro/hbm_mix.hip); the share of the time that does not scale with the pixel count (the eigen-solve and the two fixed-order
slab combines, all latency-bound; estimated from the event time of a fit on a scene cut to 1/16 of the pixels, whose streaming
part is 16 x smaller; the split between the three is read from the --profile run); the same call's wall
time including the upload from the host array; and the restatement's wall time on the host.

    python scripts/gwpca_throughput.py [--reps 20] [--batch 8] [--out FILE]
    python scripts/gwpca_throughput.py --profile     # predict_scene fed by fit_transform: run under rocprofv3 --kernel-trace --stats
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gwpca_ref as R  # noqa: E402
from hsimae_amd import GWPCA, HSIViT  # noqa: E402

STREAM_TBS = 4.9          # plain kernels, three read + one write stream (profiles/r04_hbm_mix.txt)


def events(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def workload(name, scenes, reps):
    H, W, Cb = scenes[0].shape
    dev = [torch.from_numpy(s).cuda() for s in scenes]
    pca = GWPCA()
    per = len(scenes)
    ms_all = [v / per for v in events(lambda: [pca.fit_transform(d) for d in dev], reps)]
    ms_fit = [v / per for v in events(lambda: [pca.fit(d) for d in dev], reps)]
    small = [d[: max(2, H // 16)].contiguous() for d in dev]
    ms_fit_small = [v / per for v in events(lambda: [pca.fit(d) for d in small], reps)]
    ms_tr = [v / per for v in events(lambda: [pca.transform(d) for d in dev], reps)]
    # fit = stream(n) + fixed, fit_small = stream(n / 16) + fixed  ->  fixed = (16 fit_small - fit) / 15
    eig = max(0.0, (16 * np.median(ms_fit_small) - np.median(ms_fit)) / 15)
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [pca.fit_transform(s) for s in scenes]
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / per)
    del outs
    t0 = time.perf_counter()
    R.gwpca_ref(scenes[0])
    t_host = time.perf_counter() - t0
    nbytes = 3 * H * W * Cb * 8 + H * W * 32 * 8
    med = float(np.median(ms_all))
    row = {"workload": name, "scene": [H, W, Cb], "scenes": per, "reps": reps, "ms_per_scene": round(med, 4),
           "ms_min": round(min(ms_all), 4), "ms_max": round(max(ms_all), 4), "fit_ms": round(float(np.median(ms_fit)), 4),
           "transform_ms": round(float(np.median(ms_tr)), 4), "fixed_ms_estimate": round(eig, 4), "fixed_share": round(eig / med, 3),
           "bytes_moved_mb": round(nbytes / 1e6, 1), "tb_per_s": round(nbytes / med / 1e9, 3),
           "share_of_streaming_rate": round(nbytes / med / 1e9 / STREAM_TBS, 3), "wall_with_upload_ms": round(1e3 * float(np.median(wall)), 3),
           "host_restatement_ms": round(1e3 * t_host, 1), "speedup_vs_host": round(t_host / float(np.median(wall)), 1),
           "host_threads": torch.get_num_threads()}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    pavia = R.graded(610, 340, 103, seed=11)
    if a.profile:
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            m = HSIViT(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=10, embed_dim=128, depth=12,
                       num_heads=8, s_depth=9, trunc_init=True).cuda().eval()
        for _ in range(2):
            m.predict_scene(GWPCA().fit_transform(pavia))
        torch.cuda.synchronize()
        print("profiled predict_scene(GWPCA().fit_transform(raw)) (base) x2")
        return
    rows = [workload("pavia", [pavia], a.reps),
            workload("hyspecnet_batch", [R.graded(128, 128, 224, seed=30 + i) for i in range(a.batch)], a.reps)]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
