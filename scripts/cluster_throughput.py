"""k-means throughput on the synthetic Pavia-sized scene of scripts/scene_throughput.py (610 x 340 x 32 fp64, HSIViT Base), K = 16
clusters, max_iter = 20: DualViT.cluster_scene (encoder features, and the spectra baseline) next to scene_features alone, every leg
in a fresh process; and on the same pooled features the two k-means launches per round (hsimae_kmeans_assign,
hsimae_kmeans_update) against the same round written in eager torch (x @ c.T, argmax, index_add_).

    python scripts/cluster_throughput.py [--reps 3] [--out FILE]   # the driver: one child per leg and repetition, each under its
                                                                   # own `timeout -k 10`, chained with && (a failed leg ends the run)
    python scripts/cluster_throughput.py --leg features|cluster|spectra|kernels        # one leg, one JSON line
"""
import argparse
import json
import os
import shlex
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_throughput import device_ms, wall  # noqa: E402
from scene_throughput import BANDS, H, W, make_model  # noqa: E402

K, ROUNDS = 16, 20
LEGS = ["features", "cluster", "spectra", "kernels"]
LEG_SECONDS = 300


def eager_round(x, c, bias, cosine):
    """The baseline: one Lloyd round in eager torch, the [N, K] score matrix materialised, the sums by index_add_ (fp32 atomics)."""
    s = x @ c.T
    lab = (s if bias is None else s - bias).argmax(1)
    sums = torch.zeros_like(c).index_add_(0, lab, x)
    counts = torch.bincount(lab, minlength=c.shape[0])
    new = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], c)
    if cosine:
        return lab, torch.nn.functional.normalize(new, dim=1), None
    return lab, new, 0.5 * (new * new).sum(1)


def kernels_leg(m, scene):
    from hsimae_amd import KMeans, _lib
    feats = m.scene_features(torch.from_numpy(scene).cuda())        # fp32 [207400, T * D], computed once for both sides
    N, D = feats.shape
    row = {"leg": "kernels", "N": int(N), "D": int(D), "K": K, "rounds": ROUNDS}
    for metric in ("cosine", "euclidean"):
        km = KMeans(K, metric=metric, max_iter=ROUNDS, generator=torch.Generator().manual_seed(0)).fit(feats)
        xs = km._rows(feats)
        w = {"c": km.centroids.clone(), "bias": None if km.bias is None else km.bias.clone(), "counts": km.counts.clone(),
             "sums": torch.zeros(K, D, dtype=torch.float64, device="cuda"),
             "scratch": torch.zeros(K * ((D + 63) // 64) + 1, dtype=torch.float64, device="cuda"),
             "state": torch.zeros(_lib.KMEANS_STATE, dtype=torch.float64, device="cuda")}
        labels = km.labels_.clone()
        changed = torch.zeros(_lib.KMEANS_GRID, dtype=torch.int32, device="cuda")
        tag = metric[:3]
        row[f"{tag}_assign_us"] = 1e3 * device_ms(lambda: km._assign(xs, N, w["c"], w["bias"], 1, N, 0, None, labels, None, None, changed), 10)
        row[f"{tag}_update_us"] = 1e3 * device_ms(lambda: km._update(xs, labels, w, changed), 10)
        row[f"{tag}_fit_ms"] = device_ms(lambda: KMeans(K, metric=metric, max_iter=ROUNDS, init=km.centroids).fit(feats), 3)
        c0, b0 = km.centroids.clone(), (None if km.bias is None else km.bias.clone())
        row[f"{tag}_eager_round_us"] = 1e3 * device_ms(lambda: eager_round(xs, c0, b0, metric == "cosine"), 10)
        row[f"{tag}_labels_differ_from_eager"] = int((eager_round(xs, c0, b0, metric == "cosine")[0] + 1 != km.predict(feats)[0]).sum())
        row[f"{tag}_n_iter"] = int(km.n_iter_)
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}


def leg(name):
    scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
    m = make_model("base")
    if name == "kernels":
        return kernels_leg(m, scene)
    gen = lambda: torch.Generator().manual_seed(0)                  # noqa: E731
    fn = {"features": lambda: m.scene_features(scene),
          "cluster": lambda: m.cluster_scene(scene, K, max_iter=ROUNDS, generator=gen()).labels,
          "spectra": lambda: m.cluster_scene(scene, K, features="spectra", max_iter=ROUNDS, generator=gen()).labels}[name]
    fn()                                                            # warm-up: code objects, arenas, packed weights
    _, s = wall(fn)
    return {"leg": name, "seconds": round(s, 4), "px_per_s": round(H * W / s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg)), flush=True)
        return
    me = shlex.quote(os.path.abspath(__file__))
    steps = [name for rep in range(a.reps) for name in (LEGS if rep == 0 else LEGS[:3])]
    chain = " && ".join(f"timeout -k 10 {LEG_SECONDS} {shlex.quote(sys.executable)} {me} --leg {name}" for name in steps)
    r = subprocess.run(["bash", "-c", chain], stdout=subprocess.PIPE, text=True)      # a fresh process per leg, one at a time
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    for row in rows:
        print(json.dumps(row), flush=True)
    if r.returncode:
        raise SystemExit(f"leg {steps[len(rows)]} ended with status {r.returncode}: nothing was started after it")
    for name in LEGS[:3]:
        px = [row["px_per_s"] for row in rows if row["leg"] == name]
        print(json.dumps({"leg": name, "median_px_per_s": int(np.median(px)), "reps": len(px)}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
