"""k-NN evaluation throughput on the synthetic Pavia-sized scene of scripts/scene_throughput.py (610 x 340 x 32 fp64, HSIViT Base):
DualViT.knn_scene with a bank of 640 and of 4,300 labelled pixels next to predict_scene, every leg in a fresh process, the legs
alternating; and on the same pooled features (one chunk of 8192 queries, and the whole scene) the three k-NN kernels against the
same top-k and vote written in eager torch (F.normalize, @, topk, exp, index_add).

    python scripts/knn_throughput.py [--reps 3] [--out FILE]     # the driver: starts one child per leg and repetition
    python scripts/knn_throughput.py --leg predict|knn640|knn4300|kernels640|kernels4300   # one leg, one JSON line
    python scripts/knn_throughput.py --profile                   # knn_scene (M = 640) twice: run under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene_throughput import BANDS, CLASSES, H, W, make_model  # noqa: E402

K, T, CHUNK = 20, 0.07, 8192
LEGS = ["predict", "knn640", "knn4300", "kernels640", "kernels4300"]


def bank_of(M):
    rng = np.random.default_rng(1)
    return np.sort(rng.choice(H * W, M, replace=False)), rng.integers(1, CLASSES, M)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def device_ms(fn, reps=5):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def eager_knn(feats, bank_n, labels, chunk):
    """The baseline: the same classifier in eager torch, the [chunk, M] matrix materialised per chunk of queries."""
    out = torch.empty(feats.shape[0], dtype=torch.int64, device=feats.device)
    for k0 in range(0, feats.shape[0], chunk):
        q = torch.nn.functional.normalize(feats[k0:k0 + chunk], dim=1)
        sim, idx = (q @ bank_n.T).topk(K, dim=1)
        votes = torch.zeros(q.shape[0], CLASSES, device=feats.device)
        votes.scatter_add_(1, labels[idx], torch.exp((sim - sim[:, :1]) / T))
        out[k0:k0 + chunk] = votes.argmax(1)
    return out


def kernels_leg(m, scene, M):
    from hsimae_amd import KNNClassifier
    pix, y = bank_of(M)
    s = torch.from_numpy(scene).cuda()
    feats = m.scene_features(s)                                   # fp32 [207400, 512], computed once for both sides
    knn = KNNClassifier(k=K, temperature=T, num_class=CLASSES).fit(feats[torch.from_numpy(pix).cuda()], torch.from_numpy(y))
    one = feats[:CHUNK]
    qn = knn._normalized(one)
    idx = torch.empty(CHUNK, K, dtype=torch.int32, device="cuda")
    sim = torch.empty(CHUNK, K, dtype=torch.float32, device="cuda")
    lab = torch.zeros(CHUNK, dtype=torch.int64, device="cuda")
    row = {"leg": f"kernels{M}", "M": M, "D": int(feats.shape[1]), "k": K, "chunk": CHUNK,
           "normalize_ms_per_chunk": device_ms(lambda: knn._normalized(one)),
           "topk_ms_per_chunk": device_ms(lambda: knn._topk(qn, idx, sim)),
           "vote_ms_per_chunk": device_ms(lambda: knn._vote(idx, sim, CHUNK, 1, CHUNK, 0, None, lab, None, None, None)),
           "eager_ms_per_chunk": device_ms(lambda: eager_knn(one, knn.bank, knn.labels, CHUNK)),
           "hip_scene_ms": device_ms(lambda: knn.predict(feats), 3),
           "eager_scene_ms": device_ms(lambda: eager_knn(feats, knn.bank, knn.labels, CHUNK), 3)}
    ours, theirs = knn.predict(feats)[0], eager_knn(feats, knn.bank, knn.labels, CHUNK)
    row["labels_differ_from_eager"] = int((ours != theirs).sum())
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}


def leg(name):
    scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
    m = make_model("base")
    if name.startswith("kernels"):
        return kernels_leg(m, scene, int(name[7:]))
    if name == "predict":
        fn = lambda: m.predict_scene(scene)                       # noqa: E731
    else:
        pix, y = bank_of(int(name[3:]))
        fn = lambda: m.knn_scene(scene, pix, y, k=K, temperature=T).labels      # noqa: E731
    fn()                                                          # warm-up: code objects, arenas, packed weights
    _, s = wall(fn)
    return {"leg": name, "seconds": round(s, 4), "px_per_s": round(H * W / s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
        m = make_model("base")
        pix, y = bank_of(640)
        for _ in range(2):
            m.knn_scene(scene, pix, y, k=K, temperature=T)
        print("profiled knn_scene (base, M = 640) x2")
        return
    if a.leg:
        print(json.dumps(leg(a.leg)), flush=True)
        return
    rows = []
    for rep in range(a.reps):                                     # a fresh process per leg, the legs alternating
        for name in LEGS[:3] if rep else LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=900)
            if r.returncode:
                raise SystemExit(f"leg {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            row = json.loads(r.stdout.strip().splitlines()[-1])
            row["rep"] = rep
            print(json.dumps(row), flush=True)
            rows.append(row)
    for name in LEGS[:3]:
        px = [r["px_per_s"] for r in rows if r["leg"] == name]
        print(json.dumps({"leg": name, "median_px_per_s": int(np.median(px)), "reps": len(px)}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
