"""Linear-probe throughput on HSIViT Base, 32 bands, banks of 640 and 4,300 labelled pixels of the synthetic Pavia-sized scene of
scripts/scene_throughput.py, 100 iterations, every leg in a fresh process:

    fit     LinearProbe.fit on the cached pooled features (hsimae_probe_prepare + 100 x hsimae_probe_step): milliseconds per fit,
            launches per iteration and microseconds per launch;
    eager   the same loop in eager torch on the same cached features: standardisation, nn.Linear, F.cross_entropy, autograd,
            torch.optim.AdamW with the bias in a no-decay group;
    freeze  the route the probe replaces: one epoch of dual_branch_finetuning_scene with every parameter but `cls_head` frozen
            (freeze=...), which still runs the whole encoder and decoder forward and backward for every batch.  That loop trains
            on half of the bank (the other half validates); the epoch is the difference of a 2-epoch and a 1-epoch run.

    python scripts/probe_throughput.py [--out FILE]          # the driver: one child per leg, each under its own `timeout -k 10`,
                                                             # chained with && (a failed leg ends the run)
    python scripts/probe_throughput.py --leg fit640|fit4300|eager640|eager4300|freeze640|freeze4300       # one leg, one JSON line
Not measured here: probe accuracy on a real labelled scene.
"""
import argparse
import contextlib
import io
import json
import math
import os
import shlex
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_throughput import bank_of, device_ms, wall  # noqa: E402
from scene_throughput import BANDS, CLASSES, H, W, make_model  # noqa: E402

ITERS = 100
BANKS = (640, 4300)
LEGS = [f"{kind}{M}" for kind in ("fit", "eager", "freeze") for M in BANKS]
LEG_SECONDS = 420
LAUNCHES_PER_ITER = 4            # forward, gradient partials, update, finish (hsimae_probe_prepare adds 2 per fit)


def bank_features(M):
    scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
    pix, y = bank_of(M)
    feats = make_model("base").scene_features(torch.from_numpy(scene).cuda(), pixels=pix)
    return feats, torch.from_numpy(y).cuda()


def fit_leg(M):
    from hsimae_amd import LinearProbe
    feats, y = bank_features(M)
    ms = device_ms(lambda: LinearProbe(CLASSES, max_iter=ITERS).fit(feats, y), 5)
    _, host_s = wall(lambda: LinearProbe(CLASSES, max_iter=ITERS).fit(feats, y))
    p = LinearProbe(CLASSES, max_iter=ITERS).fit(feats, y)
    hist = p.loss_history.cpu().numpy()
    launches = LAUNCHES_PER_ITER * ITERS + 2
    return {"leg": f"fit{M}", "M": M, "D": int(feats.shape[1]), "iters": ITERS, "fit_ms": round(ms, 3), "fit_wall_ms": round(1e3 * host_s, 3),
            "launches_per_iter": LAUNCHES_PER_ITER, "us_per_launch": round(1e3 * ms / launches, 2),
            "loss_first": round(float(hist[0]), 4), "loss_last": round(float(hist[-1]), 4)}


def eager_fit(feats, y):
    D = feats.shape[1]
    xs = (feats - feats.mean(0)) * torch.rsqrt(feats.var(0, unbiased=False) + 1e-6)
    lin = torch.nn.Linear(D, CLASSES - 1).cuda()
    torch.nn.init.zeros_(lin.weight)
    torch.nn.init.zeros_(lin.bias)
    opt = torch.optim.AdamW([{"params": [lin.weight], "weight_decay": 1e-4}, {"params": [lin.bias], "weight_decay": 0.0}], lr=1e-2)
    t = y - 1
    for it in range(ITERS):
        for g in opt.param_groups:
            g["lr"] = 1e-2 * 0.5 * (1 + math.cos(math.pi * it / ITERS))
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(lin(xs), t)
        loss.backward()
        opt.step()
    return loss.detach()


def eager_leg(M):
    feats, y = bank_features(M)
    ms = device_ms(lambda: eager_fit(feats, y), 5)
    _, host_s = wall(lambda: eager_fit(feats, y))
    return {"leg": f"eager{M}", "M": M, "iters": ITERS, "fit_ms": round(ms, 3), "fit_wall_ms": round(1e3 * host_s, 3),
            "loss_last": round(float(eager_fit(feats, y)), 4)}


def freeze_leg(M):
    from hsimae_amd import DualViT, dual_branch_finetuning_scene
    scene = torch.from_numpy(np.random.default_rng(0).standard_normal((H, W, BANDS))).cuda()
    pix, y = bank_of(M)
    with contextlib.redirect_stdout(io.StringIO()):
        names = DualViT(img_size=9, patch_size=3, in_chans=1, bands=BANDS, b_patch_size=8, num_class=CLASSES, embed_dim=128, depth=12,
                        num_heads=8, s_depth=9, decoder_embed_dim=64, decoder_depth=2, decoder_num_heads=8).named_parameters()
        frozen = tuple(sorted({n.split(".")[0] for n, _ in names} - {"cls_head"}))

    def run(epochs, d):
        with contextlib.redirect_stdout(io.StringIO()):
            return dual_branch_finetuning_scene(scene, pix, y, d, "probe_route.pkl", depth=12, dim=128, dec_depth=2, dec_dim=64, s_depth=9,
                                                epochs=epochs, batch_size=32, freeze=frozen, log=lambda *a: None)
    with tempfile.TemporaryDirectory() as d:
        run(1, d)                                                # warm-up: code objects, arenas, packed weights
        _, one = wall(lambda: run(1, d))
        _, two = wall(lambda: run(2, d))
    return {"leg": f"freeze{M}", "M": M, "trained_on": M // 2, "batch_size": 32, "one_epoch_call_s": round(one, 3),
            "two_epoch_call_s": round(two, 3), "epoch_s": round(two - one, 3), "frozen": list(frozen)}


def leg(name):
    kind, M = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    return {"fit": fit_leg, "eager": eager_leg, "freeze": freeze_leg}[kind](M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg)), flush=True)
        return
    me = shlex.quote(os.path.abspath(__file__))
    chain = " && ".join(f"timeout -k 10 {LEG_SECONDS} {shlex.quote(sys.executable)} {me} --leg {name}" for name in LEGS)
    r = subprocess.run(["bash", "-c", chain], stdout=subprocess.PIPE, text=True)      # a fresh process per leg, one at a time
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    if r.returncode:
        raise SystemExit(f"leg {LEGS[len(rows)]} ended with status {r.returncode}: nothing was started after it")


if __name__ == "__main__":
    main()
