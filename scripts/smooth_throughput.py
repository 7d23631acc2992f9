"""Probability-filter throughput on the synthetic Pavia-sized scene of scripts/scene_throughput.py (610 x 340 x 32) with 16 classes
(17 columns, class 0 "unlabelled"), every leg in a fresh process:

    kernel   EdgeFilter(radius).apply (one hsimae_prob_filter launch + the zeroed maps) at radius 3, 5 and 8, guide = the scene's
             first principal component: microseconds per call, device time over 1000 calls;
    eager    the same filter in eager torch on the same inputs, in its unfold form: the [H W, (2r+1)^2, K] neighbourhoods of the
             probabilities and of the guide, exp, two reductions, top-2;
    scene    HSIViT Base classify_scene(return_probs=True, on_device=True) alone, and followed by scene_guide + the default filter:
             device milliseconds of each, and the filter's share of the second.  classify_scene itself is the code of the commit
             before this one (hsimae_amd/finetune.py is untouched), so the first figure is also the parent's.

    python scripts/smooth_throughput.py [--out FILE]         # the driver: one child per leg, each under its own `timeout -k 10`,
                                                             # chained with && (a failed leg ends the run)
    python scripts/smooth_throughput.py --leg kernel3|kernel5|kernel8|eager3|eager5|eager8|scene       # one leg, one JSON line
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/smooth_throughput.py --leg profile        # the kernel's own time
Not measured here: whether the filter improves OA / AA / kappa on a real labelled scene.
"""
import argparse
import contextlib
import io
import json
import os
import shlex
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knn_throughput import device_ms  # noqa: E402
from scene_throughput import BANDS, H, W  # noqa: E402

CLASSES = 17                     # 16 classes + "unlabelled"
RADII = (3, 5, 8)
LEGS = [f"{kind}{r}" for kind in ("kernel", "eager") for r in RADII] + ["scene"]
LEG_SECONDS = 300
CALLS = 1000                     # per timed window of a kernel leg: 0.07 to 0.5 s of device time


def inputs():
    from hsimae_amd import scene_guide
    scene = torch.from_numpy(np.random.default_rng(0).standard_normal((H, W, BANDS))).cuda()
    g = torch.Generator().manual_seed(2)
    probs = torch.zeros(H * W, CLASSES)
    probs[:, 1:] = torch.softmax(2.0 * torch.randn(H * W, CLASSES - 1, generator=g), 1)
    return scene, probs.cuda(), scene_guide(scene)


def kernel_leg(r):
    from hsimae_amd import EdgeFilter
    _, probs, guide = inputs()
    f = EdgeFilter(radius=r)
    ms = device_ms(lambda: f.apply(probs, H, W, guide), CALLS)
    ms_p = device_ms(lambda: f.apply(probs, H, W, guide, return_probs=True), CALLS)
    taps = (2 * r + 1) ** 2
    return {"leg": f"kernel{r}", "radius": r, "classes": CLASSES - 1, "us": round(1e3 * ms, 1), "us_with_probs": round(1e3 * ms_p, 1),
            "gflop": round(2e-9 * H * W * taps * (CLASSES - 1), 3), "workgroups": ((H + 15) // 16) * ((W + 15) // 16)}


def eager_filter(probs, guide, scale, r, a_s, a_r):
    """The joint bilateral filter in eager torch: zero padding + a validity plane stand in for "taps outside the scene are skipped"."""
    unfold = torch.nn.functional.unfold
    K, T = probs.shape[1] - 1, (2 * r + 1) ** 2
    P = probs[:, 1:].t().reshape(1, K, H, W)
    nb = unfold(P, 2 * r + 1, padding=r).view(K, T, H * W)
    ok = unfold(torch.ones(1, 1, H, W, device=probs.device), 2 * r + 1, padding=r).view(T, H * W)
    I = (guide * scale).permute(2, 0, 1).reshape(1, -1, H, W)
    d = unfold(I, 2 * r + 1, padding=r).view(I.shape[1], T, H * W) - I.view(I.shape[1], 1, H * W)
    off = torch.arange(-r, r + 1, device=probs.device, dtype=torch.float32)
    s2 = (off[:, None] ** 2 + off[None, :] ** 2).reshape(T, 1)
    w = torch.exp2(-(a_s * s2 + a_r * (d * d).sum(0))) * ok
    out = (nb * w).sum(1) / w.sum(0)
    top = out.topk(2, dim=0)
    return 1 + top.indices[0], top.values[0], top.values[0] - top.values[1]


def eager_leg(r):
    from hsimae_amd import EdgeFilter
    _, probs, (guide, scale) = inputs()
    f = EdgeFilter(radius=r)
    ms = device_ms(lambda: eager_filter(probs, guide, scale, r, f.a_s, f.a_r), 5)
    lab = eager_filter(probs, guide, scale, r, f.a_s, f.a_r)[0]
    same = float((lab.view(H, W) == f.apply(probs, H, W, (guide, scale)).labels).float().mean())
    return {"leg": f"eager{r}", "radius": r, "us": round(1e3 * ms, 1), "labels_equal_share": round(same, 6),
            "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}


def scene_leg():
    from hsimae_amd import EdgeFilter, HSIViT, scene_guide
    scene, _, _ = inputs()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIViT(img_size=9, patch_size=3, in_chans=1, bands=BANDS, b_patch_size=8, num_class=CLASSES, embed_dim=128, depth=12,
                   num_heads=8, s_depth=9, trunc_init=True).cuda().eval()
    f = EdgeFilter()

    def smoothed():
        res = m.classify_scene(scene, return_probs=True, on_device=True)
        return f.apply(res.probs, H, W, scene_guide(scene))

    plain = device_ms(lambda: m.classify_scene(scene, return_probs=True, on_device=True), 3)
    both = device_ms(smoothed, 3)
    res = m.classify_scene(scene, return_probs=True, on_device=True)
    guide = scene_guide(scene)
    g_ms = device_ms(lambda: scene_guide(scene), 5)
    f_ms = device_ms(lambda: f.apply(res.probs, H, W, guide), 20)
    return {"leg": "scene", "model": "base", "classify_ms": round(plain, 2), "classify_smooth_ms": round(both, 2),
            "guide_ms": round(g_ms, 3), "filter_ms": round(f_ms, 4), "filter_share": round(f_ms / both, 5),
            "guide_share": round(g_ms / both, 5)}


def profile_leg():
    """For `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/smooth_throughput.py --leg profile`: 200 calls per radius after
    one warm-up; the kernel's own time is prob_filter_kernel's row of DIR's kernel_stats.csv, one run per radius being told apart
    by the order of the trace (radius 3, 5, 8)."""
    from hsimae_amd import EdgeFilter
    _, probs, guide = inputs()
    for r in RADII:
        f = EdgeFilter(radius=r)
        for _ in range(201):
            f.apply(probs, H, W, guide)
        torch.cuda.synchronize()
    return {"leg": "profile", "calls_per_radius": 201, "radii": list(RADII)}


def leg(name):
    if name == "scene":
        return scene_leg()
    if name == "profile":
        return profile_leg()
    kind = name.rstrip("0123456789")
    return {"kernel": kernel_leg, "eager": eager_leg}[kind](int(name[len(kind):]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS + ["profile"])
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
