"""Superpixel throughput on the synthetic Pavia-sized scene of scripts/scene_throughput.py (610 x 340 x 32): SLIC over the scene's
first three principal components at size 8 (3,311 centres), 10 rounds, and the vote over 16 classes (17 columns, class 0
"unlabelled"), every leg in a fresh process:

    kernel   hsimae_slic through the C ABI on preallocated buffers: the whole fit (init + 10 rounds + final assign, 12 launches),
             the same with 0 rounds (init + final assign), one round as their difference / 10, and one round measured alone
             (init = 0, rounds = 1, minus the 0-round call from the same centres); Superpixels.fit (the same plus its five
             allocations); hsimae_segment_vote in both modes, with and without the segment vectors: microseconds per call, device
             time over 200 to 1000 calls;
    eager    the same algorithm in eager torch on the same inputs: the [H W, 9] candidate distance tensor, argmin, and fp64
             index_add_ for the sums (floating-point atomics: not reproducible), one round and ten; and the share of pixels whose
             label after ten rounds equals the kernel's;
    scene    HSIViT Base classify_scene(return_probs=True, on_device=True) alone, and followed by scene_guide(scene, 3) +
             Superpixels().fit + the mean vote: device milliseconds of each, and the share of the guide, the fit and the vote in the
             second.  classify_scene itself is the code of the commit before this one (hsimae_amd/finetune.py is untouched).

    python scripts/slic_throughput.py [--out FILE]           # the driver: one child per leg, each under its own `timeout -k 10`,
                                                             # chained with && (a failed leg ends the run)
    python scripts/slic_throughput.py --leg kernel|eager|scene                                          # one leg, one JSON line
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/slic_throughput.py --leg profile          # the kernels' own times
Not measured here: whether superpixel voting improves OA / AA / kappa on a real labelled scene; the defaults are not tuned.
"""
import argparse
import contextlib
import ctypes as C
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
SIZE, COMPACTNESS, ROUNDS, CHANNELS = 8, 0.1, 10, 3
LEGS = ["kernel", "eager", "scene"]
LEG_SECONDS = 300


def inputs():
    from hsimae_amd import scene_guide
    scene = torch.from_numpy(np.random.default_rng(0).standard_normal((H, W, BANDS))).cuda()
    g = torch.Generator().manual_seed(2)
    probs = torch.zeros(H * W, CLASSES)
    probs[:, 1:] = torch.softmax(2.0 * torch.randn(H * W, CLASSES - 1, generator=g), 1)
    return scene, probs.cuda(), scene_guide(scene, CHANNELS)


class Fit:
    """hsimae_slic on buffers allocated once."""

    def __init__(self, guide, scale):
        from hsimae_amd import Superpixels, _lib
        self.lib, self._lib = _lib.load(), _lib
        self.sp = Superpixels(SIZE, COMPACTNESS, ROUNDS)
        self.guide, self.scale = guide, scale
        self.K = (-(-H // SIZE)) * (-(-W // SIZE))
        self.centres, self.tmp = torch.empty(self.K, 8, device="cuda"), torch.empty(self.K, 8, device="cuda")
        self.counts = torch.empty(self.K, dtype=torch.int32, device="cuda")
        self.labels = torch.empty(H * W, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream

    def __call__(self, init, rounds):
        p = self._lib.SlicParams(guide=self.guide.data_ptr(), guide_scale=self.scale.data_ptr(), G=CHANNELS, H=H, W=W, size=SIZE, w=self.sp.w,
                                 init=init, rounds=rounds, centres=self.centres.data_ptr(), centres_tmp=self.tmp.data_ptr(),
                                 counts=self.counts.data_ptr(), labels=self.labels.data_ptr(), dist=None)
        self._lib.check(self.lib.hsimae_slic(C.byref(p), self.stream), "hsimae_slic")


def kernel_leg():
    from hsimae_amd.segment import segment_vote
    _, probs, (guide, scale) = inputs()
    fit = Fit(guide, scale)
    whole = device_ms(lambda: fit(1, ROUNDS), 200)
    none = device_ms(lambda: fit(1, 0), 1000)
    fit(1, 3)                                             # centres off the grid; a 0-round call leaves them where they are
    stay = device_ms(lambda: fit(0, 0), 1000)
    start = fit.centres.clone()

    def one():
        fit.centres.copy_(start)
        fit(0, 1)

    def copy_only():
        fit.centres.copy_(start)
        fit(0, 0)

    single = device_ms(one, 1000) - device_ms(copy_only, 1000)
    py = device_ms(lambda: fit.sp.fit((guide, scale)), 200)
    segs = fit.sp.fit((guide, scale))
    empty = int((segs.counts == 0).sum())
    row = {"leg": "kernel", "size": SIZE, "channels": CHANNELS, "centres": fit.K, "rounds": ROUNDS, "fit_us": round(1e3 * whole, 1),
           "init_final_us": round(1e3 * none, 1), "final_us": round(1e3 * stay, 1), "round_us": round(1e2 * (whole - none), 1),
           "round_alone_us": round(1e3 * single, 1), "python_fit_us": round(1e3 * py, 1), "empty_segments": empty,
           "distance_evals_per_round": 81 * H * W}
    for mode in ("mean", "vote"):
        row[f"vote_{mode}_us"] = round(1e3 * device_ms(lambda: segment_vote(probs, segs, mode=mode), 1000), 1)
        row[f"vote_{mode}_probs_us"] = round(1e3 * device_ms(lambda: segment_vote(probs, segs, mode=mode, return_probs=True), 1000), 1)
    return row


def eager_tables(dev):
    ny, nx = -(-H // SIZE), -(-W // SIZE)
    hi = (torch.arange(H, device=dev) * ny // H)[:, None].expand(H, W).reshape(-1)
    hj = (torch.arange(W, device=dev) * nx // W)[None, :].expand(H, W).reshape(-1)
    cand, valid = [], []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            ci, cj = hi + a, hj + b
            ok = (ci >= 0) & (ci < ny) & (cj >= 0) & (cj < nx)
            cand.append(torch.where(ok, ci * nx + cj, torch.zeros_like(ci)))
            valid.append(ok)
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None].expand(H, W).reshape(-1)
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :].expand(H, W).reshape(-1)
    return torch.stack(cand, 1), torch.stack(valid, 1), yy, xx, ny * nx


def eager_assign(v, centres, cand, valid, yy, xx, w):
    c = centres[cand]                                                            # [H W, 9, G + 2]
    d = ((v[:, None, :] - c[..., :CHANNELS]) ** 2).sum(2) + w * ((yy[:, None] - c[..., CHANNELS]) ** 2 + (xx[:, None] - c[..., CHANNELS + 1]) ** 2)
    d = torch.where(valid, d, torch.full_like(d, float("inf")))
    return cand.gather(1, d.argmin(1, keepdim=True))[:, 0]


def eager_round(v, centres, cand, valid, yy, xx, w, K):
    lab = eager_assign(v, centres, cand, valid, yy, xx, w)
    vals = torch.cat([v, yy[:, None], xx[:, None]], 1).double()
    sums = torch.zeros(K, CHANNELS + 2, dtype=torch.float64, device=v.device).index_add_(0, lab, vals)
    cnt = torch.zeros(K, dtype=torch.float64, device=v.device).index_add_(0, lab, torch.ones_like(yy, dtype=torch.float64))
    return torch.where(cnt[:, None] > 0, (sums / cnt[:, None].clamp(min=1)).float(), centres)


def eager_leg():
    _, _, (guide, scale) = inputs()
    fit = Fit(guide, scale)
    fit(1, 0)
    start = fit.centres[:, :CHANNELS + 2].clone()
    v = (guide * scale).reshape(H * W, CHANNELS)
    cand, valid, yy, xx, K = eager_tables(v.device)
    w = fit.sp.w

    def ten():
        c = start
        for _ in range(ROUNDS):
            c = eager_round(v, c, cand, valid, yy, xx, w, K)
        return eager_assign(v, c, cand, valid, yy, xx, w)

    one_ms = device_ms(lambda: eager_round(v, start, cand, valid, yy, xx, w, K), 20)
    ten_ms = device_ms(ten, 5)
    fit(1, ROUNDS)
    same = float((ten().to(torch.int32) == fit.labels).float().mean())
    return {"leg": "eager", "round_us": round(1e3 * one_ms, 1), "fit_us": round(1e3 * ten_ms, 1), "labels_equal_share": round(same, 6),
            "peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}


def scene_leg():
    from hsimae_amd import HSIViT, Superpixels, scene_guide
    from hsimae_amd.segment import segment_vote
    scene, _, _ = inputs()
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIViT(img_size=9, patch_size=3, in_chans=1, bands=BANDS, b_patch_size=8, num_class=CLASSES, embed_dim=128, depth=12,
                   num_heads=8, s_depth=9, trunc_init=True).cuda().eval()
    sp = Superpixels(SIZE, COMPACTNESS, ROUNDS)

    def voted():
        res = m.classify_scene(scene, return_probs=True, on_device=True)
        return segment_vote(res.probs, sp.fit(scene_guide(scene, CHANNELS)))

    plain = device_ms(lambda: m.classify_scene(scene, return_probs=True, on_device=True), 3)
    both = device_ms(voted, 3)
    res = m.classify_scene(scene, return_probs=True, on_device=True)
    guide = scene_guide(scene, CHANNELS)
    segs = sp.fit(guide)
    g_ms = device_ms(lambda: scene_guide(scene, CHANNELS), 5)
    f_ms = device_ms(lambda: sp.fit(guide), 50)
    v_ms = device_ms(lambda: segment_vote(res.probs, segs), 200)
    return {"leg": "scene", "model": "base", "classify_ms": round(plain, 2), "classify_segment_ms": round(both, 2), "guide_ms": round(g_ms, 3),
            "fit_ms": round(f_ms, 4), "vote_ms": round(v_ms, 4), "fit_share": round(f_ms / both, 5), "vote_share": round(v_ms / both, 5),
            "guide_share": round(g_ms / both, 5)}


def profile_leg():
    """For `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/slic_throughput.py --leg profile`: 100 fits and 100 votes per
    mode after one warm-up; the kernels' own times are the rows slic_round_kernel<false> (a round), slic_round_kernel<true> (the
    final assign), slic_init_kernel and segment_vote_kernel of DIR's kernel_stats.csv."""
    from hsimae_amd.segment import segment_vote
    _, probs, (guide, scale) = inputs()
    fit = Fit(guide, scale)
    for _ in range(101):
        fit(1, ROUNDS)
    segs = fit.sp.fit((guide, scale))
    for _ in range(101):
        segment_vote(probs, segs, mode="mean")
    torch.cuda.synchronize()
    return {"leg": "profile", "fits": 101, "votes": 101}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS + ["profile"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps({"kernel": kernel_leg, "eager": eager_leg, "scene": scene_leg, "profile": profile_leg}[a.leg]()), flush=True)
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
