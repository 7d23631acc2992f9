"""Masked-reconstruction throughput on the synthetic Pavia-sized scene of scripts/scene_throughput.py (610 x 340 x 32 fp64), HSIMAE
Base (embed_dim 128, depth 12 / 9, decoder 64 x 8), mask 0.75: reconstruct_scene at stride 9 and stride 3 next to the same loop
with the way back written in eager torch (index_put_(accumulate=True) per chunk, then the division, the reductions and acos),
every leg in a fresh process, the legs alternating.

    python scripts/recon_throughput.py [--reps 3] [--out FILE]   # the driver: starts one child per leg and repetition
    python scripts/recon_throughput.py --leg hip9|eager9|hip3|eager3                # one leg, one JSON line
    python scripts/recon_throughput.py --profile                 # reconstruct_scene (stride 3) twice: run under rocprofv3 --kernel-trace --stats
"""
import argparse
import contextlib
import io
import json
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scene_throughput import BANDS, H, W  # noqa: E402

LEGS = ["hip9", "eager9", "hip3", "eager3"]
RATIO, CHUNK = 0.75, 4096


def make_model():
    from hsimae_amd import HSIMAE
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=BANDS, b_patch_size=8, embed_dim=128, depth=12, num_heads=8, s_depth=9,
                   decoder_embed_dim=64, decoder_depth=8, decoder_num_heads=8, norm_pix_loss=True, trunc_init=True)
    return m.cuda().eval()


def eager_scene(m, scene, stride, gen):
    """reconstruct_scene's loop with the way back in eager torch: the same windows, forward and noise; then per chunk one
    index_put_(accumulate=True) each for sums and counts over the un-reflected masked positions, and at the end the division,
    three reductions per pixel and acos.  -> (mse, mean_sam, coverage) as device scalars."""
    from hsimae_amd import window_centres
    from hsimae_amd.recon import _recon_chunk
    from hsimae_amd.scene_pass import ScenePass
    dev = torch.device("cuda")
    s = torch.from_numpy(scene).to(dev) if not isinstance(scene, torch.Tensor) else scene
    rows = torch.from_numpy(window_centres(H, stride)).to(dev).long()
    cols = torch.from_numpy(window_centres(W, stride)).to(dev).long()
    items = (rows[:, None] * W + cols[None, :]).reshape(-1).contiguous()
    n_win = items.numel()
    sp = ScenePass(m, s, items, _recon_chunk(m, RATIO, CHUNK, n_win))
    T, L = m.input_size[0], m.input_size[1] ** 2
    acc = torch.zeros(H * W * BANDS, dtype=torch.float32, device=dev)
    cnt = torch.zeros(H * W * BANDS, dtype=torch.float32, device=dev)
    off = torch.arange(9, device=dev) - 4
    band = torch.arange(BANDS, device=dev)
    m.want_recons = True
    with torch.no_grad():
        grid = m.get_dim_patches(T, L, RATIO)
        for w0, n in sp.chunks():
            win = sp.cut(w0, n)
            n1 = torch.rand(n, T, device=dev, generator=gen)
            n2 = torch.rand(n, L, device=dev, generator=gen)
            _, pred, mask, st = m._run_forward(win, RATIO, (n1, n2), grid, want_latent=False)
            st.release()
            it = items[w0:w0 + n]
            r = (it // W)[:, None] + off[None, :]                                        # [n, 9]
            c = (it % W)[:, None] + off[None, :]
            ok = ((r >= 0) & (r < H))[:, None, :, None] & ((c >= 0) & (c < W))[:, None, None, :] & (mask[:, 0] != 0)
            vox = ((r.clamp(0, H - 1)[:, None, :, None] * W + c.clamp(0, W - 1)[:, None, None, :]) * BANDS + band[None, :, None, None])
            idx = vox[ok]
            acc.index_put_((idx,), pred[:, 0][ok], accumulate=True)
            cnt.index_put_((idx,), torch.ones_like(idx, dtype=torch.float32), accumulate=True)
        x = s.reshape(-1, BANDS).float()
        on = cnt.view(-1, BANDS) > 0
        rec = torch.where(on, acc.view(-1, BANDS) / cnt.view(-1, BANDS).clamp(min=1), x)
        se = ((rec - x).double() ** 2 * on).sum(1)
        mm = on.sum(1)
        rd, xd = rec.double() * on, x.double() * on
        cos = (rd * xd).sum(1) / (rd.norm(dim=1) * xd.norm(dim=1))
        sam = torch.acos(cos.clamp(-1, 1))
        have = mm > 0
        return se.sum() / mm.sum(), sam[have].mean(), mm.sum() / float(H * W * BANDS)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def leg(name):
    from hsimae_amd import reconstruct_scene, window_centres
    stride = int(name[-1])
    scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
    m = make_model()
    gen = torch.Generator(device="cuda")
    n_win = len(window_centres(H, stride)) * len(window_centres(W, stride))

    def run():
        random.seed(0)
        gen.manual_seed(0)
        if name.startswith("hip"):
            r = reconstruct_scene(m, scene, mask_ratio=RATIO, stride=stride, generator=gen, batch_size=CHUNK, on_device=True)
            return r.mse, r.mean_sam, r.coverage
        return eager_scene(m, scene, stride, gen)
    run()                                                         # warm-up: code objects, arenas, packed weights
    out, s = wall(run)
    mse, sam, cov = (float(v) for v in out)
    return {"leg": name, "stride": stride, "windows": n_win, "seconds": round(s, 4), "windows_per_s": round(n_win / s),
            "px_per_s": round(H * W / s), "mse": mse, "mean_sam": sam, "coverage": cov}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        from hsimae_amd import reconstruct_scene
        scene = np.random.default_rng(0).standard_normal((H, W, BANDS))
        m = make_model()
        for _ in range(2):
            reconstruct_scene(m, scene, mask_ratio=RATIO, stride=3, batch_size=CHUNK)
        print("profiled reconstruct_scene (base, stride 3) x2")
        return
    if a.leg:
        print(json.dumps(leg(a.leg)), flush=True)
        return
    rows = []
    for rep in range(a.reps):                                     # a fresh process per leg, the legs alternating
        for name in LEGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=900)
            if r.returncode:
                raise SystemExit(f"leg {name} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            row = json.loads(r.stdout.strip().splitlines()[-1])
            row["rep"] = rep
            print(json.dumps(row), flush=True)
            rows.append(row)
    for name in LEGS:
        got = [r for r in rows if r["leg"] == name]
        print(json.dumps({"leg": name, "median_windows_per_s": int(np.median([r["windows_per_s"] for r in got])),
                          "median_px_per_s": int(np.median([r["px_per_s"] for r in got])), "reps": len(got)}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
