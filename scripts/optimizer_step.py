"""What a clipped optimizer step costs, at Base and Huge, four figures (seven with the moving average) taken on the same GPU in one run:

  1. plain        FusedAdamW.step()                                          (one launch)
  2. torch_clip   torch.nn.utils.clip_grad_norm_(...) + FusedAdamW.step()    (what a user had before max_grad_norm existed)
  3. fused_clip   FusedAdamW(max_grad_norm=..., skip_nonfinite=True).step()  (hsimae_grad_norm + hsimae_adamw_step_ctl)
  4. lamb         FusedLAMB(max_grad_norm=..., skip_nonfinite=True).step()   (hsimae_grad_norm + hsimae_lamb_step: five launches;
                  from its traffic, 10 array passes against 7, about 10 / 7 of fused_clip plus two small launches)
  5. plain_ema, fused_clip_ema, lamb_ema   1, 3 and 4 built with ema_decay=0.9999: one hsimae_ema_update more per step.  From its
                  traffic the update moves 12 bytes per element (average read and written, weight read) next to the AdamW kernel's
                  29 (four arrays read, three written, one id byte): 12 / 29 = 0.41 of the plain step is what to expect.

Gradients are present (one forward + backward first), every figure is the mean over --steps steps between two HIP events after
--warmup steps, repeated --repeats times with the four variants interleaved; the spread is max - min over the repeats.
max_norm is far above the norm, so that torch's in-place clip leaves the gradients as they are (the time does not depend on the
coefficient).  Prints one JSON line per model and writes all of them to --out.

    python scripts/optimizer_step.py [--models base,huge] [--steps 200] [--warmup 20] [--repeats 5] [--out profiles/optimizer_step.json]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from hsimae_amd import HSIMAE, FusedAdamW, FusedLAMB  # noqa: E402

MODELS = {"base": (96, 128, 8, "bf16"), "large": (96, 256, 16, "bf16"), "huge": (192, 512, 32, "bf16")}     # bench.py's widths; the
# step works on the fp32 masters and does not depend on the GEMM operand type, so the one backward that provides gradients runs in bf16


def measure(name, steps, warmup, repeats, batch, dev):
    bands, D, heads, precision = MODELS[name]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=bands, b_patch_size=8, embed_dim=D, depth=12, num_heads=heads,
                       s_depth=9, decoder_embed_dim=64, decoder_depth=8, decoder_num_heads=8, norm_pix_loss=True, trunc_init=True).to(dev)
    if precision == "fp8":
        model.set_precision("fp8")
    x = torch.rand(batch, 1, bands, 9, 9, device=dev)
    model.zero_grad(set_to_none=True)
    model(x, mask_ratio=0.75)[0].backward()
    kw = dict(lr=1e-5, weight_decay=5e-2, betas=(0.9, 0.95))
    plain, clipped = FusedAdamW(model, **kw), FusedAdamW(model, max_grad_norm=1e9, skip_nonfinite=True, **kw)
    lamb = FusedLAMB(model, max_grad_norm=1e9, skip_nonfinite=True, **kw)
    ema = dict(ema_decay=0.9999, ema_warmup=True)
    plain_ema, clipped_ema = FusedAdamW(model, **kw, **ema), FusedAdamW(model, max_grad_norm=1e9, skip_nonfinite=True, **kw, **ema)
    lamb_ema = FusedLAMB(model, max_grad_norm=1e9, skip_nonfinite=True, **kw, **ema)
    with_grad = [p for p in model.parameters() if p.grad is not None]

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(with_grad, 1e9)
        plain.step()

    variants = {"plain": plain.step, "torch_clip": torch_clip, "fused_clip": clipped.step, "lamb": lamb.step,
                "plain_ema": plain_ema.step, "fused_clip_ema": clipped_ema.step, "lamb_ema": lamb_ema.step}
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / steps)
    if int(clipped_ema.skipped_steps) != 0 or int(lamb_ema.skipped_steps) != 0 or not torch.isfinite(plain_ema.ema).all():
        raise RuntimeError("the measured steps were not clean")
    if int(clipped.skipped_steps) != 0 or int(lamb.skipped_steps) != 0 or int(lamb.table_error) != 0 or not torch.isfinite(model._flat).all():
        raise RuntimeError("the measured steps were not clean")
    res = {"model": name, "precision": precision, "parameters": int(model._flat.numel()), "tensors_with_grad": len(with_grad),
           "steps": steps, "warmup": warmup, "repeats": repeats, "gpu": torch.cuda.get_device_name(dev)}
    for k, v in times.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
    spread = max(r["max"] - r["min"] for r in (res["torch_clip_ms"], res["fused_clip_ms"]))
    res["ratio_fused_clip_to_plain"] = res["fused_clip_ms"]["median"] / res["plain_ms"]["median"]
    res["spread_ms"] = spread
    res["ratio_lamb_to_fused_clip"] = res["lamb_ms"]["median"] / res["fused_clip_ms"]["median"]
    res["lamb_spread_ms"] = res["lamb_ms"]["max"] - res["lamb_ms"]["min"]
    ratios = lamb.trust_ratios[torch.tensor(lamb.adapted(), device=dev)]
    res["lamb_trust_ratio_range"] = [float(ratios.min()), float(ratios.max())]
    for k in ("plain", "fused_clip", "lamb"):                       # what the average adds to each step, beside 12 / 29 of the plain one
        res[f"ema_adds_to_{k}_ms"] = res[k + "_ema_ms"]["median"] - res[k + "_ms"]["median"]
        res[f"ema_spread_{k}_ms"] = max(res[k + "_ema_ms"]["max"] - res[k + "_ema_ms"]["min"], res[k + "_ms"]["max"] - res[k + "_ms"]["min"])
    res["ratio_ema_to_plain_step"] = res["ema_adds_to_plain_ms"] / res["plain_ms"]["median"]
    res["ratio_ema_to_plain_step_from_traffic"] = 12 / 29
    res["fused_clip_faster_than_torch_clip_by_more_than_spread"] = res["torch_clip_ms"]["median"] - res["fused_clip_ms"]["median"] > spread
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="base,huge")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join("profiles", "optimizer_step.json"))
    args = ap.parse_args()
    if args.steps < 200:
        print("note: fewer than 200 steps per figure", file=sys.stderr)
    dev = torch.device("cuda:0")
    out = []
    for name in args.models.split(","):
        res = measure(name, args.steps, args.warmup, args.repeats, args.batch, dev)
        out.append(res)
        print(json.dumps(res))
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
