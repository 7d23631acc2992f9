"""What per-group learning rates cost in the optimizer step, on the Base model's flat buffer, all figures taken on one GPU in one
process with gradients present (one forward + backward first):

  a. adamw_step      hsimae_adamw_step                                         (the default launch)
  b. groups_2        hsimae_adamw_step_groups, the two-entry table {(lr, wd), (lr, 0)}
  c. groups_ld       hsimae_adamw_step_groups, the table and ids of FusedAdamW(layer_decay=0.75)
  d. step_default / step_ld   FusedAdamW.step() end to end, default and layer_decay=0.75   (host clock around a final synchronise)
  e. torch_ld        torch.optim.AdamW built with the same groups as c                  (host clock around a final synchronise)

a - c: HIP events around --steps launches after --warmup launches; every figure --repeats times with the variants interleaved.  The
three kernels move the same bytes, so a = b = c is expected within the spread between repeats of the same kernel; that spread (the
largest max - min of a, b, c) is what a difference is judged against.

hsimae_adamw_step_ctl runs the grouped kernel now.  `--ctl-against OTHER.so` times that entry point (and hsimae_grad_norm + it, the
clipped step's launches) in fresh child processes that load this tree's library and OTHER.so (a library built from the commit
before) in turn, --repeats times alternating.

    python scripts/optimizer_groups.py [--steps 200] [--warmup 20] [--repeats 5] [--ctl-against PATH] [--out profiles/optimizer_groups.json]
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.getcwd())

BASE = dict(img_size=9, patch_size=3, in_chans=1, bands=96, b_patch_size=8, embed_dim=128, depth=12, num_heads=8, s_depth=9,
            decoder_embed_dim=64, decoder_depth=8, decoder_num_heads=8, norm_pix_loss=True, trunc_init=True)      # bench.py's Base (C2)
KW = dict(lr=1e-5, weight_decay=5e-2, betas=(0.9, 0.95))
B1, B2, EPS = 0.9, 0.95, 1e-8


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def event_ms(torch, fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def host_ms(torch, fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(steps, warmup, repeats):
    import torch
    from hsimae_amd import HSIMAE, FusedAdamW, _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        model = HSIMAE(**BASE).to(dev)
    x = torch.rand(64, 1, BASE["bands"], 9, 9, device=dev)
    model.zero_grad(set_to_none=True)
    model(x, mask_ratio=0.75)[0].backward()
    plain, ld = FusedAdamW(model, **KW), FusedAdamW(model, layer_decay=0.75, **KW)
    plain._bind(); ld._bind()
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    flat, grad, n = model._flat, model._flat_grad, model._flat.numel()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    ptrs = (flat.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr())
    two = (_lib.AdamWGroup * 2)(_lib.AdamWGroup(KW["lr"], KW["weight_decay"]), _lib.AdamWGroup(KW["lr"], 0.0))
    table, ng = ld._table(), ld._ngroups
    count = [0]

    def a():
        count[0] += 1
        _lib.check(lib.hsimae_adamw_step(*ptrs, plain._group.data_ptr(), n, KW["lr"], B1, B2, EPS, KW["weight_decay"], count[0], stream))

    def b():
        count[0] += 1
        _lib.check(lib.hsimae_adamw_step_groups(*ptrs, plain._group.data_ptr(), 0, n, two, 2, B1, B2, EPS, count[0], None, stream))

    def c():
        count[0] += 1
        _lib.check(lib.hsimae_adamw_step_groups(*ptrs, ld._group.data_ptr(), 0, n, table, ng, B1, B2, EPS, count[0], None, stream))

    groups = [dict(params=g["params"], lr=g["lr"] * g["lr_scale"], weight_decay=g["weight_decay"]) for g in ld.param_groups if g["params"]]
    stock = torch.optim.AdamW(groups, lr=KW["lr"], betas=KW["betas"], eps=EPS)
    kernels = {"adamw_step": a, "groups_2": b, "groups_ld": c}
    hosted = {"step_default": plain.step, "step_ld": ld.step, "torch_ld": stock.step}
    times = {k: [] for k in (*kernels, *hosted)}
    for fn in (*kernels.values(), *hosted.values()):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in kernels.items():
            times[k].append(event_ms(torch, fn, steps))
        for k, fn in hosted.items():
            times[k].append(host_ms(torch, fn, steps))
    if not bool(torch.isfinite(flat).all()):
        raise RuntimeError("the measured steps were not clean")
    res = {"model": "base", "parameters": int(n), "table_entries": int(ng), "torch_groups": len(groups), "steps": steps,
           "warmup": warmup, "repeats": repeats, "gpu": torch.cuda.get_device_name(dev)}
    for k, t in times.items():
        res[k + "_ms"] = summary(t)
    res["kernel_spread_ms"] = max(res[k + "_ms"]["max"] - res[k + "_ms"]["min"] for k in kernels)
    for k in ("groups_2", "groups_ld"):
        res[k + "_minus_adamw_step_ms"] = res[k + "_ms"]["median"] - res["adamw_step_ms"]["median"]
    return res


def ctl_child(path, steps, warmup):
    """One sample for one library: hsimae_adamw_step_ctl alone, and hsimae_grad_norm + it, on a Base-sized buffer (4.6 M elements,
    ids 0 / 1 / 2 as the model has them: every eighth element frozen)."""
    import torch
    from hsimae_amd import _lib
    lib = C.CDLL(path)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.hsimae_adamw_step_ctl.argtypes = [vp, vp, vp, vp, vp, i32, i64, f32, f32, f32, f32, f32, vp, vp]
    lib.hsimae_grad_norm.argtypes = [C.POINTER(_lib.GradSeg), i32, f32, i32, i32, f32, f32, vp, vp, vp]
    dev = torch.device("cuda:0")
    n = 4614264
    g_ = torch.Generator().manual_seed(0)
    p, g = torch.rand(n, generator=g_).to(dev), (0.01 * torch.rand(n, generator=g_)).to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ids = (torch.arange(n) % 2).to(torch.uint8)
    ids[::8] = 2
    ids = ids.to(dev)
    ctl = torch.zeros(C.sizeof(_lib.ClipCtl), dtype=torch.uint8, device=dev)
    partials = torch.empty(_lib.CLIP_GRID, dtype=torch.float64, device=dev)
    segs = (_lib.GradSeg * 1)(_lib.GradSeg(g.data_ptr(), ids.data_ptr(), n))
    stream = torch.cuda.current_stream(dev).cuda_stream
    count = [0]

    def norm():
        count[0] += 1
        assert lib.hsimae_grad_norm(segs, 1, 1e9, 1, count[0], B1, B2, partials.data_ptr(), ctl.data_ptr(), stream) == 0

    def step():
        assert lib.hsimae_adamw_step_ctl(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ids.data_ptr(), 0, n, KW["lr"], B1, B2,
                                         EPS, KW["weight_decay"], ctl.data_ptr(), stream) == 0

    def both():
        norm(); step()
    norm()
    for _ in range(warmup):
        both()
    torch.cuda.synchronize()
    out = {"step_ctl_ms": event_ms(torch, step, steps), "norm_and_step_ctl_ms": event_ms(torch, both, steps)}
    if not bool(torch.isfinite(p).all()):
        raise RuntimeError("the measured steps were not clean")
    print(json.dumps(out))


def ctl_against(other, steps, warmup, repeats):
    from hsimae_amd import _lib
    libs = {"this": _lib.LIB_PATH, "other": os.path.abspath(other)}
    times = {k: {"step_ctl_ms": [], "norm_and_step_ctl_ms": []} for k in libs}
    for _ in range(repeats):
        for k, path in libs.items():                           # a fresh process per sample: one library per process
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ctl-child", path, "--steps", str(steps), "--warmup",
                                str(warmup)], capture_output=True, text=True, timeout=300)
            if r.returncode:
                raise RuntimeError(f"child for {path} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            got = json.loads(r.stdout.strip().splitlines()[-1])
            for name, t in got.items():
                times[k][name].append(t)
    return {k: {name: summary(t) for name, t in d.items()} for k, d in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ctl-against", default=None)
    ap.add_argument("--ctl-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join("profiles", "optimizer_groups.json"))
    args = ap.parse_args()
    if args.ctl_child:
        ctl_child(args.ctl_child, args.steps, args.warmup)
        return
    res = {}
    if args.ctl_against:                                       # first: this process has not opened the GPU yet
        res["step_ctl_this_library_against_other"] = ctl_against(args.ctl_against, args.steps, args.warmup, args.repeats)
    res.update(measure(args.steps, args.warmup, args.repeats))
    print(json.dumps(res))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
