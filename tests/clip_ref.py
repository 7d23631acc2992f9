"""fp64 restatements and error bounds for csrc/clip.hip (tests/test_gpu_clip.py, tests/test_clip_bound_cpu.py): the global
gradient norm, the control block (clip coefficient, skip decision, bias corrections) and the AdamW step that reads it.

A plain module, not a conftest, in the idiom of elem_ref.py: every restatement is written from the operation's formula in
float64 and an output is accepted when |y - y64| <= bound.  Nothing here is measured; every bound is a worst case:

  sumsq   the kernel squares in fp64 (the square of an fp32 value is exact there) and adds n such squares in fp64 in some fixed
          order: first-order worst case (n - 1) 2^-53 sumsq, taken as n 2^-53 sumsq; the reference (torch's pairwise fp64 sum)
          errs by about log2(n) 2^-53 sumsq, far inside it.
  norm    sqrt halves sumsq's relative error and adds its own 2^-53; one fp32 rounding (2^-24 relative).
  coef    min(1, max_norm / (norm + 1e-6)) in fp64 from the fp64 norm (two more fp64 roundings), one fp32 rounding; the
          minimum with 1 does not stretch an error.
  inv_bc1, inv_sqrt_bc2   fp64 from the fp32 betas and t = step - skipped, one fp32 rounding; pow may err by an ulp or two of
          fp64, which after the division by 1 - beta^t is amplified by beta^t / (1 - beta^t) and still far below fp32's.
  step    elem_ref.adamw_ref fed g * coef.  The multiply is one more fp32 rounding of the gradient, 2^-24 |g coef|, which
          reaches m as (1 - b1) of it, v as 2 |g coef| (1 - b2) of it and p through both; and the device computes the two
          bias-correction factors itself (the plain launcher gets them from the host): one fp32 ulp (2^-23) of slack on each,
          which reaches p as that fraction of the update.
"""
import math

import numpy as np
import torch

from elem_ref import Out, gen, skew, adamw_ref, adamw_inputs, ADAMW_HP, U  # noqa: F401  (re-exported for the two test files)

GRID = 1024                       # HSIMAE_CLIP_GRID
NORM_N_FULL = 4 * 256 * GRID + 4 * 37 + 3      # a full pass of the grid, a partial one, then a tail of 3
NORM_N = [1, 3, 4, 5, 255, 1021, NORM_N_FULL]
STEP_N = 4 * (256 + 37) + 3       # more than one workgroup of float4, a partial one, a tail of 3
E53 = 2.0 ** -53


def f32(a):
    return float(np.float32(a))


def counted(g, group):
    return torch.ones_like(g, dtype=torch.bool) if group is None else group != 2


def sumsq_ref(segs):
    """segs: [(g fp32 tensor, group uint8 tensor or None)] -> (sumsq, n counted, bound)."""
    s, n = 0.0, 0
    for g, group in segs:
        c = counted(g, group)
        with np.errstate(all="ignore"):
            s += float((g[c].double() ** 2).sum())
        n += int(c.sum())
    bound = n * E53 * s if math.isfinite(s) else 0.0
    return s, n, bound


def bias_corrections(t, b1, b2):
    """(1 / (1 - b1^t), 1 / sqrt(1 - b2^t)) in fp64 from the fp32 betas; t = 0 (a skipped first step) divides by zero as the
    device does: +inf."""
    b1, b2 = f32(b1), f32(b2)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return (1.0 / bc1 if bc1 > 0 else math.inf), (1.0 / math.sqrt(bc2) if bc2 > 0 else math.inf)


def ctl_ref(sumsq, n, max_norm, skip_nonfinite, step, skipped_before, b1, b2, norm_max_before=0.0):
    """The control block after hsimae_grad_norm.  Plain values for the exact fields (finite, apply, skipped, t), an Out with
    its bound for every floating-point one."""
    max_norm = f32(max_norm)
    finite = int(math.isfinite(sumsq))
    apply_ = int(not (skip_nonfinite and not finite))
    skipped = skipped_before + (1 - apply_)
    t = step - skipped
    rel = n * E53 / 2 + 4 * E53                              # of the fp64 norm; + 1e-6 and the division: 2 more roundings
    if finite:
        norm = math.sqrt(sumsq)
        c = max_norm / (norm + 1e-6)
        coef = 1.0 if c > 1.0 else c
        norm_max = max(f32(norm_max_before), f32(norm))
    else:
        norm = sumsq if math.isnan(sumsq) else math.inf
        coef = math.nan if math.isnan(norm) or math.isinf(max_norm) else 0.0     # x / inf = 0, inf / inf = NaN
        norm_max = f32(norm_max_before)
    i1, i2 = bias_corrections(t, b1, b2)
    out = dict(finite=finite, apply=apply_, skipped=skipped, t=t, norm_value=norm, coef_value=f32(coef) if finite else coef)
    out["sumsq"] = Out(sumsq, fixed=n * E53 * sumsq if finite else 0.0)
    out["norm"] = Out(norm, fixed=abs(norm) * (U + rel) if finite else 0.0)
    out["coef"] = Out(coef, fixed=abs(coef) * (U + rel) if finite else 0.0)
    out["norm_max"] = Out(norm_max, fixed=abs(norm_max) * (U + rel))
    out["inv_bc1"] = Out(i1, fixed=abs(i1) * (U + 64 * E53) if math.isfinite(i1) else 0.0)
    out["inv_sqrt_bc2"] = Out(i2, fixed=abs(i2) * (U + 64 * E53) if math.isfinite(i2) else 0.0)
    return out


def same_nonfinite(got, ref):
    """A non-finite reference (norm or coef of a non-finite sum) is met exactly: the same infinity, or a NaN."""
    return (math.isnan(got) and math.isnan(ref)) or got == ref


def adamw_ctl_ref(p, g, m, v, group, coef, apply_, t, lr, b1, b2, eps, wd):
    """hsimae_adamw_step_ctl: `coef` is the fp32 coefficient the step reads, t = step - skipped.  apply = 0: nothing moves."""
    if not apply_:
        return {k: Out(a.double()) for k, a in (("p", p), ("m", m), ("v", v))}
    frozen = group == 2
    gc = torch.where(frozen, torch.zeros_like(g, dtype=torch.float64), g.double() * float(coef))
    ref = adamw_ref(p, gc, m, v, group, t, lr, b1, b2, eps, wd)
    lr_, b1_, b2_, eps_ = f32(lr), f32(b1), f32(b2), f32(eps)
    i1, i2 = bias_corrections(t, b1, b2)
    i1, i2 = f32(i1), f32(i2)
    mn, vn = ref["m"].ref, ref["v"].ref
    den = torch.sqrt(vn) * i2 + eps_
    xm = gc.abs() * (1 - b1_)                                  # the multiply's rounding, as it reaches m
    xv = 2 * gc * gc * (1 - b2_)                               # ... and v (relative to v' at most 2: the root halves it)
    xp = lr_ * i1 / den * (xm + 2 * mn.abs() + 4 * mn.abs())   # through m, through v's root, and 2^-23 on each bias correction
    zero = torch.zeros_like(gc)
    return {"p": Out(ref["p"].ref, "C_ADAM", ref["p"].term + torch.where(frozen, zero, xp)),
            "m": Out(mn, "C_ADAM", ref["m"].term + torch.where(frozen, zero, xm)),
            "v": Out(vn, "C_ADAM", ref["v"].term + torch.where(frozen, zero, xv))}


def uniform_group(n, gid):
    return torch.full((n,), gid, dtype=torch.uint8)


def norm_segment(n, seed, with_group):
    """One segment: skewed gradients; with a group, NaN under every id-2 element (about a third of them)."""
    g_ = gen(seed)
    g = skew((n,), g_, 0.01, 0.05)
    group = None
    if with_group:
        group = torch.randint(0, 3, (n,), generator=g_, dtype=torch.uint8)
        g[group == 2] = float("nan")
    return g, group
