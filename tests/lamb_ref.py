"""fp64 restatement and error bound for the LAMB step of csrc/lamb.hip (hsimae_lamb_step; tests/test_gpu_lamb.py,
tests/test_lamb_bound_cpu.py), and the inputs both test files share.

A plain module, not a conftest, in the idiom of clip_ref.py / groups_ref.py.  Nothing here is measured; every bound is a first-order
worst case, in units of U = 2^-24 (the constant C_ADAM = 1 of elem_ref.py, whose terms count every rounding):

  m, v    clip_ref.adamw_ctl_ref's terms: elem_ref.adamw_ref's (2 |gc - m| (1 - b1) + |m'|;  |v| b2 + 2 gc^2 (1 - b2) + |v'|) plus the
          rounding of the multiply g * coef as it reaches them (|gc| (1 - b1);  2 gc^2 (1 - b2)).
  u       u = (m' inv_bc1) / (sqrt(v') inv_sqrt_bc2 + eps) [+ wd p].  Adam's part ua inherits m's error scaled by inv_bc1 / denom
          and carries 14 |m'| inv_bc1 / denom more, exactly clip_ref's count for the same expression (8: the denominator's root,
          scaling, + eps and v's own error; 2: g * coef through v's root; 4: one fp32 ulp on each bias correction, which the device
          forms itself) and 2 |ua| for the multiply by inv_bc1 and the division, which AdamW's form has folded into lr inv_bc1.
          With decay: 2 |wd p| (the product, and wd's own rounding is none: it is an fp32 input) + |u| (the addition).
          tu = inv_bc1 / denom (tm + 14 |m'|) + 2 |ua| + [2 |wd p| + |u|].
  r       r = sqrt(Sp / Su), Sp = sum p^2, Su = sum u^2 over the tensor, both formed in fp64 from fp32 values: squares exact,
          n additions each, n 2^-53 relative.  The u_i that enter Su are the fp32 ones: dSu <= 2 U sum |u_i| tu_i.  The root
          halves the relative error of the quotient; the division and the root add 2^-53 each, the final rounding U:
          delta_r = U sum |u_i| tu_i / Su + n 2^-53 + 4 2^-53 + U.   A ratio that the conditions force (1: not adapted, a zero
          norm, frozen) is exact; one that trust_clip cuts by more than delta_r is exactly trust_clip.
  p       p' = p - (lr r) u:  lr r tu (u's error; the apply kernel recomputes u, any contraction of its multiply-adds removes
          roundings that tu counts) + |lr r u| (2 + delta_r / U) (the products lr * r and (lr r) * u, and r's error) + |p'|.
  frozen  id 2 and every id >= ngroups: reference = input, bound 0, ratio exactly 1.
"""
import math

import torch

import clip_ref as R
from clip_ref import Out, f32, gen, skew, U  # noqa: F401  (re-exported for the two test files)

CHUNK = 4096                      # HSIMAE_LAMB_CHUNK
E53 = 2.0 ** -53
HP = dict(b1=0.9, b2=0.999, eps=1e-6)
T_STEP = 2                        # the step of the bias corrections in the ABI tests
# ids 0 / 1 as FusedAdamW knows them (decay / no decay), the hole at 2, then a slower decayed and a faster undecayed group
TABLE = [(1e-3, 0.05), (1e-3, 0.0), (-1.0, float("nan")), (5e-4, 0.05), (2e-3, 0.0)]
DEAD_ID = 200                     # an id >= ngroups

LIST_A = [1, 3, 4, 5, 7, 64, 255, 4095, 4096, 4097, 8193]
LIST_B = [1, 64 * CHUNK + 5, 1]
LIST_C = [1 + k % 9 for k in range(700)]


def tensors_of(sizes):
    """[(off, n)] packed without padding."""
    out, off = [], 0
    for n in sizes:
        out.append((off, n))
        off += n
    return out


def chunk_table(tensors):
    """The test side's own restatement of the chunk table: [(off, n, chunk0)], nchunks."""
    rows, c = [], 0
    for off, n in tensors:
        rows.append((off, n, c))
        c += -(-n // CHUNK)
    return rows, c


def lamb_ref(p, g, m, v, tensors, ids, table, coef, apply_, t, b1, b2, eps, trust_clip, always_adapt, ratios=None):
    """hsimae_lamb_step.  tensors: [(off, n)]; ids: one byte per element (a tensor's id is its first element's); table:
    [(lr, weight_decay)]; coef: the fp32 coefficient the step reads; t: the step of the bias corrections; trust_clip: None or
    <= 0 for none; ratios: forces every tensor's ratio (a list, or one number).  p, g, m, v: fp32 tensors, or fp64 ones when a
    trajectory is carried in fp64.  Returns Out objects for p, m, v and r (one ratio per tensor) and the list delta_r."""
    ng = len(table)
    ref = {k: a.double().clone() for k, a in (("p", p), ("m", m), ("v", v))}
    term = {k: torch.zeros_like(a) for k, a in ref.items()}
    nt = len(tensors)
    r_ref, r_bound, delta = torch.ones(nt, dtype=torch.float64), torch.zeros(nt, dtype=torch.float64), [0.0] * nt
    if apply_:
        b1_, b2_, eps_, coef_ = f32(b1), f32(b2), f32(eps), f32(coef)
        i1, i2 = (f32(a) for a in R.bias_corrections(t, b1, b2))
        clip = None if trust_clip is None or not trust_clip > 0 else f32(trust_clip)
        for T, (off, n) in enumerate(tensors):
            if n == 0:
                continue
            k = int(ids[off])
            if k == 2 or k >= ng:
                continue
            lr, wd = f32(table[k][0]), f32(table[k][1])
            sl = slice(off, off + n)
            pe, ge, me, ve = (a[sl].double() for a in (p, g, m, v))
            gc = ge * coef_
            mn = me + (gc - me) * (1 - b1_)
            vn = ve * b2_ + gc * gc * (1 - b2_)
            den = torch.sqrt(vn) * i2 + eps_
            ua = mn * i1 / den
            u = ua + wd * pe if wd != 0.0 else ua
            tm = 2 * (gc - me).abs() * (1 - b1_) + mn.abs() + gc.abs() * (1 - b1_)
            tv = ve.abs() * b2_ + 4 * gc * gc * (1 - b2_) + vn.abs()
            tu = i1 / den * (tm + 14 * mn.abs()) + 2 * ua.abs()
            if wd != 0.0:
                tu = tu + 2 * (wd * pe).abs() + u.abs()
            sp, su = float((pe * pe).sum()), float((u * u).sum())
            r, dr, rb = 1.0, 0.0, 0.0
            if ratios is not None:
                r = float(ratios[T]) if hasattr(ratios, "__len__") else float(ratios)
            elif (wd != 0.0 or always_adapt) and sp > 0.0 and su > 0.0:
                raw = math.sqrt(sp / su)
                dr = U * float((u.abs() * tu).sum()) / su + (n + 4) * E53 + U
                if clip is not None and raw * (1 - dr) > clip:
                    r, dr = clip, 0.0                          # cut whatever the rounding did
                else:
                    r = raw if clip is None else min(raw, clip)
                    rb = r * dr
            step = lr * r
            pn = pe - step * u
            tp = step * tu + (step * u).abs() * (2 + dr / U) + pn.abs()
            ref["p"][sl], ref["m"][sl], ref["v"][sl] = pn, mn, vn
            term["p"][sl], term["m"][sl], term["v"][sl] = tp, tm, tv
            r_ref[T], r_bound[T], delta[T] = r, rb, dr
    out = {k: Out(ref[k], "C_ADAM", term[k]) for k in "pmv"}
    out["r"] = Out(r_ref, fixed=r_bound)
    out["delta_r"] = delta
    return out


# ------------------------------------------------------------------------------------------------ inputs
SCALES = (0.03, 0.3, 30.0)       # the weights' scale per tensor: 1000 x apart, so the ratios fall on both sides of 1 at every step count


def inputs(sizes, seed, plants=None, scales=SCALES, live_ids=(0, 1, 3, 4)):
    """p, g, m, v over tensors of `sizes` packed without padding, ids per whole tensor cycling over the live table entries, the
    weights' scale cycling over `scales`.  plants: {tensor index: kind} with kind in
      "zero_w"   all-zero weights (ratio 1, still stepped)
      "zero_u"   zero gradient and moments under id 1 (no decay): u = 0, ratio 1, p bit-unchanged
      "frozen"   id 2, its gradient NaN
      "dead"     an id >= ngroups, its gradient NaN"""
    g_ = gen(seed)
    tensors = tensors_of(sizes)
    n = sum(sizes)
    p = skew((n,), g_, 0.1, 0.5)
    grad = skew((n,), g_, 0.01, 0.05)
    m = skew((n,), g_, 0.005, 0.02)
    v = (skew((n,), g_, 0.3, 0.5) ** 2 * 1e-3).float()
    ids = torch.zeros(n, dtype=torch.uint8)
    for T, (off, cnt) in enumerate(tensors):
        sl = slice(off, off + cnt)
        p[sl] *= scales[T % len(scales)] / 0.4                # skew(0.1, 0.5) has an rms of about 0.4
        ids[sl] = live_ids[T % len(live_ids)]
        kind = (plants or {}).get(T)
        if kind == "zero_w":
            p[sl] = 0.0
        elif kind == "zero_u":
            grad[sl], m[sl], v[sl], ids[sl] = 0.0, 0.0, 0.0, 1
        elif kind == "frozen":
            grad[sl], ids[sl] = float("nan"), 2
        elif kind == "dead":
            grad[sl], ids[sl] = float("nan"), DEAD_ID
        elif kind is not None:
            raise ValueError(kind)
    return dict(p=p, g=grad, m=m, v=v, ids=ids, tensors=tensors)


# every list with its planted tensors.  A and C plant all four kinds, the frozen one between two live ones; B has one tensor that
# is more than a speck, so each kind is planted on it in turn.
PLANTS_A = {2: "zero_w", 5: "zero_u", 7: "frozen", 9: "dead", 10: None}
PLANTS_C = {4: "zero_w", 250: "zero_u", 399: "frozen", 500: "dead", 699: "frozen"}
CASES = {"A": (LIST_A, PLANTS_A), "C": (LIST_C, PLANTS_C), "B": (LIST_B, {}), "B-zero_w": (LIST_B, {1: "zero_w"}),
         "B-zero_u": (LIST_B, {1: "zero_u"}), "B-frozen": (LIST_B, {1: "frozen"}), "B-dead": (LIST_B, {1: "dead"})}
B_IDS = (1, 0, 3)                 # B's large tensor decays, so it is adapted whatever always_adapt says


def case_inputs(name):
    sizes, plants = CASES[name]
    ids = B_IDS if name.startswith("B") else (0, 1, 3, 4)
    return inputs(sizes, 11 + len(name) + len(sizes), {k: v for k, v in plants.items() if v}, live_ids=ids)


def live_elements(inp, ngroups):
    return (inp["ids"] != 2) & (inp["ids"] < ngroups)
