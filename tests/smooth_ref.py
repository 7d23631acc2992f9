"""fp64 restatement and element-wise error bounds for csrc/smooth.hip (tests/test_gpu_smooth.py, tests/test_smooth_bound_cpu.py):
the joint bilateral filter over a scene's class-probability maps, and the label, confidence and margin of the filtered maps.

A plain module, not a conftest.  The bounds are worst-case first-order bounds of what the kernel rounds, nothing is tuned on a
GPU result.  The kernel's sequence, per output pixel i that has a row (every operation fp32, U = 2^-24):

  for dy = -r .. r, for dx = -r .. r, j = i + (dy, dx); a tap outside the scene or without a row is skipped
    d_g   = fl(fl(I_j,g - I_i,g) * scale_g)          two roundings: 2 U |d_g|, so 4 U on d_g^2
    d2    = fmaf(d_g, d_g, d2), g = 0 .. G - 1        one rounding each, all terms >= 0: (4 + G) U d2
    arg   = fmaf(a_r, d2, fl(a_s (dy^2 + dx^2)))      the product's rounding (U on the spatial share) and the fmaf's (U arg):
            |darg| <= ARGK U arg, ARGK = 5 + G with the range term (its share carries (4 + G) U + U, the spatial share 2 U), 1
            without it (one product).  a_s, a_r and scale_g are the fp32 values the kernel is given: the restatement reads them.
    w     = exp2(-arg)                                d(2^-x) = ln 2 2^-x dx; v_exp_f32 1 ulp (2 U, the form of knn_ref.py's
            vote weights)                             => |dw| <= BW = w (ln 2 ARGK arg + 2) U + TINY (flushed denormals)
    wsum  = fl(wsum + w)                              T taps added in order => BWS = sum BW + (T - 1) U wsum
    acc_c = fmaf(w, p_j,c, acc_c)                     one rounding per tap => BA_c = sum BW |p_j,c| + T U sum w |p_j,c|
  out_c = fl(acc_c * fl(1 / wsum))                    the reciprocal (U) and the product (U)
          => |dout_c| <= B_c = BA_c / wsum + |out_c| (BWS / wsum + 2 U) + TINY
  The centre tap has arg = 0 and w = 1 exactly, so wsum >= 1.  T <= (2 r + 1)^2 is the number of taps not skipped.
  conf = out[label] (that entry's bound), margin = out[label] - the largest other (the sum of the two entries' bounds).
  Columns below `first` are exact zeros (bound 0).
The label is an argmax over rounded values: it must equal the restatement's wherever the restatement's top-two gap exceeds
twice the sum of the two entries' bounds (`decided`).
"""
import ctypes
import math

import numpy as np

from cls_ref import TINY, U, ratio  # noqa: F401  (re-exported for the tests)
from knn_ref import header_fields  # noqa: F401
from prob_ref import products

F32 = np.float32
LN2 = math.log(2.0)
LOG2E = math.log2(math.e)


def coef(sigma):
    """fp32(log2 e / (2 sigma^2)) as a Python float, 0 for sigma None: what EdgeFilter hands the kernel."""
    return 0.0 if sigma is None else float(F32(LOG2E / (2.0 * float(sigma) ** 2)))


def rows_map(H, W, n, row_of):
    """int64 [H, W]: the row of probs behind every pixel, -1 where it has none (row_of None: row = pixel, below n)."""
    r = np.arange(H * W, dtype=np.int64) if row_of is None else np.asarray(row_of, np.int64).copy()
    r[(r < 0) | (r >= n)] = -1
    return r.reshape(H, W)


def _shift(a, dy, dx, r):
    """a padded by r on both scene axes -> the [H, W, ..] view at offset (dy, dx)."""
    H, W = a.shape[0] - 2 * r, a.shape[1] - 2 * r
    return a[r + dy:r + dy + H, r + dx:r + dx + W]


def _pad(a, r, value=0):
    return np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2), constant_values=value)


def filter_ref(probs, C, first, H, W, row_of, guide, scale, radius, a_s, a_r):
    """probs fp32 [n, ld], row_of int32 [H W] or None, guide fp32 [H, W, G] and scale fp32 [G] (both None with a_r = 0), a_s and
    a_r the fp32 coefficients as Python floats -> dict of fp64 results per PIXEL: out, bound [H W, C]; has [H W] bool (the pixel
    has a row); label; conf, conf_bound, margin, margin_bound at that label; decided; taps [H W] (T); row [H W]."""
    probs = np.asarray(probs)
    n, r = probs.shape[0], radius
    rows = rows_map(H, W, n, row_of)
    has = rows >= 0
    K = C - first
    P = np.zeros((H, W, K))
    P[has] = probs[rows[has], first:C].astype(np.float64)
    ranged = a_r != 0
    Pp, hp = _pad(P, r), _pad(has, r, False)
    if ranged:
        I = np.where(has[..., None], np.asarray(guide).astype(np.float64), 0.0)          # never read where there is no row
        Ip, sc = _pad(I, r), np.asarray(scale).astype(np.float64)
        G = I.shape[2]
    argk = 5 + G if ranged else 1
    acc, accb = np.zeros((H, W, K)), np.zeros((H, W, K))
    absacc = np.zeros((H, W, K))
    wsum, wsb, taps = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ok = _shift(hp, dy, dx, r) & has
                arg = np.full((H, W), float(a_s) * (dy * dy + dx * dx))
                if ranged:
                    d = (_shift(Ip, dy, dx, r) - I) * sc
                    arg = arg + float(a_r) * (d * d).sum(2)
                w = np.where(ok, np.exp2(-arg), 0.0)
                bw = np.where(ok, w * (LN2 * argk * arg + 2) * U + TINY, 0.0)
                pj = _shift(Pp, dy, dx, r)
                wsum += w
                wsb += bw
                taps += ok
                acc += w[..., None] * pj
                absacc += w[..., None] * np.abs(pj)
                accb += bw[..., None] * np.abs(pj)
        wsb = wsb + np.maximum(taps - 1, 0) * U * wsum
        accb = accb + taps[..., None] * U * absacc
        ws = np.where(has, wsum, 1.0)
        o = acc / ws[..., None]
        b = accb / ws[..., None] + np.abs(o) * (wsb / ws + 2 * U)[..., None] + TINY
    out, bound = np.zeros((H * W, C)), np.zeros((H * W, C))
    out[:, first:], bound[:, first:] = o.reshape(H * W, K), np.where(np.isnan(b), 0.0, b).reshape(H * W, K)
    out[~has.reshape(-1)], bound[~has.reshape(-1)] = 0.0, 0.0
    label = first + np.argmax(out[:, first:], axis=1)
    if K == 1:
        decided = np.ones(H * W, bool)
    else:
        two = np.argsort(-np.where(np.isnan(out[:, first:]), np.inf, out[:, first:]), axis=1, kind="stable")[:, :2] + first
        px = np.arange(H * W)
        gap = out[px, two[:, 0]] - out[px, two[:, 1]]
        decided = gap > 2 * (bound[px, two[:, 0]] + bound[px, two[:, 1]])
    conf, cb, margin, mb = products(out, bound, label, first)
    return {"out": out, "bound": bound, "has": has.reshape(-1), "label": label.astype(np.int64), "conf": conf, "conf_bound": cb,
            "margin": margin, "margin_bound": mb, "decided": decided | ~has.reshape(-1), "taps": taps.reshape(-1),
            "row": rows.reshape(-1), "gap": gap if K > 1 else None}


# ------------------------------------------------------------------ the kernel's sequence in exactly rounded fp32
def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 is exact in fp64; the sum is rounded to fp64, then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


FAULTS = ["reflect", "divide_by_count", "unsquared", "rowless_counted", "scale_ignored", "swap_dydx", "runner_up_with_winner"]


def emulate(probs, C, first, H, W, row_of, guide, scale, radius, a_s, a_r, fault=None):
    """The kernel's operation sequence with every fp32 operation rounded exactly (exp2 evaluated in fp64 and rounded once)
    -> (out fp32 [H W, C], label, conf, margin) per pixel, zeros where the pixel has no row.  `fault` plants one defect
    (tests/test_smooth_bound_cpu.py)."""
    probs = np.asarray(probs, F32)
    n, r = probs.shape[0], radius
    rows = rows_map(H, W, n, row_of)
    has = rows >= 0
    K = C - first
    P = np.zeros((H, W, K), F32)
    P[has] = probs[rows[has], first:C]
    ranged = a_r != 0
    mode = "symmetric" if fault in ("reflect", "swap_dydx") else "constant"      # what an out-of-scene read would fetch
    pad2, pad3 = ((r, r), (r, r)), ((r, r), (r, r), (0, 0))
    Pp = np.pad(P, pad3, mode=mode)
    hp = np.pad(has, pad2, mode="symmetric") if fault == "reflect" else _pad(has, r, False)
    if fault == "swap_dydx":
        hin = _pad(np.ones((H, W), bool), r, False)                              # the in-scene test proper
        hp_any = np.pad(has, pad2, mode="symmetric")
    if ranged:
        I = np.where(has[..., None], np.asarray(guide, F32), F32(0))
        Ip = np.pad(I, pad3, mode=mode)
        sc = np.ones_like(np.asarray(scale, F32)) if fault == "scale_ignored" else np.asarray(scale, F32)
        G = I.shape[2]
    acc = np.zeros((H, W, K), F32)
    wsum, cnt = np.zeros((H, W), F32), np.zeros((H, W), F32)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if fault == "swap_dydx":                                         # the bounds test takes dx for dy
                    ok = _shift(hin, dx, dy, r) & _shift(hp_any, dy, dx, r) & has
                elif fault == "rowless_counted":
                    ok = _shift(_pad(np.ones((H, W), bool), r, False), dy, dx, r) & has
                else:
                    ok = _shift(hp, dy, dx, r) & has
                arg = np.full((H, W), F32(a_s) * F32(dy * dy + dx * dx), F32)
                if ranged:
                    d2 = np.zeros((H, W), F32)
                    Ij = _shift(Ip, dy, dx, r)
                    for g in range(G):
                        d = (Ij[..., g] - I[..., g]) * sc[g]
                        d2 = d2 + np.abs(d) if fault == "unsquared" else _fma(d, d, d2)
                    arg = _fma(np.full((H, W), F32(a_r)), d2, arg)
                w = np.exp2(-arg.astype(np.float64)).astype(F32)
                wsum = np.where(ok, wsum + w, wsum)
                cnt = np.where(ok, cnt + F32(1), cnt)
                acc = np.where(ok[..., None], _fma(np.broadcast_to(w[..., None], acc.shape), _shift(Pp, dy, dx, r), acc), acc)
        inv = F32(1) / np.where(has, cnt if fault == "divide_by_count" else wsum, F32(1))
        o = acc * inv[..., None]
    out = np.zeros((H * W, C), F32)
    out[:, first:] = o.reshape(H * W, K)
    out[~has.reshape(-1)] = 0
    label = first + np.argmax(out[:, first:], axis=1)
    px = np.arange(H * W)
    conf = out[px, label]
    other = out.copy()
    other[:, :first] = -np.inf
    if fault != "runner_up_with_winner":
        other[px, label] = -np.inf
    with np.errstate(all="ignore"):
        second = np.where(np.isnan(other), F32(-np.inf), other).max(1)
        margin = conf.copy() if K == 1 else conf - second
    return out, label.astype(np.int64), conf, np.where(has.reshape(-1), margin, F32(0))


def worst(got, ref, first):
    """got = (out, label, conf, margin) per pixel of the code under test -> dict of the worst err / bound of out, conf and
    margin over the pixels that have a row (the two taken at got's own label), `wrong` = pixels whose label differs although
    it is determined, `open` = the share of the pixels with a row that the label rule leaves undetermined."""
    out, label, conf, margin = got
    has = ref["has"]
    C = ref["out"].shape[1]
    label = np.asarray(label, np.int64)
    ok = (label >= first) & (label < C)
    lab = np.where(ok & has, label, first)
    rc, rcb, rm, rmb = products(ref["out"], ref["bound"], lab, first)
    res = {"out": ratio(np.asarray(out)[has], ref["out"][has], ref["bound"][has]), "conf": ratio(np.asarray(conf)[has], rc[has], rcb[has]),
           "margin": ratio(np.asarray(margin)[has], rm[has], rmb[has]),
           "wrong": int(np.sum(has & (~ok | (ref["decided"] & (label != ref["label"]))))),
           "open": float(np.sum(~ref["decided"] & has)) / max(1, int(has.sum())),
           "zeros": bool(np.all(np.asarray(out)[has][:, :first] == 0))}
    res["all"] = np.inf if res["wrong"] or not res["zeros"] else max(res["out"], res["conf"], res["margin"])
    return res


# ------------------------------------------------------------------ cases
SIGMA_S, SIGMA_R = 3.0, 0.2
# (H, W, radius, C, first, G (0: a_r = 0 and a NULL guide), form).  Every scene size, radius, class layout, guide width and row
# form of the issue, and radius 2 and 4, whose tile-row pairing (csrc/smooth.hip, "LDS banks") differs from 1, 3 and 8.
# form: "null" row_of NULL, tight ldp / ldo; "padded" row_of NULL, ldp = C + 3, ldo = C + 5; "short" row_of NULL and n = H W - 5;
# "subset" a permuted subset with holes (the tile corners, one whole row) and rows that no pixel points to, ldp = C + 3, ldo = C + 1.
CASES = [
    (1, 1, 1, 2, 0, 1, "null"), (1, 1, 8, 16, 1, 3, "padded"), (1, 7, 3, 17, 1, 4, "null"), (1, 7, 8, 2, 0, 0, "subset"),
    (3, 2, 1, 18, 1, 1, "padded"), (3, 2, 8, 16, 1, 3, "subset"), (15, 17, 3, 16, 1, 1, "subset"), (15, 17, 1, 64, 1, 4, "short"),
    (16, 16, 3, 17, 1, 3, "padded"), (16, 16, 8, 2, 0, 1, "null"), (17, 33, 1, 16, 1, 0, "padded"), (17, 33, 3, 18, 1, 4, "subset"),
    (17, 33, 8, 17, 1, 1, "null"), (40, 37, 3, 17, 1, 1, "subset"), (40, 37, 8, 64, 1, 3, "padded"), (40, 37, 1, 2, 0, 4, "null"),
    (70, 50, 3, 18, 1, 3, "subset"), (70, 50, 8, 16, 1, 1, "null"), (33, 29, 2, 9, 1, 1, "subset"), (24, 24, 4, 17, 1, 3, "null"),
]


def case_id(c):
    return "%dx%d-r%d-C%d-f%d-G%d-%s" % c


def make_case(H, W, radius, C, first, G, form, seed=0):
    """-> dict of the kernel's inputs (numpy): probs fp32 [n, ldp] = softmax over [first, C) of N(0, 2^2) logits, NaN in the
    columns below `first`, in the pad columns and in the rows no pixel points to; row_of int32 [H W] or None; guide fp32
    [H, W, G] (NaN at pixels without a row) and scale fp32 [G] (a constant channel with scale 0 when G = 3), or None."""
    rng = np.random.RandomState(1000003 * seed + 7919 * H + 104729 * W + 31 * radius + 1009 * C + first + 17 * G + len(form))
    HW = H * W
    ldp, ldo = {"null": (C, C), "padded": (C + 3, C + 5), "short": (C, C), "subset": (C + 3, C + 1)}[form]
    if form == "subset":
        hole = rng.rand(H, W) < 0.15
        for cy, cx in ((15, 15), (15, 16), (16, 15), (16, 16), (0, 0)):
            if cy < H and cx < W and HW > 1:
                hole[cy, cx] = True
        if H >= 3:
            hole[H // 2] = True
        if hole.all():
            hole[-1, -1] = False
        pix = np.flatnonzero(~hole.reshape(-1))
        pix = pix[rng.permutation(pix.size)]
        n = pix.size + 3                                     # three rows that no pixel points to
        slots = rng.permutation(n)[:pix.size]
        row_of = np.full(HW, -1, np.int32)
        row_of[pix] = slots.astype(np.int32)
        row_of[np.flatnonzero(hole.reshape(-1))[::2]] = -7   # any negative value means "no row"
    else:
        n = HW - 5 if form == "short" and HW > 5 else HW
        row_of = None
    z = 2.0 * rng.standard_normal((n, C - first))
    e = np.exp(z - z.max(1, keepdims=True))
    probs = np.full((n, ldp), np.nan, F32)
    probs[:, first:C] = (e / e.sum(1, keepdims=True)).astype(F32)
    rows = rows_map(H, W, n, row_of).reshape(-1)
    used = np.zeros(n, bool)
    used[rows[rows >= 0]] = True
    probs[~used] = np.nan
    guide = scale = None
    if G:
        guide = (100.0 + 50.0 * rng.standard_normal((H, W, G))).astype(F32)
        if G == 3:
            guide[..., 1] = F32(7.5)
        span = guide.reshape(HW, G).max(0) - guide.reshape(HW, G).min(0)
        with np.errstate(all="ignore"):
            scale = np.where(span > 0, F32(1) / span, F32(0)).astype(F32)
        guide.reshape(HW, G)[rows < 0] = np.nan
    return {"probs": probs, "ldp": ldp, "ldo": ldo, "n": n, "row_of": row_of, "guide": guide, "scale": scale,
            "a_s": coef(SIGMA_S), "a_r": coef(SIGMA_R) if G else 0.0}


def case_ref(c, case):
    H, W, radius, C, first, G, form = c
    return filter_ref(case["probs"], C, first, H, W, case["row_of"], case["guide"], case["scale"], radius, case["a_s"], case["a_r"])


# ------------------------------------------------------------------ the planted scene
def planted_scene(seed=0):
    """48 x 40, five classes (labels 1 .. 5 of six columns, first = 1): four quadrants and a centred 16 x 16 block.  The guide
    is the class level / 4 + N(0, 0.01); a quarter of the pixels carry a wrong winning class (0.6 against 0.1 for the others,
    plus small noise, renormalised).  -> dict: truth int64 [H W], probs fp32 [H W, 6], guide fp32 [H, W, 1], scale fp32 [1]."""
    H, W, K = 48, 40, 5
    rng = np.random.RandomState(2014 + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    level = (yy >= H // 2) * 2 + (xx >= W // 2)
    level[(yy >= 16) & (yy < 32) & (xx >= 12) & (xx < 28)] = 4
    truth = level.reshape(-1)
    guide = (level / 4.0 + 0.01 * rng.standard_normal((H, W)))[..., None].astype(F32)
    win = truth.copy()
    wrong = rng.permutation(H * W)[:H * W // 4]
    win[wrong] = (truth[wrong] + 1 + rng.randint(0, K - 1, wrong.size)) % K
    p = np.full((H * W, K), 0.1)
    p[np.arange(H * W), win] = 0.6
    p = p + 0.01 * rng.rand(H * W, K)
    probs = np.zeros((H * W, K + 1), F32)
    probs[:, 1:] = (p / p.sum(1, keepdims=True)).astype(F32)
    span = guide.max() - guide.min()
    return {"H": H, "W": W, "C": K + 1, "first": 1, "truth": (truth + 1).astype(np.int64), "probs": probs, "guide": guide,
            "scale": np.array([F32(1) / F32(span)], F32)}


def oa(label, truth):
    return float(np.mean(np.asarray(label).reshape(-1) == np.asarray(truth).reshape(-1)))


# ------------------------------------------------------------------ the ABI
def refusals(lib, _lib):
    """(what, code returned, code expected) of every refusal: all are decided before anything is launched."""
    ok = dict(probs=1 << 20, ldp=16, n=4, C=10, first=1, H=2, W=2, row_of=1 << 21, guide=1 << 22, G=1, guide_scale=1 << 23, radius=3,
              a_s=0.08, a_r=18.0, out_probs=1 << 24, ldo=16, label_map=1 << 25, conf_map=1 << 26, margin_map=1 << 27)
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    nan, inf = float("nan"), float("inf")
    table = [(dict(H=0), E_DIMS), (dict(W=-1), E_DIMS), (dict(H=1 << 16, W=1 << 15), E_DIMS), (dict(n=-1), E_DIMS),
             (dict(C=1, first=0), E_DIMS), (dict(first=-1), E_DIMS), (dict(first=10), E_DIMS), (dict(ldp=9), E_DIMS),
             (dict(ldo=9), E_DIMS), (dict(G=0), E_DIMS), (dict(G=5), E_DIMS), (dict(radius=0), E_DIMS), (dict(radius=9), E_DIMS),
             (dict(a_s=-1.0), E_DIMS), (dict(a_s=nan), E_DIMS), (dict(a_s=inf), E_DIMS), (dict(a_r=-1.0), E_DIMS),
             (dict(a_r=nan), E_DIMS), (dict(a_r=inf), E_DIMS),
             (dict(out_probs=1 << 20), E_DIMS), (dict(out_probs=(1 << 20) + 64), E_DIMS), (dict(out_probs=(1 << 20) - 64), E_DIMS),
             (dict(C=1025, ldp=1040, ldo=1040), E_UNSUPPORTED), (dict(H=1, W=(1 << 20) + 1), E_UNSUPPORTED),
             (dict(probs=None), E_NULL), (dict(label_map=None), E_NULL), (dict(guide=None), E_NULL), (dict(guide_scale=None), E_NULL),
             (dict(probs=(1 << 20) + 2), E_ALIGN), (dict(row_of=(1 << 21) + 2), E_ALIGN), (dict(guide=(1 << 22) + 1), E_ALIGN),
             (dict(guide_scale=(1 << 23) + 2), E_ALIGN), (dict(out_probs=(1 << 24) + 3), E_ALIGN),
             (dict(label_map=(1 << 25) + 4), E_ALIGN), (dict(conf_map=(1 << 26) + 2), E_ALIGN), (dict(margin_map=(1 << 27) + 2), E_ALIGN),
             (dict(n=0), 0), (dict(n=0, a_r=0.0, guide=None, guide_scale=None, row_of=None, out_probs=None, conf_map=None,
                                   margin_map=None), 0)]
    out = [("params NULL", lib.hsimae_prob_filter(None, None), E_NULL)]
    for kw, want in table:
        a = dict(ok)
        a.update(kw)
        out.append((str(kw), lib.hsimae_prob_filter(ctypes.byref(_lib.ProbFilterParams(**a)), None), want))
    return out
