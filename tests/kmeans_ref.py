"""fp64 restatement and error bounds for csrc/kmeans.hip (tests/test_gpu_kmeans.py, tests/test_kmeans_bound_cpu.py): the
assignment of rows to centroids, the update of the centroids, and a whole Lloyd fit.

A plain module, not a conftest.  The bounds are worst-case first-order bounds of what the kernels round, nothing is tuned on a
GPU result.  U = 2^-24, TINY = 2^-120 absolute (cls_ref.py); U64 = 2^-53.

hsimae_kmeans_assign: x, c and bias are taken as given (fp32).  s64_ik = x_i . c_k - bias_k in fp64.
  dot    = the k-ordered fmaf chain of the fp32 MFMA     |dot - d64| <= bd = gamma_D sum_d |x_id c_kd|, gamma_D = D U / (1 - D U)
           (knn_ref.dots: any summation order, one rounding per product-and-add)
  score  = fl(dot - bias), one rounding                  |score - s64| <= beta = bd + U (|s64| + bd) + TINY
  (the bias is an input here, so it carries no rounding of its own; where it is compared with its fp64 value -- update -- its
   one rounding U |bias| is the bound of that check)
  Checks on EVERY row (check_assign), l = the returned cluster:
  (a) l in range, and nothing clearly better exists: s64[l] + beta[l] >= max_j (s64[j] - beta[j]);
  (b) |score - s64[l]| <= beta[l];
  (c) |margin - (best64 - second64)| <= 2 max_j beta[j]: order statistics are 1-Lipschitz in the sup norm, so this holds
      whichever near-tied centroid won; K = 1: margin is the score, bound beta;
  (d) (exact inputs only: every product and sum is exact in fp32) l = the first argmax of s64, score bit for bit, margin too.
  A NaN score orders below every number; among NaNs the lowest index.

hsimae_kmeans_update, cluster k with n_k members, m = sums / n_k:
  sums   = one fp64 chain in ascending row order: bit for bit np's sequential sum (update_ref adds row by row): the one check
           that sees a sum taken in another order, and only where the sums round (rows of very different magnitude: wide_rows;
           a few fp32 values of one magnitude add exactly in fp64 in any order); against any other fp64 summation |dsum| <= n_k U64 sum |x|
  c      = fl32(sums / n_k)                              |c - m| <= U |m| + n_k U64 mean|x| + TINY           (euclidean)
  cosine: c = normalize32(fl32(m)): knn_ref.normalize_ref's relative bound ((ceil(D / 64) + 6) / 2 + 3) U on the fp32 mean, whose
           own rounding U per element moves the norm by at most U relative and the element by U: + 2 U
  bias   = fl32(0.5 ss), ss the fp64 sum of the squares of the STORED fp32 centroid: U |bias| + D U64 |bias| + TINY
  inertia= sum_i ||x_i - c_old[l_i]||^2 in fp64, all terms >= 0: any order agrees to N D U64 relative; the check asks 1e-12
  empty cluster: centroid and bias keep their bits; a label outside [first, first + K) belongs to no cluster and is counted.
"""
import ctypes
import math

import numpy as np

from cls_ref import TINY, U, ratio  # noqa: F401
from knn_ref import F32, clusters, emulate_normalize, header_fields, normalize_ref  # noqa: F401

U64 = 2.0 ** -53
GRID = 2048
PAST_THE_GRID = GRID * 64 + 1                               # one row tile more than the grid holds workgroups
# (N, K, D): every tail in N, K and D, one-tile and many-tile centroid walks, K = 1, the stride loop
CASES = [(1, 1, 4), (1, 2, 8), (63, 63, 36), (64, 64, 8), (65, 65, 36), (130, 2, 512), (130, 130, 512), (130, 256, 1536), (5, 1024, 36),
         (PAST_THE_GRID, 2, 4)]


# ------------------------------------------------------------------ assign
def scores_ref(x, c, bias, D):
    """-> (s64 [N, K], beta [N, K]); bias None = 0."""
    x64, c64 = np.asarray(x)[:, :D].astype(np.float64), np.asarray(c)[:, :D].astype(np.float64)
    with np.errstate(all="ignore"):
        d = x64 @ c64.T
        bd = (D * U / (1 - D * U)) * (np.abs(x64) @ np.abs(c64).T)
        s = d - (0.0 if bias is None else np.asarray(bias, np.float64)[None, :]) + 0.0
        beta = bd + U * (np.abs(s) + bd) + TINY
    return s, np.where(np.isnan(beta), np.inf, beta)


def _key(s):
    return np.where(np.isnan(s), -np.inf, s)


def assign_ref(s64):
    """-> (label0 [N] = the first argmax, a NaN below every number; best64; second64 (NaN with K = 1 or when all others are NaN))."""
    N, K = s64.shape
    key = _key(s64)
    lab = np.argmax(key, axis=1)
    lab = np.where(np.isnan(s64).all(1), 0, lab)
    r = np.arange(N)
    best = s64[r, lab]
    if K == 1:
        return lab, best, np.full(N, np.nan)
    rest = key.copy()
    rest[r, lab] = -np.inf
    second = rest.max(1)
    return lab, best, np.where(np.isinf(second) & (second < 0), np.nan, second)


def check_assign(labels, score, margin, s64, beta, first, exact=False):
    """labels int64 [N], score / margin fp32 [N] or None -> dict of violation counts of (a) .. (d) and the worst err / bound."""
    labels = np.asarray(labels, np.int64)
    N, K = s64.shape
    r = np.arange(N)
    l = labels - first
    inr = (l >= 0) & (l < K)
    lc = np.where(inr, l, 0)
    lab0, best, second = assign_ref(s64)
    key = _key(s64)
    out = {"a_range": int((~inr).sum())}
    with np.errstate(all="ignore"):
        low = np.where(np.isnan(s64), -np.inf, s64 - beta).max(1)
        own, ownb = s64[r, lc], beta[r, lc]
        allnan = np.isnan(s64).all(1)
        out["a_better_left"] = int((~np.where(allnan, lc == 0, key[r, lc] + ownb >= low)).sum())
        out["b_worst"] = out["c_worst"] = 0.0
        if score is not None:
            sc = np.asarray(score, F32).astype(np.float64)
            err = np.abs(sc - own)
            ok = (err <= ownb) | (np.isnan(sc) & np.isnan(own))
            out["b_score"] = int((~ok).sum())
            rb = np.where(ok & (err > 0), err / ownb, 0.0)
            out["b_worst"] = float(np.nanmax(rb)) if rb.size else 0.0
        if margin is not None:
            mg = np.asarray(margin, F32).astype(np.float64)
            want = best if K == 1 else best - second
            mb = ownb if K == 1 else 2 * np.where(np.isnan(s64), 0.0, beta).max(1)
            err = np.abs(mg - want)
            ok = (err <= mb) | (np.isnan(mg) & np.isnan(want))
            out["c_margin"] = int((~ok).sum())
            rb = np.where(ok & (err > 0), err / mb, 0.0)
            out["c_worst"] = float(np.nanmax(rb)) if rb.size else 0.0
        if exact:
            out["d_label"] = int((l != lab0).sum())
            if score is not None:
                out["d_score"] = int((np.asarray(score, F32).view(np.int32) != best.astype(F32).view(np.int32)).sum())
            if margin is not None:
                want = (best if K == 1 else best - second).astype(F32)
                out["d_margin"] = int((np.asarray(margin, F32).view(np.int32) != want.view(np.int32)).sum())
    out["ok"] = all(v == 0 for k, v in out.items() if not k.endswith("worst"))
    return out


def emulate_assign(x, c, bias, D, first, fault=None):
    """The kernel's sequence in exactly rounded fp32 (the fmaf chain through fp64) -> (labels, score, margin).  `fault` plants
    one defect: bias_sign (dot + bias), bias_no_half (dot - 2 bias: ||c||^2 without the 1/2), tie_higher (equal scores to the
    higher index)."""
    xx, cc = np.asarray(x, F32)[:, :D].astype(np.float64), np.asarray(c, F32)[:, :D].astype(np.float64)
    s = np.zeros((xx.shape[0], cc.shape[0]), F32)
    with np.errstate(all="ignore"):
        for d in range(D):
            s = (xx[:, d:d + 1] * cc[None, :, d] + s.astype(np.float64)).astype(F32)
        if bias is not None:
            b = np.asarray(bias, F32)[None, :]
            s = s + b if fault == "bias_sign" else s - (F32(2) * b if fault == "bias_no_half" else b)
    N, K = s.shape
    key = _key(s)
    lab = K - 1 - np.argmax(key[:, ::-1], axis=1) if fault == "tie_higher" else np.argmax(key, axis=1)
    r = np.arange(N)
    best = s[r, lab]
    if K == 1:
        return lab + first, best, best.copy()
    rest = key.copy()
    rest[r, lab] = -np.inf
    with np.errstate(all="ignore"):
        second = rest.max(1).astype(F32)
        margin = best - np.where(np.isinf(second), F32(np.nan), second)
    return lab + first, best, margin


def assign_case(N, K, D, ldx, ldc, seed=0, exact=False, bias=True, nan_row=None, spherical=False):
    """(x fp32 [N, ldx], c fp32 [K, ldc], bias fp32 [K] or None); NaN in the pad columns.  exact: entries from {-1, -1/2, 0, 1/2, 1}
    and biases that are multiples of 1/4 (every score is exact in fp32, ties abound), every third centroid repeats the one before
    it with the same bias (a planted tie on every row).  Otherwise bias = 1/2 ||c||^2 rounded to fp32.  nan_row: that centroid is NaN."""
    rng = np.random.RandomState(6007 * seed + 31 * (N % 1000) + 7 * K + D)
    if exact:
        vals = np.array([-1, -0.5, 0, 0.5, 1], F32)
        x, c = vals[rng.randint(0, 5, (N, ldx))], vals[rng.randint(0, 5, (K, ldc))]
        b = (rng.randint(-8, 9, K) / 4).astype(F32)
        for j in range(2, K, 3):
            c[j], b[j] = c[j - 1], b[j - 1]
    else:
        x, c = rng.standard_normal((N, ldx)).astype(F32), rng.standard_normal((K, ldc)).astype(F32)
        if spherical:
            x[:, :D] /= np.linalg.norm(x[:, :D], axis=1, keepdims=True)
            c[:, :D] /= np.linalg.norm(c[:, :D], axis=1, keepdims=True)
        b = (0.5 * (c[:, :D].astype(np.float64) ** 2).sum(1)).astype(F32)
    x[:, D:] = np.nan
    c[:, D:] = np.nan
    if nan_row is not None:
        c[nan_row, :D] = np.nan
    return x, c, (b if bias else None)


def wide_rows(x, seed=0):
    """The rows scaled by powers of two between 2^-30 and 2^30: their fp64 sums round, so the order of the additions shows."""
    rng = np.random.RandomState(seed + 77)
    return (np.asarray(x, F32) * (2.0 ** rng.randint(-30, 31, (x.shape[0], 1))).astype(F32)).astype(F32)


def pixel_forms(N, seed=0):
    """[(name, H, W, p0, pixels int64 [N] or None)]: row order with an offset, a permutation, and a list with entries outside the map."""
    rng = np.random.RandomState(11 + seed + N % 97)
    out = [("rows", 1, N + 3, 2, None), ("permutation", 1, N, 0, rng.permutation(N).astype(np.int64))]
    pix = rng.permutation(N + 5)[:N].astype(np.int64) - 2                          # some below 0, some at or past H * W = N
    out.append(("outside", 1, N, 0, pix))
    return out


def rows_at(H, W, p0, pixels, N):
    """-> (pix int64 [N] the pixel of every row, inside bool [N])."""
    pix = p0 + np.arange(N, dtype=np.int64) if pixels is None else np.asarray(pixels, np.int64)
    return pix, (pix >= 0) & (pix < H * W)


# ------------------------------------------------------------------ update
def update_ref(x, labels, c_old, K, D, first, normalize, bias_old=None):
    """-> dict: counts int64 [K]; sums fp64 [K, D] added row by row in ascending order (the kernel's chain, bit for bit); c fp64
    [K, D] and c_bound; member [K] bool; inertia; empty; bad.  Empty clusters keep c_old."""
    xx = np.asarray(x)[:, :D].astype(np.float64)
    co = np.asarray(c_old)[:, :D].astype(np.float64)
    l = np.asarray(labels, np.int64) - first
    good = (l >= 0) & (l < K)
    sums, absum = np.zeros((K, D)), np.zeros((K, D))
    for i in np.flatnonzero(good):
        sums[l[i]] += xx[i]
    np.add.at(absum, l[good], np.abs(xx[good]))
    counts = np.bincount(l[good], minlength=K).astype(np.int64)
    member = counts > 0
    n = np.maximum(counts, 1)[:, None].astype(np.float64)
    with np.errstate(all="ignore"):
        mean = sums / n
        chain = counts[:, None] * U64 * absum / n
        if normalize:
            c, cb, _, _ = normalize_ref(mean, D)
            rel = ((math.ceil(D / 64) + 6) / 2 + 3 + 2) * U
            cb = np.abs(c) * rel + chain + np.where(c != 0, TINY, 0.0)
        else:
            c, cb = mean, U * np.abs(mean) + chain + np.where(mean != 0, TINY, 0.0)
        c = np.where(member[:, None], c, co)
        cb = np.where(member[:, None], cb, 0.0)
        d = xx[good] - co[l[good]]
        inertia = float((d * d).sum())
    return {"counts": counts, "sums": sums, "c": c, "c_bound": cb, "member": member, "inertia": inertia,
            "empty": int((~member).sum()), "bad": int((~good).sum())}


def bias_ref(c32, D):
    """From the STORED fp32 centroids -> (bias fp64 [K], bound)."""
    cc = np.asarray(c32, F32)[:, :D].astype(np.float64)
    b = 0.5 * (cc * cc).sum(1)
    return b, (U + D * U64) * np.abs(b) + np.where(b != 0, TINY, 0.0)


def emulate_update(x, labels, c_old, bias_old, K, D, first, normalize, fault=None):
    """The kernels' sequence -> (c fp32 [K, D], bias fp32 [K], sums fp64).  `fault`: empty_zeroed (an empty cluster gets a zero
    centroid and bias), no_renorm (cosine: the mean is not normalised), descending (the sum runs from the last row down)."""
    xx = np.asarray(x, F32)[:, :D].astype(np.float64)
    l = np.asarray(labels, np.int64) - first
    sums = np.zeros((K, D))
    rows = np.flatnonzero((l >= 0) & (l < K))
    for i in (rows[::-1] if fault == "descending" else rows):
        sums[l[i]] += xx[i]
    counts = np.bincount(l[rows], minlength=K)
    c = np.asarray(c_old, F32)[:, :D].copy()
    b = None if bias_old is None else np.asarray(bias_old, F32).copy()
    m = counts > 0
    c[m] = (sums[m] / counts[m, None]).astype(F32)
    if normalize and fault != "no_renorm":
        c[m] = emulate_normalize(c[m], D)[0]
    if b is not None:
        b[m] = (0.5 * (c[m].astype(np.float64) ** 2).sum(1)).astype(F32)
    if fault == "empty_zeroed":
        c[~m] = 0
        if b is not None:
            b[~m] = 0
    return c, b, sums


# ------------------------------------------------------------------ a whole fit
def fit_ref(x, seeds, metric, max_iter, first=1):
    """Lloyd in fp64 as KMeans.fit runs it: seeds (normalised for cosine) -> max_iter rounds of assign (first argmax of x . c - bias)
    and update (an empty cluster keeps its centroid) -> a final assign.  -> dict: labels, c, counts, inertia (of the last update,
    against the centroids its labels were assigned to), n_iter (rounds that changed a label; before the first round no row has
    one), min_gap (the smallest best - second score met in any round)."""
    xx = np.asarray(x, np.float64)
    c = np.asarray(seeds, np.float64).copy()
    cosine = metric == "cosine"
    if cosine:
        xx = xx / np.maximum(np.linalg.norm(xx, axis=1, keepdims=True), 1e-12)
        c = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-12)
    K = c.shape[0]
    lab = np.full(xx.shape[0], -1)
    n_iter, inertia, gap, counts = 0, None, np.inf, None

    def assign():
        s = xx @ c.T - (0.0 if cosine else 0.5 * (c * c).sum(1)[None, :])
        top = np.sort(s, axis=1)
        return np.argmax(s, axis=1), (float((top[:, -1] - top[:, -2]).min()) if K > 1 else np.inf)

    for _ in range(max_iter):
        new, g = assign()
        gap = min(gap, g)
        n_iter += int((new != lab).any())
        lab = new
        d = xx - c[lab]
        inertia = float((d * d).sum())
        counts = np.bincount(lab, minlength=K)
        sums = np.zeros_like(c)
        np.add.at(sums, lab, xx)
        m = counts > 0
        c[m] = sums[m] / counts[m, None]
        if cosine:
            c[m] = c[m] / np.maximum(np.linalg.norm(c[m], axis=1, keepdims=True), 1e-12)
    lab, g = assign()
    return {"labels": lab + first, "c": c, "counts": counts, "inertia": inertia, "n_iter": n_iter, "min_gap": min(gap, g)}


def class_seeds(bank, bank_labels, n_class):
    """One bank row per class (the first of each), in class order -> fp32 [n_class, D]."""
    return np.stack([bank[np.flatnonzero(bank_labels == k + 1)[0]] for k in range(n_class)]).astype(F32)


# ------------------------------------------------------------------ the ABI
def refusals(lib, _lib):
    """(what, code returned, code expected) of every refusal of the two entry points: all are decided before any launch."""
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    out = []

    def run(fn, struct, ok, table):
        out.append((fn + " params NULL", getattr(lib, fn)(None, None), E_NULL))
        for kw, want in table:
            a = dict(ok)
            a.update(kw)
            out.append((fn + " " + str(kw), getattr(lib, fn)(ctypes.byref(struct(**a)), None), want))

    common = [(dict(N=-1), E_DIMS), (dict(K=0), E_DIMS), (dict(D=0), E_DIMS), (dict(D=-4), E_DIMS), (dict(D=10), E_DIMS),
              (dict(first=-1), E_DIMS), (dict(ldx=8), E_DIMS), (dict(ldc=8), E_DIMS),
              (dict(K=1025), E_UNSUPPORTED), (dict(D=4100, ldx=4100, ldc=4100), E_UNSUPPORTED),
              (dict(x=None), E_NULL), (dict(c=None), E_NULL), (dict(labels=None), E_NULL),
              (dict(x=(1 << 20) + 4), E_ALIGN), (dict(c=(1 << 21) + 8), E_ALIGN), (dict(ldx=18), E_ALIGN), (dict(ldc=14), E_ALIGN),
              (dict(bias=(1 << 22) + 2), E_ALIGN), (dict(labels=(1 << 24) + 4), E_ALIGN), (dict(changed=(1 << 27) + 2), E_ALIGN),
              (dict(N=0), 0)]
    run("hsimae_kmeans_assign", _lib.KmeansAssignParams,
        dict(x=1 << 20, ldx=16, c=1 << 21, ldc=16, bias=1 << 22, N=4, K=3, D=12, first=1, H=2, W=2, p0=0, pixels=None,
             labels=1 << 24, score=1 << 25, margin=1 << 26, changed=1 << 27),
        common + [(dict(H=0), E_DIMS), (dict(W=0), E_DIMS), (dict(pixels=(1 << 23) + 4), E_ALIGN), (dict(score=(1 << 25) + 2), E_ALIGN),
                  (dict(margin=(1 << 26) + 1), E_ALIGN), (dict(N=0, x=None, c=None, labels=None), 0)])
    run("hsimae_kmeans_update", _lib.KmeansUpdateParams,
        dict(x=1 << 20, ldx=16, labels=1 << 24, N=4, K=3, D=12, first=1, normalize=0, c=1 << 21, ldc=16, bias=1 << 22,
             counts=1 << 28, sums=1 << 29, changed=1 << 27, scratch=1 << 30, state=1 << 31),
        common + [(dict(counts=None), E_NULL), (dict(sums=None), E_NULL), (dict(scratch=None), E_NULL), (dict(state=None), E_NULL),
                  (dict(counts=(1 << 28) + 4), E_ALIGN), (dict(sums=(1 << 29) + 4), E_ALIGN), (dict(scratch=(1 << 30) + 4), E_ALIGN),
                  (dict(state=(1 << 31) + 4), E_ALIGN),
                  (dict(N=0, x=None, c=None, labels=None, counts=None, sums=None, scratch=None, state=None), 0)])
    return out
