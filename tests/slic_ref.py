"""fp64 restatement and error bounds for csrc/slic.hip (tests/test_gpu_slic.py, tests/test_slic_bound_cpu.py): SLIC superpixels in
gSLIC's gather form over a guide image, and the vote of every superpixel over its pixels' class probabilities.

A plain module, not a conftest.  The bounds are worst-case first-order bounds of what the kernel rounds; nothing is tuned on a
GPU result.  The definition (hsimae_amd/segment.py states it too), U = 2^-24:

  grid      ny = ceil(H / S), nx = ceil(W / S), K = ny nx, centre k = i nx + j; home cell of (y, x) = (y ny // H, x nx // W).
  start     centre (i, j) at pixel y = (2 i + 1) H // (2 ny), x = (2 j + 1) W // (2 nx), features v_g = fl(scale_g I_g) there.
  distance  of pixel p to centre c, every operation fp32:
              v_g = fl(scale_g I_g(p))                       |dv_g| <= U |v_g|
              t_g = fl(v_g - c_g)                            |dt_g| <= U |v_g| + U |t_g| =: e_g; on t_g^2: 2 |t_g| e_g + e_g^2
              d   = fmaf(t_g, t_g, d), g = 0 .. G - 1        one rounding each, all terms >= 0: G U F, F = sum_g t_g^2
              dy  = fl(y - c_y), dx = fl(x - c_x)            U each: 2 U on each square
              s   = fmaf(dx, dx, fl(dy dy))                  the product's rounding and the fmaf's: |ds| <= 4 U s
              d   = fmaf(w, s, d)                            the spatial share carries 4 U, the fmaf U d
            => |dd| <= BETA = sum_g (2 |t_g| e_g + e_g^2) + G U F + 5 U w s + U d + TINY.  w is the fp32 the kernel is given.
  assign    the centres of the 3 x 3 cells around the home cell in ascending k (cells outside the grid left out); the smallest
            d wins, ties to the lower k, a NaN d loses to every number, all NaN: the home cell's centre (distance NaN).
  update    mean (v_0 .. v_{G-1}, y, x) over a centre's pixels: fp64 sums, one ascending-x chain per scene row, then the row
            partials in ascending y, one fp64 division, one rounding to fp32.  numpy repeats that order exactly (`ordered_sums`),
            so the restatement's centres are the kernel's bit for bit; the bound that is asserted is the fp32 rounding U |mean|
            plus n 2^-53 mean|v| for the sums.  A centre with no pixel keeps its bits.
  vote      per segment with cnt classified pixels: mode 0 v_c = fp32(sum / cnt) with the same ordered fp64 sum; mode 1
            v_c = fp32(m_c / cnt), m_c the classified pixels whose own argmax (first on ties, NaN the maximum) is c.
            Bound: U |v_c| + cnt 2^-53 mean|p| + TINY.  label = argmax v (first on ties), conf = v_label, margin = its lead.
A label is an argmin over rounded values: the checks demand that nothing CLEARLY better exists
(d64[l] - BETA[l] <= min_j (d64[j] + BETA[j])), and `open` is the share of pixels whose two best candidates lie within the bounds
of each other: the cases are chosen (and tests/test_slic_bound_cpu.py proves it without a GPU) so that it stays below 2 %.
"""
import ctypes

import numpy as np

from cls_ref import TINY, U, U64, ratio  # noqa: F401  (re-exported for the tests)
from knn_ref import header_fields  # noqa: F401

F32 = np.float32
CW = 8                                                     # floats per centre: G features, y, x, pad


def weight(compactness, size):
    """fp32(m^2 / S^2) as a Python float: what Superpixels hands the kernel."""
    return float(F32(float(compactness) ** 2 / int(size) ** 2))


def grid(H, W, S):
    return -(-H // S), -(-W // S)


def homes(H, W, S):
    """-> (hi int64 [H], hj int64 [W]): the home cell row of every scene row, the home cell column of every scene column."""
    ny, nx = grid(H, W, S)
    return np.arange(H, dtype=np.int64) * ny // H, np.arange(W, dtype=np.int64) * nx // W


def features(guide, scale):
    """fp32 [H, W, G]: v_g = fl(scale_g I_g), one correctly rounded fp32 product."""
    return (np.asarray(guide, F32) * np.asarray(scale, F32)[None, None, :]).astype(F32)


def init_centres(guide, scale, S):
    """fp32 [K, 8]: the grid centres (features, y, x, pad 0)."""
    H, W, G = guide.shape
    ny, nx = grid(H, W, S)
    v = features(guide, scale)
    c = np.zeros((ny * nx, CW), F32)
    for i in range(ny):
        for j in range(nx):
            y, x = (2 * i + 1) * H // (2 * ny), (2 * j + 1) * W // (2 * nx)
            c[i * nx + j, :G] = v[y, x]
            c[i * nx + j, G], c[i * nx + j, G + 1] = y, x
    return c


def candidates(H, W, S, fault=None):
    """int64 [H, W, 9]: the centre index of every candidate in ascending order, -1 where the cell lies outside the grid."""
    ny, nx = grid(H, W, S)
    hi, hj = homes(H, W, S)
    out = np.full((H, W, 9), -1, np.int64)
    q = 0
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            ci, cj = (hi + a)[:, None], (hj + b)[None, :]
            ok = (ci >= 0) & (ci < ny) & (cj >= 0) & (cj < nx)
            if fault == "border_cell_dropped":             # the bounds test is one cell too tight on the far side
                ok = ok & (cj < nx - 1 + (b <= 0))
            out[..., q] = np.where(ok, ci * nx + cj, -1)
            q += 1
    return out


def distances(guide, scale, centres, w, S):
    """-> (cand int64 [H, W, 9], d64 [H, W, 9], beta [H, W, 9]); d64 is NaN where the distance is NaN and +inf at a candidate
    that does not exist."""
    H, W, G = guide.shape
    cand = candidates(H, W, S)
    I = np.asarray(guide, F32).astype(np.float64) * np.asarray(scale, F32).astype(np.float64)[None, None, :]    # exact products
    c = np.asarray(centres, F32).astype(np.float64)[np.maximum(cand, 0)]                                        # [H, W, 9, 8]
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        t = I[:, :, None, :] - c[..., :G]
        e = U * np.abs(I)[:, :, None, :] + U * np.abs(t)
        F = (t * t).sum(3)
        s = (yy[..., None] - c[..., G]) ** 2 + (xx[..., None] - c[..., G + 1]) ** 2
        d = F + w * s
        beta = (2 * np.abs(t) * e + e * e).sum(3) + G * U * F + 5 * U * w * s + U * d + TINY
    d = np.where(cand >= 0, d, np.inf)
    beta = np.where((cand >= 0) & ~np.isnan(d), beta, 0.0)
    return cand, d, beta


def duplicates(cand, centres, G):
    """bool [H, W, 9]: the candidate's centre equals, bit for bit, that of an earlier candidate of the same pixel.  Equal inputs
    give equal fp32 distances, so such a candidate ties exactly and loses to the lower index: it can never be the label, and the
    pair is decided, not open."""
    bits = np.ascontiguousarray(np.asarray(centres, F32)[:, :G + 2]).view(np.int32)[np.maximum(cand, 0)]
    dup = np.zeros(cand.shape, bool)
    for q in range(1, 9):
        for e in range(q):
            dup[..., q] |= (cand[..., q] >= 0) & (cand[..., e] >= 0) & np.all(bits[..., q, :] == bits[..., e, :], axis=-1)
    return dup


def first_argmin(cand, d, H, W, S):
    """The assign rule on a distance array: smallest wins, first on ties, NaN loses, all NaN -> the home cell's centre.
    -> (label int64 [H, W], its distance)."""
    ny, nx = grid(H, W, S)
    hi, hj = homes(H, W, S)
    key = np.where(np.isnan(d), np.inf, d)
    q = np.argmin(key, axis=2)                             # the first of equals
    best = np.take_along_axis(key, q[..., None], 2)[..., 0]
    lab = np.take_along_axis(cand, q[..., None], 2)[..., 0]
    home = hi[:, None] * nx + hj[None, :]
    none = np.isinf(best)                                  # every existing candidate is NaN
    return np.where(none, home, lab), np.where(none, np.nan, np.take_along_axis(d, q[..., None], 2)[..., 0])


def assign_ref(guide, scale, centres, w, S):
    """The fp64 restatement of one assign -> dict: label, dist [H, W]; cand, d, beta, dup [H, W, 9]; open bool [H, W] (the two
    best candidates, `duplicates` left out, lie within their bounds of each other)."""
    H, W, G = guide.shape
    cand, d, beta = distances(guide, scale, centres, w, S)
    lab, dist = first_argmin(cand, d, H, W, S)
    dup = duplicates(cand, centres, G)
    key = np.where(np.isnan(d) | dup, np.inf, d)
    order = np.argsort(key, axis=2, kind="stable")[..., :2]
    k2 = np.take_along_axis(key, order, 2)
    b2 = np.take_along_axis(beta, order, 2)
    with np.errstate(all="ignore"):
        open_ = np.isfinite(k2[..., 1]) & (k2[..., 1] - k2[..., 0] <= b2[..., 0] + b2[..., 1])
    return {"label": lab, "dist": dist, "cand": cand, "d": d, "beta": beta, "dup": dup, "open": open_}


def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 is exact in fp64; the sum is rounded to fp64, then to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


ASSIGN_FAULTS = ["tie_upward", "border_cell_dropped", "spatial_unweighted"]


def emulate_assign(guide, scale, centres, w, S, fault=None):
    """The kernel's distance sequence with every fp32 operation rounded exactly, and its scan -> (label int64 [H, W], dist fp32
    [H, W], counts int64 [K]).  `fault` plants one defect (tests/test_slic_bound_cpu.py)."""
    H, W, G = guide.shape
    ny, nx = grid(H, W, S)
    cand = candidates(H, W, S, fault)
    v = features(guide, scale)
    c = np.asarray(centres, F32)[np.maximum(cand, 0)]
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        d = np.zeros((H, W, 9), F32)
        for g in range(G):
            t = (v[:, :, None, g] - c[..., g]).astype(F32)
            d = _fma(t, t, d)
        dy = (yy.astype(F32)[..., None] - c[..., G]).astype(F32)
        dx = (xx.astype(F32)[..., None] - c[..., G + 1]).astype(F32)
        s = _fma(dx, dx, (dy * dy).astype(F32))
        d = (d + s).astype(F32) if fault == "spatial_unweighted" else _fma(np.full_like(s, F32(w)), s, d)
    hi, hj = homes(H, W, S)
    lab = hi[:, None] * nx + hj[None, :]
    best = np.full((H, W), np.nan, F32)
    for q in range(9):
        dq = d[..., q]
        with np.errstate(all="ignore"):
            better = dq <= best if fault == "tie_upward" else dq < best
        take = (cand[..., q] >= 0) & ~np.isnan(dq) & (np.isnan(best) | better)
        lab, best = np.where(take, cand[..., q], lab), np.where(take, dq, best)
    return lab, best, np.bincount(lab.reshape(-1), minlength=ny * nx)


def ordered_sums(values, seg, K):
    """values fp64 [H, W, D], seg int [H, W] in 0 .. K - 1 (negative: the pixel takes no part) -> fp64 [K, D]: per segment the
    sum in the kernel's order: one ascending-x chain per scene row, then the row partials in ascending y.  (Adding the 0.0 of a
    row without a member changes nothing.)"""
    H, W, D = values.shape
    rows = np.zeros((H, K + 1, D))
    ar = np.arange(H)
    s = np.where(seg < 0, K, seg)
    for x in range(W):
        rows[ar, s[:, x]] += values[:, x]                  # (row, segment) pairs are distinct within a column
    tot = np.zeros((K + 1, D))
    for y in range(H):
        tot += rows[y]
    return tot[:K]


def update_ref(guide, scale, label, centres, fault=None):
    """One update from a label map -> (new centres fp32 [K, 8] in the kernel's order of operations, bound fp64 [K, 8], counts)."""
    H, W, G = guide.shape
    K = centres.shape[0]
    v = features(guide, scale).astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    vals = np.concatenate([v, yy[..., None].astype(np.float64), xx[..., None].astype(np.float64)], axis=2)
    cnt = np.bincount(label.reshape(-1), minlength=K)
    with np.errstate(all="ignore"):
        tot = ordered_sums(vals, label, K)
        mean = tot / np.maximum(cnt, 1)[:, None]
        mabs = ordered_sums(np.abs(vals), label, K) / np.maximum(cnt, 1)[:, None]
        bound = U * np.abs(mean) + cnt[:, None] * U64 * mabs + TINY
    new = np.asarray(centres, F32).copy()
    has = cnt > 0
    new[has, :G + 2] = mean[has].astype(F32)
    if fault == "empty_overwritten":
        new[~has, :G + 2] = 0
    b = np.zeros((K, CW))
    b[has, :G + 2] = np.where(np.isnan(bound[has]), 0.0, bound[has])
    return new, b, cnt


def fit_ref(guide, scale, S, compactness, max_iter, centres=None):
    """The whole definition in numpy: max_iter rounds of assign (the fp32 sequence, emulate_assign) and update, then one final
    assign -> (label int64 [H, W], centres fp32 [K, 8], counts)."""
    w = weight(compactness, S)
    c = init_centres(guide, scale, S) if centres is None else np.asarray(centres, F32).copy()
    for _ in range(max_iter):
        lab, _, _ = emulate_assign(guide, scale, c, w, S)
        c, _, _ = update_ref(guide, scale, lab, c)
    lab, _, cnt = emulate_assign(guide, scale, c, w, S)
    return lab, c, cnt


# ------------------------------------------------------------------ the checks (the code under test: the GPU, or the emulation)
def check_assign(guide, scale, centres, w, S, label, dist, counts, exact=False):
    """One assign against its own inputs -> dict: `wrong` (labels out of range, not a candidate, a duplicate, or clearly beaten), `dist` (worst
    |dist - d64[label]| / beta), `counts` (they are the labels' counts), `open` (share), `first` (exact=True: labels equal the first
    argmin of the restatement), `all` (inf unless everything holds, else `dist`)."""
    H, W, G = guide.shape
    ny, nx = grid(H, W, S)
    ref = assign_ref(guide, scale, centres, w, S)
    label = np.asarray(label, np.int64).reshape(H, W)
    hit = ref["cand"] == label[..., None]
    q = np.argmax(hit, axis=2)[..., None]
    in_cand = hit.any(2) & (label >= 0) & (label < ny * nx) & ~np.take_along_axis(ref["dup"], q, 2)[..., 0]
    dl = np.take_along_axis(ref["d"], q, 2)[..., 0]
    bl = np.take_along_axis(ref["beta"], q, 2)[..., 0]
    key = np.where(np.isnan(ref["d"]), np.inf, ref["d"])
    with np.errstate(all="ignore"):
        limit = (key + ref["beta"]).min(2)
        # a NaN distance may only win when every candidate is NaN, and then it is the home cell's centre
        none = np.isinf(key.min(2))
        beaten = np.where(none, label != ref["label"], np.isnan(dl) | ~(dl - bl <= limit))
    wrong = int(np.sum(~in_cand | beaten))
    res = {"wrong": wrong, "open": float(ref["open"].mean()), "dist": 0.0,
           "counts": counts is None or np.array_equal(np.asarray(counts, np.int64), np.bincount(label.reshape(-1).clip(0, ny * nx - 1), minlength=ny * nx)),
           "first": (not exact) or np.array_equal(label, ref["label"])}
    if dist is not None and wrong == 0:
        res["dist"] = ratio(np.asarray(dist).reshape(H, W), dl, bl)
    res["all"] = res["dist"] if wrong == 0 and res["counts"] and res["first"] else np.inf
    return res


def check_update(guide, scale, label, start, got):
    """New centres `got` fp32 [K, 8] against the mean over `label` (what the code under test itself chose from `start`) -> dict:
    `ratio` (worst err / bound over the moved slots), `bits` (equal to the restatement bit for bit, pads and empty centres
    included), `kept` (empty centres and pads keep start's bits), `all`."""
    want, bound, cnt = update_ref(guide, scale, np.asarray(label, np.int64), start)
    G = guide.shape[2]
    got = np.asarray(got, F32)
    has = cnt > 0
    kept = np.array_equal(got[~has].view(np.int32), np.asarray(start, F32)[~has].view(np.int32)) and \
        np.array_equal(got[:, G + 2:].view(np.int32), np.asarray(start, F32)[:, G + 2:].view(np.int32))
    r = ratio(got[has, :G + 2], want[has, :G + 2].astype(np.float64), bound[has, :G + 2]) if has.any() else 0.0
    return {"ratio": r, "bits": np.array_equal(got.view(np.int32), want.view(np.int32)), "kept": kept, "empty": int((~has).sum()),
            "all": r if kept else np.inf}


# ------------------------------------------------------------------ cases of hsimae_slic
COMPACTNESS = 0.1
# (H, W, S, G, variant).  variant: "" random guide; "dyadic" small integers with scale 1/4 and w = 2^-4, every operation exact;
# "const" a constant channel with scale 0; "nan" one NaN guide value; "empty" a start whose last centre coincides with the one
# before it along its axis (it loses every tie and gets no pixel).
CASES = [
    (1, 1, 2, 1, ""), (1, 9, 4, 1, ""), (7, 5, 8, 1, ""), (8, 8, 8, 2, "dyadic"), (9, 17, 8, 1, ""), (17, 33, 4, 4, ""),
    (23, 19, 3, 3, ""), (48, 40, 8, 1, "planted"), (33, 70, 32, 1, ""), (64, 5, 2, 1, ""), (130, 130, 2, 1, ""),
    (9, 17, 8, 1, "dyadic"), (17, 33, 4, 4, "dyadic"), (23, 19, 3, 3, "const"), (17, 33, 4, 4, "nan"), (9, 17, 8, 1, "nan"),
    (9, 17, 8, 1, "empty"), (23, 19, 3, 3, "empty"), (64, 5, 2, 1, "empty"),
]


def case_id(c):
    return "%dx%d-S%d-G%d%s" % (c[0], c[1], c[2], c[3], "-" + c[4] if c[4] else "")


def make_case(H, W, S, G, variant, seed=0):
    """-> dict: guide fp32 [H, W, G], scale fp32 [G], w (Python float), start fp32 [K, 8] (the centres a round starts from: the
    grid centres, with the coincident pair for "empty"), exact (every operation of the first assign is exact)."""
    rng = np.random.RandomState(1000003 * seed + 7919 * H + 104729 * W + 31 * S + 17 * G + len(variant))
    w = weight(COMPACTNESS, S)
    if variant == "planted":
        import smooth_ref
        s = smooth_ref.planted_scene(seed)
        guide, scale = s["guide"], s["scale"]
    elif variant == "dyadic":
        guide = rng.randint(0, 5, size=(H, W, G)).astype(F32)
        scale = np.full(G, 0.25, F32)
        w = weight(S / 4.0, S)                             # 2^-4
    else:
        guide = (100.0 + 50.0 * rng.standard_normal((H, W, G))).astype(F32)
        if variant == "const":
            guide[..., 1] = F32(7.5)
        span = guide.reshape(-1, G).max(0) - guide.reshape(-1, G).min(0)
        with np.errstate(all="ignore"):
            scale = np.where(span > 0, F32(1) / span, F32(0)).astype(F32)
        if variant == "nan":
            guide[H // 2, W // 3, G - 1] = np.nan
    start = init_centres(guide, scale, S)
    if variant == "empty":
        ny, nx = grid(H, W, S)
        K = ny * nx
        start[K - 1] = start[K - 2] if nx > 1 else start[K - 1 - nx]
    return {"guide": np.ascontiguousarray(guide, F32), "scale": scale, "w": w, "start": start, "exact": variant == "dyadic"}


# ------------------------------------------------------------------ the vote
def own_argmax(p, first):
    """first + argmax over the columns [first, C) of every row: first on ties, NaN counts as the maximum (torch.argmax)."""
    z = np.asarray(p)[:, first:]
    with np.errstate(all="ignore"):
        return first + np.argmax(np.where(np.isnan(z), np.inf, z), axis=1)


def vote_ref(probs, n, C, first, row_of, label, S, mode, fill, fault=None):
    """probs fp32 [n, ld], row_of int32 [H W] or None, label int [H, W] (a SLIC map) -> dict: vec fp32 [K, C] (the kernel's
    order of operations; rows of segments without a classified pixel are 0), bound fp64 [K, C], cnt [K], seg_label / conf /
    margin per segment (from vec, fp32), written bool [H W] (the pixels the maps are written at), seg [H W]."""
    H, W = label.shape
    ny, nx = grid(H, W, S)
    K = ny * nx
    row = np.arange(H * W, dtype=np.int64) if row_of is None else np.asarray(row_of, np.int64).copy()
    row[(row < 0) | (row >= n)] = -1
    has = (row >= 0).reshape(H, W)
    seg = np.asarray(label, np.int64)
    counted = np.ones_like(has) if fault == "mean_over_unclassified" else has
    cnt = np.bincount(seg[counted], minlength=K)
    P = np.zeros((H, W, C - first))
    P[has] = np.asarray(probs)[row.reshape(H, W)[has], first:C].astype(np.float64)
    vec, bound = np.zeros((K, C), F32), np.zeros((K, C))
    live = cnt > 0
    with np.errstate(all="ignore"):
        if mode == 0:
            tot = ordered_sums(P, np.where(has, seg, -1), K)
            mabs = ordered_sums(np.abs(P), np.where(has, seg, -1), K)
            mean = tot / np.maximum(cnt, 1)[:, None]
            b = U * np.abs(mean) + cnt[:, None] * U64 * mabs / np.maximum(cnt, 1)[:, None] + TINY
        else:
            own = np.full((H, W), -1, np.int64)
            own[has] = own_argmax(np.asarray(probs)[row.reshape(H, W)[has], :C], first)
            m = np.zeros((K, C - first))
            np.add.at(m, (seg[has], own[has] - first), 1.0)
            mean = m / np.maximum(cnt, 1)[:, None]
            b = U * np.abs(mean) + TINY
    vec[live, first:] = mean[live].astype(F32)
    bound[live, first:] = np.where(np.isnan(b[live]), 0.0, b[live])
    seg_label = own_argmax(vec, first)
    conf = vec[np.arange(K), seg_label]
    other = vec.astype(np.float64).copy()
    other[:, :first] = -np.inf
    other[np.arange(K), seg_label] = -np.inf
    second = np.where(np.isnan(other), -np.inf, other).max(1).astype(F32)
    with np.errstate(all="ignore"):
        margin = conf.copy() if C - first == 1 else (conf - second).astype(F32)
    written = live[seg] & (has | bool(fill and fault != "fill_ignored"))
    return {"vec": vec, "bound": bound, "cnt": cnt, "label": seg_label.astype(np.int64), "conf": conf, "margin": margin,
            "written": written.reshape(-1), "seg": seg.reshape(-1), "live": live}


def check_vote(ref, first, C, vec, seg_count, label_map, conf_map, margin_map, fill_value):
    """What a vote wrote against the restatement `ref` and against ITSELF -> dict: `vec` (worst err / bound of the segment
    vectors of live segments), `count` (seg_count exact), `self` (per written pixel: the label is the first argmax of the vector
    that was written for its segment, conf is that vector's entry bit for bit, margin its fp32 lead over the runner-up),
    `untouched` (every pixel that must not be written, and the vector rows of dead segments, still hold the fill value), `all`."""
    live, seg, written = ref["live"], ref["seg"], ref["written"]
    vec = np.asarray(vec, F32)
    K = vec.shape[0]
    r = ratio(vec[live][:, first:C], ref["vec"][live][:, first:C].astype(np.float64), ref["bound"][live][:, first:C]) if live.any() else 0.0
    zeros = bool(np.all(vec[live][:, :first] == 0))
    lab = own_argmax(vec[:, :C], first)
    conf = vec[np.arange(K), lab]
    other = vec[:, :C].astype(np.float64).copy()
    other[:, :first] = -np.inf
    other[np.arange(K), lab] = -np.inf
    second = np.where(np.isnan(other), -np.inf, other).max(1).astype(F32)
    with np.errstate(all="ignore"):
        margin = conf.copy() if C - first == 1 else (conf - second).astype(F32)
    lm, cm, mm = np.asarray(label_map), np.asarray(conf_map, F32), np.asarray(margin_map, F32)
    sw = seg[written]
    self_ok = bool(np.array_equal(lm[written], lab[sw]) and np.array_equal(cm[written].view(np.int32), conf[sw].view(np.int32)) and
                   np.array_equal(mm[written].view(np.int32), margin[sw].view(np.int32)))
    untouched = bool(np.all(lm[~written] == fill_value) and np.all(cm[~written] == fill_value) and np.all(mm[~written] == fill_value) and
                     np.all(vec[~live] == fill_value) and np.all(vec[:, C:] == fill_value))
    count = seg_count is None or np.array_equal(np.asarray(seg_count, np.int64), ref["cnt"])
    res = {"vec": r, "count": count, "self": self_ok, "untouched": untouched, "zeros": zeros}
    res["all"] = r if count and self_ok and untouched and zeros else np.inf
    return res


def emulate_vote(probs, n, C, first, row_of, label, S, mode, fill, fill_value, fault=None):
    """The vote as the kernel writes it (from vote_ref's kernel-order vectors) -> (vec fp32 [K, C], seg_count, label_map int64,
    conf_map, margin_map [H W]); untouched elements hold `fill_value`.  `fault` plants one defect."""
    good = vote_ref(probs, n, C, first, row_of, label, S, mode, fill)
    bad = vote_ref(probs, n, C, first, row_of, label, S, mode, fill, fault)
    vec = np.where(good["live"][:, None], bad["vec"], F32(fill_value)).astype(F32)
    HW = good["seg"].size
    lm, cm, mm = np.full(HW, fill_value, np.int64), np.full(HW, fill_value, F32), np.full(HW, fill_value, F32)
    wr = bad["written"] & good["live"][good["seg"]]
    sw = good["seg"][wr]
    lm[wr], cm[wr], mm[wr] = bad["label"][sw], bad["conf"][sw], bad["margin"][sw]
    return vec, good["cnt"].copy(), lm, cm, mm


# (H, W, S, C, first, form, mode, fill).  form: "all" row_of NULL, tight ldp / ldo; "padded" row_of NULL, ldp = C + 3, ldo = C + 5;
# "subset" a permuted subset with holes, one whole segment without a classified pixel, rows no pixel points to, padded;
# "ties" dyadic probabilities that tie two classes in every segment (the sums are exact: the first must win).
VOTE_CASES = [
    (9, 17, 8, 2, 0, "all", 0, 0), (9, 17, 8, 2, 1, "subset", 1, 1), (23, 19, 3, 18, 1, "subset", 0, 0), (23, 19, 3, 18, 1, "subset", 0, 1),
    (23, 19, 3, 18, 0, "padded", 1, 0), (17, 33, 4, 40, 1, "subset", 1, 1), (17, 33, 4, 40, 0, "padded", 0, 0), (17, 33, 4, 18, 1, "ties", 0, 1),
    (17, 33, 4, 18, 0, "ties", 1, 0), (48, 40, 8, 40, 1, "subset", 0, 1), (33, 70, 32, 18, 1, "subset", 1, 1), (33, 70, 32, 2, 0, "all", 0, 0),
    (1, 9, 4, 18, 1, "subset", 0, 1), (130, 130, 2, 2, 0, "subset", 0, 1),
]


def vote_id(c):
    return "%dx%d-S%d-C%d-f%d-%s-m%d-fill%d" % c


_SEGS = {}


def segments_of(H, W, S, seed=0):
    """A SLIC map of a random one-channel guide (the restatement's own fit, three rounds), cached: int32 [H, W]."""
    if (H, W, S, seed) not in _SEGS:
        case = make_case(H, W, S, 1, "", seed + 5)
        _SEGS[H, W, S, seed] = fit_ref(case["guide"], case["scale"], S, COMPACTNESS, 3)[0].astype(np.int32)
    return _SEGS[H, W, S, seed]


def make_vote_case(H, W, S, C, first, form, mode, fill, seed=0):
    """-> dict: probs fp32 [n, ldp] (NaN in the columns below `first`, in the pad and in rows no pixel points to), ldp, ldo, n,
    row_of int32 [H W] or None, label int32 [H, W], dead (a segment without a classified pixel, or None)."""
    rng = np.random.RandomState(1000003 * seed + 7919 * H + 104729 * W + 31 * S + 1009 * C + first + len(form) + 2 * mode + fill)
    HW = H * W
    label = segments_of(H, W, S, seed)
    ldp, ldo = {"all": (C, C), "padded": (C + 3, C + 5), "subset": (C + 3, C + 1), "ties": (C, C)}[form]
    dead = None
    if form == "subset":
        hole = rng.rand(H, W) < 0.4
        present = np.unique(label)
        dead = int(present[len(present) // 2])
        hole[label == dead] = True
        if hole.all():
            hole[label != dead] = False
        pix = np.flatnonzero(~hole.reshape(-1))
        pix = pix[rng.permutation(pix.size)]
        n = pix.size + 3
        slots = rng.permutation(n)[:pix.size]
        row_of = np.full(HW, -1, np.int32)
        row_of[pix] = slots.astype(np.int32)
        row_of[np.flatnonzero(hole.reshape(-1))[::2]] = -7
    else:
        n, row_of = HW, None
    K = C - first
    probs = np.full((n, ldp), np.nan, F32)
    if form == "ties":
        # every pixel: 1/2 on class a or b (alternating by pixel parity within its segment), the rest spread in eighths: the two
        # classes tie exactly in every segment with an even number of pixels, and every sum is exact
        a, b = first + K // 3, first + K // 3 + 2
        p = np.zeros((n, K), F32)
        order = np.zeros(HW, np.int64)
        flat = label.reshape(-1)
        for k in np.unique(flat):
            idx = np.flatnonzero(flat == k)
            order[idx] = np.arange(idx.size)
        p[np.arange(n), np.where(order % 2 == 0, a, b) - first] = 0.5
        p[:, 0] += F32(0.25)
        p[:, K - 1] += F32(0.25)
        probs[:, first:C] = p
    else:
        z = 2.0 * rng.standard_normal((n, K))
        e = np.exp(z - z.max(1, keepdims=True))
        probs[:, first:C] = (e / e.sum(1, keepdims=True)).astype(F32)
    if row_of is not None:
        used = np.zeros(n, bool)
        used[row_of[row_of >= 0]] = True
        probs[~used] = np.nan
    return {"probs": probs, "ldp": ldp, "ldo": ldo, "n": n, "row_of": row_of, "label": label, "dead": dead}


def oa(label, truth):
    return float(np.mean(np.asarray(label).reshape(-1) == np.asarray(truth).reshape(-1)))


def purity(seg, truth):
    """The share of pixels that carry the majority truth of their segment."""
    seg, truth = np.asarray(seg).reshape(-1), np.asarray(truth).reshape(-1)
    good = 0
    for k in np.unique(seg):
        good += np.bincount(truth[seg == k]).max()
    return good / seg.size


# ------------------------------------------------------------------ the ABI
def refusals(lib, _lib):
    """(what, code returned, code expected) of every refusal of the two entry points: all are decided before anything is launched."""
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    nan, inf = float("nan"), float("inf")
    out = []

    def run(fn, struct, ok, table):
        out.append((fn + " params NULL", getattr(lib, fn)(None, None), E_NULL))
        for kw, want in table:
            a = dict(ok)
            a.update(kw)
            out.append((fn + " " + str(kw), getattr(lib, fn)(ctypes.byref(struct(**a)), None), want))

    ok = dict(guide=1 << 20, guide_scale=1 << 21, G=2, H=4, W=4, size=2, w=0.01, init=1, rounds=2, centres=1 << 22, centres_tmp=1 << 23,
              counts=1 << 24, labels=1 << 25, dist=1 << 26)
    run("hsimae_slic", _lib.SlicParams, ok, [
        (dict(H=0), E_DIMS), (dict(W=-1), E_DIMS), (dict(H=1 << 16, W=1 << 15), E_DIMS), (dict(G=0), E_DIMS), (dict(G=5), E_DIMS),
        (dict(size=1), E_DIMS), (dict(size=33), E_DIMS), (dict(rounds=-1), E_DIMS), (dict(init=2), E_DIMS), (dict(w=-1.0), E_DIMS),
        (dict(w=nan), E_DIMS), (dict(w=inf), E_DIMS), (dict(centres_tmp=1 << 22), E_DIMS), (dict(centres_tmp=(1 << 22) + 64), E_DIMS),
        (dict(labels=1 << 20), E_DIMS), (dict(dist=(1 << 20) + 32), E_DIMS), (dict(dist=1 << 25), E_DIMS), (dict(counts=1 << 21), E_DIMS),
        (dict(guide=None), E_NULL), (dict(guide_scale=None), E_NULL), (dict(centres=None), E_NULL), (dict(labels=None), E_NULL),
        (dict(centres_tmp=None), E_NULL),
        (dict(guide=(1 << 20) + 2), E_ALIGN), (dict(guide_scale=(1 << 21) + 1), E_ALIGN), (dict(centres=(1 << 22) + 2), E_ALIGN),
        (dict(centres_tmp=(1 << 23) + 3), E_ALIGN), (dict(counts=(1 << 24) + 2), E_ALIGN), (dict(labels=(1 << 25) + 1), E_ALIGN),
        (dict(dist=(1 << 26) + 2), E_ALIGN)])
    ok = dict(probs=1 << 20, ldp=16, n=16, C=10, first=1, row_of=1 << 21, labels=1 << 22, H=4, W=4, size=2, mode=0, fill=0,
              out_probs=1 << 23, ldo=16, seg_count=1 << 24, label_map=1 << 25, conf_map=1 << 26, margin_map=1 << 27)
    run("hsimae_segment_vote", _lib.SegmentVoteParams, ok, [
        (dict(H=0), E_DIMS), (dict(W=-1), E_DIMS), (dict(H=1 << 16, W=1 << 15), E_DIMS), (dict(n=-1), E_DIMS), (dict(C=1, first=0), E_DIMS),
        (dict(first=-1), E_DIMS), (dict(first=10), E_DIMS), (dict(ldp=9), E_DIMS), (dict(ldo=9), E_DIMS), (dict(size=1), E_DIMS),
        (dict(size=33), E_DIMS), (dict(mode=2), E_DIMS), (dict(mode=-1), E_DIMS), (dict(fill=2), E_DIMS),
        (dict(out_probs=1 << 20), E_DIMS), (dict(out_probs=(1 << 20) + 64), E_DIMS), (dict(label_map=1 << 22), E_DIMS),
        (dict(conf_map=1 << 21), E_DIMS), (dict(margin_map=1 << 26), E_DIMS), (dict(seg_count=(1 << 25) + 8), E_DIMS),
        (dict(C=1025, ldp=1040, ldo=1040), E_UNSUPPORTED),
        (dict(probs=None), E_NULL), (dict(labels=None), E_NULL), (dict(label_map=None), E_NULL),
        (dict(probs=(1 << 20) + 2), E_ALIGN), (dict(row_of=(1 << 21) + 2), E_ALIGN), (dict(labels=(1 << 22) + 1), E_ALIGN),
        (dict(out_probs=(1 << 23) + 3), E_ALIGN), (dict(seg_count=(1 << 24) + 2), E_ALIGN), (dict(label_map=(1 << 25) + 4), E_ALIGN),
        (dict(conf_map=(1 << 26) + 2), E_ALIGN), (dict(margin_map=(1 << 27) + 2), E_ALIGN)])
    return out
