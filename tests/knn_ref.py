"""fp64 restatement and error bounds for csrc/knn.hip (tests/test_gpu_knn.py, tests/test_knn_bound_cpu.py): the row
normalisation, the k most similar bank rows of every query, and the weighted vote of the neighbours.

A plain module, not a conftest.  The bounds are worst-case first-order bounds of what the kernels round, nothing is tuned on a
GPU result.  U = 2^-24 (cls_ref.py), TINY = 2^-120 absolute for flushed / denormal results.

hsimae_row_normalize, D columns, m = ceil(D / 64) terms per lane:
  ss   = lane-strided fmaf(x, x, ss) from 0, then 6 shuffle steps   all terms >= 0: |dss| / ss <= (m + 6) U
  n    = sqrtf(ss)                                                    half of that, + U
  r    = 1 / fmaxf(n, eps32)                                          + U (IEEE division); max() is 1-Lipschitz
  out  = x * r                                                        + U
      => |dout| <= |out| NREL,  NREL = ((m + 6) / 2 + 3) U;  |dn| <= n ((m + 6) / 2 + 1) U
  n clearly below eps32 = fl32(1e-12): the divisor is the constant itself (the restatement uses the same fp32 constant): 2 U |out|.
  A zero element gives an exact zero (bound 0), so a zero row gives zeros.

hsimae_knn_topk: the inputs are taken as given (fp32), only the dot product rounds:
  |sim_ij - s64_ij| <= beta_ij = gamma_D sum_d |q_id b_jd|,  gamma_D = D U / (1 - D U)    (any summation order, one rounding per
  product-and-add: the fmaf chain of the fp32 MFMA).  Checks that hold on EVERY row (check_topk):
  (a) indices distinct and in range; the list descending, equal similarities by ascending index, NaN last;
  (b) every returned sim within beta of the fp64 dot product of its own index;
  (c) nothing better left out: for every bank row j not returned, s64_ij <= s64_i,last + beta_ij + beta_i,last;
  (d) (exact inputs only) idx equals the first k of the fp64 stable descending argsort, sim bit for bit.

hsimae_knn_vote, neighbour j of a row (rank order), t_j = (sim_j - sim_0) invT with invT the fp32 value the kernel is given:
  w_j     = exp2(fl(fl(fl(sim_j - sim_0) invT) fl(log2 e)))   three roundings of the argument and the constant fl32(log2 e)
            (0.24 U off): (3.25 |t_j|) U on w_j; v_exp_f32 1 ulp: 2 U    => |dw_j| <= BW_j = w_j (3.25 |t_j| + 2) U + TINY
  score_c = the n_c weights of class c added in rank order from 0     => BS_c = sum BW_j + (n_c - 1) U score_c
  total   = sum_c score_c, m' = ceil((C - first) / 64) per lane, 6 shuffle steps => BT = sum_c BS_c + (m' + 6) U total
  p_c     = fl(score_c * fl(1 / total))                               => |dp_c| <= BS_c / total + p_c (BT / total + 2 U) + TINY
  conf = p[label] (that entry's bound), margin = p[label] - p[second] (the sum of the two).  Columns below `first`: exact zeros.
  The label must equal the restatement's wherever its top-two gap exceeds twice the sum of the two entries' bounds (`decided`).

Predict (normalise -> top-k -> vote), restated from the DEVICE's normalised rows: a row is decided when the fp64 gap between
rank k and rank k + 1 exceeds beta_k + beta_(k+1) (the neighbour SET is determined) and the top-two class gap exceeds twice the
bounds, which now also carry the similarity error: p_c 2 max_j (beta_j + beta_0) invT to first order.
"""
import ctypes
import math
import re

import numpy as np

from cls_ref import SHAPES, TINY, U, ratio  # noqa: F401  (re-exported for the tests)
from prob_ref import _lane_sum, pixel_forms, products, rows_of_pixels  # noqa: F401

F32 = np.float32
LOG2E32 = F32(1.4426950408889634)
LOG2E_REL = abs(float(LOG2E32) - 1.4426950408889634) / 1.4426950408889634
ARG = 3.0 + math.ceil(100 * LOG2E_REL / U) / 100         # 3.25: three roundings of the argument + the constant's own error
EPS32 = F32(1e-12)
VOTE_SHAPES = [s for s in SHAPES if s[1] <= 200]
KS = [1, 2, 20, 64]
TEMPS = [1.0, 0.07, 0.01]


def inv_t32(T):
    """What the binding passes: the host's fp64 1 / T rounded once to fp32."""
    return F32(1.0 / T)


# ------------------------------------------------------------------ normalise
def normalize_ref(x, D):
    """x [N, ld] -> (out fp64 [N, D], bound, norms fp64 [N], norms bound)."""
    xx = np.asarray(x)[:, :D].astype(np.float64)
    n = np.sqrt((xx * xx).sum(1))
    m = math.ceil(D / 64)
    nrel = ((m + 6) / 2 + 1) * U
    out = xx / np.maximum(n, float(EPS32))[:, None]
    rel = np.where(n * (1 + nrel) < float(EPS32), 2 * U, ((m + 6) / 2 + 3) * U)
    bound = np.abs(out) * rel[:, None] + np.where(out != 0, TINY, 0.0)
    return out, bound, n, n * nrel + np.where(n != 0, TINY, 0.0)


def emulate_normalize(x, D, fault=None):
    """The kernel's sequence with every fp32 operation rounded (the fmaf through fp64) -> (out fp32 [N, D], norms fp32 [N])."""
    xx = np.asarray(x, F32)[:, :D]
    N = xx.shape[0]
    lanes = np.zeros((N, 64), F32)
    for c in range(D):
        lanes[:, c % 64] = (xx[:, c].astype(np.float64) * xx[:, c].astype(np.float64) + lanes[:, c % 64].astype(np.float64)).astype(F32)
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, idx ^ s]
    n = np.sqrt(lanes[:, 0])
    d = n + EPS32 if fault == "eps_added" else np.maximum(n, EPS32)
    with np.errstate(all="ignore"):
        r = F32(1) / d
    return xx * r[:, None], n


def normalize_case(N, D, ld, seed=0):
    """fp32 [N, ld] with NaN in the pad columns; with N >= 5: row 0 zero, row 1 tiny (norm < 1e-12), row 2 huge (1e15 per
    element), row 3 a single non-zero element."""
    rng = np.random.RandomState(17 * seed + 3 * N + D)
    x = rng.standard_normal((N, ld)).astype(F32)
    x[:, D:] = np.nan
    if N >= 5:
        x[0, :D] = 0
        x[1, :D] *= F32(1e-14)
        x[2, :D] *= F32(1e15)
        x[3, :D] = 0
        x[3, D // 2] = -3.0
    return x


# ------------------------------------------------------------------ top-k
def dots(q, b, D):
    """-> (s64 [Q, M] with -0 folded into +0, beta [Q, M])."""
    q64, b64 = np.asarray(q)[:, :D].astype(np.float64), np.asarray(b)[:, :D].astype(np.float64)
    with np.errstate(all="ignore"):
        s = q64 @ b64.T + 0.0
        beta = (D * U / (1 - D * U)) * (np.abs(q64) @ np.abs(b64).T)
    return s, np.where(np.isnan(beta), np.inf, beta)


def order_of(s):
    """Stable descending argsort of every row, NaN last (among equals and among NaNs: ascending index)."""
    key = np.where(np.isnan(s), -np.inf, s)
    nan_last = np.isnan(s).astype(np.int8)
    return np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), -key, nan_last), axis=1)


def check_topk(idx, sim, q, b, D, k, exact=False, ref=None):
    """-> dict of violation counts of (a) .. (d) and the worst |sim - s64| / beta; `ok` when all are 0."""
    idx, sim = np.asarray(idx, np.int64), np.asarray(sim, F32)
    Q, M = np.asarray(q).shape[0], np.asarray(b).shape[0]
    s64, beta = dots(q, b, D) if ref is None else ref
    out = {"shape": int(idx.shape != (Q, k) or sim.shape != (Q, k))}
    if out["shape"]:
        out["ok"] = False
        return out
    rows = np.arange(Q)[:, None]
    inr = (idx >= 0) & (idx < M)
    ci = np.where(inr, idx, 0)
    srt = np.sort(ci, 1)
    out["a_range"] = int((~inr).sum())
    out["a_distinct"] = int((srt[:, 1:] == srt[:, :-1]).sum()) if k > 1 else 0
    s0, s1, i0, i1 = sim[:, :-1], sim[:, 1:], idx[:, :-1], idx[:, 1:]
    n0, n1 = np.isnan(s0), np.isnan(s1)
    with np.errstate(all="ignore"):
        fine = np.where(n0, n1 & (i0 < i1), n1 | (s0 > s1) | ((s0 == s1) & (i0 < i1)))
    out["a_sorted"] = int((~fine).sum())
    own, ownb = s64[rows, ci], beta[rows, ci]
    numbers = (~np.isnan(s64)).sum(1)
    nan_ok = np.isnan(sim) & np.isnan(own) & (np.arange(k)[None, :] >= numbers[:, None])      # a NaN only once the numbers ran out
    with np.errstate(all="ignore"):
        err = np.abs(sim.astype(np.float64) - own)
        within = (err <= ownb) | nan_ok
    out["b_sim"] = int((~within).sum())
    with np.errstate(all="ignore"):
        rb = np.where((err > 0) & ~nan_ok, err / ownb, 0.0)
    out["b_worst"] = float(np.where(np.isnan(rb), np.inf, rb).max()) if rb.size else 0.0
    left = np.ones((Q, M), bool)
    left[rows, ci] = False
    last, lastb = own[:, -1:], ownb[:, -1:]
    with np.errstate(all="ignore"):
        better = left & ~np.isnan(s64) & (np.isnan(last) | (s64 > last + beta + lastb))
    out["c_left_out"] = int(better.sum())
    if exact:
        want = order_of(s64)[:, :k]
        out["d_idx"] = int((idx != want).sum())
        out["d_sim"] = int((sim.view(np.int32) != s64[rows, want].astype(F32).view(np.int32)).sum())
    out["ok"] = all(v == 0 for key, v in out.items() if key != "b_worst")
    return out


def emulate_topk(q, b, D, k, fault=None):
    """The kernel's dot product (the k-ordered fmaf chain from +0, each step rounded to fp32 through fp64) and the stable
    selection -> (idx int32 [Q, k], sim fp32 [Q, k]).  `fault` plants one defect."""
    qq, bb = np.asarray(q, F32)[:, :D].astype(np.float64), np.asarray(b, F32)[:, :D].astype(np.float64)
    s = np.zeros((qq.shape[0], bb.shape[0]), F32)
    with np.errstate(all="ignore"):
        for d in range(D):
            s = (qq[:, d:d + 1] * bb[None, :, d] + s.astype(np.float64)).astype(F32)
    s = s + F32(0)
    if fault == "tie_higher_index":
        M = s.shape[1]
        order = M - 1 - order_of(s[:, ::-1])
    else:
        order = order_of(s)
    if fault == "drop_kth":
        order = np.concatenate([order[:, :k - 1], order[:, k:]], 1)
    idx = order[:, :k].copy()
    if fault == "unsorted" and k > 1:
        idx[:, [0, k - 1]] = idx[:, [k - 1, 0]]
    sim = s[np.arange(s.shape[0])[:, None], idx]
    if fault == "transposed_idx":
        idx = np.ascontiguousarray(idx.T).reshape(idx.shape)
    return idx.astype(np.int32), sim


def topk_case(Q, M, D, ldq, ldb, seed=0, exact=False, nan_row=None):
    """(q fp32 [Q, ldq], bank fp32 [M, ldb]); NaN in the pad columns.  exact: entries from {-1, -1/2, 0, 1/2, 1} (every dot product
    is exact in fp32, ties abound) and every third bank row repeats the row before it.  nan_row: that bank row is NaN."""
    rng = np.random.RandomState(7919 * seed + 31 * Q + 7 * M + D)
    if exact:
        vals = np.array([-1, -0.5, 0, 0.5, 1], F32)
        q, b = vals[rng.randint(0, 5, (Q, ldq))], vals[rng.randint(0, 5, (M, ldb))]
        for j in range(2, M, 3):
            b[j] = b[j - 1]
    else:
        q, b = rng.standard_normal((Q, ldq)).astype(F32), rng.standard_normal((M, ldb)).astype(F32)
    q[:, D:] = np.nan
    b[:, D:] = np.nan
    if nan_row is not None:
        b[nan_row, :D] = np.nan
    return q, b


# ------------------------------------------------------------------ vote
def vote_ref(idx, sim, labels, C, first, invT, sim_err=None):
    """idx [Q, k], sim [Q, k] (fp32 as the kernel reads them, or fp64), labels int64 [M] -> dict: p, bound [Q, C]; label; conf,
    conf_bound, margin, margin_bound at that label; decided; bad [Q] (rows with a neighbour or label out of range: all zero).
    sim_err [Q]: an error of the similarities themselves (predict), carried into the bounds as p_c 2 sim_err invT."""
    idx, labels = np.asarray(idx, np.int64), np.asarray(labels, np.int64)
    s = np.asarray(sim).astype(np.float64)
    Q, k = idx.shape
    M = labels.shape[0]
    rows = np.arange(Q)[:, None]
    inr = (idx >= 0) & (idx < M)
    lab = labels[np.where(inr, idx, 0)]
    good = inr & (lab >= first) & (lab < C)
    bad = ~good.all(1)
    lab = np.where(good, lab, first)
    invT = float(invT)
    with np.errstate(all="ignore"):
        t = (s - s[:, :1]) * invT
        w = np.exp(t)
        bw = w * (ARG * np.abs(t) + 2) * U + TINY
        score, bs, cnt = np.zeros((Q, C)), np.zeros((Q, C)), np.zeros((Q, C))
        np.add.at(score, (np.broadcast_to(rows, idx.shape), lab), w)
        np.add.at(bs, (np.broadcast_to(rows, idx.shape), lab), bw)
        np.add.at(cnt, (np.broadcast_to(rows, idx.shape), lab), 1.0)
        bs = bs + np.maximum(cnt - 1, 0) * U * score
        total = score.sum(1, keepdims=True)
        bt = bs.sum(1, keepdims=True) + (math.ceil((C - first) / 64) + 6) * U * total
        p = score / total
        bound = bs / total + p * (bt / total + 2 * U) + np.where(p != 0, TINY, 0.0)
        if sim_err is not None:
            bound = bound + p * 2 * np.asarray(sim_err)[:, None] * invT
    p[bad], bound[bad] = 0.0, 0.0
    bound = np.where(np.isnan(bound), 0.0, bound)
    label = first + np.argmax(p[:, first:], axis=1)
    if C - first == 1:
        decided = np.ones(Q, bool)
    else:
        two = np.argsort(-np.where(np.isnan(p[:, first:]), np.inf, p[:, first:]), axis=1, kind="stable")[:, :2] + first
        r1 = np.arange(Q)
        gap = p[r1, two[:, 0]] - p[r1, two[:, 1]]
        decided = gap > 2 * (bound[r1, two[:, 0]] + bound[r1, two[:, 1]])
    conf, cb, margin, mb = products(p, bound, label, first)
    label = np.where(bad, 0, label)
    for a in (conf, cb, margin, mb):
        a[bad] = 0.0
    return {"p": p, "bound": bound, "label": label.astype(np.int64), "conf": conf, "conf_bound": cb, "margin": margin,
            "margin_bound": mb, "decided": decided | bad, "bad": bad}


def emulate_vote(idx, sim, labels, C, first, invT, fault=None, T=None):
    """The kernel's sequence in exactly rounded fp32 (exp2 in fp64, rounded once) -> (p fp32 [Q, C], label, conf, margin)."""
    idx, labels = np.asarray(idx, np.int64), np.asarray(labels, np.int64)
    s = np.asarray(sim, F32)
    Q, k = idx.shape
    lab = labels[idx]
    invT = F32(T) if fault == "T_not_invT" else F32(invT)
    with np.errstate(all="ignore"):
        d = s if fault == "no_shift" else s - s[:, :1]
        arg = (d * invT) * LOG2E32
        w = np.exp2(arg.astype(np.float64)).astype(F32)
        score = np.zeros((Q, C), F32)
        r1 = np.arange(Q)
        for j in range(k):
            score[r1, lab[:, j]] = score[r1, lab[:, j]] + w[:, j]
        total = _lane_sum(score[:, first:])
        p = score * (F32(1) / total)[:, None]
        if fault == "class0_nonzero":
            p[:, 0] = F32(1e-6)
        key = p[:, first:]
        if fault == "tie_higher_class":
            label = first + key.shape[1] - 1 - np.argmax(key[:, ::-1], axis=1)
        else:
            label = first + np.argmax(key, axis=1)
        conf = p[r1, label]
        other = p.copy()
        other[:, :first] = -np.inf
        other[r1, label] = -np.inf
        margin = conf.copy() if C - first == 1 else conf - other.max(1)
    return p, label.astype(np.int64), conf, margin


def vote_worst(got, ref, first):
    """got = (p, label, conf, margin) of the code under test -> worst err / bound of p, conf, margin (the two at got's own label),
    `wrong` = decided rows whose label differs, `open` = the share of rows left undecided, `zeros` = columns below first are 0."""
    p, label, conf, margin = got
    label = np.asarray(label, np.int64)
    C = ref["p"].shape[1]
    ok = ((label >= first) & (label < C)) | (ref["bad"] & (label == 0))
    lab = np.where(ok & ~ref["bad"], label, first)
    rc, rcb, rm, rmb = products(ref["p"], ref["bound"], lab, first)
    for a in (rc, rcb, rm, rmb):
        a[ref["bad"]] = 0.0
    out = {"p": ratio(p, ref["p"], ref["bound"]), "conf": ratio(conf, rc, rcb), "margin": ratio(margin, rm, rmb),
           "wrong": int(np.sum(~ok | (ref["decided"] & (label != ref["label"])))),
           "open": float(np.sum(~ref["decided"])) / max(1, label.shape[0]),
           "zeros": bool(np.all(np.asarray(p)[:, :first] == 0))}
    out["all"] = np.inf if out["wrong"] or not out["zeros"] else max(out["p"], out["conf"], out["margin"])
    return out


def vote_case(Q, C, first, k, T, M=300, seed=0):
    """(idx int32 [Q, k], sim fp32 [Q, k] descending, labels int64 [M] in [first, C)): continuous random similarities (the best
    in [0.5, 1), exponential gaps of mean 0.02 below it: exact ties do not occur), arbitrary neighbours.  With Q >= 6 the last
    two rows are equal."""
    rng = np.random.RandomState(100003 * seed + 1009 * k + 7 * Q + C + 31 * first + int(1000 * T))
    gaps = rng.exponential(0.02, (Q, k))
    gaps[:, 0] = 0
    sim = (rng.uniform(0.5, 1.0, (Q, 1)) - np.cumsum(gaps, 1)).astype(F32)
    sim = -np.sort(-sim, axis=1)
    idx = rng.randint(0, M, (Q, k)).astype(np.int32)
    labels = rng.randint(first, C, M).astype(np.int64)
    if Q >= 6:                                              # pixel_forms' index list repeats the last pixel: equal rows
        idx[Q - 1], sim[Q - 1] = idx[Q - 2], sim[Q - 2]
    return idx, sim, labels


def tie_cases():
    """Planted exact ties -> [(idx, sim, labels, C, first, want label)]: equal similarities, so every weight is exactly 1;
    k = 2 with two classes, k = 4 with 2 + 2: the lower class wins."""
    lab = np.array([0, 5, 3, 3, 5, 1], np.int64)
    half = np.full((1, 2), 0.75, F32)
    quad = np.full((1, 4), 0.25, F32)
    return [(np.array([[1, 2]], np.int32), half, lab, 7, 1, 3), (np.array([[2, 1]], np.int32), half, lab, 7, 1, 3),
            (np.array([[1, 3, 4, 2]], np.int32), quad, lab, 7, 1, 3), (np.array([[1, 0]], np.int32), half, lab, 6, 0, 0)]


# ------------------------------------------------------------------ predict
def predict_ref(qn, bn, labels, k, C, first, invT):
    """qn [Q, D], bn [M, D]: the device's normalised rows (fp32) -> vote_ref's dict on the fp64 neighbours, with `decided` also
    requiring that the neighbour set is determined, and `idx` the fp64 neighbours."""
    D = np.asarray(qn).shape[1]
    s64, beta = dots(qn, bn, D)
    order = order_of(s64)
    rows = np.arange(s64.shape[0])[:, None]
    top = order[:, :k]
    st, bt = s64[rows, top], beta[rows, top]
    if s64.shape[1] > k:
        nxt = order[:, k]
        r1 = np.arange(s64.shape[0])
        set_ok = st[:, -1] - s64[r1, nxt] > bt[:, -1] + beta[r1, nxt]
    else:
        set_ok = np.ones(s64.shape[0], bool)
    ref = vote_ref(top, st, labels, C, first, invT, sim_err=(bt + bt[:, :1]).max(1))
    ref["decided"] = ref["decided"] & set_ok
    ref["idx"] = top
    return ref


def clusters(n_class=7, D=32, per_class=20, Q=1000, seed=0):
    """Gaussian clusters -> (bank fp32 [n_class * per_class, D], bank labels 1 .. n_class, queries fp32 [Q, D], their classes)."""
    rng = np.random.RandomState(4242 + seed)
    centres = 1.5 * rng.standard_normal((n_class, D))
    by = np.repeat(np.arange(n_class), per_class)
    qy = rng.randint(0, n_class, Q)
    bank = (centres[by] + rng.standard_normal((by.size, D))).astype(F32)
    qs = (centres[qy] + rng.standard_normal((Q, D))).astype(F32)
    return bank, (by + 1).astype(np.int64), qs, (qy + 1).astype(np.int64)


# ------------------------------------------------------------------ the ABI
def header_fields(hdr, name):
    """[(field, ctype)] of `typedef struct { .. } name;` in the header text (a pointer is declared alone: `type* name`)."""
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)
        for field in m.group(3).split(","):
            fields.append((field.strip(), ctypes.c_void_p if m.group(2) else ctype[m.group(1)]))
    return fields


def refusals(lib, _lib):
    """(what, code returned, code expected) of every refusal of the three entry points: all are decided before any launch."""
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    out = []

    def run(fn, struct, ok, table):
        out.append((fn + " params NULL", getattr(lib, fn)(None, None), E_NULL))
        for kw, want in table:
            a = dict(ok)
            a.update(kw)
            out.append((fn + " " + str(kw), getattr(lib, fn)(ctypes.byref(struct(**a)), None), want))

    run("hsimae_row_normalize", _lib.RowNormalizeParams, dict(x=1 << 20, ld=16, N=4, D=12, out=1 << 21, ldo=12, norms=1 << 22),
        [(dict(N=-1), E_DIMS), (dict(D=-1), E_DIMS), (dict(ld=11), E_DIMS), (dict(ldo=11), E_DIMS),
         (dict(x=None), E_NULL), (dict(out=None), E_NULL),
         (dict(x=(1 << 20) + 2), E_ALIGN), (dict(out=(1 << 21) + 1), E_ALIGN), (dict(norms=(1 << 22) + 2), E_ALIGN),
         (dict(N=0), 0), (dict(N=0, x=None, out=None), 0), (dict(D=0, ld=0, ldo=0), 0)])
    run("hsimae_knn_topk", _lib.KnnTopkParams,
        dict(q=1 << 20, ldq=16, bank=1 << 21, ldb=16, Q=4, M=30, D=12, k=5, idx=1 << 22, sim=1 << 23),
        [(dict(Q=-1), E_DIMS), (dict(M=-1), E_DIMS), (dict(D=0), E_DIMS), (dict(D=-4), E_DIMS), (dict(D=10), E_DIMS),
         (dict(k=0), E_DIMS), (dict(k=31), E_DIMS), (dict(ldq=8), E_DIMS), (dict(ldb=8), E_DIMS),
         (dict(k=65, M=100), E_UNSUPPORTED), (dict(M=(1 << 20) + 1), E_UNSUPPORTED), (dict(D=4100, ldq=4100, ldb=4100), E_UNSUPPORTED),
         (dict(q=None), E_NULL), (dict(bank=None), E_NULL), (dict(idx=None), E_NULL), (dict(sim=None), E_NULL),
         (dict(q=(1 << 20) + 4), E_ALIGN), (dict(bank=(1 << 21) + 8), E_ALIGN), (dict(ldq=18), E_ALIGN), (dict(ldb=14), E_ALIGN),
         (dict(idx=(1 << 22) + 2), E_ALIGN), (dict(sim=(1 << 23) + 1), E_ALIGN),
         (dict(Q=0), 0), (dict(Q=0, q=None, idx=None, sim=None), 0)])
    run("hsimae_knn_vote", _lib.KnnVoteParams,
        dict(idx=1 << 20, sim=1 << 21, Q=4, k=5, M=30, bank_labels=1 << 22, C=10, first=1, inv_temperature=1 / 0.07, H=2, W=2, p0=0,
             pixels=None, label_map=1 << 23, conf_map=1 << 24, margin_map=1 << 25, probs=1 << 26, ldp=16, bad=1 << 27),
        [(dict(Q=-1), E_DIMS), (dict(M=0), E_DIMS), (dict(k=0), E_DIMS), (dict(C=1, first=0), E_DIMS), (dict(first=-1), E_DIMS),
         (dict(first=10), E_DIMS), (dict(ldp=9), E_DIMS), (dict(H=0), E_DIMS), (dict(W=0), E_DIMS),
         (dict(inv_temperature=0.0), E_DIMS), (dict(inv_temperature=-1.0), E_DIMS), (dict(inv_temperature=float("nan")), E_DIMS),
         (dict(inv_temperature=float("inf")), E_DIMS),
         (dict(k=65), E_UNSUPPORTED), (dict(C=1025, ldp=1040), E_UNSUPPORTED),
         (dict(idx=None), E_NULL), (dict(sim=None), E_NULL), (dict(bank_labels=None), E_NULL), (dict(label_map=None), E_NULL),
         (dict(bad=None), E_NULL),
         (dict(idx=(1 << 20) + 2), E_ALIGN), (dict(sim=(1 << 21) + 1), E_ALIGN), (dict(bank_labels=(1 << 22) + 4), E_ALIGN),
         (dict(pixels=(1 << 28) + 4), E_ALIGN), (dict(label_map=(1 << 23) + 4), E_ALIGN), (dict(conf_map=(1 << 24) + 2), E_ALIGN),
         (dict(margin_map=(1 << 25) + 2), E_ALIGN), (dict(probs=(1 << 26) + 3), E_ALIGN), (dict(bad=(1 << 27) + 2), E_ALIGN),
         (dict(Q=0), 0), (dict(Q=0, idx=None, sim=None, bank_labels=None, label_map=None, bad=None), 0)])
    return out
