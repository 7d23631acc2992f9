"""fp64 restatement, fp32 emulations and error bounds for csrc/svm.hip (tests/test_gpu_svm.py, tests/test_svm_bound_cpu.py).

A plain module, not a conftest.  Nothing is tuned on a GPU result.  U = 2^-24, TINY = 2^-120 (cls_ref.py).

hsimae_svm_gram, element (t, s), D columns, gamma_D = D U / (1 - D U), beta_ts = gamma_D sum_d |x_td x_sd| (knn_ref.dots):
  dot, n_t = dot_tt, n_s   the fmaf chain: |d dot| <= beta_ts, |d n_t| <= beta_tt
  d2 = fmaf(-2, dot, fl(n_t + n_s)), clamped at 0 (1-Lipschitz; the true d2 is >= 0)
       three roundings / error sources: E_d2 = 2 beta_ts + beta_tt + beta_ss + U (n_t + n_s) + U d2
  g2 = fl(gamma fl32(log2 e)): relative (1 + LOG2E_REL / U) U <= 1.25 U;  arg = fl(-g2 d2): + U
       |d arg| <= E_arg = |arg| (ARG - 1) U + gamma log2(e) E_d2,  ARG - 1 = 2.25 as knn_ref derives its 3.25 for three roundings
  K = exp2(arg), v_exp_f32 1 ulp (2 U, knn_ref): |dK| <= K (2^E_arg - 1) + 2 U K + TINY
  The diagonal is the constant 1: bound 0.

hsimae_svm_predict: the same with n_q the lane-strided sum of squares, m = ceil(D / 64) terms per lane and 6 tree steps:
  |d n_q| <= (m + 6) U n_q in place of beta_tt; n_s is the packed fp32 value, beta_ss off the true one.  BK = the bound above.
  dec_p = the fmaf chain over the n_p support rows of the pair in order: |d dec| <= sum |coef| BK + gamma_(n_p) sum |coef K|
  d_p = fl(dec_p - rho_p): + U |d_p|.

The solver is restated exactly (smo): every fp64 operation of the kernel is one IEEE operation and there is no reduction over
floating-point values, so alpha, G, rho and the iteration count must be BIT-EQUAL when both start from the same K.

Optimality certificate (certificate): with f_t = sum_s alpha_s y_s K_ts, primal P = 1/2 a'Qa + C sum_t max(0, 1 - y_t (f_t - rho)),
dual D = e'a - 1/2 a'Qa; weak duality gives 0 <= D* - D <= P - D.  Let G_t = (Qa)_t - 1 = y_t f_t - 1, so that
1 - y_t (f_t - rho) = -G_t + y_t rho, and P - D = a'Qa - e'a + C sum_t xi_t = sum_t (alpha_t G_t + C xi_t) (using y'a = 0:
sum_t alpha_t G_t = sum_t alpha_t (G_t - y_t rho)).  At eps-KKT stopping, m(a) - M(a) < eps with rho inside [M, m] up to eps
(calculate_rho takes it between the two), so per t, with h_t = G_t - y_t rho = -(1 - y_t (f_t - rho)):
  alpha_t = 0:       the term is C max(0, -h_t); KKT: h_t >= -eps, so the term <= C eps
  0 < alpha_t < C:   |h_t| <= eps: alpha_t h_t + C max(0, -h_t) <= C eps
  alpha_t = C:       h_t <= eps: C h_t + C max(0, -h_t) = C max(h_t, 0) <= C eps
  => 0 <= P - D <= n C eps.
"""
import ctypes
import math
import re

import numpy as np

from cls_ref import TINY, U  # noqa: F401
from knn_ref import ARG, F32, LOG2E32, dots  # noqa: F401

TAU = 1e-12
GD = lambda D: D * U / (1 - D * U)  # noqa: E731


# ------------------------------------------------------------------ fp32 helpers
def chain_dot(a, b):
    """The k-ordered fmaf chain from +0, each step rounded to fp32 through fp64 -> fp32 [A, B]."""
    a64, b64 = np.asarray(a, F32).astype(np.float64), np.asarray(b, F32).astype(np.float64)
    s = np.zeros((a64.shape[0], b64.shape[0]), F32)
    with np.errstate(all="ignore"):
        for d in range(a64.shape[1]):
            s = (a64[:, d:d + 1] * b64[None, :, d] + s.astype(np.float64)).astype(F32)
    return s


def kernel_value32(dot, nt, ns, gamma, fault=None):
    """d2 / g2 / exp2 in exactly rounded fp32 (exp2 in fp64, rounded once)."""
    with np.errstate(all="ignore"):
        sm = (np.asarray(nt, F32)[:, None] + np.asarray(ns, F32)[None, :]).astype(F32)
        d2 = (np.float64(-2.0) * dot.astype(np.float64) + sm.astype(np.float64)).astype(F32)
        if fault != "no_clamp":
            d2 = np.where(d2 < 0, F32(0), d2)
        g2 = F32(F32(gamma) * LOG2E32)
        arg = ((-g2) * d2).astype(F32)
        return np.exp2(arg.astype(np.float64)).astype(F32)


def lane_sumsq(x):
    """hsimae_row_normalize's sum of squares: lane-strided fmaf, then the xor tree -> fp32 [N]."""
    xx = np.asarray(x, F32)
    lanes = np.zeros((xx.shape[0], 64), F32)
    for c in range(xx.shape[1]):
        lanes[:, c % 64] = (xx[:, c].astype(np.float64) ** 2 + lanes[:, c % 64].astype(np.float64)).astype(F32)
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, idx ^ s]
    return lanes[:, 0]


# ------------------------------------------------------------------ Gram
def gram_emulate(x, D, gammas, fault=None):
    """-> (K fp32 [n_gamma, M, M], sumsq fp32 [M]) by the kernel's sequence."""
    xx = np.asarray(x, F32)[:, :D]
    dot = chain_dot(xx, xx)
    n = np.diagonal(dot).copy()
    K = np.stack([kernel_value32(dot, n, n, g) for g in gammas])
    if fault == "asymmetric":
        K = np.stack([kernel_value32(dot, n, n * F32(1 + 2 ** -20), g) for g in gammas])
    if fault != "diag_computed":
        for k in K:
            np.fill_diagonal(k, F32(1))
    else:
        K = np.stack([kernel_value32(dot, lane_sumsq(xx) * F32(1 + 2 ** -20), n, g) for g in gammas])
    return K, n


def kernel_bound(K64, arg64, gamma, e_d2):
    with np.errstate(all="ignore"):
        e_arg = np.abs(arg64) * (ARG - 1) * U + gamma * math.log2(math.e) * e_d2
        b = K64 * np.expm1(math.log(2.0) * e_arg) + 2 * U * K64 + TINY
    return np.where(np.isnan(b), np.inf, b)


def gram_ref(x, D, gammas):
    """-> (K fp64 [n_gamma, M, M], bound)."""
    xx = np.asarray(x)[:, :D].astype(np.float64)
    s, beta = dots(xx, xx, D)
    n = np.diagonal(s)
    bn = np.diagonal(beta)
    with np.errstate(all="ignore"):
        d2 = np.maximum(n[:, None] + n[None, :] - 2 * s, 0.0)
        e = 2 * beta + bn[:, None] + bn[None, :] + U * (n[:, None] + n[None, :]) + U * d2
    Ks, Bs = [], []
    for g in gammas:
        with np.errstate(all="ignore"):
            K = np.exp(-float(g) * d2)
        b = kernel_bound(K, float(g) * math.log2(math.e) * d2, float(g), e)
        np.fill_diagonal(K, 1.0)
        np.fill_diagonal(b, 0.0)
        Ks.append(K)
        Bs.append(b)
    return np.stack(Ks), np.stack(Bs)


def gram_case(M, D, ldx, seed=0, dup=True, nan_row=None):
    """fp32 [M, ldx] with NaN in the pad; with M >= 3 row 2 repeats row 0 (dup)."""
    rng = np.random.RandomState(1000 * seed + 13 * M + D)
    x = (rng.standard_normal((M, ldx)) * 0.7).astype(F32)
    x[:, D:] = np.nan
    if dup and M >= 3:
        x[2] = x[0]
    if nan_row is not None:
        x[nan_row, :D] = np.nan
    return x


# ------------------------------------------------------------------ the solver
def _argbest(vals, mask, fault=None):
    """Index of the largest vals[mask]; ties to the lower index, a NaN never wins; -1 when there is none."""
    ok = mask & ~np.isnan(vals)
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return -1
    v = vals[idx]
    if fault == "tie_higher_index":
        return int(idx[v.size - 1 - np.argmax(v[::-1])])
    return int(idx[np.argmax(v)])


def smo(K, na, nb, C, eps=1e-3, max_iter=10 ** 6, alpha=None, G=None, fault=None):
    """libsvm's SMO with WSS 2 as svm_solve_kernel runs it.  K: the [n, n] kernel block of the problem's rows (fp32 or fp64; read
    as fp64), rows of class a first.  -> dict(alpha, G, rho, iterations (of this call), converged, gap, n_sv, n_bounded)."""
    n = na + nb
    K = np.asarray(K).astype(np.float64)
    y = np.where(np.arange(n) < na, 1.0, -1.0)
    pos = y > 0
    alpha = np.zeros(n) if alpha is None else np.array(alpha, np.float64)
    G = -np.ones(n) if G is None else np.array(G, np.float64)
    C = float(C)
    it, conv, gap = 0, 0, 0.0
    with np.errstate(all="ignore"):
        while True:
            yg = np.where(pos, G, -G)
            ub, lb = alpha >= C, alpha <= 0.0
            up, low = np.where(pos, ~ub, ~lb), np.where(pos, ~lb, ~ub)
            i = _argbest(-yg, up, fault)
            gmax = -yg[i] if i >= 0 else -np.inf
            cand = yg[low & ~np.isnan(yg)]
            m2 = (cand.max() if cand.size else -np.inf) + 0.0              # -0 counts as +0
            gap = gmax + m2 if i >= 0 else -np.inf
            if i < 0 or gap < eps:
                conv = 1
                break
            if it >= max_iter:
                break
            b = gmax + yg
            q = 2.0 - 2.0 * K[i]
            q = np.where(q > 0.0, q, TAU)
            if fault == "first_order":
                j = _argbest(yg, low & (b > 0.0), fault)
            else:
                j = _argbest((b * b) / q, low & (b > 0.0), fault)
            if j < 0:
                conv = 1
                break
            oi, oj, gi, gj = alpha[i], alpha[j], G[i], G[j]
            quad = 2.0 - 2.0 * K[i, j]
            if not quad > 0.0:
                quad = TAU
            ai, aj = oi, oj
            clip = fault != "unclipped"
            if pos[i] != pos[j]:
                delta = (-gi - gj) / quad
                diff = ai - aj
                ai, aj = ai + delta, aj + delta
                if clip:
                    if diff > 0.0:
                        if aj < 0.0:
                            aj, ai = 0.0, diff
                    elif ai < 0.0:
                        ai, aj = 0.0, -diff
                    if diff > 0.0:
                        if ai > C:
                            ai, aj = C, C - diff
                    elif aj > C:
                        aj, ai = C, C + diff
            else:
                delta = (gi - gj) / quad
                sm = ai + aj
                ai, aj = ai - delta, aj + delta
                if clip:
                    if sm > C:
                        if ai > C:
                            ai, aj = C, sm - C
                    elif aj < 0.0:
                        aj, ai = 0.0, sm
                    if sm > C:
                        if aj > C:
                            aj, ai = C, sm - C
                    elif ai < 0.0:
                        ai, aj = 0.0, sm
            di, dj = ai - oi, aj - oj
            qi = np.where(pos == pos[i], K[i], -K[i])
            qj = np.where(pos == pos[j], K[j], -K[j])
            G = G + (qi * di + qj * dj)
            alpha[i], alpha[j] = ai, aj
            it += 1
        yg = np.where(pos, G, -G)
        ub, lb = alpha >= C, alpha <= 0.0
        free = ~ub & ~lb
        hi = (ub & ~pos) | (lb & pos)
        lo = (ub & pos) | (lb & ~pos)
        if fault == "rho_bounded_only" or not free.any():
            u = yg[hi].min() if hi.any() else np.inf
            l = yg[lo].max() if lo.any() else -np.inf
            rho = (u + l) / 2.0
        else:
            s = 0.0
            for v in yg[free]:
                s = s + v
            rho = s / float(free.sum())
    if not (np.isfinite(alpha).all() and np.isfinite(G).all()):
        conv = -3
    return {"alpha": alpha, "G": G, "rho": float(rho), "iterations": it, "converged": conv, "gap": float(gap),
            "n_sv": int((alpha > 0).sum()), "n_bounded": int(ub.sum())}


def certificate(K, na, nb, C, alpha, rho):
    """-> (P - D, n C): the duality gap of (alpha, rho) in fp64 and what eps multiplies in its bound."""
    n = na + nb
    K = np.asarray(K).astype(np.float64)
    y = np.where(np.arange(n) < na, 1.0, -1.0)
    f = K @ (alpha * y)
    quad = float((alpha * y) @ f)
    xi = np.maximum(0.0, 1.0 - y * (f - rho))
    primal = 0.5 * quad + C * xi.sum()
    dual = alpha.sum() - 0.5 * quad
    return primal - dual, n * C


def pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def fit_ref(K, starts, counts, C, eps=1e-3, max_iter=10 ** 6, fault=None):
    """Every pair of a class-sorted bank with kernel matrix K [M, M] -> list of smo() results in pair order."""
    out = []
    for a, b in pairs(len(counts)):
        rows = np.concatenate([np.arange(starts[a], starts[a] + counts[a]), np.arange(starts[b], starts[b] + counts[b])])
        out.append(smo(np.asarray(K)[np.ix_(rows, rows)], counts[a], counts[b], C, eps, max_iter, fault=fault))
    return out


# ------------------------------------------------------------------ pack
def pack_ref(sols, starts, counts, fault=None):
    """libsvm's compact model from the pair solutions -> dict(sv_index, sv_start, coef fp32 [n - 1, S], rho fp32 [P])."""
    n = len(counts)
    pr = pairs(n)
    al = {}
    for (a, b), s in zip(pr, sols):
        al[(a, b)] = s["alpha"][:counts[a]]
        al[(b, a)] = s["alpha"][counts[a]:]
    sv_index, sv_start, cols = [], [0], []
    for c in range(n):
        for t in range(counts[c]):
            if any(al[(c, o)][t] > 0 for o in range(n) if o != c):
                sv_index.append(starts[c] + t)
                col = []
                for j in range(n - 1):
                    o = j if j < c else j + 1
                    if fault == "wrong_opponent":
                        o = (j + 1 if j + 1 < c else j + 2) if j < n - 2 else (0 if c != 0 else 1)
                    v = al[(c, o)][t]
                    col.append(F32(v if c < o else -v))
                cols.append(col)
        sv_start.append(len(sv_index))
    coef = np.array(cols, F32).reshape(len(sv_index), n - 1).T.copy()
    return {"sv_index": np.array(sv_index, np.int32), "sv_start": np.array(sv_start, np.int32), "coef": coef,
            "rho": np.array([s["rho"] for s in sols], F32)}


# ------------------------------------------------------------------ predict
def _pair_rows(sv_start, a, b):
    return np.arange(sv_start[a], sv_start[a + 1]), np.arange(sv_start[b], sv_start[b + 1])


def votes_of(dec, n, first, fault=None):
    """Decision values [Q, P] -> (label, votes int [Q, n]): d > 0 votes for a, else b; ties to the lower class."""
    Q = dec.shape[0]
    votes = np.zeros((Q, n), np.int64)
    for p, (a, b) in enumerate(pairs(n)):
        w = dec[:, p] > 0
        if fault == "b_sign_flipped":
            w = ~w if b == n - 1 else w
        votes[np.arange(Q), np.where(w, a, b)] += 1
    if fault == "tie_higher_class":
        best = n - 1 - np.argmax(votes[:, ::-1], 1)
    else:
        best = np.argmax(votes, 1)
    return (first + best).astype(np.int64), votes


def shares_of(votes, label, first, num_class):
    """-> (probs fp32 [Q, num_class], conf, margin) exactly as the kernel forms them."""
    n = votes.shape[1]
    P = F32(n * (n - 1) // 2)
    sh = votes.astype(F32) / P
    probs = np.zeros((votes.shape[0], num_class), F32)
    probs[:, first:first + n] = sh
    r = np.arange(votes.shape[0])
    other = votes.copy()
    other[r, label - first] = -1
    conf = sh[r, label - first]
    return probs, conf, conf - other.max(1).astype(F32) / P


def predict_emulate(q, sv, sv_sumsq, sv_start, coef, rho, gamma, D, fault=None):
    """The kernel's decision values in exactly rounded fp32 -> fp32 [Q, P]."""
    qq, ss = np.asarray(q, F32)[:, :D], np.asarray(sv, F32)[:, :D]
    Kv = kernel_value32(chain_dot(qq, ss), lane_sumsq(qq), sv_sumsq, gamma)
    n = len(sv_start) - 1
    dec = np.zeros((qq.shape[0], n * (n - 1) // 2), F32)
    for p, (a, b) in enumerate(pairs(n)):
        ra, rb = _pair_rows(sv_start, a, b)
        acc = np.zeros(qq.shape[0], F32)
        for rows, c in ((ra, coef[b - 1]), (rb, coef[a])):
            for s in rows:
                acc = (np.float64(c[s]) * Kv[:, s].astype(np.float64) + acc.astype(np.float64)).astype(F32)
        dec[:, p] = acc - F32(rho[p])
    return dec


def predict_ref(q, sv, sv_sumsq, sv_start, coef, rho, gamma, D):
    """fp64 decision values of the packed model and their bound -> (dec [Q, P], bound)."""
    qq, ss = np.asarray(q)[:, :D].astype(np.float64), np.asarray(sv)[:, :D].astype(np.float64)
    s, beta = dots(qq, ss, D)
    nq, ns = (qq * qq).sum(1), (ss * ss).sum(1)
    bss = GD(D) * ns
    m = math.ceil(D / 64)
    d2 = np.maximum(nq[:, None] + ns[None, :] - 2 * s, 0.0)
    e = 2 * beta + (m + 6) * U * nq[:, None] + bss[None, :] + np.abs(np.asarray(sv_sumsq, np.float64) - ns)[None, :] \
        + U * (nq[:, None] + ns[None, :]) + U * d2
    K = np.exp(-float(gamma) * d2)
    BK = kernel_bound(K, float(gamma) * math.log2(math.e) * d2, float(gamma), e)
    n = len(sv_start) - 1
    c64 = np.asarray(coef, np.float64)
    dec, bound = np.zeros((qq.shape[0], n * (n - 1) // 2)), np.zeros((qq.shape[0], n * (n - 1) // 2))
    for p, (a, b) in enumerate(pairs(n)):
        ra, rb = _pair_rows(sv_start, a, b)
        rows = np.concatenate([ra, rb])
        cf = np.concatenate([c64[b - 1][ra], c64[a][rb]])
        acc = K[:, rows] @ cf
        npair = max(1, rows.size)
        bsum = BK[:, rows] @ np.abs(cf) + GD(npair) * (K[:, rows] @ np.abs(cf))
        dec[:, p] = acc - float(rho[p])
        bound[:, p] = bsum + U * np.abs(dec[:, p]) + TINY
    return dec, bound


def model_case(n, S, D, seed=0):
    """A synthetic packed model: S support rows spread over n classes (a class may have none) -> dict of host arrays."""
    rng = np.random.RandomState(seed + 13 * n + S)
    cuts = np.sort(rng.randint(0, S + 1, n - 1))
    sv = (0.6 * rng.standard_normal((S, D))).astype(F32)
    return {"n": n, "M": S, "D": D, "gamma": 1.0 / D, "sv_start": np.r_[0, cuts, S].astype(np.int32), "sv": sv,
            "coef": rng.uniform(-2, 2, (n - 1, S)).astype(F32), "rho": rng.uniform(-0.3, 0.3, n * (n - 1) // 2).astype(F32),
            "sv_sumsq": np.diagonal(chain_dot(sv, sv)).copy()}


def decided_rows(dec, tau, n):
    """The label rule: a row is decided when the winner's votes from pairs with |d| >= tau exceed every other class's certain
    plus uncertain votes -> (decided bool [Q], label index of the certain winner)."""
    Q = dec.shape[0]
    sure, maybe = np.zeros((Q, n), np.int64), np.zeros((Q, n), np.int64)
    tau = np.broadcast_to(np.asarray(tau, np.float64), dec.shape)
    for p, (a, b) in enumerate(pairs(n)):
        cert = np.abs(dec[:, p]) >= tau[:, p]
        w = np.where(dec[:, p] > 0, a, b)
        np.add.at(sure, (np.flatnonzero(cert), w[cert]), 1)
        for c in (a, b):
            np.add.at(maybe, (np.flatnonzero(~cert), np.full(int((~cert).sum()), c)), 1)
    best = np.argmax(sure, 1)
    r = np.arange(Q)
    rival = sure + maybe
    rival[r, best] = -1
    return sure[r, best] > rival.max(1), best


def clusters(n_class, D=32, per_class=20, Q=400, seed=0):
    """The Gaussian family of the label rule: centres 1.0 N(0, I), unit noise -> (bank fp32 sorted by class, labels 1 ..,
    queries fp32, their classes)."""
    rng = np.random.RandomState(777 + 31 * n_class + seed)
    centres = rng.standard_normal((n_class, D))
    by = np.repeat(np.arange(n_class), per_class)
    qy = rng.randint(0, n_class, Q)
    bank = (centres[by] + rng.standard_normal((by.size, D))).astype(F32)
    qs = (centres[qy] + rng.standard_normal((Q, D))).astype(F32)
    return bank, (by + 1).astype(np.int64), qs, (qy + 1).astype(np.int64)


def pair_case(na, nb, D=8, seed=0, spread=1.0):
    """Two overlapping Gaussian classes -> fp32 [na + nb, D], class a first."""
    rng = np.random.RandomState(5 + 1009 * seed + 7 * na + nb)
    x = rng.standard_normal((na + nb, D))
    x[:na] += spread * rng.standard_normal(D)
    return x.astype(F32)


# ------------------------------------------------------------------ the ABI
def header_fields(hdr, name):
    """[(field, ctype)] of `typedef struct { .. } name;` in the header text; `float gamma[N]` arrays included."""
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
    consts = {k: int(v) for k, v in re.findall(r"#define (HSIMAE_SVM_\w+) (\d+)", hdr)}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)
        for field in m.group(3).split(","):
            field = field.strip()
            arr = re.match(r"(\w+)\[(\w+)\]$", field)
            if arr:
                fields.append((arr.group(1), ctype[m.group(1)] * consts.get(arr.group(2), 0)))
            else:
                fields.append((field, ctypes.c_void_p if m.group(2) else ctype[m.group(1)]))
    return fields


def refusals(lib, _lib):
    """(what, code returned, code expected) of the refusals of the four entry points: all are decided before any launch."""
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    out = []

    def run(fn, struct, ok, table):
        out.append((fn + " params NULL", getattr(lib, fn)(None, None), E_NULL))
        for kw, want in table:
            a = dict(ok)
            a.update(kw)
            out.append((fn + " " + str(kw), getattr(lib, fn)(ctypes.byref(struct(**a)), None), want))

    g16 = lambda *v: (ctypes.c_float * 16)(*v)  # noqa: E731
    run("hsimae_svm_gram", _lib.SvmGramParams,
        dict(x=1 << 20, ldx=16, M=10, D=12, n_gamma=2, gamma=g16(0.5, 1.0), K=1 << 21, ldk=12, sumsq=1 << 22),
        [(dict(M=-1), E_DIMS), (dict(D=0), E_DIMS), (dict(D=10), E_DIMS), (dict(ldx=8), E_DIMS), (dict(ldk=9), E_DIMS),
         (dict(n_gamma=0), E_DIMS), (dict(gamma=g16(0.5, 0.0)), E_DIMS), (dict(gamma=g16(float("nan"), 1.0)), E_DIMS),
         (dict(gamma=g16(0.5, float("inf"))), E_DIMS), (dict(gamma=g16(-1.0, 1.0)), E_DIMS),
         (dict(M=8193, ldk=8196), E_UNSUPPORTED), (dict(D=4100, ldx=4100), E_UNSUPPORTED), (dict(n_gamma=17), E_UNSUPPORTED),
         (dict(x=None), E_NULL), (dict(K=None), E_NULL), (dict(sumsq=None), E_NULL),
         (dict(x=(1 << 20) + 4), E_ALIGN), (dict(ldx=18), E_ALIGN), (dict(K=(1 << 21) + 2), E_ALIGN), (dict(sumsq=(1 << 22) + 1), E_ALIGN),
         (dict(M=0, ldk=0), 0), (dict(M=0, ldk=0, x=None, K=None, sumsq=None), 0)])
    run("hsimae_svm_solve", _lib.SvmSolveParams,
        dict(K=1 << 20, ldk=12, M=10, n_k=1, table=1 << 21, n_problems=3, resume=0, max_iter=100, eps=1e-3, alpha=1 << 22, grad=1 << 23,
             alpha_len=60, state=1 << 24),
        [(dict(n_problems=-1), E_DIMS), (dict(M=0), E_DIMS), (dict(ldk=9), E_DIMS), (dict(n_k=0), E_DIMS), (dict(max_iter=-1), E_DIMS),
         (dict(eps=0.0), E_DIMS), (dict(eps=float("nan")), E_DIMS), (dict(eps=float("inf")), E_DIMS), (dict(alpha_len=-1), E_DIMS),
         (dict(M=8193, ldk=8196), E_UNSUPPORTED),
         (dict(K=None), E_NULL), (dict(table=None), E_NULL), (dict(alpha=None), E_NULL), (dict(grad=None), E_NULL), (dict(state=None), E_NULL),
         (dict(K=(1 << 20) + 2), E_ALIGN), (dict(table=(1 << 21) + 4), E_ALIGN), (dict(alpha=(1 << 22) + 4), E_ALIGN),
         (dict(grad=(1 << 23) + 4), E_ALIGN), (dict(state=(1 << 24) + 4), E_ALIGN),
         (dict(n_problems=0), 0), (dict(n_problems=0, K=None, table=None, alpha=None, grad=None, state=None), 0)])
    run("hsimae_svm_pack", _lib.SvmPackParams,
        dict(table=1 << 20, first_problem=0, n_class=3, alpha=1 << 21, alpha_len=60, state=1 << 22, x=1 << 23, ldx=16, M=10, D=12,
             sumsq=1 << 24, sv_index=1 << 25, sv_start=1 << 26, coef=1 << 27, ldc=10, rho=1 << 28, sv=1 << 29, ldsv=12, sv_sumsq=1 << 30),
        [(dict(first_problem=-1), E_DIMS), (dict(n_class=1), E_DIMS), (dict(M=0), E_DIMS), (dict(D=0), E_DIMS), (dict(ldx=8), E_DIMS),
         (dict(ldsv=8), E_DIMS), (dict(ldc=9), E_DIMS), (dict(alpha_len=-1), E_DIMS),
         (dict(n_class=33), E_UNSUPPORTED), (dict(M=8193, ldc=8193), E_UNSUPPORTED),
         (dict(table=None), E_NULL), (dict(alpha=None), E_NULL), (dict(state=None), E_NULL), (dict(x=None), E_NULL), (dict(sumsq=None), E_NULL),
         (dict(sv_index=None), E_NULL), (dict(sv_start=None), E_NULL), (dict(coef=None), E_NULL), (dict(rho=None), E_NULL),
         (dict(sv=None), E_NULL), (dict(sv_sumsq=None), E_NULL),
         (dict(table=(1 << 20) + 4), E_ALIGN), (dict(alpha=(1 << 21) + 4), E_ALIGN), (dict(sv_start=(1 << 26) + 2), E_ALIGN),
         (dict(coef=(1 << 27) + 1), E_ALIGN)])
    run("hsimae_svm_predict", _lib.SvmPredictParams,
        dict(q=1 << 20, ldq=16, Q=4, D=12, sv=1 << 21, ldsv=12, sv_sumsq=1 << 22, sv_start=1 << 23, S_max=10, coef=1 << 24, ldc=10,
             rho=1 << 25, n_class=3, first=1, gamma=0.5, H=2, W=2, p0=0, pixels=None, label_map=1 << 26, conf_map=1 << 27,
             margin_map=1 << 28, probs=1 << 29, ldp=4, decision=1 << 30, ldd=3, outside=1 << 31),
        [(dict(Q=-1), E_DIMS), (dict(D=0), E_DIMS), (dict(D=10), E_DIMS), (dict(ldq=8), E_DIMS), (dict(ldsv=8), E_DIMS), (dict(S_max=-1), E_DIMS),
         (dict(ldc=9), E_DIMS), (dict(n_class=1), E_DIMS), (dict(first=-1), E_DIMS), (dict(H=0), E_DIMS), (dict(W=0), E_DIMS),
         (dict(gamma=0.0), E_DIMS), (dict(gamma=float("nan")), E_DIMS), (dict(gamma=float("inf")), E_DIMS), (dict(ldp=3), E_DIMS),
         (dict(ldd=2), E_DIMS),
         (dict(n_class=33, ldp=40, ldd=600), E_UNSUPPORTED), (dict(D=4100, ldq=4100, ldsv=4100), E_UNSUPPORTED),
         (dict(S_max=8193, ldc=8196), E_UNSUPPORTED),
         (dict(q=None), E_NULL), (dict(sv=None), E_NULL), (dict(sv_sumsq=None), E_NULL), (dict(sv_start=None), E_NULL),
         (dict(coef=None), E_NULL), (dict(rho=None), E_NULL), (dict(label_map=None), E_NULL),
         (dict(q=(1 << 20) + 4), E_ALIGN), (dict(sv=(1 << 21) + 8), E_ALIGN), (dict(ldq=18), E_ALIGN), (dict(ldsv=14), E_ALIGN),
         (dict(pixels=(1 << 32) + 4), E_ALIGN), (dict(label_map=(1 << 26) + 4), E_ALIGN), (dict(conf_map=(1 << 27) + 2), E_ALIGN),
         (dict(probs=(1 << 29) + 2), E_ALIGN), (dict(decision=(1 << 30) + 1), E_ALIGN), (dict(outside=(1 << 31) + 2), E_ALIGN),
         (dict(Q=0), 0), (dict(Q=0, q=None, label_map=None), 0)])
    return out
