"""fp64 restatement, fp32 emulation and error bounds for csrc/probe.hip (tests/test_gpu_probe.py, tests/test_probe_bound_cpu.py):
the linear probe's column statistics and standardised operands, one AdamW iteration (forward, gradient partials, update, state
block), the logits and the head folded back to the raw features.

A plain module, not a conftest.  U = 2^-24, E53 = 2^-53, TINY = 2^-120 (cls_ref.py).  Nothing is tuned on a GPU result: every bound
is a first-order worst case of what the kernels round, and every stage is checked from what the stage before it actually
produced (the device's own fp32 arrays are the next stage's exact inputs), so no bound has to carry an earlier stage's error.

prepare   per column, fp64 chains over the nv valid rows: |mean - mu| <= U |mu| + nv E53 mean|x|;  rstd: U r + 4 nv E53 r, r = 1 /
          sqrt(var + eps32).  xs = fl(fl(x - mean) rstd) is two IEEE operations on the stored mean and rstd: BIT-EXACT; xt = xs^T.
forward   z_ic: the fmaf chain over Kp terms: bz = gamma_Kp sum_k |xs w|, gamma_K = K U / (1 - K U) (knn_ref's bound).
          t = z_c - m; arg = fl(fl(t) fl(log2 e)): two roundings and the constant (0.24 U): e_c within e_c (2.25 |t| U + 2 U (v_exp_f32,
          1 ulp) + bz_c + bz_max) of exp(t64) (the last two: the error of the difference of two logits);
          sum: at most one term per lane, 6 tree steps: dsum <= sum de + 6 U sum;  inv = 1 / sum (U), p = e inv (U);
          g = fl(fl(p - [c = y]) fl(1 / nv)): dg <= (dp + 3 U |p - [c = y]|) / nv + TINY.
          loss_i = log(sum) - (z_y - m) in fp64 from fp32 values: dsum / sum + bz_y + bz_max; the mean adds n E53.
gradient  scratch[s][c][k]: the fmaf chain over the segment's len rows: gamma_len sum_i |g x|.
update    dW = scratch[0] + scratch[1] + .. in fp32, ascending: IEEE additions of the stored partials: the AdamW element is checked
          against elem_ref.adamw_ref fed exactly that dW (its bound C_ADAM U term, as groups_ref / clip_ref use it), and
          ||dW||^2 = the fp64 sum of its squares within (64 Kp) E53 of it: a partial sum formed in another order (a swapped segment
          order) moves dW by ulps of fp32, 10^5 times that bound.
fold      weight = fl(w rstd): U |w rstd|;  bias: fp64 chain, one fp32 rounding: U |b| + D E53 sum |w mean rstd|.

Trajectory: T steps on the device against fit_ref (fp64 throughout from the fp32 inputs).  The gate per element of w is TRAJ_MARGIN
times the largest deviation, over the elements of w, of the CPU emulation (emulate_fit: every fp32 operation of the kernels in
their order) from fit_ref at the same inputs.  TRAJ_MARGIN = 16: the device's operations err at most twice what the emulation's
do (v_exp_f32 is 1 ulp where the emulated exp2 is rounded correctly; the compiler may contract a multiply-add the emulation
rounds twice): 2; the emulation is ONE realisation of the rounding noise and the device another, and the largest of ~10^3 .. 10^4
elements of one realisation against the other's: 4; and 2 for safety.  The gate is never derived from a GPU result.
"""
import ctypes
import math

import numpy as np
import torch

from cls_ref import TINY, U, ratio  # noqa: F401
from elem_ref import adamw_ref
from knn_ref import LOG2E32, LOG2E_REL, clusters, header_fields  # noqa: F401

F32 = np.float32
E53 = 2.0 ** -53
SEG = 256                    # HSIMAE_PROBE_SEG
ROWS = 64                    # HSIMAE_PROBE_ROWS
ARG = 2.0 + math.ceil(100 * LOG2E_REL / U) / 100          # 2.25: two roundings of the argument + the constant's own error
TRAJ_MARGIN = 16.0           # (module docstring)
NS = [1, 63, 64, 65, 255, 256, 257, 600]
DS = [4, 32, 36, 132]
CLASSES = [(2, 0), (8, 1), (64, 1)]
HP = dict(lr=0.05, wd=0.05, b1=0.9, b2=0.999, eps=1e-8)    # the step cases: lr wd = 2.5e-3 per step, far above 3 U: a decayed bias shows
BN_EPS = 1e-6


def f32(a):
    return float(F32(a))


def gamma(K):
    return K * U / (1 - K * U)


def rup4(n):
    return (n + 3) // 4 * 4


def valid_of(y, first, C):
    y = np.asarray(y, np.int64)
    return (y >= first) & (y < C)


def lr_at(lr, t, T, schedule="cosine"):
    """LinearProbe.lr_at: the host's fp64 value (the launch rounds it to fp32)."""
    return lr * 0.5 * (1.0 + math.cos(math.pi * t / T)) if schedule == "cosine" else lr


# ------------------------------------------------------------------ fp64 restatement
def prepare_ref(x, y, D, C, first, eps=BN_EPS):
    """-> dict: mean, rstd fp64 [D] and their bounds, valid [n], nv, bad, xs fp64 [n, D + 1] (column D = 1; invalid rows 0)."""
    xx = np.asarray(x)[:, :D].astype(np.float64)
    valid = valid_of(y, first, C)
    nv = int(valid.sum())
    if nv:
        mu = xx[valid].mean(0)
        var = ((xx[valid] - mu) ** 2).mean(0)
        r = 1.0 / np.sqrt(var + f32(eps))
        absmean = np.abs(xx[valid]).mean(0)
    else:
        mu, r, absmean = np.zeros(D), np.zeros(D), np.zeros(D)
    xs = np.zeros((xx.shape[0], D + 1))
    xs[valid, :D] = (xx[valid] - mu) * r
    xs[valid, D] = 1.0
    return {"mean": mu, "mean_bound": U * np.abs(mu) + nv * E53 * absmean + TINY, "rstd": r, "rstd_bound": U * r + 4 * nv * E53 * r,
            "valid": valid, "nv": nv, "bad": int((~valid).sum()), "xs": xs}


def forward_ref(xs, w, y, first, C, nv=None):
    """xs [n, K] (fp64, or the device's fp32 operand), w [C', K] -> dict: z [n, C], g [n, C] (0 below first and for invalid rows),
    loss (mean over the nv valid rows) and the bounds g_bound, loss_bound for fp32 inputs."""
    xs, w = np.asarray(xs).astype(np.float64), np.asarray(w)[:C].astype(np.float64)
    K = min(xs.shape[1], w.shape[1])
    xs, w = xs[:, :K], w[:, :K]
    n = xs.shape[0]
    valid = valid_of(y, first, C)
    nv = int(valid.sum()) if nv is None else nv
    z = xs @ w.T
    bz = gamma(K) * (np.abs(xs) @ np.abs(w).T)
    zr, bzr = z[:, first:], bz[:, first:]
    m = zr.max(1, keepdims=True)
    t = zr - m
    e = np.exp(t)
    s = e.sum(1, keepdims=True)
    p = e / s
    bzmax = bzr.max(1, keepdims=True)
    de = e * (ARG * np.abs(t) * U + 2 * U + bzr + bzmax) + TINY
    dsum = de.sum(1, keepdims=True) / s + 6 * U
    dp = de / s + p * (dsum + 2 * U)
    yc = np.where(valid, np.asarray(y, np.int64) - first, 0)
    rows = np.arange(n)
    oh = np.zeros_like(p)
    oh[rows, yc] = 1.0
    inv_n = 1.0 / nv if nv else 0.0
    g, gb = np.zeros((n, C)), np.zeros((n, C))
    g[:, first:] = np.where(valid[:, None], (p - oh) * inv_n, 0.0)
    gb[:, first:] = np.where(valid[:, None], (dp + 3 * U * np.abs(p - oh)) * inv_n + TINY, 0.0)
    li = np.log(s[:, 0]) - t[rows, yc]
    bli = dsum[:, 0] + bzr[rows, yc] + bzmax[:, 0]
    loss = float(li[valid].sum() * inv_n)
    lb = float(bli[valid].sum() * inv_n + (n + 4) * E53 * np.abs(li[valid]).sum() * inv_n)
    return {"z": z, "z_bound": bz, "g": g, "g_bound": gb, "loss": loss, "loss_bound": lb, "p": p}


def segments(n):
    return [(s0, min(SEG, rup4(n) - s0)) for s0 in range(0, n, SEG)]


def grad_ref(gt, xt, n):
    """gt [64, ldn], xt [Kp, ldn] (the device's fp32 arrays) -> (scratch fp64 [S, 64, Kp], bound)."""
    g, x = np.asarray(gt).astype(np.float64), np.asarray(xt).astype(np.float64)
    out, bound = [], []
    for s0, ln in segments(n):
        out.append(g[:, s0:s0 + ln] @ x[:, s0:s0 + ln].T)
        bound.append(gamma(ln) * (np.abs(g[:, s0:s0 + ln]) @ np.abs(x[:, s0:s0 + ln]).T))
    return np.stack(out), np.stack(bound)


def ascending_sum32(scratch, descending=False):
    """dW as probe_update_kernel forms it: the partials added in fp32 in ascending segment order, from the first."""
    sc = np.asarray(scratch, F32)
    order = range(sc.shape[0] - 1, -1, -1) if descending else range(sc.shape[0])
    acc = None
    for s in order:
        acc = sc[s].copy() if acc is None else acc + sc[s]
    return acc


def groups_of(D, Kp, C, first):
    """elem_ref.adamw_ref's group per element of [64, Kp]: 0 decayed weight, 1 the bias column (no decay), 2 never touched."""
    grp = np.full((ROWS, Kp), 2, np.uint8)
    grp[first:C, :D] = 0
    grp[first:C, D] = 1
    return torch.from_numpy(grp)


def update_ref(dw32, w, m, v, D, C, first, step, hp):
    """-> elem_ref's {p, m, v} Outs for the [64, Kp] arrays, and ||dW||^2 with its bound."""
    Kp = dw32.shape[1]
    grp = groups_of(D, Kp, C, first)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, F32)))                # noqa: E731
    out = adamw_ref(t(w), t(dw32), t(m), t(v), grp, step, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"])
    live = (grp != 2).numpy()
    sq = float((np.asarray(dw32, np.float64)[live] ** 2).sum())
    return out, sq, ROWS * Kp * E53 * sq


def fold_ref(w, mean, rstd, D, C, first):
    w, mean, rstd = (np.asarray(a).astype(np.float64) for a in (w, mean, rstd))
    W = np.zeros((C, D))
    b = np.zeros(C)
    W[first:] = w[first:C, :D] * rstd
    b[first:] = w[first:C, D] - (w[first:C, :D] * mean * rstd).sum(1)
    bb = np.zeros(C)
    bb[first:] = U * np.abs(b[first:]) + (D + 2) * E53 * (np.abs(w[first:C, :D] * mean * rstd).sum(1) + np.abs(w[first:C, D])) + TINY
    return W, U * np.abs(W) + TINY, b, bb


def adamw64(p, g, m, v, step, lr, wd, b1, b2, eps, decay):
    """torch.optim.AdamW's element in fp64 (decay: the mask of decayed elements) -> (p, m, v)."""
    p = np.where(decay, p * (1 - lr * wd), p)
    m = m + (g - m) * (1 - b1)
    v = v * b2 + g * g * (1 - b2)
    den = np.sqrt(v) / math.sqrt(1 - b2 ** step) + eps
    return p - lr / (1 - b1 ** step) * m / den, m, v


def step_ref(xs, y, W, M, V, first, C, step, lr, hp):
    """One iteration in fp64 on W, M, V [C, D + 1] (rows below first stay 0) -> (W, M, V, loss, dW)."""
    f = forward_ref(xs, W, y, first, C)
    dW = f["g"].T @ xs
    dW[:first] = 0.0
    decay = np.ones_like(W, bool)
    decay[:, -1] = False
    Wn, Mn, Vn = adamw64(W, dW, M, V, step, f32(lr), f32(hp["wd"]), f32(hp["b1"]), f32(hp["b2"]), f32(hp["eps"]), decay)
    Wn[:first], Mn[:first], Vn[:first] = 0.0, 0.0, 0.0
    return Wn, Mn, Vn, f["loss"], dW


def fit_ref(x, y, D, C, first, T, hp, schedule="cosine", bn_eps=BN_EPS):
    """The whole fit in fp64 from the fp32 inputs (hyper-parameters as the fp32 values the launches carry)
    -> dict: w [C, D + 1], losses [T], mean, rstd, grad_norm."""
    pr = prepare_ref(x, y, D, C, first, bn_eps)
    W = np.zeros((C, D + 1))
    M, V = np.zeros_like(W), np.zeros_like(W)
    losses = []
    for t in range(T):
        W, M, V, loss, dW = step_ref(pr["xs"], y, W, M, V, first, C, t + 1, lr_at(hp["lr"], t, T, schedule), hp)
        losses.append(loss)
    return {"w": W, "losses": np.array(losses), "mean": pr["mean"], "rstd": pr["rstd"], "grad_norm": float(np.sqrt((dW ** 2).sum()))}


def logits_ref(x, mean, rstd, w, D, C, first):
    """Logits of raw rows in fp64 from a restated fit (w [C, D + 1]); columns below first are 0."""
    xs = (np.asarray(x)[:, :D].astype(np.float64) - mean) * rstd
    z = xs @ np.asarray(w)[:C, :D].T + np.asarray(w)[:C, D]
    z[:, :first] = 0.0
    return z


# ------------------------------------------------------------------ the kernels' fp32 sequences
def emulate_prepare(x, y, D, C, first, eps=BN_EPS):
    xx = np.asarray(x, F32)[:, :D]
    n, Kp, ldn = xx.shape[0], D + 4, rup4(xx.shape[0])
    valid = valid_of(y, first, C)
    nv = int(valid.sum())
    if nv:
        x64 = xx[valid].astype(np.float64)
        mu = np.cumsum(x64, axis=0)[-1] / nv                     # (cumsum adds in order)
        ss = np.cumsum((x64 - mu) ** 2, axis=0)[-1]
        mean, rstd = mu.astype(F32), (1.0 / np.sqrt(ss / nv + float(F32(eps)))).astype(F32)
    else:
        mean, rstd = np.zeros(D, F32), np.zeros(D, F32)
    return {"mean": mean, "rstd": rstd, **operands(xx, valid, mean, rstd), "bad": n - nv, "nv": nv}


def operands(x, valid, mean, rstd):
    """xs fp32 [n, Kp] and xt fp32 [Kp, rup4(n)] from the STORED mean and rstd: two IEEE operations per element."""
    xx = np.asarray(x, F32)
    n, D = xx.shape
    xs = np.zeros((n, D + 4), F32)
    with np.errstate(all="ignore"):
        xs[:, :D] = (xx - np.asarray(mean, F32)) * np.asarray(rstd, F32)
    xs[:, D] = 1
    xs[~valid] = 0
    xt = np.zeros((D + 4, rup4(n)), F32)
    xt[:, :n] = xs.T
    return {"xs": xs, "xt": xt}


def chain32(a, b):
    """[r, K] x [c, K] -> [r, c]: the k-ordered fmaf chain from +0, every step rounded to fp32 (through fp64)."""
    a64, b64 = np.asarray(a, F32).astype(np.float64), np.asarray(b, F32).astype(np.float64)
    acc = np.zeros((a64.shape[0], b64.shape[0]), F32)
    for k in range(a64.shape[1]):
        acc = (a64[:, k:k + 1] * b64[None, :, k] + acc.astype(np.float64)).astype(F32)
    return acc


def emulate_forward(xs, w, y, first, C, nv, fault=None):
    """-> (gt fp32 [64, rup4(n)], loss (the mean, as probe_finish_kernel forms it), z fp32 [n, 64])."""
    xs, w = np.asarray(xs, F32), np.asarray(w, F32)
    n = xs.shape[0]
    z = chain32(xs, w)
    valid = valid_of(y, first, C)
    lo = 0 if fault == "class0_in_softmax" else first
    zr = z[:, lo:C]
    m = zr.max(1, keepdims=True)
    e = np.exp2(((zr - m) * LOG2E32).astype(np.float64)).astype(F32)
    lanes = np.zeros((n, 64), F32)
    lanes[:, :C - lo] = e
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, idx ^ s]
    total = lanes[:, :1]
    p = e * (F32(1) / total)
    denom = nv - 1 if fault == "n_minus_1" else nv
    inv_n = F32(1.0 / denom) if denom > 0 else F32(0)
    rows = np.arange(n)
    yc = np.where(valid, np.asarray(y, np.int64) - lo, 0)
    oh = np.zeros_like(p)
    oh[rows, yc] = 1
    g = np.zeros((n, 64), F32)
    g[:, lo:C] = np.where(valid[:, None], (p - oh) * inv_n, F32(0))
    g[:, :first] = 0
    gt = np.zeros((64, rup4(n)), F32)
    gt[:, :n] = g.T
    li = np.where(valid, np.log(total[:, 0].astype(np.float64)) - (zr[rows, yc].astype(np.float64) - m[:, 0].astype(np.float64)), 0.0)
    parts = []
    for i0 in range(0, n, 64):                                   # a wave adds its 16 rows in order, the four waves in order
        wv = [0.0] * 4
        for r in range(i0, min(n, i0 + 64)):
            wv[(r - i0) // 16] += li[r]
        parts.append(((wv[0] + wv[1]) + wv[2]) + wv[3])
    return gt, lane_tree64(parts) / nv if nv else 0.0, z


def lane_tree64(parts):
    """probe_finish_kernel: lane l adds the partials l, l + 64, .. in order; the xor tree adds the lanes."""
    lanes = np.zeros(64)
    for g, v in enumerate(parts):
        lanes[g % 64] += v
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[idx ^ s]
    return float(lanes[0])


def emulate_grad(gt, xt, n):
    gt, xt = np.asarray(gt, F32), np.asarray(xt, F32)
    return np.stack([chain32(gt[:, s0:s0 + ln], xt[:, s0:s0 + ln]) for s0, ln in segments(n)])


def emulate_update(scratch, w, m, v, D, C, first, step, lr, hp, fault=None):
    """adamw_one's operation order in fp32 -> (w, m, v fp32 [64, Kp], ||dW||^2)."""
    dw = ascending_sum32(scratch, descending=fault == "seg_swapped")
    Kp = dw.shape[1]
    live = np.zeros((ROWS, Kp), bool)
    live[first:C, :D + 1] = True
    decay = live.copy()
    if fault != "bias_decayed":
        decay[:, D] = False
    lr, wd, b1, b2, eps = (F32(a) for a in (lr, hp["wd"], hp["b1"], hp["b2"], hp["eps"]))
    i1 = F32(1.0 / (1.0 - float(b1) ** step))
    i2 = F32(1.0 / math.sqrt(1.0 - float(b2) ** step))
    w, m, v = (np.asarray(a, F32) for a in (w, m, v))
    one = F32(1)
    with np.errstate(all="ignore"):
        x = np.where(decay, w * (one - lr * wd), w)
        mn = m + (dw - m) * (one - b1)
        vn = v * b2 + dw * dw * (one - b2)
        den = np.sqrt(vn) * i2 + eps
        pn = x - lr * i1 * (mn / den)
    sq = float((dw.astype(np.float64)[live] ** 2).sum())
    return np.where(live, pn, w), np.where(live, mn, m), np.where(live, vn, v), sq


def emulate_step(pre, y, w, m, v, D, C, first, step, lr, hp, fault=None):
    """One hsimae_probe_step on the emulated (or the device's) operands `pre` -> dict of everything the launch leaves."""
    n = pre["xs"].shape[0]
    gt, loss, _ = emulate_forward(pre["xs"], w, y, first, C, pre["nv"], fault)
    scratch = emulate_grad(gt, pre["xt"], n)
    wn, mn, vn, sq = emulate_update(scratch, w, m, v, D, C, first, step, lr, hp, fault)
    return {"gt": gt, "scratch": scratch, "w": wn, "m": mn, "v": vn,
            "state": np.array([loss, step, sq, pre["bad"], pre["nv"], 0, 0, 0], np.float64)}


def emulate_fit(x, y, D, C, first, T, hp, schedule="cosine", bn_eps=BN_EPS):
    pre = emulate_prepare(x, y, D, C, first, bn_eps)
    w, m, v = (np.zeros((ROWS, D + 4), F32) for _ in range(3))
    losses = []
    for t in range(T):
        o = emulate_step(pre, y, w, m, v, D, C, first, t + 1, lr_at(hp["lr"], t, T, schedule), hp)
        w, m, v = o["w"], o["m"], o["v"]
        losses.append(o["state"][0])
    return {"w": w, "losses": np.array(losses), "mean": pre["mean"], "rstd": pre["rstd"]}


# ------------------------------------------------------------------ the checks (the same for the emulation and the device)
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int32), b.view(np.int32)))


def check_prepare(got, x, y, D, C, first, eps=BN_EPS):
    """got: dict mean, rstd, xs [n, Kp], xt [Kp, >= rup4(n)], state [8] -> dict of worst ratios and exact verdicts; `ok`."""
    ref = prepare_ref(x, y, D, C, first, eps)
    n = np.asarray(x).shape[0]
    ops = operands(np.asarray(x, F32)[:, :D], ref["valid"], got["mean"], got["rstd"])
    out = {"mean": ratio(got["mean"], ref["mean"], ref["mean_bound"]), "rstd": ratio(got["rstd"], ref["rstd"], ref["rstd_bound"]),
           "xs_exact": same_bits(got["xs"], ops["xs"]), "xt_exact": same_bits(np.asarray(got["xt"])[:, :rup4(n)], ops["xt"]),
           "state": bool(np.array_equal(np.asarray(got["state"], np.float64), [0, 0, 0, ref["bad"], ref["nv"], 0, 0, 0]))}
    out["ok"] = out["mean"] <= 1 and out["rstd"] <= 1 and out["xs_exact"] and out["xt_exact"] and out["state"]
    return out


def check_step(got, pre, y, w, m, v, D, C, first, step, lr, hp):
    """got: what one hsimae_probe_step left (gt, scratch, w, m, v, state); pre: the operands it ran on (xs, xt, nv, bad); w, m, v:
    its inputs -> dict of the stages' worst ratios and exact verdicts; `ok` when every ratio is <= 1 and every verdict holds."""
    n, Kp = pre["xs"].shape
    f = forward_ref(pre["xs"], np.asarray(w)[:, :Kp], y, first, C, pre["nv"])
    gt = np.asarray(got["gt"])[:, :rup4(n)]
    gfull, gbound = np.zeros((ROWS, rup4(n))), np.zeros((ROWS, rup4(n)))
    gfull[:C, :n], gbound[:C, :n] = f["g"].T, f["g_bound"].T
    out = {"g": ratio(gt, gfull, gbound), "loss": ratio(got["state"][0], f["loss"], f["loss_bound"])}
    s64, sb = grad_ref(gt, np.asarray(pre["xt"])[:, :rup4(n)], n)
    out["scratch"] = ratio(got["scratch"], s64, sb)
    dw = ascending_sum32(got["scratch"])
    ref, sq, sqb = update_ref(dw, w, m, v, D, C, first, step, dict(hp, lr=lr))
    for key, name in (("p", "w"), ("m", "m"), ("v", "v")):
        out[name] = ref[key].ratio(torch.from_numpy(np.ascontiguousarray(got[name], F32)))
    out["norm"] = ratio(got["state"][2], sq, sqb)
    st = np.asarray(got["state"], np.float64)
    out["state"] = bool(st[1] == step and st[3] == pre["bad"] and st[4] == pre["nv"] and not st[5:].any())
    out["ok"] = all(out[k] <= 1 for k in ("g", "loss", "scratch", "w", "m", "v", "norm")) and out["state"]
    return out


# ------------------------------------------------------------------ cases
def step_case(n, D, C, first, ldx=None, seed=0):
    """x fp32 [n, ldx] (NaN in the pad columns; column 1 constant when D > 1; columns of unequal scale and offset), labels int64
    [n] in [first, C) (with C - first >= 3 the last class has no member; with n >= 4 row 2 carries the label C: a bad one), and
    w, m, v fp32 [64, D + 4] of a fit under way (zeros outside rows [first, C) and behind column D)."""
    ldx = D if ldx is None else ldx
    rng = np.random.RandomState(9176 * seed + 131 * n + 7 * D + C)
    scale = np.exp(rng.uniform(-2, 2, D))
    x = (rng.standard_normal((n, ldx)) * np.r_[scale, np.ones(ldx - D)] + np.r_[3 * rng.standard_normal(D), np.zeros(ldx - D)]).astype(F32)
    if D > 1:
        x[:, 1] = F32(0.7)
    x[:, D:] = np.nan
    hi = C - 1 if C - first >= 3 else C
    y = rng.randint(first, hi, n).astype(np.int64)
    if n >= 4:
        y[2] = C
    w, m, v = (np.zeros((ROWS, D + 4), F32) for _ in range(3))
    w[first:C, :D + 1] = 0.3 * rng.standard_normal((C - first, D + 1))
    m[first:C, :D + 1] = 0.01 * rng.standard_normal((C - first, D + 1))
    v[first:C, :D + 1] = 1e-4 * rng.rand(C - first, D + 1)
    return x, y, w, m, v


def traj_case(n=300, D=36, C=8, first=1, seed=0):
    """A separable-ish bank for the trajectory test: class centres 1.5 apart in scale, unit noise."""
    rng = np.random.RandomState(515 + seed)
    y = rng.randint(first, C, n).astype(np.int64)
    centres = 1.5 * rng.standard_normal((C, D))
    return (centres[y] + rng.standard_normal((n, D))).astype(F32), y


TRAJ_HP = dict(lr=1e-2, wd=1e-4, b1=0.9, b2=0.999, eps=1e-8)    # LinearProbe's defaults
TRAJ_STEPS = 20


# ------------------------------------------------------------------ the head GEMM's operand rounding
UB = 2.0 ** -9               # bf16: 8 significand bits, round to nearest


def head_bound(x, weight, bias):
    """|model.head logits - the fp64 product of the fp32 folded head| at most: both operands of the head GEMM are rounded to bf16
    (2 UB + UB^2 per product), the K products are accumulated in fp32 in some order (gamma_K), the bias is added in fp32 (U)."""
    x, weight = np.asarray(x).astype(np.float64), np.asarray(weight).astype(np.float64)
    K = x.shape[1]
    mag = np.abs(x) @ np.abs(weight).T
    z = x @ weight.T + np.asarray(bias, np.float64)
    return (2 * UB + UB * UB + gamma(K + 1)) * mag + 2 * U * np.abs(z) + TINY


# ------------------------------------------------------------------ the ABI
def refusals(lib, _lib):
    """(what, code returned, code expected) of every refusal of the four entry points: all are decided before any launch."""
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    out = []

    def run(fn, struct, ok, table):
        out.append((fn + " params NULL", getattr(lib, fn)(None, None), E_NULL))
        for kw, want in table:
            a = dict(ok)
            a.update(kw)
            out.append((fn + " " + str(kw), getattr(lib, fn)(ctypes.byref(struct(**a)), None), want))

    shape = [(dict(n=-1), E_DIMS), (dict(D=0), E_DIMS), (dict(D=10), E_DIMS), (dict(C=1, first=0), E_DIMS), (dict(first=-1), E_DIMS),
             (dict(first=8), E_DIMS), (dict(Kp=12), E_DIMS), (dict(Kp=20), E_DIMS), (dict(C=65), E_UNSUPPORTED),
             (dict(D=4100, Kp=4104), E_UNSUPPORTED)]
    big = (1 << 20) + 1
    run("hsimae_probe_prepare", _lib.ProbePrepareParams,
        dict(x=1 << 20, ldx=16, labels=1 << 21, n=30, D=12, C=8, first=1, eps=1e-6, mean=1 << 22, rstd=1 << 23, xs=1 << 24, Kp=16,
             xt=1 << 25, ldn=32, state=1 << 26),
        shape + [(dict(ldx=8), E_DIMS), (dict(ldn=28), E_DIMS), (dict(eps=0.0), E_DIMS), (dict(eps=float("nan")), E_DIMS),
                 (dict(eps=float("inf")), E_DIMS), (dict(n=big, ldn=big + 3), E_UNSUPPORTED),
                 (dict(x=None), E_NULL), (dict(labels=None), E_NULL), (dict(mean=None), E_NULL), (dict(rstd=None), E_NULL),
                 (dict(xs=None), E_NULL), (dict(xt=None), E_NULL), (dict(state=None), E_NULL),
                 (dict(x=(1 << 20) + 4), E_ALIGN), (dict(xs=(1 << 24) + 8), E_ALIGN), (dict(xt=(1 << 25) + 4), E_ALIGN),
                 (dict(ldx=18), E_ALIGN), (dict(ldn=34), E_ALIGN), (dict(labels=(1 << 21) + 4), E_ALIGN),
                 (dict(mean=(1 << 22) + 4), E_ALIGN), (dict(state=(1 << 26) + 4), E_ALIGN),
                 (dict(n=0), 0), (dict(n=0, x=None, labels=None, xs=None, xt=None, state=None), 0)])
    run("hsimae_probe_step", _lib.ProbeStepParams,
        dict(xs=1 << 20, xt=1 << 21, Kp=16, ldn=32, labels=1 << 22, n=30, D=12, C=8, first=1, w=1 << 23, m=1 << 24, v=1 << 25,
             gt=1 << 26, scratch=1 << 27, loss_part=1 << 28, norm_part=1 << 29, lr=0.01, weight_decay=1e-4, b1=0.9, b2=0.999, eps=1e-8,
             step=1, state=1 << 30, loss_hist=1 << 31),
        shape + [(dict(ldn=28), E_DIMS), (dict(step=0), E_DIMS), (dict(lr=-1.0), E_DIMS), (dict(lr=float("nan")), E_DIMS),
                 (dict(weight_decay=-1.0), E_DIMS), (dict(eps=-1.0), E_DIMS), (dict(b1=1.0), E_DIMS), (dict(b2=-0.1), E_DIMS),
                 (dict(n=big, ldn=big + 3), E_UNSUPPORTED),
                 (dict(xs=None), E_NULL), (dict(xt=None), E_NULL), (dict(labels=None), E_NULL), (dict(w=None), E_NULL),
                 (dict(m=None), E_NULL), (dict(v=None), E_NULL), (dict(gt=None), E_NULL), (dict(scratch=None), E_NULL),
                 (dict(loss_part=None), E_NULL), (dict(norm_part=None), E_NULL), (dict(state=None), E_NULL),
                 (dict(xs=(1 << 20) + 4), E_ALIGN), (dict(xt=(1 << 21) + 8), E_ALIGN), (dict(w=(1 << 23) + 4), E_ALIGN),
                 (dict(gt=(1 << 26) + 4), E_ALIGN), (dict(ldn=34), E_ALIGN), (dict(m=(1 << 24) + 2), E_ALIGN),
                 (dict(loss_part=(1 << 28) + 4), E_ALIGN), (dict(state=(1 << 30) + 4), E_ALIGN), (dict(loss_hist=(1 << 31) + 2), E_ALIGN),
                 (dict(n=0), 0), (dict(n=0, xs=None, xt=None, w=None, state=None), 0)])
    run("hsimae_probe_logits", _lib.ProbeLogitsParams,
        dict(x=1 << 20, ldx=16, mean=1 << 21, rstd=1 << 22, w=1 << 23, Kp=16, n=30, D=12, C=8, first=1, z=1 << 24, ldz=8),
        shape + [(dict(ldx=8), E_DIMS), (dict(ldz=7), E_DIMS), (dict(n=big), E_UNSUPPORTED),
                 (dict(x=None), E_NULL), (dict(mean=None), E_NULL), (dict(rstd=None), E_NULL), (dict(w=None), E_NULL), (dict(z=None), E_NULL),
                 (dict(x=(1 << 20) + 4), E_ALIGN), (dict(w=(1 << 23) + 8), E_ALIGN), (dict(mean=(1 << 21) + 4), E_ALIGN),
                 (dict(ldx=18), E_ALIGN), (dict(z=(1 << 24) + 2), E_ALIGN), (dict(n=0), 0), (dict(n=0, x=None, z=None), 0)])
    run("hsimae_probe_fold", _lib.ProbeFoldParams,
        dict(w=1 << 20, Kp=16, mean=1 << 21, rstd=1 << 22, D=12, C=8, first=1, weight=1 << 23, ldw=12, bias=1 << 24),
        [kv for kv in shape if "n" not in kv[0]] +
        [(dict(ldw=8), E_DIMS), (dict(w=None), E_NULL), (dict(mean=None), E_NULL), (dict(rstd=None), E_NULL), (dict(weight=None), E_NULL),
         (dict(bias=None), E_NULL), (dict(w=(1 << 20) + 2), E_ALIGN), (dict(weight=(1 << 23) + 1), E_ALIGN), (dict(bias=(1 << 24) + 2), E_ALIGN)])
    return out
