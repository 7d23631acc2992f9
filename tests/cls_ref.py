"""fp64 restatement and element-wise error bounds for csrc/cls.hip (tests/test_gpu_cls.py, tests/test_cls_bound_cpu.py):
cross-entropy with an ignored class (+ gradient, argmax), the confusion counts and the scores.

A plain module, not a conftest.  The bounds are worst-case first-order bounds of what the kernels round, nothing is tuned on a
GPU result.  With U = 2^-24, d_j = z_j - max z, p = softmax:

  e_j = exp2(fl(fl(d_j) * fl(log2 e)))   three roundings of the argument (3 U |d_j| on e_j), v_exp_f32 1 ulp (2 U)
  s = sum e_j                            per lane ceil(C / 64) terms in order, then 6 shuffle steps: (ceil(C / 64) + 6) U
      => |ds| / s <= SREL = (ceil(C / 64) + 8) U + 3 U sum_j p_j |d_j|
  loss_i = fl(fl(log2(s) * ln 2) - d_y)  v_log_f32 1 ulp + the constant + the product: 4 U |log s|;  U |d_y|;  U |loss_i|
  loss = fl32(fp64 sum / n)              the fp64 sum's own rounding is N 2^-53, then U |loss|
  g_ij = fl(fl(fl(e_j * fl(1 / s)) - onehot) * fl(1 / n))
      => |dg| <= [ p_j (3 |d_j| U + 2 U + SREL + 2 U) + 3 U |p_j - onehot| ] / n
  flushed denormals (v_exp_f32 flushes): 2^-126 per term, absolute.
"""
import math

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -120


def valid_rows(y, C, ignore_index):
    y = np.asarray(y, np.int64)
    return (y != ignore_index) & (y >= 0) & (y < C)


def cls_ref(logits, y, C, ignore_index=0, first=0, ldd=None):
    """logits [N, ld] (columns >= C are pad and not read), y [N] -> dict of fp64 results and bounds:
    loss, loss_bound, n_valid, dlogits [N, ldd], dlogits_bound, pred [N], bad."""
    z = np.asarray(logits)[:, :C].astype(np.float64)
    y = np.asarray(y, np.int64)
    N = z.shape[0]
    ldd = C if ldd is None else ldd
    valid = valid_rows(y, C, ignore_index)
    bad = bool(np.any((y != ignore_index) & ~((y >= 0) & (y < C))))
    n = int(valid.sum())
    yc = np.where(valid, y, 0)
    rows = np.arange(N)
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(z), -np.inf, z).max(1) if N else np.zeros(0)
        d = z - m[:, None]
        e = np.exp(d)
        s = e.sum(1)
        p = e / s[:, None]
        logs = np.log(s)
        li = logs - d[rows, yc]
        oh = np.zeros_like(z)
        oh[rows, yc] = 1.0
        pd_ = (p * np.abs(d))
        pd_[p == 0] = 0.0                                  # 0 * inf at d = -inf
        srel = (math.ceil(C / 64) + 8) * U + 3 * U * pd_.sum(1)
        b_li = U * (np.abs(d[rows, yc]) + 4 * np.abs(logs) + np.abs(li)) + srel + C * TINY
        ad = np.where(p == 0, 0.0, np.abs(d))
        b_g = p * ((3 * ad + 4) * U + srel[:, None]) + 3 * U * np.abs(p - oh) + TINY
        if n:
            loss = li[valid].sum() / n
            loss_bound = b_li[valid].sum() / n + U * abs(loss) + N * U64 * np.abs(li[valid]).sum() / n
        else:
            loss, loss_bound = np.nan, 0.0
        dl = np.zeros((N, ldd))
        db = np.zeros((N, ldd))
        if n:
            dl[valid, :C] = (p - oh)[valid] / n
            db[valid, :C] = b_g[valid] / n
        pred = first + np.argmax(z[:, first:], axis=1) if N else np.zeros(0, np.int64)    # first maximum, first NaN
    return {"loss": loss, "loss_bound": loss_bound, "n_valid": n, "dlogits": dl, "dlogits_bound": db, "pred": pred.astype(np.int64),
            "bad": bad, "valid": valid}


def ratio(got, ref, bound):
    """Worst |got - ref| / bound, element-wise.  NaN where the reference has NaN is agreement; NaN / inf anywhere else, or any
    difference where the bound is 0, is infinitely bad."""
    got, ref, bound = (np.asarray(a, np.float64) for a in np.broadcast_arrays(got, ref, bound))
    if got.size == 0:
        return 0.0
    both_nan = np.isnan(got) & np.isnan(ref)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(both_nan, 0.0, r)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def confusion_ref(gt, pred, C, cm=None, mask=None):
    """-> (cm int64 [C, C] with the counts added, masked pred, bad)."""
    gt, pred = np.asarray(gt, np.int64).reshape(-1), np.asarray(pred, np.int64).reshape(-1)
    cm = np.zeros((C, C), np.int64) if cm is None else cm.copy()
    if mask is not None:
        pred = np.where(np.asarray(mask, np.int64).reshape(-1) != 0, pred, 0)
    keep = gt != 0
    ok = keep & (gt >= 0) & (gt < C) & (pred >= 0) & (pred < C)
    np.add.at(cm, (gt[ok], pred[ok]), 1)
    return cm, pred, bool(np.any(keep & ~ok))


def scores_ref(cm):
    """finetune_train.scores from the counts -> (out fp64 [3 + 2 (C - 1)], bound): OA, AA, kappa, recall_1.., present_1..
    Every count sum is an exact integer; each quotient is one fp64 rounding here and one in the kernel, AA a sum of <= C - 1
    terms in [0, 1] in another order, kappa a quotient of two differences."""
    cm = np.asarray(cm, np.int64)
    C = cm.shape[0]
    row = cm[1:, :].sum(1).astype(np.float64)
    col = cm[1:, 1:].sum(0).astype(np.float64)
    dg = np.diag(cm)[1:].astype(np.float64)
    n = row.sum()
    present = row > 0
    with np.errstate(all="ignore"):
        oa = dg.sum() / n
        rec = np.where(present, dg / np.where(present, row, 1.0), 0.0)
        aa = rec[present].sum() / present.sum() if present.any() else np.nan
        pe = float((row * col).sum()) / (n * n)
        kappa = (oa - pe) / (1 - pe) if pe < 1 else 0.0
        out = np.concatenate([[oa, aa, kappa], rec, present.astype(np.float64)])
        bound = np.zeros_like(out)
        bound[0] = 2 * U64 * abs(oa)
        bound[1] = 2 * U64 * (C + 2)
        if pe < 1:
            num = U64 * (abs(oa) + pe + abs(oa - pe))
            bound[2] = 2 * (num / (1 - pe) + abs(kappa) * U64 * 2 / (1 - pe) + U64 * abs(kappa))
        bound[3:3 + C - 1] = 2 * U64 * rec
    bound = np.where(np.isnan(bound), 0.0, bound)
    return out, bound


SHAPES = [(1, 2, 16), (5, 3, 16), (63, 16, 16), (64, 17, 32), (65, 33, 48), (257, 64, 64), (512, 65, 80), (8193, 200, 208),
          (3, 1024, 1024)]
MODES = ["random", "none_ignored", "all_ignored", "one_valid"]


def make_case(N, C, ld, mode, ignore_index=0, seed=0):
    """(logits fp32 [N, ld], targets int64 [N], nan_row or None).  Pad columns [C, ld) hold NaN: a kernel that reads one as a
    class shows it.  Row 0: +-1e4; row 1: tied maxima (the maximum three times, also in the last column); row 2: NaN.  With
    fewer than 3 rows, row 0 is the tied one."""
    rng = np.random.RandomState(1000 * seed + 7 * N + C)
    z = (3.0 * rng.standard_normal((N, ld))).astype(np.float32)
    z[:, C:] = np.nan
    nan_row = None

    def tie(r):
        top = np.float32(np.abs(z[r, :C]).max() + 1)
        z[r, [min(1, C - 1), C // 2, C - 1]] = top

    if N >= 3:
        z[0, :C] = np.where(rng.rand(C) < 0.5, 1e4, -1e4).astype(np.float32)
        z[0, C - 1] = 1e4
        tie(1)
        z[2, rng.randint(0, C)] = np.nan
        nan_row = 2
    else:
        tie(0)
    others = [c for c in range(C) if c != ignore_index]
    y = rng.choice(others, size=N).astype(np.int64)
    if mode == "random":
        y[rng.rand(N) < 1 / 3] = ignore_index
        if nan_row is not None:
            y[nan_row] = ignore_index                     # keeps the loss finite: the bound is exercised
    elif mode == "all_ignored":
        y[:] = ignore_index
    elif mode == "one_valid":
        keep = min(1, N - 1)
        y[np.arange(N) != keep] = ignore_index
    elif mode != "none_ignored":
        raise ValueError(mode)
    return z, y, nan_row
