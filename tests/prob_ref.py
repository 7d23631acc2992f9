"""fp64 restatement and element-wise error bounds for csrc/prob.hip (tests/test_gpu_prob.py, tests/test_prob_bound_cpu.py):
the class probabilities of a chunk averaged over its views, the label, the confidence and the margin.

A plain module, not a conftest.  The bounds are worst-case first-order bounds of what the kernel rounds, nothing is tuned on a
GPU result.  With U = 2^-24, the classes c in [first, C), d_c = z_c - max z over them, p = softmax over them (cls_ref.py's
terms for e_c, s and e * (1 / s), the class count being C - first):

  e_c = exp2(fl(fl(d_c) * fl(log2 e)))   three roundings of the argument (3 U |d_c| on e_c), v_exp_f32 1 ulp (2 U)
  s = sum e_c                            per lane ceil((C - first) / 64) terms in order, then 6 shuffle steps
      => |ds| / s <= SREL = (ceil((C - first) / 64) + 8) U + 3 U sum_c p_c |d_c|
  p_c = fl(e_c * fl(1 / s))              => |dp_c| <= B_c = p_c ((3 |d_c| + 4) U + SREL) + 2^-120 (flushed denormals)
  acc_v = fl(acc_(v-1) + p_c)            one rounding per accumulated view: U |acc_v|, v = 1 .. V - 1 (none at view 0)
  mean_c = fl(acc * fl(1 / V))           two roundings, 2 U mean_c; both vanish when V is a power of two
      => |dmean_c| <= (sum_v B_c,v + U sum_(v >= 1) acc_v) / V + [V not a power of two] 2 U mean_c
  conf = mean[label]                     the bound of that entry
  margin = mean[label] - mean[second]    the sum of the two entries' bounds
Columns below `first` are exact zeros (bound 0).
The label with more than one view is an argmax over rounded means: it must equal the restatement's wherever the restatement's
top-two gap exceeds twice the sum of the two entries' bounds (`decided`); with one view it is the argmax of the logits, exact.
"""
import ctypes
import math
import struct
import zlib

import numpy as np

from cls_ref import SHAPES, TINY, U, ratio  # noqa: F401  (re-exported for the tests)

VIEWS = [1, 2, 3, 4]
F32 = np.float32
LOG2E32 = F32(1.4426950408889634)


def view_probs(z, C, first):
    """One view's logits [N, ld] -> (p fp64 [N, C], bound [N, C]); only columns [first, C) are read."""
    zz = np.asarray(z)[:, first:C].astype(np.float64)
    N = zz.shape[0]
    p = np.zeros((N, C))
    b = np.zeros((N, C))
    with np.errstate(all="ignore"):
        m = np.where(np.isnan(zz), -np.inf, zz).max(1)
        d = zz - m[:, None]
        e = np.exp(d)
        s = e.sum(1)
        q = e / s[:, None]
        ad = np.where(q == 0, 0.0, np.abs(d))
        srel = (math.ceil((C - first) / 64) + 8) * U + 3 * U * (q * ad).sum(1)
        p[:, first:] = q
        b[:, first:] = q * ((3 * ad + 4) * U + srel[:, None]) + TINY
    return p, np.where(np.isnan(b), 0.0, b)


def argmax_nan_first(a):
    """np.argmax along axis 1: the first maximum, and the first NaN if there is one (torch.argmax, arg_better)."""
    return np.argmax(a, axis=1)


def products(mean, bound, label, first):
    """conf, margin and their bounds for the given labels (the kernel's own, or the restatement's)."""
    N, C = mean.shape
    rows = np.arange(N)
    label = np.asarray(label, np.int64)
    conf, cb = mean[rows, label], bound[rows, label]
    if C - first == 1:
        return conf, cb, conf.copy(), cb.copy()
    other = mean.copy()
    other[:, :first] = -np.inf
    other[rows, label] = -np.inf
    sec = argmax_nan_first(other)
    with np.errstate(all="ignore"):
        margin = conf - other[rows, sec]
        mb = cb + bound[rows, sec]
    return conf, cb, margin, np.where(np.isnan(mb), 0.0, mb)


def prob_ref(views, C, first):
    """views fp32 [V, N, ld] -> dict: mean, bound [N, C]; label [N]; conf, conf_bound, margin, margin_bound [N] at that label;
    decided [N] bool: rows where the label of the rounded means is determined (all rows with one view)."""
    views = np.asarray(views)
    V, N = views.shape[0], views.shape[1]
    acc = accb = None
    with np.errstate(all="ignore"):
        for v in range(V):
            p, b = view_probs(views[v], C, first)
            if v == 0:
                acc, accb = p, b
            else:
                acc = acc + p
                accb = accb + b + U * np.where(np.isnan(acc), 0.0, np.abs(acc))
        mean = acc / V
        pow2 = V & (V - 1) == 0
        bound = accb / V + (0.0 if pow2 else 2 * U) * np.where(np.isnan(mean), 0.0, np.abs(mean))
        bound[:, :first] = 0.0
        if V == 1:
            label = first + argmax_nan_first(views[0][:, first:C].astype(np.float64))
            decided = np.ones(N, bool)
        else:
            label = first + argmax_nan_first(mean[:, first:])
            if C - first == 1:
                decided = np.ones(N, bool)
            else:
                order = np.argsort(-np.where(np.isnan(mean[:, first:]), np.inf, mean[:, first:]), axis=1, kind="stable")[:, :2] + first
                rows = np.arange(N)
                gap = mean[rows, order[:, 0]] - mean[rows, order[:, 1]]
                decided = gap > 2 * (bound[rows, order[:, 0]] + bound[rows, order[:, 1]])      # (False for a NaN row)
    conf, cb, margin, mb = products(mean, bound, label, first)
    return {"mean": mean, "bound": bound, "label": label.astype(np.int64), "conf": conf, "conf_bound": cb, "margin": margin,
            "margin_bound": mb, "decided": decided}


# ------------------------------------------------------------------ the kernel's sequence in exactly rounded fp32
def _lane_sum(e):
    """[N, n] fp32 -> [N]: lane l adds its columns l, l + 64, .. in order, then the xor tree over the 64 lanes."""
    N, n = e.shape
    lanes = np.zeros((N, 64), F32)
    for c in range(n):
        lanes[:, c % 64] = lanes[:, c % 64] + e[:, c]
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, idx ^ s]
    return lanes[:, 0]


def _pick(key, last_of_tie=False):
    """arg_better over the columns of key [N, n]: NaN first, else the maximum, ties to the lowest (or, planted, highest) index."""
    if last_of_tie:
        return key.shape[1] - 1 - np.argmax(key[:, ::-1], axis=1)
    return np.argmax(key, axis=1)


def emulate(views, C, first, fault=None, stale=0.5):
    """The kernel's operation sequence with every fp32 operation rounded exactly (exp2 evaluated in fp64 and rounded once)
    -> (mean [N, C] fp32, label, conf, margin).  `fault` plants one defect (tests/test_prob_bound_cpu.py)."""
    views = np.asarray(views, F32)
    V, N = views.shape[0], views.shape[1]
    lo = 0 if fault == "softmax_from_0" else first
    hi = C + 1 if fault == "pad_column" and views.shape[2] > C else C
    acc = np.full((N, hi), F32(stale))                     # what the caller's buffer held before
    with np.errstate(all="ignore"):
        for v in range(V):
            z = views[v][:, lo:hi]
            m = np.zeros(N, F32) if fault == "no_max" else np.where(np.isnan(z), F32(-np.inf), z).max(1)
            arg = (z - m[:, None]).astype(F32) * LOG2E32
            e = np.exp2(arg.astype(np.float64)).astype(F32)
            rs = F32(1) / _lane_sum(e)
            p = np.zeros((N, hi), F32)
            p[:, lo:] = e * rs[:, None]
            p[:, :first] = 0
            if v == 0 and fault != "acc_read_at_view_0" or fault == "last_view_only":
                acc = p
            else:
                acc = acc + p
        div = V - 1 if fault == "divide_by_v_minus_1" and V > 1 else V
        mean = (acc * (F32(1) / F32(div)))[:, :C]
        if V == 1 or fault == "label_from_logits":
            key = views[V - 1][:, first:C]
        else:
            key = mean[:, first:]
        label = first + _pick(key, fault == "ties_to_highest")
        rows = np.arange(N)
        conf = mean[rows, np.minimum(label + 1, C - 1) if fault == "conf_wrong_class" else label]
        other = mean.copy()
        other[:, :first] = -np.inf
        if fault != "margin_against_label":
            other[rows, label] = -np.inf
        second = np.where(np.isnan(other), F32(-np.inf), other).max(1)
        margin = conf.copy() if C - first == 1 else np.where(np.isnan(conf), conf, conf - second)
    return mean, label.astype(np.int64), conf, margin


FAULTS = ["softmax_from_0", "no_max", "pad_column", "acc_read_at_view_0", "last_view_only", "divide_by_v_minus_1",
          "conf_wrong_class", "margin_against_label", "ties_to_highest", "label_from_logits"]


def worst(got, views, C, first, ref=None, planted=True):
    """got = (mean, label, conf, margin) of the code under test -> dict of the worst err / bound of mean, conf and margin (the
    two taken at got's own label: conf must be the mean AT the label that was written) and the label verdict:
    `wrong` = rows whose label differs although it is determined (planted row 1, the exact three-way tie, always is),
    `open` = the share of the non-planted rows left out as undetermined.  planted=False: the rows are not make_case's."""
    mean, label, conf, margin = got
    ref = prob_ref(views, C, first) if ref is None else ref
    label = np.asarray(label, np.int64)
    ok = (label >= first) & (label < C)
    lab = np.where(ok, label, first)
    rc, rcb, rm, rmb = products(ref["mean"], ref["bound"], lab, first)
    N = label.shape[0]
    must = ref["decided"].copy()
    free = np.ones(N, bool)
    if planted and N >= PLANTED:
        must[1] = True
        free[:PLANTED] = False
    out = {"mean": ratio(mean, ref["mean"], ref["bound"]), "conf": ratio(conf, rc, rcb), "margin": ratio(margin, rm, rmb),
           "wrong": int(np.sum(~ok | (must & (label != ref["label"])))),
           "open": float(np.sum(~ref["decided"] & free)) / max(1, int(free.sum())),
           "zeros": bool(np.all(np.asarray(mean)[:, :first] == 0))}
    out["all"] = np.inf if out["wrong"] or not out["zeros"] else max(out["mean"], out["conf"], out["margin"])
    return out


# ------------------------------------------------------------------ cases
PLANTED = 3          # rows 0 .. 2 of a case with N >= 3


def make_case(N, C, ld, first, V, seed=0):
    """views fp32 [V, N, ld]: 3 N(0, 1) logits per view, NaN in the pad columns [C, ld) (a kernel that reads one shows it).
    With N >= 3: row 0 is +-1e4; row 1 holds its maximum three times and is the same in every view (the label must be the
    lowest tied index exactly); row 2 has one NaN.  With N >= 6 the last two rows are equal (the pixel list repeats one)."""
    rng = np.random.RandomState(100003 * seed + 1009 * V + 7 * N + C + 31 * first)
    z = (3.0 * rng.standard_normal((V, N, ld))).astype(np.float32)
    z[:, :, C:] = np.nan
    if N >= 3:
        for v in range(V):
            z[v, 0, :C] = np.where(rng.rand(C) < 0.5, 1e4, -1e4).astype(np.float32)
            z[v, 0, C - 1] = 1e4
        top = np.float32(np.abs(z[0, 1, :C]).max() + 1)
        z[0, 1, sorted({min(first + 1, C - 1), (first + C) // 2, C - 1})] = top
        z[:, 1] = z[0, 1]
        z[rng.randint(0, V), 2, rng.randint(first, C)] = np.nan
    if N >= 6:
        z[:, N - 1] = z[:, N - 2]
    return z


def cases():
    """(N, C, ld, first, V): every shape with first 0 and 1 and every view count.  first = 1 leaves at least two classes
    everywhere but at (1, 2, 16), which is the one-class case."""
    out = []
    for (N, C, ld) in SHAPES:
        for first in (0, 1):
            for V in VIEWS:
                out.append((N, C, ld, first, V))
    return out


def pixel_forms(N):
    """-> [(name, H, W, p0, pixels or None)]: a p0 range inside a larger map, and an index list in reversed order with an
    out-of-range entry (N >= 2) and a repeated one (N >= 6: the rows of the repeated pixel hold the same logits)."""
    H, W = 3, (N + 7 + 2) // 3
    pix = np.arange(N, dtype=np.int64)[::-1].copy() + 2
    if N >= 2:
        pix[0] = H * W + 5
    if N >= 6:
        pix[N - 1] = pix[N - 2]
    return [("range", H, W, 4, None), ("list", H, W, 0, pix)]


def rows_of_pixels(H, W, p0, pixels, N):
    """int64 [H * W]: the row of the chunk that writes each pixel of the maps, -1 where nothing is written."""
    HW = H * W
    pix = p0 + np.arange(N) if pixels is None else np.asarray(pixels)
    row_of = np.full(HW, -1, np.int64)
    for k in range(N):                                    # any of a repeated pixel's rows: their values are equal by construction
        if 0 <= pix[k] < HW:
            row_of[pix[k]] = k
    return row_of


def refusals(lib, _lib):
    """(what, code returned, code expected) of every refusal: all are decided before anything is launched."""
    ok = dict(logits=1 << 20, ld=16, N=4, C=10, first=1, view=0, n_views=1, acc=1 << 21, lda=16, H=2, W=2, p0=0, pixels=None,
              label_map=1 << 22, conf_map=1 << 23, margin_map=1 << 24, probs=1 << 25, ldp=16)
    E_DIMS, E_UNSUPPORTED, E_ALIGN, E_NULL = -1, -2, -3, -4
    table = [(dict(N=-1), E_DIMS), (dict(C=1, first=0), E_DIMS), (dict(first=-1), E_DIMS), (dict(first=10), E_DIMS),
             (dict(n_views=0), E_DIMS), (dict(n_views=9, view=8), E_DIMS), (dict(view=-1), E_DIMS), (dict(view=1), E_DIMS),
             (dict(n_views=4, view=4), E_DIMS), (dict(ld=9), E_DIMS), (dict(lda=9), E_DIMS), (dict(ldp=9), E_DIMS),
             (dict(H=0), E_DIMS), (dict(W=0), E_DIMS),
             (dict(C=1025, ld=1040, lda=1040, ldp=1040), E_UNSUPPORTED),
             (dict(logits=None), E_NULL), (dict(acc=None), E_NULL), (dict(label_map=None), E_NULL),
             (dict(logits=(1 << 20) + 2), E_ALIGN), (dict(acc=(1 << 21) + 1), E_ALIGN), (dict(label_map=(1 << 22) + 4), E_ALIGN),
             (dict(conf_map=(1 << 23) + 2), E_ALIGN), (dict(margin_map=(1 << 24) + 2), E_ALIGN), (dict(probs=(1 << 25) + 3), E_ALIGN),
             (dict(pixels=(1 << 26) + 4), E_ALIGN),
             (dict(N=0), 0), (dict(N=0, logits=None, acc=None, label_map=None), 0)]
    out = [("params NULL", lib.hsimae_class_prob(None, None), E_NULL)]
    for kw, want in table:
        a = dict(ok)
        a.update(kw)
        out.append((str(kw), lib.hsimae_class_prob(ctypes.byref(_lib.ClassProbParams(**a)), None), want))
    return out


def decode_png(data):
    """The pixels of an 8-bit RGB PNG whose scanlines all use filter 0 -> uint8 [H, W, 3]; every chunk's CRC is checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body)
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, flt, lace) == (8, 2, 0, 0, 0)
    lines = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert np.all(lines[:, 0] == 0)
    return lines[:, 1:].reshape(h, w, 3)
