"""The attention kernels, instantiation by instantiation, against a float64 reference (tests/attn_ref.py) on a real MI355X.

hs_attn_fwd / hs_attn_bwd (csrc/attn.hip dispatch) launch one attn16_{fwd,bwd}_kernel<NT, HD, 4, MODE0> per call, and
hsimae_attn_block_fwd / _bwd (the fused attention halves, as hsimae_forward / hsimae_backward run them) one of
blk128_fwd_kernel<NT, 2>, blk128_bwd_kernel<NT, 2, RC>, blk256_fwd_kernel<NT, 2>, blk256_bwd_kernel<NT, 2>.  TABLE lists
the 42 instantiations the rules can launch and `expected()` restates the rules; the first test proves that the cases below
reach every row.  Every output is compared element by element under the bound of attn_ref (never max-over-max), inside
NaN canaries (guard rows after nsamples * Ts, guard columns outside the documented column ranges).  The worst err / bound
per case is printed ("RATIO ...", run with -s).
"""
import ctypes as C
import os
import sys

import pytest
import torch

from hsimae_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EDIMS, EUNSUP, EALIGN, ENULL = 0, -1, -2, -3, -4
GUARD = 3


# ------------------------------------------------------------------------------------------------ the dispatch rules
def _table():
    t = set()
    for k in ("attn16_fwd", "attn16_bwd"):
        t |= {(k, nt, 16, m0) for nt in (1, 2, 3, 4, 7) for m0 in (0, 1)}
        t |= {(k, nt, 8, m0) for nt in (4, 7, 14) for m0 in (0, 1)}
    t |= {("blk128_fwd", nt) for nt in (1, 2)} | {("blk128_bwd", nt, rc) for nt in (1, 2) for rc in (0, 1)}
    t |= {("blk256_fwd", nt) for nt in (1, 2)} | {("blk256_bwd", nt) for nt in (1, 2)}
    return t


TABLE = _table()


def expected(kind, hd_or_d, Ts, mode, rc=0):
    """Row of TABLE a call launches (kind: fwd / bwd stand-alone with the head dim, or blk_fwd / blk_bwd with d)."""
    nt = (Ts + 15) // 16
    if kind in ("fwd", "bwd"):
        NT = next(x for x in ((1, 2, 3, 4, 7) if hd_or_d == 16 else (4, 7, 14)) if x >= nt)
        return ("attn16_" + kind, NT, hd_or_d, int(mode == 0))
    NT = 1 if Ts <= 16 else 2
    name = ("blk128_" if hd_or_d == 128 else "blk256_") + kind[4:]
    return (name, NT, rc) if name == "blk128_bwd" else (name, NT)


def inst_name(t):
    if t[0].startswith("attn16"):
        return "%s_kernel<%d, %d, 4, %s>" % (t[0], t[1], t[2], "true" if t[3] else "false")
    if t[0] == "blk128_bwd":
        return "blk128_bwd_kernel<%d, 2, %s>" % (t[1], "true" if t[2] else "false")
    return "%s_kernel<%d, 2>" % (t[0], t[1])


# ------------------------------------------------------------------------------------------------ the cases
def rup(x, m):
    return (x + m - 1) // m * m


def _alone_cases():
    """(hd, heads, Ts, mode, len_l, padded, nsamples, spread)."""
    cs = []
    widths16 = [(1, False), (2, False), (8, False), (9, True), (16, False), (32, False)]
    widths8 = [(8, False), (9, True), (1, False), (2, False)]
    i = 0
    for hd, tss, widths in ((16, (1, 15, 16, 17, 14, 27, 31, 32, 33, 48, 54, 64, 65, 108, 112), widths16),
                            (8, (1, 16, 17, 54, 64, 65, 108, 112, 113, 216, 224), widths8)):
        for Ts in tss:
            for mode, len_l in ((0, 9), (1, max(1, Ts // 3) if Ts % 3 else 9 if Ts % 9 == 0 else Ts // 3), (2, 7)):
                heads, padded = widths[i % len(widths)]
                cs.append((hd, heads, Ts, mode, len_l, padded, 1 + i % 3, 6.0 if i % 2 else 1.5))
                i += 1
    # singleton classes (o = v, dv = dO), ragged classes (Ts % len_l != 0), one token
    for hd, heads, Ts, mode, len_l, padded in ((16, 9, 27, 1, 1, True), (16, 2, 27, 2, 27, False), (8, 9, 54, 1, 1, True),
                                               (8, 2, 108, 2, 108, False), (16, 8, 27, 1, 7, False), (16, 8, 27, 2, 5, False),
                                               (8, 8, 216, 1, 50, False), (16, 1, 1, 1, 1, False), (16, 16, 64, 2, 1, False)):
        cs.append((hd, heads, Ts, mode, len_l, padded, 3, 1.5))
    return cs


ALONE = _alone_cases()
# fused: (d, Ts, mode, len_l, nsamples, spread); 515 samples: the persistent loop runs twice and its last pair is half empty
BLOCK = [(d, Ts, mode, len_l, n, sp) for d in (128, 256) for Ts, mode, len_l, n, sp in
         ((1, 0, 9, 1, 1.0), (14, 1, 7, 2, 1.0), (15, 2, 5, 3, 4.0), (16, 1, 1, 3, 1.0), (17, 2, 17, 2, 1.0), (27, 2, 9, 3, 4.0),
          (27, 1, 9, 515, 1.0), (31, 1, 4, 3, 1.0), (32, 0, 9, 2, 4.0), (14, 2, 7, 515, 1.0))]


def alone_id(c):
    hd, heads, Ts, mode, len_l, padded, n, sp = c
    return f"hd{hd}-h{heads}-T{Ts}-m{mode}-l{len_l}-{'pad' if padded else 'dense'}-n{n}-s{sp}"


def block_id(c):
    d, Ts, mode, len_l, n, sp = c
    return f"d{d}-T{Ts}-m{mode}-l{len_l}-n{n}-s{sp}"


def test_dispatch_coverage():
    """Every case lands on a row of TABLE, and the cases reach every row."""
    reached = set()
    for hd, heads, Ts, mode, len_l, padded, n, sp in ALONE:
        reached |= {expected("fwd", hd, Ts, mode), expected("bwd", hd, Ts, mode)}
    for d, Ts, mode, len_l, n, sp in BLOCK:
        reached |= {expected("blk_fwd", d, Ts, mode), expected("blk_bwd", d, Ts, mode, 0)}
        if d == 128:
            reached.add(expected("blk_bwd", d, Ts, mode, 1))
    assert reached <= TABLE, sorted(reached - TABLE)
    missing = TABLE - reached
    assert not missing, "instantiations without a case: " + ", ".join(inst_name(t) for t in sorted(missing))
    assert len(TABLE) == 42


# ------------------------------------------------------------------------------------------------ plumbing
def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def untouched(buf, ref, mask, what):
    assert torch.equal(bits(buf)[mask], bits(ref)[mask]), f"{what}: canary region written"


def outside(rows, ld, M, ranges):
    """True outside rows [0, M) x the column ranges."""
    m = torch.ones(rows, ld, dtype=torch.bool, device=DEV)
    for a, b in ranges:
        m[:M, a:b] = False
    return m


def report(case, what, r):
    print(f"RATIO {what:<6s} {r:7.4f}  {inst_name(case[0]) if isinstance(case, tuple) and isinstance(case[0], tuple) else case}")
    assert r <= 1.0, f"{what}: err / bound = {r:.3g}"


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def nan(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------ stand-alone kernels
def alone_layout(hd, heads, padded):
    d = hd * heads
    dp = rup(d, 32) if padded else d
    return d, dict(ld=3 * dp, ldo=dp, lddo=dp, kv_off=dp if padded else 0)


def alone_inputs(case, seed):
    hd, heads, Ts, mode, len_l, padded, n, sp = case
    d, lay = alone_layout(hd, heads, padded)
    rows = n * Ts
    kvo = lay["kv_off"] or d
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = nan(rows + GUARD, lay["ld"], torch.bfloat16)
    for i in range(3):
        qkv[:rows, i * kvo:i * kvo + d] = (torch.randn(rows, d, device=DEV, generator=g) * sp + 0.1).to(torch.bfloat16)
    dout = nan(rows + GUARD, lay["lddo"], torch.bfloat16)
    dout[:rows, :d] = torch.randn(rows, d, device=DEV, generator=g).to(torch.bfloat16)
    return d, lay, qkv, dout


def alone_call(bwd, hd, heads, Ts, mode, len_l, n, lay, qkv, o, lse, dout=None, dqkv=None, row0=0, over=None):
    d = hd * heads
    kw = dict(qkv=ptr(qkv, row0 * lay["ld"]), ld=lay["ld"], d=d, heads=heads, hd=hd, Ts=Ts, nsamples=n, mode=mode, len_l=len_l,
              o=ptr(o, row0 * lay["ldo"]), ldo=lay["ldo"], lse=ptr(lse, row0 * heads), dout=ptr(dout, row0 * lay["lddo"]),
              lddo=lay["lddo"], dqkv=ptr(dqkv, row0 * lay["ld"]), kv_off=lay["kv_off"])
    kw.update(over or {})
    p = _lib.AttnParams(**{k: v for k, v in kw.items() if v is not None})
    lib = _lib.load()
    rc = (lib.hsimae_attn_bwd if bwd else lib.hsimae_attn_fwd)(C.byref(p), stream())
    torch.cuda.synchronize()
    return rc


def singleton_rows(Ts, mode, len_l):
    c = R.classes(Ts, mode, len_l)
    cnt = torch.bincount(c)
    return cnt[c] == 1


@pytest.mark.parametrize("case", ALONE, ids=alone_id)
def test_attn16(case):
    hd, heads, Ts, mode, len_l, padded, n, sp = case
    d, lay, qkv, dout = alone_inputs(case, 100 + ALONE.index(case))
    rows = n * Ts
    kvo = lay["kv_off"] or d
    o = nan(rows + GUARD, lay["ldo"], torch.bfloat16)
    lse = nan(rows + GUARD, heads, torch.float32)
    o0, lse0 = o.clone(), lse.clone()
    assert alone_call(False, hd, heads, Ts, mode, len_l, n, lay, qkv, o, lse) == OK
    untouched(o, o0, outside(rows + GUARD, lay["ldo"], rows, [(0, d)]), "o")
    untouched(lse, lse0, outside(rows + GUARD, heads, rows, [(0, heads)]), "lse")
    ref = R.attn_fwd64(qkv[:rows].float(), d, heads, Ts, mode, len_l, lay["kv_off"])
    fi = (expected("fwd", hd, Ts, mode),)
    report(fi, "o", R.ratio(o[:rows, :d], ref["o"], ref["bo"]))
    report(fi, "lse", R.ratio(lse[:rows], ref["lse"], ref["blse"]))

    dqkv = nan(rows + GUARD, lay["ld"], torch.bfloat16)
    dqkv0 = dqkv.clone()
    assert alone_call(True, hd, heads, Ts, mode, len_l, n, lay, qkv, o, lse, dout, dqkv) == OK
    untouched(dqkv, dqkv0, outside(rows + GUARD, lay["ld"], rows, [(0, d), (kvo, kvo + d), (2 * kvo, 2 * kvo + d)]), "dqkv")
    NT = expected("bwd", hd, Ts, mode)[1]
    bref = R.attn_bwd64(qkv[:rows].float(), dout[:rows, :d].float(), lse[:rows], d, heads, Ts, mode, len_l, lay["kv_off"],
                        pdp=NT <= 4, o=o[:rows, :d].float())
    bi = (expected("bwd", hd, Ts, mode),)
    for i, nm in enumerate(("dq", "dk", "dv")):
        report(bi, nm, R.ratio(dqkv[:rows, i * kvo:i * kvo + d], bref[nm], bref["b" + nm]))

    # singleton classes: o is v bit for bit and dv is dO (dq / dk are within the bound above)
    single = singleton_rows(Ts, mode, len_l).to(DEV).repeat(n)
    if bool(single.any()):
        assert same_bits(o[:rows, :d][single], qkv[:rows, 2 * kvo:2 * kvo + d][single])
        assert same_bits(dqkv[:rows, 2 * kvo:2 * kvo + d][single], dout[:rows, :d][single])

    # the last sample launched alone (pointer offsets) computes bit for bit what it computed inside the batch
    s = n - 1
    o1, lse1, dq1 = o.clone(), lse.clone(), dqkv.clone()
    o1[s * Ts:rows], lse1[s * Ts:rows], dq1[s * Ts:rows] = float("nan"), float("nan"), float("nan")
    assert alone_call(False, hd, heads, Ts, mode, len_l, 1, lay, qkv, o1, lse1, row0=s * Ts) == OK
    assert alone_call(True, hd, heads, Ts, mode, len_l, 1, lay, qkv, o1, lse1, dout, dq1, row0=s * Ts) == OK
    assert same_bits(o1, o) and same_bits(lse1, lse) and same_bits(dq1, dqkv)


# ------------------------------------------------------------------------------------------------ fused attention halves
def pack(W, transpose):
    """fp32 W [rows, cols] -> bf16 image (hsimae_pack_matrix): [rows][cols], or [cols][rows] of W^T."""
    N, K = (W.shape[1], W.shape[0]) if transpose else W.shape
    img = torch.zeros(N * K, dtype=torch.bfloat16, device=DEV)
    W = W.contiguous().float()
    dsc = (_lib.PackDesc * 1)()
    dsc[0] = _lib.PackDesc(src=W.data_ptr(), rows=W.shape[0], cols=W.shape[1], transpose=int(transpose), n_off=0, k_off=0,
                           KS=K // 32, dst=img.data_ptr())
    table = torch.frombuffer(bytearray(bytes(dsc)), dtype=torch.uint8).clone().to(DEV)
    _lib.check(_lib.load().hsimae_pack_matrix(table.data_ptr(), 1, W.numel(), stream()))
    torch.cuda.synchronize()
    return img


class Block:
    """Weights of one attention half (d = 128 / 256) and its ABI struct."""

    def __init__(self, d, seed, spread):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.d, self.heads = d, d // 16
        self.Wqkv = torch.randn(3 * d, d, device=DEV, generator=g) * (0.1 * spread * (128 / d) ** 0.5)
        self.Wp = torch.randn(d, d, device=DEV, generator=g) * 0.08
        self.n1w = 1 + 0.2 * torch.randn(d, device=DEV, generator=g)
        self.n1b = 0.1 * torch.randn(d, device=DEV, generator=g)
        self.bqkv = 0.2 * torch.randn(3 * d, device=DEV, generator=g)
        self.pb = 0.1 * torch.randn(d, device=DEV, generator=g)
        self.imgs = (pack(self.Wqkv, False), pack(self.Wp, False), pack(self.Wqkv, True), pack(self.Wp, True))
        self.w = _lib.AttnBlockWeights(n1w=self.n1w.data_ptr(), n1b=self.n1b.data_ptr(), bqkv=self.bqkv.data_ptr(),
                                       pb=self.pb.data_ptr(), qkv=self.imgs[0].data_ptr(), p=self.imgs[1].data_ptr(),
                                       qkvT=self.imgs[2].data_ptr(), pT=self.imgs[3].data_ptr())


def blk_fwd(B, x, u, qkv, o, lse, x1, rs, Ts, n, mode, len_l, row0=0, w=None, d=None, heads=None):
    d_ = B.d if d is None else d
    rc = _lib.load().hsimae_attn_block_fwd(C.byref(B.w if w is None else w), ptr(x, row0 * B.d), ptr(u, row0 * B.d),
                                           ptr(qkv, row0 * 3 * B.d), ptr(o, row0 * B.d), ptr(lse, row0 * B.heads),
                                           ptr(x1, row0 * B.d), ptr(rs, row0), d_, B.heads if heads is None else heads, Ts, n,
                                           mode, len_l, stream())
    torch.cuda.synchronize()
    return rc


def blk_bwd(B, qkv, u, o, lse, dx1b, dx1, x, dqkv, dx, dgamma, dbeta, det, acc, Ts, n, mode, len_l, row0=0, w=None, d=None,
            heads=None):
    rc = _lib.load().hsimae_attn_block_bwd(C.byref(B.w if w is None else w), ptr(qkv, row0 * 3 * B.d), ptr(u, row0 * B.d),
                                           ptr(o, row0 * B.d), ptr(lse, row0 * B.heads), ptr(dx1b, row0 * B.d),
                                           ptr(dx1, row0 * B.d), ptr(x, row0 * B.d), ptr(dqkv, row0 * 3 * B.d), ptr(dx, row0 * B.d),
                                           ptr(dgamma), ptr(dbeta), ptr(det), acc, B.d if d is None else d,
                                           B.heads if heads is None else heads, Ts, n, mode, len_l, stream())
    torch.cuda.synchronize()
    return rc


def block_inputs(d, rows, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = nan(rows + GUARD, d, torch.float32)
    x[:rows] = torch.randn(rows, d, device=DEV, generator=g) * 1.5 + 0.3
    if rows > 4:
        x[2] = 300 + torch.randn(d, device=DEV, generator=g)      # large mean
    rs = (torch.rand(rows, device=DEV, generator=g) < 0.8).float() * 1.25
    rs[0] = 0.0
    dx1b = nan(rows + GUARD, d, torch.bfloat16)
    dx1b[:rows] = (torch.randn(rows, d, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    dx1 = nan(rows + GUARD, d, torch.float32)
    dx1[:rows] = torch.randn(rows, d, device=DEV, generator=g)
    prefill = torch.randn(rows, d, device=DEV, generator=g)
    return x, rs, dx1b, dx1, prefill


def fwd_outputs(d, heads, rows, save_qkv=True):
    return dict(u=nan(rows + GUARD, d, torch.bfloat16), qkv=nan(rows + GUARD, 3 * d, torch.bfloat16) if save_qkv else None,
                o=nan(rows + GUARD, d, torch.bfloat16), lse=nan(rows + GUARD, heads, torch.float32),
                x1=nan(rows + GUARD, d, torch.float32))


def run_fwd(B, x, rs, Ts, n, mode, len_l, save_qkv=True, row0=0, outs=None):
    rows = n * Ts
    f = outs if outs is not None else fwd_outputs(B.d, B.heads, rows, save_qkv)
    canary = {k: v.clone() for k, v in f.items() if v is not None}
    assert blk_fwd(B, x, f["u"], f["qkv"] if save_qkv else None, f["o"], f["lse"], f["x1"], rs, Ts, n, mode, len_l, row0) == OK
    if outs is None:
        for k, v in canary.items():
            untouched(f[k], v, outside(v.shape[0], v.shape[1], rows, [(0, v.shape[1])]), k)
    return f


def bwd_outputs(d, rows, prefill, accumulate):
    dx = nan(rows + GUARD, d, torch.float32)
    if accumulate:
        dx[:rows] = prefill
    flat = torch.full((2 * d + 8,), float("nan"), device=DEV)
    flat[:2 * d] = torch.linspace(-0.5, 0.5, 2 * d, device=DEV)          # dgamma | dbeta add onto non-zero prefills
    return dict(dqkv=nan(rows + GUARD, 3 * d, torch.bfloat16), dx=dx, flat=flat)


def run_bwd(B, f, x, dx1b, dx1, prefill, Ts, n, mode, len_l, accumulate, rc=False, det=False, row0=0, outs=None):
    rows, d = n * Ts, B.d
    b = outs if outs is not None else bwd_outputs(d, rows, prefill, accumulate)
    canary = {k: v.clone() for k, v in b.items()}
    acc = torch.full((2 * d,), 12345, dtype=torch.int64, device=DEV) if det else None        # contents irrelevant on entry
    assert blk_bwd(B, None if rc else f["qkv"], f["u"], f["o"], f["lse"], dx1b, dx1, x, b["dqkv"], b["dx"], b["flat"][:d],
                   b["flat"][d:2 * d], acc, accumulate, Ts, n, mode, len_l, row0) == OK
    if outs is None:
        for k in ("dqkv", "dx"):
            v = canary[k]
            untouched(b[k], v, outside(v.shape[0], v.shape[1], rows, [(0, v.shape[1])]), k)
        assert same_bits(b["flat"][2 * d:], canary["flat"][2 * d:]), "past dbeta: canary written"
    return b


@pytest.mark.parametrize("case", BLOCK, ids=block_id)
def test_attention_block(case):
    d, Ts, mode, len_l, n, sp = case
    seed = 500 + BLOCK.index(case)
    B = Block(d, seed, sp)
    heads, rows = B.heads, n * Ts
    x, rs, dx1b, dx1, prefill = block_inputs(d, rows, seed)
    f = run_fwd(B, x, rs, Ts, n, mode, len_l)
    fi = (expected("blk_fwd", d, Ts, mode),)
    # LayerNorm-1 from x, q|k|v from the kernel's own u, the attention from its own q|k|v, x1 from its own o
    u64, xhat, _, kappa = R.ln64(x[:rows], B.n1w, B.n1b)
    report(fi, "u", R.ratio(f["u"][:rows], u64, R.ln_out_bound(u64, xhat, kappa, B.n1w, B.n1b)))
    q64, bq = R.linear64(f["u"][:rows].float(), R.bf(B.Wqkv), B.bqkv)
    report(fi, "qkv", R.ratio(f["qkv"][:rows], q64, bq + R.UB * q64.abs()))
    ref = R.attn_fwd64(f["qkv"][:rows].float(), d, heads, Ts, mode, len_l)
    report(fi, "o", R.ratio(f["o"][:rows], ref["o"], ref["bo"]))
    report(fi, "lse", R.ratio(f["lse"][:rows], ref["lse"], ref["blse"]))
    x164, bx1 = R.x1_64(x[:rows], f["o"][:rows], B.Wp, B.pb, rs)
    report(fi, "x1", R.ratio(f["x1"][:rows], x164, bx1))
    dropped = rs == 0
    assert bool(dropped.any()) and same_bits(f["x1"][:rows][dropped], x[:rows][dropped]), "rowscale 0: x1 must be x"
    single = singleton_rows(Ts, mode, len_l).to(DEV).repeat(n)
    if bool(single.any()):
        assert same_bits(f["o"][:rows][single], f["qkv"][:rows, 2 * d:][single]), "singleton class: o must be v"

    # backward (fp32 atomics), against the reference on the kernel's q|k|v, lse and dqkv
    acc_mode = int(BLOCK.index(case) % 2 == 0)
    b = run_bwd(B, f, x, dx1b, dx1, prefill, Ts, n, mode, len_l, acc_mode)
    bi = (expected("blk_bwd", d, Ts, mode, 0),)
    dO, eta = R.dout64(dx1b[:rows], B.Wp)
    bref = R.attn_bwd64(f["qkv"][:rows].float(), dO, f["lse"][:rows], d, heads, Ts, mode, len_l, pdp=True, eta=eta)
    for i, nm in enumerate(("dq", "dk", "dv")):
        report(bi, nm, R.ratio(b["dqkv"][:rows, i * d:(i + 1) * d], bref[nm], bref["b" + nm]))
    if bool(single.any()):
        # singleton classes: dv is dO (within the bound: the kernel's dO is its own fp32 product rounded to bf16), dq = dk = 0
        # within the bound; not exactly, since P = exp2(fma(s, sc, -lse)) recovers the rounding of s * sc that lse carries
        # (P = 1 +- a few 2^-24), and dS = P (dP - P dP) is then a few 2^-24 dP instead of 0
        nz = int((b["dqkv"][:rows, :2 * d][single] != 0).sum())
        print(f"SINGLETON {inst_name(bi[0])}: {nz} of {int(single.sum()) * 2 * d} dq / dk elements not exactly 0")
    dres = dx1[:rows] + (prefill if acc_mode else 0)
    dx64, bdx, dg64, bg, db64, bb = R.ln1_bwd64(b["dqkv"][:rows], B.Wqkv, x[:rows], B.n1w, dres)
    report(bi, "dx", R.ratio(b["dx"][:rows], dx64, bdx))
    pre = torch.linspace(-0.5, 0.5, 2 * d, device=DEV).double()
    report(bi, "dgamma", R.ratio(b["flat"][:d], pre[:d] + dg64, bg + R.C2 * R.U * (pre[:d].abs() + dg64.abs())))
    report(bi, "dbeta", R.ratio(b["flat"][d:2 * d], pre[d:] + db64, bb + R.C2 * R.U * (pre[d:].abs() + db64.abs())))

    # deterministic commits: the same data path, bit-reproducible dgamma / dbeta
    bd = run_bwd(B, f, x, dx1b, dx1, prefill, Ts, n, mode, len_l, acc_mode, det=True)
    bd2 = run_bwd(B, f, x, dx1b, dx1, prefill, Ts, n, mode, len_l, acc_mode, det=True)
    assert same_bits(bd["dqkv"], b["dqkv"]) and same_bits(bd["dx"], b["dx"])
    assert same_bits(bd["flat"], bd2["flat"]), "deterministic dgamma / dbeta differ between two runs"
    report(bi, "dgamma", R.ratio(bd["flat"][:d], pre[:d] + dg64, bg + R.C2 * R.U * (pre[:d].abs() + dg64.abs())))
    report(bi, "dbeta", R.ratio(bd["flat"][d:2 * d], pre[d:] + db64, bb + R.C2 * R.U * (pre[d:].abs() + db64.abs())))

    if d == 128:
        # q|k|v not saved (the default schedule): the forward's other outputs and the recomputing backward (RC) are bit-identical
        fr = run_fwd(B, x, rs, Ts, n, mode, len_l, save_qkv=False)
        for k in ("u", "o", "lse", "x1"):
            assert same_bits(fr[k], f[k]), f"forward without saved q|k|v: {k} differs"
        br = run_bwd(B, fr, x, dx1b, dx1, prefill, Ts, n, mode, len_l, acc_mode, rc=True, det=True)
        print(f"RATIO rc     exact    {inst_name(expected('blk_bwd', d, Ts, mode, 1))}")
        assert same_bits(br["dqkv"], bd["dqkv"]) and same_bits(br["dx"], bd["dx"]), "RC backward differs from saved q|k|v"
        assert same_bits(br["flat"], bd["flat"]), "RC backward: dgamma / dbeta differ"

    # the last sample alone (pointer offsets): every per-row output bit-identical to the batched launch
    s = n - 1
    f1 = {k: v.clone() for k, v in f.items()}
    for v in f1.values():
        v[s * Ts:rows] = float("nan")
    run_fwd(B, x, rs, Ts, 1, mode, len_l, row0=s * Ts, outs=f1)
    for k in f:
        assert same_bits(f1[k], f[k]), f"sample launched alone: {k} differs"
    b1 = {k: v.clone() for k, v in bd.items()}
    b1["dqkv"][s * Ts:rows] = float("nan")
    b1["dx"][s * Ts:rows] = prefill[s * Ts:] if acc_mode else float("nan")
    run_bwd(B, f, x, dx1b, dx1, prefill, Ts, 1, mode, len_l, acc_mode, row0=s * Ts, outs=b1)
    assert same_bits(b1["dqkv"], bd["dqkv"]) and same_bits(b1["dx"], bd["dx"]), "sample launched alone: backward differs"


# ------------------------------------------------------------------------------------------------ refusals
def test_attn16_refusals():
    hd, heads, Ts, n = 16, 2, 27, 2
    d, lay = alone_layout(hd, heads, False)
    # buffers large enough for any call in the list (2 x 225 rows, rows up to 128 wide): a call refused by mistake stays in bounds
    R_ = 2 * 225 + GUARD
    g = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn(R_, 128, device=DEV, generator=g).to(torch.bfloat16)
    dout = torch.randn(R_, 64, device=DEV, generator=g).to(torch.bfloat16)
    o = nan(R_, 64, torch.bfloat16)
    lse = nan(R_, 4, torch.float32)
    dqkv = nan(R_, 128, torch.bfloat16)
    base = (o.clone(), lse.clone(), dqkv.clone())
    refused = [  # (backward?, overrides, code)
        (0, dict(d=48), EDIMS), (0, dict(ld=100), EDIMS), (0, dict(ldo=34), EDIMS), (0, dict(ldo=24), EDIMS),
        (0, dict(mode=3), EUNSUP), (0, dict(mode=-1), EUNSUP), (0, dict(Ts=0), EDIMS), (0, dict(Ts=-4), EDIMS),
        (0, dict(len_l=0), EDIMS), (0, dict(mode=2, len_l=-1), EDIMS), (0, dict(kv_off=24), EDIMS), (0, dict(kv_off=36), EDIMS),
        (0, dict(kv_off=-8), EDIMS), (0, dict(kv_off=40), EDIMS), (0, dict(qkv=None), ENULL), (0, dict(o=None), ENULL),
        (0, dict(Ts=113), EUNSUP), (0, dict(hd=8, heads=4, Ts=225), EUNSUP), (0, dict(hd=32, heads=1), EUNSUP),
        (1, dict(lddo=28), EDIMS), (1, dict(lddo=36), EDIMS), (1, dict(dout=None), ENULL), (1, dict(dqkv=None), ENULL),
        (1, dict(lse=None), EUNSUP), (1, dict(mode=5), EUNSUP), (1, dict(len_l=0), EDIMS), (1, dict(kv_off=36), EDIMS),
        (1, dict(Ts=0), EDIMS), (1, dict(Ts=113), EUNSUP),
    ]
    for bwd, over, code in refused:
        kw = dict(over)
        for k in ("qkv", "o", "dout", "dqkv", "lse"):
            if k in kw and kw[k] is None:
                kw[k] = 0
        rc = alone_call(bwd, hd, heads, Ts, 1, 9, n, lay, qkv, o, lse, dout, dqkv, over=kw)
        assert rc == code, (bwd, over, rc, code)
        assert same_bits(o, base[0]) and same_bits(lse, base[1]) and same_bits(dqkv, base[2]), (bwd, over, "output written")
    # no-ops and the NULL parameter block
    assert alone_call(0, hd, heads, Ts, 1, 9, 0, lay, qkv, o, lse) == OK
    assert alone_call(1, hd, heads, Ts, 1, 9, -3, lay, qkv, o, lse, dout, dqkv) == OK
    assert alone_call(0, hd, heads, Ts, 0, 0, n, lay, qkv, o, lse) == OK            # mode 0 ignores len_l
    assert _lib.load().hsimae_attn_fwd(None, stream()) == ENULL and _lib.load().hsimae_attn_bwd(None, stream()) == ENULL
    assert same_bits(dqkv, base[2])


def test_attention_block_refusals():
    B = Block(128, 9, 1.0)
    d, Ts, n = 128, 27, 2
    rows = n * Ts
    x, rs, dx1b, dx1, prefill = block_inputs(d, rows, 9)
    f = fwd_outputs(d, 8, rows)
    b = bwd_outputs(d, rows, prefill, 0)
    acc = torch.zeros(2 * d, dtype=torch.int64, device=DEV)
    canary = [t.clone() for t in list(f.values()) + list(b.values())]
    nul = _lib.AttnBlockWeights.from_buffer_copy(B.w)
    nul.pT = None
    x_mis = x.view(-1)[1:].view(-1)

    def fwd(**k):
        a = dict(B=B, x=x, u=f["u"], qkv=f["qkv"], o=f["o"], lse=f["lse"], x1=f["x1"], rs=rs, Ts=Ts, n=n, mode=1, len_l=9)
        a.update(k)
        return blk_fwd(**a)

    def bwd(**k):
        a = dict(B=B, qkv=f["qkv"], u=f["u"], o=f["o"], lse=f["lse"], dx1b=dx1b, dx1=dx1, x=x, dqkv=b["dqkv"], dx=b["dx"],
                 dgamma=b["flat"][:d], dbeta=b["flat"][d:2 * d], det=None, acc=0, Ts=Ts, n=n, mode=1, len_l=9)
        a.update(k)
        return blk_bwd(**a)

    for call in (fwd, bwd):
        assert call(d=128, heads=16) == EUNSUP
        assert call(d=256, heads=8) == EUNSUP
        assert call(d=192, heads=12) == EUNSUP
        assert call(Ts=33) == EUNSUP
        assert call(Ts=0) == EDIMS
        assert call(mode=3) == EUNSUP
        assert call(len_l=0) == EDIMS
        assert call(mode=2, len_l=-2) == EDIMS
        assert call(n=-1) == EDIMS
        assert call(n=0) == OK
        assert call(w=nul) == ENULL
        assert call(x=None) == ENULL
        assert call(lse=None) == ENULL
        assert call(x=x_mis) == EALIGN
    assert fwd(qkv=f["qkv"].view(-1)[1:]) == EALIGN
    assert fwd(x1=None) == ENULL
    assert bwd(dqkv=None) == ENULL and bwd(dgamma=None) == ENULL and bwd(u=None) == ENULL
    assert bwd(det=acc, dbeta=b["flat"][d + 1:2 * d + 1]) == EDIMS           # det_acc needs dbeta == dgamma + d
    B2 = Block(256, 9, 1.0)
    f2 = fwd_outputs(256, 16, rows)
    assert blk_fwd(B2, x, f2["u"], None, f2["o"], f2["lse"], f2["x1"], None, Ts, n, 1, 9) == EUNSUP     # no RC at d = 256
    assert blk_bwd(B2, None, f2["u"], f2["o"], f2["lse"], dx1b, dx1, x, b["dqkv"], b["dx"], b["flat"][:d], b["flat"][d:2 * d],
                   None, 0, Ts, n, 1, 9) == EUNSUP
    big = (1 << 31) // (32 * 768) + 1                     # nsamples * Ts * 3 d >= 2^31: the kernel's 32-bit offsets
    assert blk_fwd(B2, x, f2["u"], f2["qkv"], f2["o"], f2["lse"], f2["x1"], None, 32, big, 0, 9) == EUNSUP
    for t, c in zip(list(f.values()) + list(b.values()), canary):
        assert same_bits(t, c), "a refused call wrote an output"
