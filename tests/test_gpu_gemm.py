"""hsimae_gemm, branch by branch, against a float64 reference (tests/gemm_ref.py) on a real MI355X.

hs_gemm (csrc/gemm.hip) launches one gemm_kernel<AK, EPI, KC, BM, F8, NCH> per call, chosen by plan_gemm (csrc/plan.h) from the
A kind, the epilogue, the precision, N, K and the tiling.  gemm_ref.TABLE lists every instantiation that rule can launch and
gemm_ref.expected() restates the rule (tests/test_launch_plan_cpu.py holds both against the library's own); the first test
proves that the cases below reach every row of TABLE, so a branch added later without a case fails here.  Every case
compares element by element under the bound of gemm_ref (never max-over-max), surrounds every output with canaries (NaN / sentinel fill, guard rows after M, guard columns between N and ld), and checks the
[n_valid, N) column contract of the header.  The worst err / bound per case is printed ("RATIO ...", run with -s).
"""
import ctypes as C
import os
import sys

import pytest
import torch

from hsimae_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN, AB, AF = _lib.A_F32_LN, _lib.A_BF16, _lib.A_F32
EB, EF, ER, EP, ES, ESB, ELB = (_lib.E_BF16, _lib.E_F32, _lib.E_RES_F32, _lib.E_POS_F32, _lib.E_SWIGLU, _lib.E_SWIGLU_BWD,
                                _lib.E_LN_BWD)
BF16, FP8 = _lib.PREC_BF16, _lib.PREC_FP8
OK, EDIMS, EUNSUP, ENULL = 0, -1, -2, -4
GUARD_ROWS = 3
EPS_FN = R.EPS_FN           # __expf / rcp in the SiLU epilogues (relative, on top of the bf16 rounding of the result)

from gemm_ref import F8_PLAIN, PLAIN, TABLE, expected, inst_name  # noqa: E402  (the dispatch rule: shared with the CPU test of plan_gemm)


# ------------------------------------------------------------------------------------------------ the cases
# (ak, epi, prec, N, n_valid, K, bm, kc).  N / n_valid: 16 (the head), 80, 144 (k-outer with a partly empty chunk), 256,
# 272 / 384 / 512 (NCH = 4 with 3 / 3 / 4 live chunks), 1376; K: 32 .. 3072 (288, 1056: partial 256- / 512-chunks).
def _cases():
    cs = []
    for epi in (EB, ES, EF):                               # LayerNorm prologue (bf16)
        nv = (lambda n: n - 8) if epi == EF else (lambda n: n - 5)
        for N, K, bm in [(80, 96, 0), (144, 128, 0), (272, 256, 0), (272, 256, 128), (384, 352, 0), (384, 352, 128),
                         (1376, 512, 0), (1376, 512, 64)]:
            cs.append((LN, epi, BF16, N, nv(N), K, bm, 0))
        for N, K, bm in [(272, 256, 0), (144, 512, 128), (80, 96, 0)]:     # fp8 (compared in RMS: see test_layernorm_fp8)
            cs.append((LN, epi, FP8, N, nv(N), K, bm, 0))
    for ak, epi in PLAIN:
        nv = (lambda n: n - 5) if epi == EB else (lambda n: n - 8)
        for N, K, bm, kc in [(16, 3072, 0, 0), (80, 32, 0, 0), (128, 1024, 0, 0), (144, 288, 0, 0), (272, 352, 0, 0),
                             (384, 1056, 0, 0), (512, 1536, 0, 0), (1376, 96, 0, 0), (256, 1024, 128, 256), (256, 352, 64, 0),
                             (1376, 512, 128, 128)]:
            cs.append((ak, epi, BF16, N, nv(N), K, bm, kc))
    for N, K, bm, kc in [(352, 128, 0, 0), (352, 512, 0, 0), (192, 1056, 0, 0), (352, 512, 128, 256), (1376, 512, 0, 0)]:
        cs.append((AF, ESB, BF16, N, N, K, bm, kc))
    for ak, epi in F8_PLAIN:
        nv = (lambda n: n) if epi == ESB else (lambda n: n - 5) if epi == EB else (lambda n: n - 8)
        for N, K, bm in [(80, 96, 0), (144, 1056, 0), (384, 1536, 0), (512, 3072, 0), (1376, 512, 128), (16, 3072, 0),
                         (272, 1024, 128)]:
            cs.append((ak, epi, FP8, N, nv(N), K, bm, 0))
    return cs


CASES = _cases()
LN_BWD_CASES = [(BF16, 128, 384), (BF16, 256, 768), (BF16, 512, 1536), (BF16, 512, 288), (FP8, 256, 1024), (FP8, 512, 1536),
                (BF16, 128, 96), (BF16, 256, 288)]


def case_id(c):
    ak, epi, prec, N, nv, K, bm, kc = c
    return f"{'fp8' if prec else 'bf16'}-a{ak}-e{epi}-N{N}-nv{nv}-K{K}-bm{bm}-kc{kc}"


def test_dispatch_coverage():
    """Every case lands on a row of TABLE, and the cases reach every row."""
    reached = {expected(*c[:4], c[5], c[6], c[7]) for c in CASES}
    reached |= {expected(AB, ELB, prec, N, K) for prec, N, K in LN_BWD_CASES}
    assert reached <= TABLE, sorted(reached - TABLE)
    missing = TABLE - reached
    assert not missing, "instantiations without a case: " + ", ".join(inst_name(t) for t in sorted(missing))
    assert len(TABLE) == 90


# ------------------------------------------------------------------------------------------------ plumbing
def stream():
    return torch.cuda.current_stream().cuda_stream


def rup(x, m):
    return (x + m - 1) // m * m


def pack(W, N_img, K):
    """fp32 W [n, K] -> bf16 image [N_img, K] (hsimae_pack_matrix), zero rows past n."""
    img = torch.zeros(N_img * K, dtype=torch.bfloat16, device=DEV)
    W = W.contiguous().float()
    d = (_lib.PackDesc * 1)()
    d[0] = _lib.PackDesc(src=W.data_ptr(), rows=W.shape[0], cols=W.shape[1], transpose=0, n_off=0, k_off=0, KS=K // 32,
                         dst=img.data_ptr())
    table = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).clone().to(DEV)
    _lib.check(_lib.load().hsimae_pack_matrix(table.data_ptr(), 1, W.numel(), stream()))
    torch.cuda.synchronize()
    return img


def pack8(W, N_img, K):
    """fp32 W [n, K] -> (e4m3 image, e8m0 scale image) with desc.fp8 = 1."""
    KS = (K + 127) // 128
    img = torch.zeros((N_img // 16) * KS * 64 * 32, dtype=torch.uint8, device=DEV)
    sc = torch.zeros((N_img // 16) * ((KS + 3) // 4) * 64 * 4, dtype=torch.uint8, device=DEV)
    W = W.contiguous().float()
    d = (_lib.PackDesc * 1)()
    d[0] = _lib.PackDesc(src=W.data_ptr(), rows=W.shape[0], cols=W.shape[1], transpose=0, n_off=0, k_off=0, KS=KS,
                         dst=img.data_ptr(), fp8=1, scales=sc.data_ptr())
    table = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).clone().to(DEV)
    _lib.check(_lib.load().hsimae_pack_matrix(table.data_ptr(), 1, W.numel(), stream()))
    torch.cuda.synchronize()
    return img, sc


def call(akind, epi, bm=0, kc=0, **kw):
    p = _lib.GemmParams()
    for k, v in kw.items():
        setattr(p, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = _lib.load().hsimae_gemm_tiled(C.byref(p), akind, epi, bm, kc, stream())
    torch.cuda.synchronize()
    return rc


def nan_like(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=DEV)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def untouched(buf, ref, mask, what):
    """Canary check: where mask is set, buf still holds ref's bits."""
    assert torch.equal(bits(buf)[mask], bits(ref)[mask]), f"{what}: canary region written"


def col_mask(rows, ld, keep_cols, M):
    """True outside rows [0, M) x the given column ranges."""
    m = torch.ones(rows, ld, dtype=torch.bool, device=DEV)
    for a, b in keep_cols:
        m[:M, a:b] = False
    return m


def report(case, what, r):
    print(f"RATIO {what:<10s} {r:7.4f}  {inst_name(expected(*case[:4], case[5], case[6], case[7])) if len(case) == 8 else case}"
          f"  {case_id(case) if len(case) == 8 else ''}")
    assert r <= 1.0, f"{what}: err / bound = {r:.3g}"


def a_rows(M, K, ld, dtype, seed, fp8):
    """Operand rows [M, ld]: asymmetric values, a constant row, a large row with a large mean; NaN past K (never read)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(M, K, device=DEV, generator=g) * 0.7 + 0.05
    if fp8:            # per-32-block dynamic range: the MX scales differ along a row
        a = a * torch.exp2(torch.randint(-3, 3, (M, K // 32), device=DEV, generator=g).float()).repeat_interleave(32, 1)
    if M > 3:
        a[1] = 0.3
        a[2] = 40.0 + torch.randn(K, device=DEV, generator=g)
    out = torch.full((M, ld), float("nan"), device=DEV)
    out[:, :K] = a
    return out.to(dtype)


# ------------------------------------------------------------------------------------------------ the matrix
def run_case(case, M, seed, rowscale=False, res2=True, ln_width=0, extreme_bias=False):
    """Launch one case with canaries; returns (inputs, outputs) for the checks.  rowscale: DropPath factors (a_rowscale on
    A_F32 operands, out_rowscale in E_RES_F32).  extreme_bias: every 7th bias entry at -1000 / +1000."""
    ak, epi, prec, N, nv, K, bm, kc = case
    fp8 = prec == FP8
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    lda, ldo, ldr = K + 8, N + 16, N + 8
    inp = {"M": M}
    A = a_rows(M, K, lda, torch.bfloat16 if ak == AB else torch.float32, seed, fp8)
    if ak == LN and ln_width:
        A[:, ln_width:K] = float("nan")                        # storage padding: must not be read
    W = torch.randn(N, K, device=DEV, generator=g) * 0.1 + 0.01
    W2 = torch.randn(N, K, device=DEV, generator=g) * 0.1 - 0.01
    bias = torch.randn(N, device=DEV, generator=g) * 0.3
    bias2 = torch.randn(N, device=DEV, generator=g) * 0.3
    if extreme_bias:
        bias[3::7], bias[5::7] = -1000.0, 1000.0
    kw = dict(A=A, lda=lda, M=M, N=N, K=K, n_valid=nv, ldo=ldo, prec=prec)
    if fp8:
        kw["W8"], kw["S8"] = pack8(W, N, K)
        if epi == ES:
            kw["W8b"], kw["S8b"] = pack8(W2, N, K)
    else:
        kw["W"] = pack(W, N, K)
        if epi == ES:
            kw["W2"] = pack(W2, N, K)
    if epi != ESB:
        kw["bias"] = bias
    if epi == ES:
        kw["bias2"] = bias2
    out_dtype = torch.float32 if epi in (EF, ER, EP) else torch.bfloat16
    hoff = N + 8
    if epi == ESB:
        ldo = 2 * N + 24
        kw["ldo"] = ldo
    out = nan_like(M + GUARD_ROWS, ldo, out_dtype)
    kw["out"] = out
    if ak == LN:
        gamma = 1 + 0.2 * torch.randn(K, device=DEV, generator=g)
        beta = 0.1 * torch.randn(K, device=DEV, generator=g)
        kw.update(gamma=gamma, beta=beta, ln_width=ln_width)
        u = nan_like(M + GUARD_ROWS, K + 8, torch.bfloat16)
        kw.update(u_out=u, ldu=K + 8)
        inp.update(gamma=gamma, beta=beta, u=u)
    rs = None
    if rowscale and (ak == AF or epi == ER):      # factors 0 or 1 / keep, constant over runs of 9 rows; row 0 dropped
        keep = 0.8
        rs = (torch.rand((M + 8) // 9, device=DEV, generator=g) < keep).float().div(keep).repeat_interleave(9)[:M].contiguous()
        rs[0] = 0.0
        kw["a_rowscale" if ak == AF else "out_rowscale"] = rs
    if epi == ER:
        res = torch.full((M, ldr), float("nan"), device=DEV)
        res[:, :nv] = torch.randn(M, nv, device=DEV, generator=g)
        kw.update(res=res, ldr=ldr)
        inp["res"] = res
        if res2:
            r2 = torch.full((M, ldr), float("nan"), device=DEV)
            r2[:, :nv] = torch.randn(M, nv, device=DEV, generator=g)
            kw["res2"] = r2
            inp["res2"] = r2
    if epi == EP:
        P = 37
        pos = torch.randn(P, N + 8, device=DEV, generator=g)
        ids = torch.randint(0, P, (M,), device=DEV, dtype=torch.int32, generator=g)
        kw.update(pos=pos, ids=ids, ldpos=N + 8)
        inp.update(pos=pos, ids=ids)
    if epi in (ES, ESB):
        ldh = 2 * N + 24
        if epi == ES:
            h13 = nan_like(M + GUARD_ROWS, ldh, torch.bfloat16)
        else:                                               # pre-activations as the forward leaves them
            h13 = (torch.randn(M, ldh, device=DEV, generator=g) * 2).to(torch.bfloat16)
        kw.update(h13=h13, ldh=ldh, hoff=hoff)
        inp["h13"] = h13
    inp.update(A=A, W=W, W2=W2, bias=bias, bias2=bias2, rs=rs, out=out, hoff=hoff)
    canary = out.clone(), (inp["u"].clone() if "u" in inp else None), (inp["h13"].clone() if epi == ES else None)
    rc = call(ak, epi, bm, kc, **kw)
    assert rc == OK, f"hsimae_gemm_tiled returned {rc}"
    return inp, canary


def operand_a(case, inp):
    """The A operand exactly as the kernel multiplies it (fp32 values)."""
    ak, epi, prec, N, nv, K, bm, kc = case
    M = inp["M"]
    if ak == LN:
        return inp["u"][:M, :K].float()
    a = inp["A"][:, :K].float()
    if inp["rs"] is not None and ak == AF:
        a = a * inp["rs"][:, None]                       # fp32 product, then rounded as the kernel stages it
    if prec == FP8:
        return R.mx_e4m3(a if ak == AF else R.bf(a))
    return R.bf(a)


def operand_w(prec, W):
    return R.mx_e4m3(W) if prec == FP8 else R.bf(W)


def check_case(case, inp, canary, ln_width=0):
    ak, epi, prec, N, nv, K, bm, kc = case
    M, out = inp["M"], inp["out"]
    worst = 0.0
    a = operand_a(case, inp)
    y64, ab = R.prod64(a, operand_w(prec, inp["W"][:nv]))
    acc = R.acc_bound(K, ab, prec == FP8)
    b = inp["bias"][:nv].double()
    o = out[:M, :nv]
    if ak == LN:                                          # the staged LayerNorm output against fp64
        lw = ln_width or K
        u64, xh, rstd, kappa = R.ln64(inp["A"][:, :K].float().nan_to_num(0.0), inp["gamma"], inp["beta"], lw)
        r = R.ratio(inp["u"][:M, :K], u64, R.ln_out_bound(u64, xh, kappa, inp["gamma"], inp["beta"], lw))
        report(case, "ln-out", r)
        assert torch.equal(inp["u"][:M, lw:K].float(), torch.zeros(M, K - lw, device=DEV))   # columns past ln_width: zeros
        untouched(inp["u"], canary[1], col_mask(M + GUARD_ROWS, K + 8, [(0, K)], M), "u_out")
    if epi in (EF, ER, EP):
        ref = y64 + b
        mag = ref.abs() + b.abs()
        if epi == ER:
            s = inp["rs"][:, None].double() if inp["rs"] is not None else 1.0
            r1 = inp["res"][:, :nv].double()
            r2 = inp["res2"][:, :nv].double() if "res2" in inp else 0.0
            ref = ref * s + r1 + r2
            acc = acc * (s if isinstance(s, float) else s.abs())
            mag = mag * (s if isinstance(s, float) else s.abs()) + r1.abs() + (r2.abs() if "res2" in inp else 0.0) + ref.abs()
            if inp["rs"] is not None:                      # dropped rows: exactly the residual(s)
                z = inp["rs"] == 0
                exact = inp["res"][:, :nv] + (inp["res2"][:, :nv] if "res2" in inp else 0.0)
                assert torch.equal(o[z], exact[z]), "DropPath factor 0: out != res (+ res2)"
        if epi == EP:
            pp = inp["pos"][inp["ids"].long(), :nv].double()
            ref = ref + pp
            mag = mag + pp.abs() + ref.abs()
        worst = R.ratio(o, ref, acc + R.C2 * R.U * mag)
        report(case, "out", worst)
        # [n_valid, N), columns past N and rows past M: untouched
        untouched(out, canary[0], col_mask(M + GUARD_ROWS, out.shape[1], [(0, nv)], M), "out")
    elif epi == EB:
        ref = y64 + b
        bnd = acc * (1 + R.UB) + R.UB * ref.abs() + R.C2 * R.U * (ref.abs() + b.abs())
        report(case, "out", R.ratio(o, ref, bnd))
        if ak == AF and inp["rs"] is not None:
            z = inp["rs"] == 0
            assert torch.equal(o[z], R.bf(inp["bias"][:nv]).expand(int(z.sum()), nv).to(torch.bfloat16)), "DropPath 0 row"
        assert bool((out[:M, nv:N].float() == 0).all()), "E_BF16: columns [n_valid, N) are not exact zeros"
        untouched(out, canary[0], col_mask(M + GUARD_ROWS, out.shape[1], [(0, N)], M), "out")
    elif epi == ES:
        h13, hoff = inp["h13"], inp["hoff"]
        y3, ab3 = R.prod64(a, operand_w(prec, inp["W2"][:nv]))
        b3 = inp["bias2"][:nv].double()
        for what, hh, ref, ac, bb in (("h1", h13[:M, :nv], y64 + b, acc, b), ("h3", h13[:M, hoff:hoff + nv], y3 + b3,
                                                                               R.acc_bound(K, ab3, prec == FP8), b3)):
            bnd = ac * (1 + R.UB) + R.UB * ref.abs() + R.C2 * R.U * (ref.abs() + bb.abs())
            report(case, what, R.ratio(hh, ref, bnd))
        a1, a3 = h13[:M, :nv].double(), h13[:M, hoff:hoff + nv].double()
        gref = a1 * torch.sigmoid(a1) * a3
        report(case, "gate", R.ratio(o, gref, (R.UB + EPS_FN) * gref.abs()))
        assert bool((out[:M, nv:N].float() == 0).all()) and bool((h13[:M, nv:N].float() == 0).all()) and \
            bool((h13[:M, hoff + nv:hoff + N].float() == 0).all()), "E_SWIGLU: columns [n_valid, N) are not exact zeros"
        untouched(out, canary[0], col_mask(M + GUARD_ROWS, out.shape[1], [(0, N)], M), "out")
        untouched(h13, canary[2], col_mask(M + GUARD_ROWS, h13.shape[1], [(0, N), (hoff, hoff + N)], M), "h13")
    elif epi == ESB:
        hoff = inp["hoff"]
        a1, a3 = inp["h13"][:M, :N].double(), inp["h13"][:M, hoff:hoff + N].double()
        s = torch.sigmoid(a1)
        D1, D3 = a3 * s * (1 + a1 * (1 - s)), a1 * s
        for what, o2, D, mag in (("d1", out[:M, :N], D1, a3.abs() * s * (1 + a1.abs() * (1 - s))),
                                 ("d3", out[:M, hoff:hoff + N], D3, D3.abs())):
            ref = y64 * D
            bnd = acc * D.abs() * (1 + R.UB) + R.UB * ref.abs() + 4 * EPS_FN * y64.abs() * mag
            report(case, what, R.ratio(o2, ref, bnd))
        if ak == AF and inp["rs"] is not None:
            z = inp["rs"] == 0
            assert bool((out[:M][z][:, :N].float() == 0).all()) and bool((out[:M][z][:, hoff:hoff + N].float() == 0).all())
        untouched(out, canary[0], col_mask(M + GUARD_ROWS, out.shape[1], [(0, N), (hoff, hoff + N)], M), "out")


def row_counts(bm):
    return [1, bm - 1, bm + 1, 1000, 3001]


@pytest.mark.parametrize("case", [c for c in CASES if not (c[0] == LN and c[2] == FP8)], ids=case_id)
def test_gemm_branch(case):
    bm = expected(*case[:4], case[5], case[6], case[7])[3]
    for i, M in enumerate(row_counts(bm)):
        inp, canary = run_case(case, M, seed=17 * i + case[3], rowscale=i % 2 == 1, res2=i % 4 != 3)
        check_case(case, inp, canary)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == LN and c[2] == FP8], ids=case_id)
def test_layernorm_fp8(case):
    """A_F32_LN in fp8: a LayerNorm one fp32 bit off can move an element across an e4m3 boundary, so the product is
    compared in RMS against the MX image of the fp64 LayerNorm; the bf16 copy (u_out) and the canaries as everywhere."""
    ak, epi, prec, N, nv, K, bm, kc = case
    for i, M in enumerate((1, 63, 65, 1000)):
        inp, canary = run_case(case, M, seed=5 + i)
        u64, xh, rstd, kappa = R.ln64(inp["A"][:, :K].float(), inp["gamma"], inp["beta"])
        report(case, "ln-out", R.ratio(inp["u"][:M, :K], u64, R.ln_out_bound(u64, xh, kappa, inp["gamma"], inp["beta"])))
        uq = R.mx_e4m3(u64.float())
        y1 = R.prod64(uq, R.mx_e4m3(inp["W"][:nv]))[0] + inp["bias"][:nv].double()
        out = inp["out"]
        if epi == ES:
            y3 = R.prod64(uq, R.mx_e4m3(inp["W2"][:nv]))[0] + inp["bias2"][:nv].double()
            h13, hoff = inp["h13"], inp["hoff"]
            if M > 1:
                assert R.rms_rel(h13[:M, :nv], y1) < 3e-3 and R.rms_rel(h13[:M, hoff:hoff + nv], y3) < 3e-3
                assert R.rms_rel(out[:M, :nv], torch.nn.functional.silu(y1) * y3) < 1e-2
            assert bool((out[:M, nv:N].float() == 0).all()) and bool((h13[:M, nv:N].float() == 0).all())
            untouched(h13, canary[2], col_mask(M + GUARD_ROWS, h13.shape[1], [(0, N), (hoff, hoff + N)], M), "h13")
        elif M > 1:
            assert R.rms_rel(out[:M, :nv], y1) < 3e-3
        if epi == EB:
            assert bool((out[:M, nv:N].float() == 0).all())
        untouched(out, canary[0], col_mask(M + GUARD_ROWS, out.shape[1], [(0, nv if epi == EF else N)], M), "out")


def test_swiglu_extreme_preactivations():
    """E_SWIGLU with gate pre-activations near -1000 and +1000 (through the bias): below -88.72 the exponential of the forward
    SiLU overflows.  The gate must be finite and inside the usual check on the kernel's own h13.  (At -1000 sigmoid is 0 in
    float64 as well; between -88.72 and -745 the reference is a number below bf16's range that the relative check cannot admit.)"""
    case = (LN, ES, BF16, 272, 267, 256, 0, 0)
    for i, M in enumerate((65, 333)):
        inp, canary = run_case(case, M, seed=41 + i, extreme_bias=True)
        h1 = inp["h13"][:M, :267].float()
        assert float(h1.min()) < -900 and float(h1.max()) > 900
        assert bool(torch.isfinite(inp["out"][:M, :272].float()).all()), "E_SWIGLU: the gate is not finite"
        check_case(case, inp, canary)


@pytest.mark.parametrize("prec", [BF16, FP8])
@pytest.mark.parametrize("K,lw", [(160, 144), (96, 72)])
def test_layernorm_over_a_narrower_width(K, lw, prec):
    """ln_width < K (rows stored wider than the LayerNorm): statistics over the first ln_width columns only, zeros past it in
    u_out and in the staged operand (the padding columns hold NaN and must not be read)."""
    for epi in (EB, EF):
        case = (LN, epi, prec, 144, 136, K, 0, 0)
        for i, M in enumerate((129, 1000)):
            inp, canary = run_case(case, M, seed=31 + i, ln_width=lw)
            if prec == BF16:
                check_case(case, inp, canary, ln_width=lw)
                continue
            u64, xh, rstd, kappa = R.ln64(inp["A"][:, :K].float().nan_to_num(0.0), inp["gamma"], inp["beta"], lw)
            report(case, "ln-out", R.ratio(inp["u"][:M, :K], u64, R.ln_out_bound(u64, xh, kappa, inp["gamma"], inp["beta"], lw)))
            assert bool((inp["u"][:M, lw:K].float() == 0).all())
            y1 = R.prod64(R.mx_e4m3(u64.float()), R.mx_e4m3(inp["W"][:136]))[0] + inp["bias"][:136].double()
            assert R.rms_rel(inp["out"][:M, :136], y1) < 3e-3


def test_zero_rows_is_a_no_op():
    for case in [(AB, EF, BF16, 144, 136, 288, 0, 0), (LN, ES, BF16, 80, 75, 96, 0, 0), (AB, EB, FP8, 384, 379, 1536, 0, 0)]:
        ak, epi, prec, N, nv, K, bm, kc = case
        out = nan_like(4, N + 16, torch.float32)
        A = torch.zeros(4, K, device=DEV)
        rc = call(ak, epi, A=A, lda=K, M=0, N=N, K=K, n_valid=nv, out=out, ldo=N + 16, prec=prec)
        assert rc == OK and bool(out.isnan().all())


# ------------------------------------------------------------------------------------------------ E_LN_BWD
def ln_bwd_inputs(prec, N, K, M, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ldr, ldo = N + 8, N + 16
    A = a_rows(M, K, K + 8, torch.bfloat16, seed, prec == FP8)
    W = torch.randn(N, K, device=DEV, generator=g) * 0.05 + 0.002
    x = torch.full((M, ldr), float("nan"), device=DEV)
    x[:, :N] = torch.randn(M, N, device=DEV, generator=g) * 2 + 0.5
    if M > 4:
        x[3, :N] = 0.25                                       # zero variance
        x[4, :N] = 300 + torch.randn(N, device=DEV, generator=g)   # large mean
    res = torch.full((M, ldr), float("nan"), device=DEV)
    res[:, :N] = torch.randn(M, N, device=DEV, generator=g)
    gamma = 1 + 0.2 * torch.randn(N, device=DEV, generator=g)
    kw = dict(A=A, lda=K + 8, M=M, N=N, K=K, n_valid=N, lnx=x, res=res, ldr=ldr, gamma=gamma, prec=prec)
    if prec == FP8:
        kw["W8"], kw["S8"] = pack8(W, N, K)
    else:
        kw["W"] = pack(W, N, K)
    return kw, W, ldo


def ln_bwd_ref(kw, W, prec):
    M, N, K = kw["M"], kw["N"], kw["K"]
    a = kw["A"][:, :K].float()
    a = R.mx_e4m3(a) if prec == FP8 else a
    du64, ab = R.prod64(a, R.mx_e4m3(W) if prec == FP8 else R.bf(W))
    dx64, dg64, db64, xhat, rstd, kappa = R.ln_bwd64(du64, kw["lnx"][:, :N], kw["gamma"], N)
    acc = R.acc_bound(K, ab, prec == FP8)
    bnd = R.ln_bwd_bound(acc, du64, xhat, rstd, kappa, kw["gamma"])
    # dgamma / dbeta: sums over rows of du * xhat and du (each term's error: the product's plus the x-hat's)
    # fp32 sums: a thread's rows in sequence, a 16-lane tree, one commit per workgroup (fixed point: 2^-44 per commit)
    e_xh = R.C_LN * R.U * (1 + kappa) * (xhat.abs() + 1)
    depth = 12 + (M + 31) // 32
    bg = (acc * xhat.abs() + du64.abs() * e_xh).sum(0) + depth * R.U * (du64 * xhat).abs().sum(0) + 2.0 ** -44 * depth
    bb = acc.sum(0) + depth * R.U * du64.abs().sum(0) + 2.0 ** -44 * depth
    return dx64, bnd, dg64, bg, db64, bb


def run_ln_bwd(kw, ldo, accumulate=0, inplace=False, u_out=False, det=False, prev=None):
    M, N = kw["M"], kw["N"]
    kw = dict(kw)
    if inplace:
        out = torch.full((M + GUARD_ROWS, kw["ldr"]), float("nan"), device=DEV)
        out[:M] = kw["res"]
        kw["res"], kw["ldo"] = out, kw["ldr"]
    else:
        out = nan_like(M + GUARD_ROWS, ldo, torch.float32)
        if prev is not None:
            out[:M, :N] = prev
        kw["ldo"] = ldo
    kw["out"], kw["accumulate"] = out, accumulate
    flat = torch.zeros(3 * N + 40, device=DEV)                 # dgamma at 8, dbeta at N + 24: a flat gradient buffer
    dg, db = flat[8:8 + N], flat[N + 24:2 * N + 24]
    kw.update(dgamma=dg, dbeta=db)
    acc64 = None
    if det:
        acc64 = torch.zeros(flat.numel(), dtype=torch.int64, device=DEV)
        kw.update(det_base=flat, det_acc=acc64)
    u = None
    if u_out:
        u = nan_like(M + GUARD_ROWS, N + 8, torch.bfloat16)
        kw.update(u_out=u, ldu=N + 8)
    canary = out.clone()
    rc = call(AB, ELB, **kw)
    assert rc == OK, rc
    if det:
        conv = flat.double() + acc64.double() * 2.0 ** -44      # what the library's conversion pass does
        dg, db = conv[8:8 + N].float(), conv[N + 24:2 * N + 24].float()
        assert bool((flat[:8] == 0).all() and (flat[8 + N:N + 24] == 0).all() and (flat[2 * N + 24:] == 0).all())
        assert bool((acc64[:8] == 0).all() and (acc64[8 + N:N + 24] == 0).all() and (acc64[2 * N + 24:] == 0).all())
    return out, canary, dg, db, u, (flat, acc64)


@pytest.mark.parametrize("prec,N,K", LN_BWD_CASES, ids=lambda v: str(v))
def test_ln_bwd(prec, N, K):
    case = (prec, N, K)
    name = inst_name(expected(AB, ELB, prec, N, K))
    Ms = (1, 31, 33, 1000) if N == 512 else (1, 63, 65, 1000)
    for i, M in enumerate(Ms):
        kw, W, ldo = ln_bwd_inputs(prec, N, K, M, seed=100 + i)
        dx64, bnd, dg64, bg, db64, bb = ln_bwd_ref(kw, W, prec)
        res64 = kw["res"][:M, :N].double()
        for mode in ("plain", "accumulate", "inplace", "det"):
            prev = torch.randn(M, N, device=DEV) if mode == "accumulate" else None
            out, canary, dg, db, u, _ = run_ln_bwd(kw, ldo, accumulate=int(mode == "accumulate"), inplace=mode == "inplace",
                                                   u_out=N > 128, det=mode == "det", prev=prev)
            ref = dx64 + res64 + (prev.double() if prev is not None else 0.0)
            mag = R.C2 * R.U * (ref.abs() + res64.abs() + (prev.double().abs() if prev is not None else 0.0) + dx64.abs())
            r = R.ratio(out[:M, :N], ref, bnd + mag)
            print(f"RATIO dx-{mode:<8s} {r:7.4f}  {name}  M={M} {case}")
            assert r <= 1, (mode, r)
            r = max(R.ratio(dg, dg64, bg), R.ratio(db, db64, bb))
            print(f"RATIO dgb-{mode:<7s} {r:7.4f}  {name}  M={M} {case}")
            assert r <= 1, (mode, r)
            untouched(out, canary, col_mask(out.shape[0], out.shape[1], [(0, N)], M), "out")
            if u is not None:                                  # the bf16 copy of the result
                r = R.ratio(u[:M, :N], ref, (bnd + mag) * (1 + R.UB) + R.UB * ref.abs())
                print(f"RATIO u-{mode:<9s} {r:7.4f}  {name}  M={M} {case}")
                assert r <= 1 and torch.equal(u[:M, :N], out[:M, :N].to(torch.bfloat16))
                assert bool(u[M:].isnan().all()) and bool(u[:, N:].isnan().all())


@pytest.mark.parametrize("prec,N,K", [(BF16, 128, 384), (BF16, 256, 768), (BF16, 512, 1536), (FP8, 256, 1024), (FP8, 512, 1536)],
                         ids=lambda v: str(v))
def test_ln_bwd_deterministic_commits(prec, N, K):
    """det_base / det_acc: bit-identical on a second call, and a non-finite addend poisons its slot with NaN."""
    kw, W, ldo = ln_bwd_inputs(prec, N, K, 700, seed=7)
    first = run_ln_bwd(kw, ldo, det=True)
    second = run_ln_bwd(kw, ldo, det=True)
    assert torch.equal(bits(first[0]), bits(second[0]))
    assert torch.equal(first[5][1], second[5][1]) and torch.equal(bits(first[2]), bits(second[2]))
    kw = dict(kw)
    A = kw["A"].clone()
    A[5, 3] = float("inf")                                    # row 5's du is not finite: its workgroup's column sums neither
    kw["A"] = A
    _, _, dg, db, _, _ = run_ln_bwd(kw, ldo, det=True)
    assert bool(dg.isnan().all()) and bool(db.isnan().all())


def test_ln_bwd_bf16_n512():
    """The bf16 N = 512 form gemm_kernel<0, 6, 256, 32, 0, 4>: no caller in the library reaches it (plan_block chooses the
    LayerNorm-backward epilogue at d = 512 only in fp8), run on its own so that a fault in it is attributed to it."""
    kw, W, ldo = ln_bwd_inputs(BF16, 512, 1056, 97, seed=3)
    dx64, bnd, dg64, bg, db64, bb = ln_bwd_ref(kw, W, BF16)
    out, canary, dg, db, u, _ = run_ln_bwd(kw, ldo, u_out=True)
    ref = dx64 + kw["res"][:97, :512].double()
    r = R.ratio(out[:97, :512], ref, bnd + R.C2 * R.U * (ref.abs() + dx64.abs() + kw["res"][:97, :512].double().abs()))
    print(f"RATIO dx-n512     {r:7.4f}")
    assert r <= 1 and max(R.ratio(dg, dg64, bg), R.ratio(db, db64, bb)) <= 1
    untouched(out, canary, col_mask(out.shape[0], out.shape[1], [(0, 512)], 97), "out")


# ------------------------------------------------------------------------------------------------ tiling invariance
TILINGS = [(bm, kc) for bm in (0, 64, 128) for kc in (0, 128, 256) if (bm, kc) != (0, 0)]
TILE_CASES = [c for c in CASES if c[6] == 0 and c[7] == 0 and c[3] in (16, 144, 384, 512, 1376)]


@pytest.mark.parametrize("case", TILE_CASES, ids=case_id)
def test_tiling_is_bit_identical(case):
    """hsimae_gemm_tiled: every forced (bm, kc) gives the default dispatch's bits (the header's promise)."""
    M = 333

    def outputs(bm, kc):
        c = case[:6] + (bm, kc)
        inp, _ = run_case(c, M, seed=9)
        o = [bits(inp["out"][:M]).clone()]
        if "u" in inp:
            o.append(bits(inp["u"][:M]).clone())
        if case[1] == ES:
            o.append(bits(inp["h13"][:M]).clone())
        return o

    base = outputs(0, 0)
    for bm, kc in TILINGS:
        got = outputs(bm, kc)
        for x, y in zip(base, got):
            assert torch.equal(x, y), f"tiling bm={bm} kc={kc} differs from the default ({inst_name(expected(*case[:4], case[5], bm, kc))})"


def test_ln_bwd_tiling_is_ignored_and_bit_identical():
    kw, W, ldo = ln_bwd_inputs(BF16, 128, 384, 333, seed=11)
    base = run_ln_bwd(kw, ldo, det=True)
    for bm, kc in TILINGS:
        k2 = dict(kw)
        flat = torch.zeros(3 * 128 + 40, device=DEV)
        acc64 = torch.zeros(flat.numel(), dtype=torch.int64, device=DEV)
        out = nan_like(333 + GUARD_ROWS, ldo, torch.float32)
        k2.update(out=out, ldo=ldo, dgamma=flat[8:136], dbeta=flat[152:280], det_base=flat, det_acc=acc64)
        assert call(AB, ELB, bm, kc, **k2) == OK
        assert torch.equal(bits(out), bits(base[0])) and torch.equal(acc64, base[5][1])


# ------------------------------------------------------------------------------------------------ refusals
def refusal_kw(ak=AB, epi=EF, prec=BF16, N=128, K=128, M=40):
    A = torch.zeros(M, K + 8, device=DEV, dtype=torch.bfloat16 if ak == AB else torch.float32)
    kw = dict(A=A, lda=K + 8, M=M, N=N, K=K, n_valid=N, ldo=N + 16, prec=prec)
    if prec == FP8:
        kw["W8"], kw["S8"] = pack8(torch.zeros(N, rup(K, 32), device=DEV), N, rup(K, 32))
    else:
        kw["W"] = torch.zeros(rup(N, 16) * rup(K, 32), dtype=torch.bfloat16, device=DEV)
    if ak == LN:
        kw.update(gamma=torch.ones(max(K, 8) + 8, device=DEV), beta=torch.zeros(max(K, 8) + 8, device=DEV))
    if epi == ELB:
        kw.update(lnx=torch.zeros(M, N, device=DEV), res=torch.zeros(M, N, device=DEV), ldr=N, gamma=torch.ones(N, device=DEV),
                  dgamma=torch.zeros(N, device=DEV), dbeta=torch.zeros(N, device=DEV))
    if epi == ER:
        kw.update(res=torch.zeros(M, N, device=DEV), ldr=N)
    if epi == EP:
        kw.update(pos=torch.zeros(4, N, device=DEV), ids=torch.zeros(M, dtype=torch.int32, device=DEV), ldpos=N)
    return kw


REFUSALS = [
    # (id, a kind, epilogue, prec, N, K, field overrides, expected code)
    ("lnbwd-N384", AB, ELB, BF16, 384, 128, {}, EUNSUP),
    ("lnbwd-N64", AB, ELB, BF16, 64, 128, {}, EUNSUP),
    ("lnbwd-N1024", AB, ELB, BF16, 1024, 128, {}, EUNSUP),
    ("lnbwd-nvalid128", AB, ELB, BF16, 128, 128, {"n_valid": 120}, EUNSUP),
    ("lnbwd-nvalid256", AB, ELB, BF16, 256, 128, {"n_valid": 248}, EUNSUP),
    ("lnbwd-nvalid512", AB, ELB, BF16, 512, 128, {"n_valid": 504}, EUNSUP),
    ("lnbwd-u_out-N128", AB, ELB, BF16, 128, 128, {"u_out": "buf", "ldu": 128}, EUNSUP),
    ("lnbwd-fp8-N128", AB, ELB, FP8, 128, 128, {}, EUNSUP),
    ("lnbwd-fp8-N256-noW8", AB, ELB, FP8, 256, 128, {"W8": None}, ENULL),
    ("lnbwd-fp8-N512-noS8", AB, ELB, FP8, 512, 128, {"S8": None}, ENULL),
    ("fp8-pos", AB, EP, FP8, 128, 128, {}, EUNSUP),
    ("fp8-noW8", AB, EF, FP8, 128, 128, {"W8": None}, ENULL),
    ("fp8-noS8", AF, EB, FP8, 128, 128, {"S8": None}, ENULL),
    ("fp8-swiglu-noW8b", LN, ES, FP8, 128, 128, {"h13": "buf", "ldh": 256, "hoff": 128}, ENULL),
    ("ln-K544", LN, EF, BF16, 128, 544, {}, EUNSUP),
    ("ln-fp8-K544", LN, EF, FP8, 128, 544, {}, EUNSUP),
    ("K%32", AB, EF, BF16, 128, 112, {}, EDIMS),
    ("N%16", AB, EF, BF16, 120, 128, {"n_valid": 120}, EDIMS),
    ("lda%8", AB, EF, BF16, 128, 128, {"lda": 132}, EDIMS),
    ("ldo%8", AB, EF, BF16, 128, 128, {"ldo": 140}, EDIMS),
    ("nvalid%8-f32", AB, EF, BF16, 128, 128, {"n_valid": 124}, EDIMS),
    ("nvalid%8-res", AB, ER, BF16, 128, 128, {"n_valid": 124}, EDIMS),
    ("nvalid%8-pos", AB, EP, BF16, 128, 128, {"n_valid": 124}, EDIMS),
    ("ln_width%8", LN, EF, BF16, 128, 160, {"ln_width": 148}, EDIMS),
    ("ln_width>K", LN, EF, BF16, 128, 160, {"ln_width": 168}, EDIMS),
    ("ln_width<0", LN, EF, BF16, 128, 160, {"ln_width": -8}, EDIMS),
    ("akind-bad", 3, EF, BF16, 128, 128, {}, EUNSUP),
    ("a_f32-res", AF, ER, BF16, 128, 128, {}, EUNSUP),
    ("tiled-bm32", AB, EF, BF16, 128, 128, {"_bm": 32}, EDIMS),
    ("tiled-kc512", AB, EF, BF16, 128, 128, {"_kc": 512}, EDIMS),
]
for _n in ("lnx", "res", "gamma", "dgamma", "dbeta"):
    for _N in (128, 256, 512):
        REFUSALS.append((f"lnbwd-N{_N}-no-{_n}", AB, ELB, BF16, _N, 128, {_n: None}, EUNSUP))


@pytest.mark.parametrize("rid,ak,epi,prec,N,K,over,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(rid, ak, epi, prec, N, K, over, code):
    kw = refusal_kw(ak if ak in (AB, AF, LN) else AB, epi, prec, N, K)
    over = dict(over)
    bm, kc = over.pop("_bm", 0) if "_bm" in over else 0, over.pop("_kc", 0) if "_kc" in over else 0
    for k, v in over.items():
        if v == "buf":
            v = nan_like(kw["M"] + GUARD_ROWS, 2 * N + 16, torch.bfloat16)
            kw[k + "_buf"] = v
        kw[k] = v
    out = nan_like(kw["M"] + GUARD_ROWS, kw["ldo"] if kw["ldo"] % 8 == 0 else kw["ldo"] + 8, torch.float32)
    kw["out"] = out
    bufs = {k: v for k, v in kw.items() if k.endswith("_buf")}
    for k in bufs:
        kw.pop(k)
    rc = call(ak, epi, bm, kc, **kw)
    assert rc == code, f"{rid}: hsimae_gemm returned {rc}, expected {code}"
    assert bool(out.isnan().all()), f"{rid}: a refused call wrote its output"
    for k, v in bufs.items():
        assert bool(v.isnan().all()), f"{rid}: a refused call wrote {k[:-4]}"
