"""fp64 reference, element-wise error bound and dispatch rule of hsimae_gemm (tests/test_gpu_gemm.py, tests/test_gemm_bound_cpu.py,
tests/test_launch_plan_cpu.py).

A plain module, not a conftest: the GPU tests and the CPU test of the bound import the same functions.

The reference is evaluated in float64 on exactly the operands the kernel multiplies (bf16-rounded A and W, the kernel's
own bf16 LayerNorm output, or the MX e4m3 images).  A kernel result y is accepted element by element when

    |y - y64| <= C1 * sqrt(K / 32) * 2^-24 * (|A| |W|^T)_ij  +  C2 * 2^-24 * mag_ij  (+ the epilogue's own roundings, e.g. bf16: 2^-8 |y64|)

The first term is the dot-product accumulation in fp32, the second the fp32 roundings of the epilogue (bias, residual,
output), mag being the sum of the magnitudes the epilogue adds.  A bound is only useful if it is tight: the tests print the
worst err / bound they saw per branch.
"""
import math

import torch

U = 2.0 ** -24           # fp32 unit roundoff
UB = 2.0 ** -8           # bf16 unit roundoff (8-bit significand: half an ulp, relative)
# Accumulation.  The products inside one 32-deep bf16 MFMA step are exact and the running sum is rounded to fp32 once per
# step, so the deterministic bound is (K / 32) * 2^-24 * (|A| |W|^T).  On random-sign data those roundings do not add up
# in one direction: measured on MI355X the worst error stays near 2 * 2^-24 * (|A| |W|^T) at every K from 32 to 3072, and
# the deterministic form was 15-60x above it at K >= 1024, too loose to catch a lost low-order contribution.  The bound
# uses its probabilistic form instead (Higham & Mary 2019): C1 * sqrt(K / 32) * 2^-24 * (|A| |W|^T).
C1 = 1.0
# fp8 (MX): the matrix core aligns the 128 scaled products of a step internally with a limited number of bits below the
# largest, so each step adds an error of up to ~2^-14 of its own sum of |a w| whatever K is (measured: up to 2^-13.8 at K = 96,
# 2^-15.4 at K = 512).  One term for every K: 2^-13.
C1_F8 = 2048.0
# The epilogue's fp32 roundings (the output and each add), in units of 2^-24 of the sum of the magnitudes involved.
C2 = 4.0
# LayerNorm statistics in fp32 (a tree sum over the row, x - mean, rsqrt): relative to (1 + kappa), kappa = rstd * mean|x|.
C_LN = 16.0
# __expf / v_rcp_f32 in the SiLU epilogues and the fused MLP kernels: relative error of silu and its derivative factors, on top of
# the bf16 rounding of the result (tests/test_gpu_gemm.py, tests/mlp_ref.py)
EPS_FN = 2.0 ** -18


# ------------------------------------------------------------------------------------------------ the dispatch rule
# hs_gemm launches one gemm_kernel<AK, EPI, KC, BM, F8, NCH> per call; csrc/plan.h plan_gemm picks it from the A kind, the epilogue,
# the precision, N, K and the tiling.  TABLE lists every instantiation that rule can launch and `expected()` restates the rule.
# tests/test_launch_plan_cpu.py compares both with the library's own rule and list (no GPU); tests/test_gpu_gemm.py proves that
# its cases reach every row.  The constants are those of include/hsimae_hip.h (HSIMAE_A_*, HSIMAE_E_*, HSIMAE_PREC_*).
AB, AF, LN = 0, 1, 2
EB, EF, ER, EP, ES, ESB, ELB = 0, 1, 2, 3, 4, 5, 6
BF16, FP8 = 0, 1
PLAIN = [(AB, ER), (AB, EP), (AB, EF), (AB, EB), (AF, EB), (AF, EF)]          # bf16: no prologue, no gate pair
F8_PLAIN = [(AB, ER), (AB, EF), (AB, EB), (AF, ESB), (AF, EB), (AF, EF)]      # fp8: no prologue, no gate pair


def _table():
    t = set()
    for epi in (EB, ES, EF):
        # LayerNorm prologue: the whole row is one chunk (KC from K), 64-row panels when the weights are small; fp8: 512
        t |= {(LN, epi, 128, 128, 0, 1), (LN, epi, 256, 64, 0, 1), (LN, epi, 256, 128, 0, 1), (LN, epi, 512, 64, 0, 1),
              (LN, epi, 512, 128, 0, 1), (LN, epi, 512, 64, 1, 1), (LN, epi, 512, 128, 1, 1)}
    for ak, epi in PLAIN:
        # k-outer with 2 / 4 accumulator sets, else n-outer with 128 / 256-deep chunks on 64 / 128-row panels
        t |= {(ak, epi, 256, 64, 0, 2), (ak, epi, 256, 64, 0, 4), (ak, epi, 256, 64, 0, 1), (ak, epi, 256, 128, 0, 1),
              (ak, epi, 128, 64, 0, 1), (ak, epi, 128, 128, 0, 1)}
    t |= {(AF, ESB, kc, bm, 0, 1) for kc in (128, 256) for bm in (64, 128)}
    for ak, epi in F8_PLAIN:
        t |= {(ak, epi, 512, 32 if ak == AB else 64, 1, 2), (ak, epi, 512, 32 if ak == AB else 64, 1, 4),
              (ak, epi, 512, 64, 1, 1), (ak, epi, 512, 128, 1, 1)}
    t |= {(AB, ELB, 128, 128, 0, 1), (AB, ELB, 256, 64, 0, 2), (AB, ELB, 256, 32, 0, 4), (AB, ELB, 512, 32, 1, 2),
          (AB, ELB, 512, 32, 1, 4)}
    return t


TABLE = _table()


def small_weights(N, K, dual):
    if K < 256:
        return False
    if dual:
        return N * K <= 400 * 1024
    return N * K <= (800 if K <= 512 else 400) * 1024


def expected(ak, epi, prec, N, K, bm=0, kc=0):
    """(AK, EPI, KC, BM, F8, NCH) of the kernel hs_gemm (hs_gemm_tiled with bm / kc) launches: a restatement of the rule."""
    if epi == ELB:
        if N == 512:
            return (AB, ELB, 512, 32, 1, 4) if prec == FP8 else (AB, ELB, 256, 32, 0, 4)
        if N == 256:
            return (AB, ELB, 512, 32, 1, 2) if prec == FP8 else (AB, ELB, 256, 64, 0, 2)
        return (AB, ELB, 128, 128, 0, 1)
    if prec == FP8:
        if ak != LN and epi != ES and K > 512 and 128 < N <= 512 and bm != 128:
            return (ak, epi, 512, 32 if ak == AB else 64, 1, 2 if N <= 256 else 4)
        return (ak, epi, 512, 128 if bm == 128 else 64, 1, 1)
    bm64 = bm == 64 if bm else small_weights(N, K, epi == ES)
    if ak == LN:
        kcx = 128 if K <= 128 else 256 if K <= 256 else 512
        return (ak, epi, kcx, 128 if kcx == 128 or not bm64 else 64, 0, 1)
    if epi != ESB and not bm and K > 256 and 128 < N <= 512:
        return (ak, epi, 256, 64, 0, 2 if N <= 256 else 4)
    kc256 = kc == 256 if kc else (bm64 and 256 <= K <= 1024)
    return (ak, epi, 256 if kc256 else 128, 64 if bm64 else 128, 0, 1)


def inst_name(t):
    return "gemm_kernel<%d, %d, %d, %d, %d, %d>" % t


def bf(x):
    """fp32 value of the bf16 rounding (round to nearest even) of x."""
    return x.to(torch.bfloat16).float()


def mx_e4m3(x):
    """MX quantisation along the last dim (32-element blocks, e8m0 scale 2^(floor(log2 amax) - 8), saturating e4m3, RNE),
    returned de-quantised in fp32.  The last dim must be a multiple of 32.  (Same rule as the kernel's put_a8 and the
    fp8 weight pack.)"""
    sh = x.shape
    b = x.float().reshape(-1, sh[-1] // 32, 32)
    am = b.abs().amax(dim=-1, keepdim=True)
    e = torch.floor(torch.log2(am.clamp_min(2.0 ** -120))) - 8
    e = e.clamp(-126, 127)
    scale = torch.exp2(e)
    q = (b / scale).clamp(-448, 448).to(torch.float8_e4m3fn).float()
    return (q * scale).reshape(sh)


def prod64(a, w):
    """(a @ w^T, |a| @ |w|^T) in float64 from the operands as given (already rounded to what the kernel multiplies)."""
    a, w = a.double(), w.double()
    return a @ w.t(), a.abs() @ w.abs().t()


def acc_bound(K, absprod, fp8=False):
    """Accumulation term of the bound: (C1 * sqrt(K / 32) [+ C1_F8]) * 2^-24 * (|A| |W|^T)."""
    return (C1 * math.sqrt(K / 32) + (C1_F8 if fp8 else 0.0)) * U * absprod


def ln64(x, gamma, beta, width=None, eps=1e-5, unbiased=False):
    """LayerNorm over the first `width` columns of x in float64 (biased variance, as nn.LayerNorm); columns past `width`
    come out 0.  Returns (y, xhat, rstd [M, 1], kappa [M, 1]) with kappa = rstd * mean|x|, the row's condition for the
    fp32 statistics."""
    x = x.double()
    K = x.shape[1]
    w = K if not width else width
    xv = x[:, :w]
    mean = xv.mean(1, keepdim=True)
    var = xv.var(1, keepdim=True, unbiased=unbiased)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xv - mean) * rstd
    y = torch.zeros_like(x)
    y[:, :w] = xhat * gamma[:w].double() + beta[:w].double()
    xh = torch.zeros_like(x)
    xh[:, :w] = xhat
    kappa = rstd * xv.abs().mean(1, keepdim=True)
    return y, xh, rstd, kappa


def ln_stat_bound(xhat, kappa, gamma, beta, width=None):
    """The statistics part of ln_out_bound: the error of the fp32 LayerNorm value before it is rounded to bf16."""
    K = xhat.shape[1]
    w = K if not width else width
    g = torch.zeros(K, dtype=torch.float64, device=xhat.device)
    b = torch.zeros_like(g)
    g[:w], b[:w] = gamma[:w].double().abs(), beta[:w].double().abs()
    return C_LN * U * (1 + kappa) * g * (xhat.abs() + 1) + C2 * U * b


def ln_out_bound(y64, xhat, kappa, gamma, beta, width=None):
    """Bound for the bf16 LayerNorm output (u_out) against ln64: one bf16 rounding plus the fp32 statistics' error."""
    return UB * y64.abs() + (1 + UB) * ln_stat_bound(xhat, kappa, gamma, beta, width)


def ln_bwd64(du, x, gamma, width):
    """LayerNorm backward in float64: dL/dx for dL/dy = du (first `width` columns), and the per-row pieces the bound needs.
    Returns dx, dgamma, dbeta, xhat, rstd, kappa."""
    _, xhat, rstd, kappa = ln64(x, gamma, torch.zeros_like(gamma), width)
    xhat = xhat[:, :width]
    du = du.double()[:, :width]
    t = du * gamma.double()[:width]
    a = t.mean(1, keepdim=True)
    b = (t * xhat).mean(1, keepdim=True)
    dx = rstd * (t - a - xhat * b)
    return dx, (du * xhat).sum(0), du.sum(0), xhat, rstd, kappa


def ln_bwd_bound(dacc, du64, xhat, rstd, kappa, gamma):
    """Bound for dx of the LayerNorm backward: the propagated product error dacc (element-wise bound on du) plus the fp32
    evaluation of the statistics and of rstd (t - a - xhat b)."""
    g = gamma.double().abs()[: du64.shape[1]]
    e = dacc * g
    prop = rstd * (e + e.mean(1, keepdim=True) + xhat.abs() * (e * xhat.abs()).mean(1, keepdim=True))
    t = du64.abs() * g
    mag = rstd * (t + t.mean(1, keepdim=True) + (xhat.abs() + 1) * (t * (xhat.abs() + 1)).mean(1, keepdim=True))
    return prop + C_LN * U * (1 + kappa) * mag


def ratio(y, y64, bnd):
    """Worst err / bound of y against y64 (inf if y is not finite where y64 is, or off where the bound is 0)."""
    y = y.double()
    if not torch.isfinite(y).all():
        return math.inf
    err = (y - y64).abs()
    if bool(((bnd <= 0) & (err > 0)).any()):
        return math.inf
    return float((err / bnd.clamp_min(1e-300)).max()) if err.numel() else 0.0


def rms_rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-300))
