"""fp64 reference, element-wise error bounds, launch rule and fp32 emulation of the fused MLP half (csrc/fused_enc.hip:
hsimae_enc_mlp_fwd / hsimae_enc_mlp_bwd; tests/test_gpu_mlp.py, tests/test_mlp_bound_cpu.py).

A plain module, not a conftest: the GPU tests and the CPU test of the bounds import the same functions.

What the kernels compute (W1 | W3 [hidden, D], W2 [D, hidden], all multiplied as bf16; HP = hidden rounded up to 32):

    u2  = bf16(LN2(x1))                                      LayerNorm in fp32, one bf16 rounding
    h1  = u2 W1^T + b1,  h3 = u2 W3^T + b3                   K = D, fp32 accumulation that starts from the bias
    g   = bf16(silu(h1) * h3)                                one bf16 rounding; columns [hidden, HP) are exact zeros
    x2  = fma(b2 + g W2^T, rs, x1) (+ res2)                  K = HP, one fused multiply-add, then a second fp32 add
    dyb = bf16(dy * rs_mlp)                                  fp32 product, one bf16 rounding
    dg  = dyb W2                                             K = D
    dh1 = bf16(dg * h3 * s * (1 + h1 (1 - s))),  dh3 = bf16(dg * h1 * s),  s = sigmoid(h1)
    du2 = dh1 W1 + dh3 W3                                    from the bf16 values, one accumulator: K = 2 HP
    dx1 = dy + LNbwd(du2)                                    the unscaled dy
    dx1b = bf16(dx1 * rs_attn)
    g_n2w += sum_rows du2 * xhat,  g_n2b += sum_rows du2     rows below M only, float atomics: any order

Every stage is evaluated in float64 on exactly the operands the kernel takes at that stage, and each rounding has its term:

  * a product of K bf16 pairs accumulated in fp32: acc_bound(K, |A| |W|^T) (gemm_ref.py: C1 sqrt(K / 32) 2^-24);
  * the fp32 adds of an epilogue (bias, residual, output): C2 2^-24 times the magnitudes added;
  * a bf16 rounding of a result v: UB |v| = 2^-8 |v|;
  * __expf and v_rcp_f32 in silu and its derivative factors: EPS_FN = 2^-18 relative (gemm_ref.EPS_FN, as the SiLU epilogues of
    hsimae_gemm), plus TINY = 2^-100 absolute: below a = -88.7 the fp32 exponential overflows, sigmoid comes out 0 and the
    kernel's -0 stands for a value of a e^a < 2^-120 in magnitude (the figure tests/test_mlp_bound_cpu.py holds silu_nr to);
  * the fp32 LayerNorm statistics: ln_stat_bound / ln_out_bound / ln_bwd_bound of gemm_ref.py.

Backward (`bwd_ratios`).  The kernel emits the operand of every later stage (u2, dyb, g, dh1 | dh3, dx1), so each stage is held
against float64 evaluated on the EMITTED operands of the stage before, and no rounding has to be carried across stages:

    u2            ln64(x1)                       ln_out_bound
    dyb           bf16(dy * rs_mlp)              bit equality
    dx1b          bf16(dx1_kernel * rs_attn)     bit equality
    g             h = u2_k W^T + b, the gate     UB |g| + (1 + UB)(|dg/dh1| e_h1 + |dg/dh3| e_h3 + EPS_FN |g| + second order) + TINY,
                                                 e_h = acc_bound(D, |u2_k| |W|^T) + C2 U (|h| + |b|)
    dh1, dh3      dg = dyb_k W2, times D(h)      (1 + UB)(e_dg |D| + |dg| (|dD/dh1| e_h1 + |dD/dh3| e_h3) + 4 EPS_FN |dg| mag) + UB |ref| + TINY,
                                                 e_dg = acc_bound(D, |dyb_k| |W2|): the E_SWIGLU_BWD form of tests/test_gpu_gemm.py plus
                                                 the dependence of the derivative factor D on the error of the recomputed h1, h3
    dx1           dy + LNbwd(dh1_k W1 + dh3_k W3)   ln_bwd_bound(dacc, ...) + C2 U (|dy| + |dx1|), dacc = acc_bound(2 HP, |dh1_k||W1| + |dh3_k||W3|)
    g_n2w         g0 + sum du2 xhat              sum(dacc |xhat| + |du2| e_xhat) + n U (sum|du2 xhat| + |g0|),
                                                 e_xhat = C_LN U (1 + kappa)(|xhat| + 1); the last term is the any-order form
                                                 wgrad_ref.bound_db uses for a summation order it cannot know
    g_n2b         g0 + sum du2                   sum dacc + n U (sum|du2| + |g0|)

n = min(M + 2, n2_depth): M + 2 holds for any order of M addends (one rounding per addend, the product's and the commit's);
`n2_depth` counts the roundings an addend can meet in the order the kernel does fix: a thread adds its R LPR / 256 rows in turn
(LPR = D / 8 lanes per row), the 256 / LPR partial sums of a column are added in turn, and each of the ceil(M / R) panels commits
one float atomic, in any order; 2 more for the product and the value the element held.  At M = 1000 that is 42 (D = 128), not 1002.

Rows whose rs_mlp is 0 must come out exactly: dyb = dh1 = dh3 = 0 and dx1 bit-equal to dy (their ratio is inf otherwise); columns
[hidden, HP) of g, dh1, dh3 must be exact zeros.

Forward (`fwd_ref`).  The forward kernel saves no intermediate, and its LayerNorm and SiLU need not round as the backward's do,
so the bf16 operands are not known bit for bit.  The reference operand is bf16(u64), and the kernel's may differ from it by one
bf16 ulp exactly where u64 lies within the fp32 statistics' error e_stat of a rounding midpoint:

    flip(v, e) = the bf16 ulp of v where v is within e of a midpoint, 0 elsewhere; e + ulp where e is not below half an ulp
    eta_u = flip(u64, e_stat),  e_stat = ln_stat_bound
    e_h   = acc_bound(D, |ub| |W|^T) + eta_u |W|^T + C2 U (|h| + |b|)
    e_pre = |dg/dh1| e_h1 + |dg/dh3| e_h3 + EPS_FN |g| + second order + TINY (|h3| + 1)
    eta_g = flip(g64, e_pre)
    |x2 - x2_64| <= |rs| (acc_bound(HP, |gb| |W2|^T) + eta_g |W2|^T) + C2 U (|rs| (|y| + |b2|) + |x1| + |res2| + |x2|)

(A blanket UB |u| in place of flip would be several tens of times the accumulation error and would let a dropped k-step of one
chunk pass.)  float64 -> bf16 goes through fp32 here (`bf64`); a value that the first rounding moves onto a midpoint lies
within 2^-25 of it, inside e_stat / e_pre, so it is flagged by flip either way.

`expected` restates the dispatch of launch_fwd / launch_bwd_t (csrc/fused_enc.hip) and mlp_shape (csrc/plan.h).  The late-store
form has one more condition: planar operands of 4 GB or more (2 * NCH * plane_rows * 128 bytes >= 2^32 - 256) fall back to the
early-store kernel.  No GPU test that runs in seconds reaches it, so it has no case and `expected` does not model it.

`emulate` is an fp32 restatement in torch of the kernels' order (64-column hidden chunks, 32-deep k-steps, the half-full last
chunk at HP = 352, bf16 roundings at the same points, silu with and without the Newton step) with switches for planted faults:
tests/test_mlp_bound_cpu.py holds it inside every bound, and every planted fault outside.
"""
import math

import torch

from gemm_ref import (U, UB, C1, C2, C_LN, EPS_FN, bf, prod64, acc_bound, ln64, ln_out_bound, ln_stat_bound, ln_bwd64,  # noqa: F401
                      ln_bwd_bound, ratio)

TINY = 2.0 ** -100                                        # fp32 underflow of the exponential / of a product (see above)
SHAPES = {128: (352, 48), 256: (704, 48), 64: (192, 64)}  # d -> (HP, rows of a panel)
MODEL_HIDDEN = {128: 344, 256: 684, 64: 172}              # Base, Large, the decoder
RS = [0.0, 1.0, 1.0 / 0.9, 1.0 / 0.7, 1.3]                # DropPath factors: 0, 1 and non-powers of two
LOG2E = 1.4426950408889634


def rup(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ the launch rule
def expected(d, hidden, plane_rows=0, have_dh13=True):
    """(D, HP, R, late) of the kernel a call launches, None where hsimae_enc_mlp_* answers HSIMAE_EUNSUPPORTED.  The forward
    kernel is <D, HP>; `late` names the backward's late-store form (planar operands at D >= 256)."""
    hp = rup(hidden, 32)
    if d not in SHAPES or SHAPES[d][0] != hp:
        return None
    return d, hp, SHAPES[d][1], bool(d >= 256 and have_dh13 and plane_rows > 0)


def fwd_name(e):
    return "enc_mlp_fwd_kernel<%d, %d>" % e[:2]


def bwd_name(e):
    return "enc_mlp_bwd_kernel<%d, %d, %s>" % (e[0], e[1], "true" if e[3] else "false")


INSTANTIATIONS = {fwd_name((d, hp)) for d, (hp, _) in SHAPES.items()} | {bwd_name((d, hp, 0, False)) for d, (hp, _) in SHAPES.items()} | \
    {bwd_name((256, 704, 48, True))}


# ------------------------------------------------------------------------------------------------ cases
class Mlp:
    """Parameters of one MLP half.  W1 | W3 [hidden, d], W2 [d, hidden] in fp32 (what is packed); *b = their bf16 values in fp32."""

    def __init__(self, d, hidden, seed, device="cpu", w1_scale=None):
        self.d, self.hidden = d, hidden
        self.HP, self.R = SHAPES[d]
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)         # noqa: E731
        self.gamma, self.beta = 1 + 0.2 * rn(d), 0.1 * rn(d)
        self.W1, self.W3, self.W2 = rn(hidden, d) * 0.1 + 0.01, rn(hidden, d) * 0.1 - 0.01, rn(d, hidden) * 0.1 + 0.005
        self.b1, self.b3, self.b2 = rn(hidden) * 0.3, rn(hidden) * 0.3, rn(d) * 0.3
        if w1_scale is not None:                              # extremes: some rows of W1 scaled (rows, factor)
            rows, f = w1_scale
            self.W1[rows] = self.W1[rows] * f
        for k in ("gamma", "beta", "W1", "W3", "W2", "b1", "b3", "b2"):
            setattr(self, k, getattr(self, k).to(device))
        self.W1b, self.W3b, self.W2b = bf(self.W1), bf(self.W3), bf(self.W2)


def make_inputs(p, M, seed, device="cpu"):
    """x1, dy, res2 [M, d], row factors [M] from RS (constant over runs of 5 rows, every factor present from M = 21 on) and the
    values g_n2w / g_n2b hold before the call.  Row 1 is constant, row 2 has a large mean (M > 3)."""
    g = torch.Generator().manual_seed(seed)
    d = p.d
    x1 = torch.randn(M, d, generator=g) * 1.5 + 0.3
    if M > 3:
        x1[1] = 0.3
        x1[2] = 40.0 + torch.randn(d, generator=g)
    dy = torch.randn(M, d, generator=g) * 0.1
    res2 = torch.randn(M, d, generator=g)
    idx = torch.arange(M) // 5
    fac = torch.tensor(RS)
    inp = dict(x1=x1, dy=dy, res2=res2, rs=fac[(idx + 1) % 5].clone(), rs_mlp=fac[(idx + 2) % 5].clone(), rs_attn=fac[(idx + 4) % 5].clone(),
               g0w=torch.randn(d, generator=g), g0b=torch.randn(d, generator=g))
    return {k: v.to(device).contiguous() for k, v in inp.items()}


# ------------------------------------------------------------------------------------------------ pieces of the reference
def bf64(v):
    """float64 -> bf16 value in float64 (through fp32: see the module docstring)."""
    return v.float().to(torch.bfloat16).double()


def ulp_bf(v):
    """bf16 ulp of |v| (float64): 2^(floor(log2 |v|) - 7)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -120))        # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 8)


def flip(v, e):
    """Operand error of bf16(v') against bf16(v) for |v' - v| <= e: one ulp where a rounding midpoint lies within e of v (in
    v's binade, or the one just under its lower edge), 0 elsewhere; e + ulp where e is not below half an ulp."""
    a = v.abs().clamp_min(2.0 ** -120)
    ulp = ulp_bf(a)
    q = a / ulp
    dist = ((q - torch.floor(q)) - 0.5).abs() * ulp
    dist = torch.minimum(dist, a - (128 * ulp - ulp / 4))
    out = torch.where(dist <= e, ulp, torch.zeros_like(ulp))
    return torch.where(e >= ulp / 2, e + ulp_bf(a + e), out)


def gate64(h1, h3):
    """g = silu(h1) h3 in float64 with s = sigmoid(h1), dg/dh1 and dg/dh3."""
    s = torch.sigmoid(h1)
    return h1 * s * h3, s, h3 * s * (1 + h1 * (1 - s)), h1 * s


def gate_err(h1, h3, e1, e3):
    """Error of the fp32 gate before its bf16 rounding, for pre-activation errors e1, e3: first order, the second-order terms
    (|d2 silu| <= 1/2, the cross term) and the function error of __expf / v_rcp_f32."""
    g, s, d1, d3 = gate64(h1, h3)
    return d1.abs() * e1 + d3.abs() * e3 + e1 * e3 + 0.5 * h3.abs() * e1 * e1 + EPS_FN * g.abs() + TINY * (h3.abs() + 1)


def hidden64(p, u, eta=None):
    """h1, h3 in float64 from the operand u (fp32 values of bf16) with their error bounds e_h1, e_h3."""
    out = []
    for W, b in ((p.W1b, p.b1), (p.W3b, p.b3)):
        h, ab = prod64(u, W)
        h = h + b.double()
        e = acc_bound(p.d, ab) + C2 * U * (h.abs() + b.double().abs())
        if eta is not None:
            e = e + eta @ W.double().abs().t()
        out += [h, e]
    return out


# ------------------------------------------------------------------------------------------------ forward
def fwd_ref(p, x1, res2=None, rs=None):
    """(x2 in float64, its element-wise bound, the float64 h1) for x1 [M, d], optional res2 [M, d] and row factors rs [M]."""
    xd = x1.double()
    u64, xh, rstd, kappa = ln64(x1, p.gamma, p.beta)
    e_stat = ln_stat_bound(xh, kappa, p.gamma, p.beta)
    h1, e1, h3, e3 = hidden64(p, bf64(u64), flip(u64, e_stat))
    g64 = gate64(h1, h3)[0]
    e_pre = gate_err(h1, h3, e1, e3)
    W2 = p.W2b.double()
    y, ay = prod64(bf64(g64), W2)
    b2 = p.b2.double()
    y = y + b2
    r = rs.double()[:, None] if rs is not None else torch.ones_like(xd[:, :1])
    r2 = res2.double() if res2 is not None else torch.zeros_like(xd)
    x2 = xd + r * y + r2
    bnd = r.abs() * (acc_bound(p.HP, ay) + flip(g64, e_pre) @ W2.abs().t()) + \
        C2 * U * (r.abs() * (y.abs() + b2.abs()) + xd.abs() + r2.abs() + x2.abs())
    return x2, bnd, h1


def exact(a, b):
    """0 where the two tensors hold the same bits, inf elsewhere (a `ratio` for outputs that must be bit-equal)."""
    same = a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                    b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
    return 0.0 if same else math.inf


def fwd_ratio(p, x2, x1, res2=None, rs=None):
    """Worst err / bound of the kernel's x2; inf when a row whose factor is 0 is not bit-equal to x1 (+ res2)."""
    ref, bnd, _ = fwd_ref(p, x1, res2, rs)
    r = ratio(x2, ref, bnd)
    if rs is not None and bool((rs == 0).any()):
        z = rs == 0
        r = max(r, exact(x2[z], (x1 + res2)[z] if res2 is not None else x1[z]))
    return r


# ------------------------------------------------------------------------------------------------ backward
def bwd_ratios(p, inp, out, full=None):
    """Worst err / bound per output of one backward call.  inp: x1, dy [M, d], rs_mlp, rs_attn [M] or None, g0w, g0b [d].
    out: u2, dyb, dx1b [M, d] bf16, g, dh1, dh3 [M, HP] bf16 (row-major), dx1 [M, d], gw, gb [d]; an output the call did not write
    is None and its stage operands are taken from `full`, the outputs of the call that wrote every group on the same data."""
    d, h, HP = p.d, p.hidden, p.HP
    x1, dy = inp["x1"], inp["dy"]
    M = x1.shape[0]
    rsm, rsa = inp.get("rs_mlp"), inp.get("rs_attn")
    src = lambda k: out[k] if out.get(k) is not None else full[k]          # noqa: E731
    r = {}
    zero = rsm == 0 if rsm is not None else torch.zeros(M, dtype=torch.bool, device=x1.device)
    dyb_ref = (dy * rsm[:, None] if rsm is not None else dy).to(torch.bfloat16)
    if out.get("u2") is not None:
        u64, xh, rstd, kappa = ln64(x1, p.gamma, p.beta)
        r["u2"] = ratio(out["u2"], u64, ln_out_bound(u64, xh, kappa, p.gamma, p.beta))
        r["dyb"] = exact(out["dyb"], dyb_ref)
    u2k, dybk = src("u2").float(), src("dyb").float()
    h1, e1, h3, e3 = hidden64(p, u2k)
    g64, s, d1, d3 = gate64(h1, h3)
    pad0 = lambda t: 0.0 if bool((t[:, h:].float() == 0).all()) else math.inf   # noqa: E731  columns [hidden, HP): exact zeros
    if out.get("g") is not None:
        bnd = UB * g64.abs() + (1 + UB) * gate_err(h1, h3, e1, e3) + TINY
        r["g"] = max(ratio(out["g"][:, :h], g64, bnd), pad0(out["g"]))
        dg, adg = prod64(dybk, p.W2b.t())                     # dyb [M, d] @ W2 [d, hidden]
        e_dg = acc_bound(d, adg)
        D1, D3 = d1, d3                                       # d(silu(h1) h3) / dh1 and / dh3 are the two derivative factors
        dD1_h1 = h3.abs() * s * (1 - s) * (2 + h1.abs())
        dD_h3 = (s * (1 + h1 * (1 - s))).abs()                # = |dD1/dh3| = |dD3/dh1|
        mag1 = h3.abs() * s * (1 + h1.abs() * (1 - s))
        for name, o, D, dep, mag in (("dh1", out["dh1"], D1, dD1_h1 * e1 + dD_h3 * e3, mag1), ("dh3", out["dh3"], D3, dD_h3 * e1, D3.abs())):
            ref = dg * D
            bnd = (1 + UB) * (e_dg * D.abs() + dg.abs() * dep + 4 * EPS_FN * dg.abs() * mag) + UB * ref.abs() + TINY
            r[name] = max(ratio(o[:, :h], ref, bnd), pad0(o))
            if bool(zero.any()) and not bool((o[zero].float() == 0).all()):
                r[name] = math.inf
    if bool(zero.any()) and out.get("dyb") is not None and not bool((out["dyb"][zero].float() == 0).all()):
        r["dyb"] = math.inf
    # dx1 and the LayerNorm-2 parameter gradients from the emitted dh1 | dh3
    dh1k, dh3k = src("dh1")[:, :h].double(), src("dh3")[:, :h].double()
    W1, W3 = p.W1b.double(), p.W3b.double()
    du = dh1k @ W1 + dh3k @ W3
    dacc = acc_bound(2 * HP, dh1k.abs() @ W1.abs() + dh3k.abs() @ W3.abs())
    dx64, dgam, dbet, xhat, rstd, kappa = ln_bwd64(du, x1, p.gamma, d)
    ref = dy.double() + dx64
    bnd = ln_bwd_bound(dacc, du, xhat, rstd, kappa, p.gamma) + C2 * U * (dy.double().abs() + ref.abs()) + TINY
    r["dx1"] = ratio(out["dx1"], ref, bnd)
    if bool(zero.any()):
        r["dx1"] = max(r["dx1"], exact(out["dx1"][zero], dy[zero]))
    if out.get("dx1b") is not None:
        r["dx1b"] = exact(out["dx1b"], (out["dx1"] * rsa[:, None] if rsa is not None else out["dx1"]).to(torch.bfloat16))
    e_xh = C_LN * U * (1 + kappa) * (xhat.abs() + 1)
    g0w, g0b = inp["g0w"].double(), inp["g0b"].double()
    n = n2_depth(d, M)
    bw = (dacc * xhat.abs() + du.abs() * e_xh).sum(0) + n * U * ((du * xhat).abs().sum(0) + g0w.abs())
    bb = dacc.sum(0) + n * U * (du.abs().sum(0) + g0b.abs())
    r["g_n2w"] = ratio(out["gw"], g0w + dgam, bw)
    r["g_n2b"] = ratio(out["gb"], g0b + dbet, bb)
    return r


def n2_depth(d, M):
    """Roundings one addend of g_n2w / g_n2b can meet (see the module docstring)."""
    R, lpr = SHAPES[d][1], d // 8
    return min(M + 2, R * lpr // 256 + 256 // lpr + cdiv(M, R) + 2)


# ------------------------------------------------------------------------------------------------ fp32 emulation
FAULTS = ("half_chunk_dropped", "bias_not_zeroed", "rs_on_residual", "res2_before_scale", "dyb_unscaled", "dh_swapped",
          "no_derivative_term", "ln_bwd_no_mean", "n2b_over_pad_rows", "dx1_scaled_dy")


def fma32(a, b, c):
    """fp32 fused multiply-add (the product is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def silu32(a, newton=True, fixed=True):
    """(silu, sigmoid) as the kernels form them in fp32: d = 1 + exp2(-log2(e) a), r = 1 / d, for the forward one Newton step
    r = fma(fma(-d, r, 1), r, r), the residual passed through fmin(., 1) in the fixed formula (common.h silu_nr)."""
    d = 1 + torch.exp2(a * torch.tensor(-LOG2E, dtype=torch.float32, device=a.device))
    r = 1 / d
    if newton:
        res = fma32(-d, r, torch.ones_like(d))
        if fixed:
            res = torch.fmin(res, torch.ones_like(res))
        r = fma32(res, r, r)
    return a * r, r


def _ln32(x, gamma, beta):
    mean = x.sum(1, keepdim=True) * (1.0 / x.shape[1])
    f = x - mean
    rstd = torch.rsqrt((f * f).sum(1, keepdim=True) * (1.0 / x.shape[1]) + 1e-5)
    return f * rstd * gamma + beta, f * rstd, rstd


def emulate(p, inp, res2=True, rowscale=True, newton=True, fixed=True, fault=None):
    """The two kernels in fp32, in their order, on whole panels (rows past M: x1 = dy = 0, as the bounds-checked loads return).
    Returns x2 and the backward's outputs as `bwd_ratios` takes them."""
    assert fault is None or fault in FAULTS
    d, h, HP, R = p.d, p.hidden, p.HP, p.R
    NCH, KSD = cdiv(HP, 64), d // 32
    HC = NCH * 64
    half_last = HP % 64 != 0
    M = inp["x1"].shape[0]
    Mp = cdiv(M, R) * R

    def rows(t, fill=0.0):
        o = torch.full((Mp,) + t.shape[1:], fill, dtype=torch.float32)
        o[:M] = t
        return o

    x1, dy = rows(inp["x1"]), rows(inp["dy"])
    if fault == "n2b_over_pad_rows":
        # a kernel without the row guard: the panel's rows past M are fetched from whatever follows in the buffers and summed.
        # (Rows that read as zeros would not show: dy = 0 gives dyb = dg = dh1 = dh3 = du2 = 0 whatever u2 is.)
        gen = torch.Generator().manual_seed(M)
        x1[M:], dy[M:] = torch.randn(Mp - M, d, generator=gen), 0.1 * torch.randn(Mp - M, d, generator=gen)
    r2 = rows(inp["res2"]) if res2 else None
    rs = rows(inp["rs"], 1.0)[:, None] if rowscale else torch.ones(Mp, 1)
    rsm = rows(inp["rs_mlp"], 1.0)[:, None] if rowscale else torch.ones(Mp, 1)
    rsa = rows(inp["rs_attn"], 1.0)[:, None] if rowscale else torch.ones(Mp, 1)

    def padded(W, n0, n1):
        o = torch.zeros(n0, n1)
        o[:W.shape[0], :W.shape[1]] = W
        return o

    W1, W3, W2 = padded(p.W1b, HC, d), padded(p.W3b, HC, d), padded(p.W2b, d, HC)
    b1, b3 = torch.zeros(HC), torch.zeros(HC)
    b1[:h], b3[:h] = p.b1, p.b3
    if fault == "bias_not_zeroed":
        b1[h:HP], b3[h:HP] = 0.37, -0.21
    u2 = bf(_ln32(x1, p.gamma, p.beta)[0])

    def pre(c):
        cols = slice(64 * c, 64 * c + 64)
        a1, a3 = b1[cols].expand(Mp, 64).clone(), b3[cols].expand(Mp, 64).clone()
        for ks in range(KSD):
            k = slice(32 * ks, 32 * ks + 32)
            a1 = a1 + u2[:, k] @ W1[cols, k].t()
            a3 = a3 + u2[:, k] @ W3[cols, k].t()
        return cols, a1, a3

    def ksteps(c):
        if half_last and c == NCH - 1:
            return [] if fault == "half_chunk_dropped" else [0]
        return [0, 1]

    # forward
    xr = p.b2.expand(Mp, d).clone()
    for c in range(NCH):
        cols, a1, a3 = pre(c)
        gc = bf(silu32(a1, newton, fixed)[0] * a3)
        for ks in ksteps(c):
            xr = xr + gc[:, 32 * ks:32 * ks + 32] @ W2[:, 64 * c + 32 * ks:64 * c + 32 * ks + 32].t()
    if fault == "rs_on_residual":
        x2 = (xr + x1) * rs
    elif fault == "res2_before_scale":
        x2 = fma32(xr + (r2 if r2 is not None else 0.0), rs, x1)
    else:
        x2 = fma32(xr, rs, x1)
    if r2 is not None and fault != "res2_before_scale":
        x2 = x2 + r2

    # backward
    dyb = bf(dy * rsm)
    dyb_used = bf(dy) if fault == "dyb_unscaled" else dyb
    g, dh1, dh3 = torch.zeros(Mp, HC), torch.zeros(Mp, HC), torch.zeros(Mp, HC)
    du = torch.zeros(Mp, d)
    for c in range(NCH):
        cols, a1, a3 = pre(c)
        dg = torch.zeros(Mp, 64)
        for ks in range(KSD):
            k = slice(32 * ks, 32 * ks + 32)
            dg = dg + dyb_used[:, k] @ W2[k, cols]
        sl, sg = silu32(a1, newton=False)
        g[:, cols] = bf(sl * a3)
        dh1[:, cols] = bf(dg * a3 * sg if fault == "no_derivative_term" else dg * a3 * sg * (1 + a1 * (1 - sg)))
        dh3[:, cols] = bf(dg * sl)
        for ks in ksteps(c):
            k = slice(64 * c + 32 * ks, 64 * c + 32 * ks + 32)
            p1, p3 = (dh3, dh1) if fault == "dh_swapped" else (dh1, dh3)
            du = du + p1[:, k] @ W1[k]
            du = du + p3[:, k] @ W3[k]
    _, xh, rstd = _ln32(x1, p.gamma, p.beta)
    t = du * p.gamma
    a = t.sum(1, keepdim=True) * (1.0 / d)
    b = (t * xh).sum(1, keepdim=True) * (1.0 / d)
    if fault == "ln_bwd_no_mean":
        a = torch.zeros_like(a)
    dx1 = (dy * rsm if fault == "dx1_scaled_dy" else dy) + rstd * (t - a - xh * b)
    nb = Mp if fault == "n2b_over_pad_rows" else M
    out = dict(x2=x2[:M], u2=u2[:M].to(torch.bfloat16), dyb=dyb[:M].to(torch.bfloat16), g=g[:M, :HP].to(torch.bfloat16),
               dh1=dh1[:M, :HP].to(torch.bfloat16), dh3=dh3[:M, :HP].to(torch.bfloat16), dx1=dx1[:M],
               dx1b=(dx1 * rsa)[:M].to(torch.bfloat16), gw=inp["g0w"] + (du * xh)[:M].sum(0), gb=inp["g0b"] + du[:nb].sum(0))
    if not rowscale:
        out["dx1b"] = dx1[:M].to(torch.bfloat16)
    return out
