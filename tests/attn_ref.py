"""fp64 reference and element-wise error bound for the attention kernels (tests/test_gpu_attn.py, tests/test_attn_bound_cpu.py).

A plain module, not a conftest: the GPU tests and the CPU test of the bound import the same functions.

Every stage is evaluated in float64 on exactly the operands the kernel takes at that stage: its own saved bf16 u / q|k|v / o,
bf16-rounded weights, and (fused backward) the product dx1b Wp whose bf16 rounding the kernel forms inside, carried as an
input error `eta`.  The backward recomputes P from the lse the forward stored, so the reference does too: P = 2^(s - lse).

What the kernels round (attn.hip attn16_* / blk128_*, attn_wide.hip blk256_*), and the term of the bound it gives:
  * scores: one K = 16 bf16 MFMA per pair (exact products, fp32 sums), times hd^-1/2 log2(e) in fp32, minus the row max
    (forward) or the stored lse (backward, one fma): a score error ds = C_S 2^-24 (|q| |k|^T) sc + 2^-24 (|s| + |s - m|);
  * hardware exp2 (v_exp_f32): each unnormalised probability e_ij carries a relative error
    eps_ij = ln2 ds_ij + C_EXP 2^-24; in o = sum_j e_ij v_j / sum_j e_ij it adds (P eps) |V| + rowsum(P eps) |o|;
  * e_ij rounded to bf16 as the B operand of P V (the sum in the denominator is not): 2^-8 (P |V|);
  * the fp32 P V accumulation over the keys: C_PV sqrt(keys) 2^-24 (P |V|), and the bf16 output: 2^-8 |o|;
  * lse = m + log2(sum e) with hardware log2: (rowsum(P eps) + keys 2^-24) / ln2 + C_EXP 2^-24 (1 + |lse - m|) + 2 2^-24 |lse|;
  * backward: dP = dO v^T (K = 16 MFMA): C_S 2^-24 |dO| |V|^T (+ |eta| |V|^T); delta = sum_j P dP (inside the core, every fused
    kernel and attn16_bwd up to 64 tokens) or rowsum(dO o) from the saved bf16 o (attn16_bwd past 64 tokens); dS = P (dP - delta)
    and P both rounded to bf16 as MFMA operands: the dS error is (2^-8 + eps + 2 2^-24) |dS| + P (e_dP + e_delta);
    dq = hd^-1/2 dS K -> 2^-8 |dq| + hd^-1/2 (e_dS |K| + C_PV sqrt(keys) 2^-24 |dS| |K|), dk likewise with Q,
    dv = bf16(P)^T dO -> 2^-8 |dv| + ((2^-8 + eps) P)^T |dO| + P^T |eta| + C_PV sqrt(queries) 2^-24 P^T |dO|.
Underflow of exp2 / bf16 below 2^-126 is covered by an absolute floor of 2^-100.  The tests print the worst err / bound per
instantiation ("RATIO ..."); a bound far above the worst error seen would not catch a subtly wrong kernel.
"""
import math

import torch

from gemm_ref import C2, C_LN, U, UB, acc_bound, bf, ln_bwd64, ln_bwd_bound, ln64, ln_out_bound, prod64  # noqa: F401

LN2 = math.log(2.0)
C_S = 4.0        # score / dP accumulation (16 exact products, fp32 sums), in 2^-24 of sum |q||k|
C_EXP = 4.0      # v_exp_f32 / v_log_f32: relative (exp2) / absolute (log2) error, in 2^-24
C_PV = 2.0       # fp32 accumulation of P V, dS K, dS^T Q, P^T dO and of delta, in sqrt(terms) 2^-24
FLOOR = 2.0 ** -100


def classes(Ts, mode, len_l, device="cpu"):
    i = torch.arange(Ts, device=device)
    return i // len_l if mode == 1 else i % len_l if mode == 2 else torch.zeros_like(i)


def allow_mask(Ts, mode, len_l, device="cpu", cls=None):
    c = classes(Ts, mode, len_l, device) if cls is None else cls.to(device)
    return c[:, None] == c[None, :]


def heads_of(t, Ts, heads, hd, off=0):
    """Rows [n * Ts, >= off + heads * hd] -> [n, heads, Ts, hd] float64 (columns off .. of every row)."""
    n = t.shape[0] // Ts
    return t[:, off:off + heads * hd].double().reshape(n, Ts, heads, hd).permute(0, 2, 1, 3)


def rows_of(x):
    """[n, heads, Ts, c] -> [n * Ts, heads * c]."""
    n, h, T, c = x.shape
    return x.permute(0, 2, 1, 3).reshape(n * T, h * c)


def qkv_heads(qkv, d, heads, Ts, kv_off=0):
    hd = d // heads
    kvo = kv_off or d
    return [heads_of(qkv, Ts, heads, hd, i * kvo) for i in range(3)]


def sc_log2(hd):
    return hd ** -0.5 / LN2


def attn_fwd64(qkv, d, heads, Ts, mode, len_l, kv_off=0, cls=None):
    """Forward of the masked attention from the q|k|v the kernel read.  Returns dict: o [rows, d], bo (its bound), lse
    [rows, heads] (log2 units), blse, P [n, heads, Ts, Ts] (for the backward's use of the same operands)."""
    hd = d // heads
    q, k, v = qkv_heads(qkv, d, heads, Ts, kv_off)
    allow = allow_mask(Ts, mode, len_l, qkv.device, cls)
    sc = sc_log2(hd)
    s = (q @ k.transpose(-1, -2)) * sc
    sa = (q.abs() @ k.abs().transpose(-1, -2)) * sc
    sm = s.masked_fill(~allow, -math.inf)
    m = sm.amax(-1, keepdim=True)
    lse = m + torch.log2(torch.exp2(sm - m).sum(-1, keepdim=True))
    P = torch.exp2(sm - lse)
    o = P @ v
    va = v.abs()
    pv = P @ va
    eps = LN2 * (C_S * U * sa + U * s.abs() + U * (s - m).abs()) + C_EXP * U
    Pe = P * eps
    nk = allow.sum(-1, keepdim=True).double()
    bo = (UB * o.abs() + UB * pv + Pe @ va + Pe.sum(-1, keepdim=True) * o.abs() + C_PV * nk.sqrt() * U * pv
          + 2 * U * o.abs() + FLOOR)
    blse = ((Pe.sum(-1, keepdim=True) + nk * U) / LN2 + C_EXP * U * (1 + (lse - m).abs()) + 2 * U * lse.abs())
    return dict(o=rows_of(o), bo=rows_of(bo), lse=rows_of(lse), blse=rows_of(blse), P=P)


def attn_bwd64(qkv, dout, lse, d, heads, Ts, mode, len_l, kv_off=0, pdp=True, o=None, eta=None, cls=None):
    """Backward from the operands the kernel read: q|k|v, dO (bf16 values; or the fp64 product with its error eta [rows, d]),
    the stored lse [rows, heads] and, for the rowsum(dO o) form (pdp=False), the saved bf16 o.  Returns dict of dq, dk, dv
    [rows, d] and their bounds bdq, bdk, bdv."""
    hd = d // heads
    q, k, v = qkv_heads(qkv, d, heads, Ts, kv_off)
    do = heads_of(dout, Ts, heads, hd)
    et = heads_of(eta, Ts, heads, hd) if eta is not None else torch.zeros_like(do)
    n = q.shape[0]
    L = lse.double().reshape(n, Ts, heads).permute(0, 2, 1)[..., None]
    allow = allow_mask(Ts, mode, len_l, qkv.device, cls)
    sc = sc_log2(hd)
    s = (q @ k.transpose(-1, -2)) * sc
    sa = (q.abs() @ k.abs().transpose(-1, -2)) * sc
    P = torch.exp2(s - L).masked_fill(~allow, 0.0)
    eps = (LN2 * (C_S * U * sa + U * s.abs() + U * (s - L).abs()) + C_EXP * U).masked_fill(~allow, 0.0)
    dP = do @ v.transpose(-1, -2)
    edP = C_S * U * (do.abs() @ v.abs().transpose(-1, -2)) + et.abs() @ v.abs().transpose(-1, -2)
    nk = allow.sum(-1, keepdim=True).double()
    if pdp:
        delta = (P * dP).sum(-1, keepdim=True)
        edl = (P * (eps * dP.abs() + edP)).sum(-1, keepdim=True) + C_PV * nk.sqrt() * U * (P * dP.abs()).sum(-1, keepdim=True)
    else:
        oh = heads_of(o, Ts, heads, hd)
        delta = (do * oh).sum(-1, keepdim=True)
        edl = hd * U * (do.abs() * oh.abs()).sum(-1, keepdim=True) + (et.abs() * oh.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    edS = (UB + eps + 2 * U) * dS.abs() + P * (edP + edl)
    scale = hd ** -0.5
    kt = k.abs()
    qa = q.abs()
    nq = allow.sum(0).double()[None, None, :, None]
    dq = scale * (dS @ k)
    bdq = UB * dq.abs() + scale * (edS @ kt + C_PV * nk.sqrt() * U * (dS.abs() @ kt)) + 2 * U * dq.abs() + FLOOR
    dk = scale * (dS.transpose(-1, -2) @ q)
    bdk = (UB * dk.abs() + scale * (edS.transpose(-1, -2) @ qa + C_PV * nq.sqrt() * U * (dS.abs().transpose(-1, -2) @ qa))
           + 2 * U * dk.abs() + FLOOR)
    dv = P.transpose(-1, -2) @ do
    Pt = P.transpose(-1, -2)
    bdv = (UB * dv.abs() + ((UB + eps) * P).transpose(-1, -2) @ do.abs() + Pt @ et.abs() + C_PV * nq.sqrt() * U * (Pt @ do.abs())
           + FLOOR)
    return dict(dq=rows_of(dq), dk=rows_of(dk), dv=rows_of(dv), bdq=rows_of(bdq), bdk=rows_of(bdk), bdv=rows_of(bdv))


def linear64(a, W, b=None):
    """y = a W^T (+ b) in float64 from the operands as given, and the bound of its fp32 evaluation (not the output rounding)."""
    y, ab = prod64(a, W)
    mag = ab.clone()
    if b is not None:
        y = y + b.double()
        mag = mag + b.double().abs()
    return y, acc_bound(a.shape[1], ab) + C2 * U * mag


def x1_64(x, o, Wp, pb, rs=None):
    """x1 = x + rs * (o Wp^T + pb) from the kernel's bf16 o and the bf16 Wp, with its bound."""
    y, by = linear64(o.float(), bf(Wp), pb)
    r = torch.ones(x.shape[0], 1, dtype=torch.float64, device=x.device) if rs is None else rs.double()[:, None]
    x1 = x.double() + r * y
    return x1, r.abs() * by + C2 * U * (x.double().abs() + (r * y).abs())


def dout64(dx1b, Wp):
    """dO = dx1b Wp in float64 and the error of the kernel's bf16 dO against it (fp32 sums, one bf16 rounding)."""
    dO, ab = prod64(dx1b.float(), bf(Wp).t())
    return dO, UB * dO.abs() + (1 + UB) * acc_bound(dx1b.shape[1], ab)


def ln1_bwd64(dqkv, Wqkv, x, gamma, dres):
    """du = dq|dk|dv Wqkv (from the kernel's bf16 dqkv), then the LayerNorm-1 backward plus the residual gradient dres.
    Returns dx, bdx, dgamma, bdgamma, dbeta, bdbeta."""
    d = x.shape[1]
    du, ab = prod64(dqkv.float(), bf(Wqkv).t())
    acc = acc_bound(dqkv.shape[1], ab)
    dxl, dg, db, xhat, rstd, kappa = ln_bwd64(du, x, gamma, d)
    bnd = ln_bwd_bound(acc, du, xhat, rstd, kappa, gamma) + C2 * U * (dres.double().abs() + dxl.abs())
    M = x.shape[0]
    e_xh = C_LN * U * (1 + kappa) * (xhat.abs() + 1)
    # fp32 sums over the rows (a thread's rows in sequence, a 16 / 32-lane tree, one commit per workgroup; fixed point: 2^-44 per
    # commit), and the rows' own errors (independent from row to row): the smaller of the deterministic and the probabilistic
    # form of the sum over the rows (the deterministic one was 40x above the worst error seen at M = 14000)
    def rows_sum(t):
        return torch.minimum(t.sum(0), 4 * t.pow(2).sum(0).sqrt() + t.amax(0))
    depth = 12 + math.sqrt(M)
    fx = 2.0 ** -44 * (12 + M / 32)
    bg = rows_sum(acc * xhat.abs() + du.abs() * e_xh) + depth * U * (du * xhat).abs().sum(0) + fx
    bb = rows_sum(acc) + depth * U * du.abs().sum(0) + fx
    return dres.double() + dxl, bnd, dg, bg, db, bb


def ratio(y, y64, bnd):
    """Worst err / bound of y against y64 (inf if y is not finite where y64 is, or off where the bound is 0)."""
    y = y.double()
    if not torch.isfinite(y).all():
        return math.inf
    err = (y - y64).abs()
    if bool(((bnd <= 0) & (err > 0)).any()):
        return math.inf
    return float((err / bnd.clamp_min(1e-300)).max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------ kernel emulation (CPU test)
def emu_fwd(qkv, d, heads, Ts, mode, len_l, kv_off=0, cls=None, drop_tile=False):
    """What the forward kernels compute, in fp32 with their bf16 roundings: (o bf16 values [rows, d], lse [rows, heads]).
    drop_tile: the last key tile (keys >= 16 (nt - 1)) left out."""
    hd = d // heads
    q, k, v = (t.float() for t in qkv_heads(qkv, d, heads, Ts, kv_off))
    allow = allow_mask(Ts, mode, len_l, qkv.device, cls)
    if drop_tile:
        allow = allow.clone()
        allow[:, 16 * ((Ts - 1) // 16):] = False
    sc = torch.tensor(hd ** -0.5, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    s = ((q @ k.transpose(-1, -2)) * sc).masked_fill(~allow, -math.inf)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp2(s - m)
    lsum = e.sum(-1, keepdim=True)
    o = bf((bf(e) @ v) * (1.0 / lsum))
    lse = m + torch.log2(lsum)
    return rows_of(o), rows_of(lse)


def emu_bwd(qkv, dout, lse, d, heads, Ts, mode, len_l, kv_off=0, pdp=True, o=None, delta_shift=0):
    """What the backward kernels compute, fp32 with bf16 P / dS operands and outputs: (dq, dk, dv) [rows, d].
    delta_shift: delta taken from the row that many queries further on (a planted fault)."""
    hd = d // heads
    q, k, v = (t.float() for t in qkv_heads(qkv, d, heads, Ts, kv_off))
    do = heads_of(dout, Ts, heads, hd).float()
    n = q.shape[0]
    L = lse.float().reshape(n, Ts, heads).permute(0, 2, 1)[..., None]
    allow = allow_mask(Ts, mode, len_l, qkv.device)
    sc = torch.tensor(hd ** -0.5, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    P = torch.exp2((q @ k.transpose(-1, -2)) * sc - L).masked_fill(~allow, 0.0)
    dP = do @ v.transpose(-1, -2)
    if pdp:
        delta = (P * dP).sum(-1, keepdim=True)
    else:
        delta = (do * heads_of(o, Ts, heads, hd).float()).sum(-1, keepdim=True)
    if delta_shift:
        delta = torch.roll(delta, -delta_shift, dims=2)
    dS = bf(P * (dP - delta))
    scale = hd ** -0.5
    dq = bf(scale * (dS @ k))
    dk = bf(scale * (dS.transpose(-1, -2) @ q))
    dv = bf(bf(P).transpose(-1, -2) @ do)
    return rows_of(dq), rows_of(dk), rows_of(dv)
