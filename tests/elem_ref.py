"""fp64 restatements and element-wise error bounds for csrc/elem.hip (tests/test_gpu_elem.py, tests/test_elem_bound_cpu.py):
masking, patch gather, LayerNorm forward / backward, decoder sequence assembly, the loss with its reconstruction images,
AdamW, and the fine-tuning head's pooling and backward.

A plain module, not a conftest.  Every restatement is written from the operation's formula (the kernel comments and
oracle/hsimae_oracle.py) in float64; nothing is transcribed from a kernel.  An output y is accepted element by element when

    |y - y64| <= fixed + C * 2^-24 * term

`fixed` is what the output format alone costs (2^-8 |y64| for a bf16 output, 0 for fp32), `term` the sum of the magnitudes that
enter the element (given below per operation), C one constant per output family.  The constants are not derived: each is the
worst (|err| - fixed) / (2^-24 term) measured on an MI355X over the whole matrix of tests/test_gpu_elem.py (`Out.need`, which
the GPU tests print as "asks C"), rounded up to the next power of two (profiles/EXPERIMENTS.md has the table).  tests/test_elem_bound_cpu.py keeps them honest: with them every
fp32 emulation passes and every planted fault fails.  Exact outputs (masking, mask_img, patch gather, the kept rows of the
assembly forward, every padding or frame region) carry fixed = term = 0: any difference is infinitely bad.
"""
import math

import numpy as np
import torch

import gemm_ref as GR
from gemm_ref import U, UB, bf, ln64  # noqa: F401  (re-exported: both test files take them from here)

# Measured on one MI355X (worst ask over every case of tests/test_gpu_elem.py that uses the constant; per-branch table in
# profiles/EXPERIMENTS.md), rounded up to the next power of two.
# LayerNorm forward: term = (1 + kappa) |gamma| (|xhat| + 1) + |beta| + |y|, kappa = rstd * mean|x| (gemm_ref.ln64).
C_LNF = 2.0       # measured worst 1.73 (d = 40); 0.73 .. 1.49 at the other widths
# LayerNorm backward dx: term = (1 + kappa) * mag of gemm_ref.ln_bwd_bound + |dres| + |previous dx| + |dx|.
C_LNB = 1.0       # measured worst 0.84 (d = 72); 0.65 .. 0.79 at the other widths, 0.51 .. 0.56 in deterministic mode
# dgamma / dbeta, sums over M rows: term = sqrt(M) sum |du xhat| + sum |du| (1 + kappa) (|xhat| + 1) (+ what was there), and
# sqrt(M) sum |du|.  In deterministic mode each workgroup's addend is also rounded to 2^-44: + workgroups * 2^-45, absolute.
C_LNG = 0.5       # measured worst 0.399 (dbeta, d = 512), dgamma 0.238 (d = 264)
# Assembly forward, masked rows (mean token + pos): term = sqrt(K) mean_k |y| + |mean| + |pos| + |out|.
C_ASF = 1.0       # measured worst 0.887 (fast16, K = 14); 0.46 .. 0.75 on the other kernels
# Assembly backward (bf16): term = sqrt(TL - K) sum_masked |dyfull| / K + |mean gradient| + |dyfull| + |dy|.
# Not measurable: on every case the whole error stayed inside the bf16 rounding 2^-8 |dy| (ask 0).  The fp32 part is the same
# sequence as the forward's masked rows (a column sum, a scaling by 1 / K, one addition), so it takes the forward's constant.
C_ASB = C_ASF
# Loss.  Under norm_pix the target (t - mean) / std carries the fp32 rounding of the mean, amplified by A = mean|t| / std
# (std >= 1e-3: a flat patch has A ~ 1000 |t|): dt = A + |target|.  dpred: term = 2 mask inv_scale (dt + |diff|).
C_DP = 2.0        # measured worst 1.42 (row form, T = 30), 1.28 (per-sample form, T = 29); without norm_pix the bf16 rounding hides it (ask 0)
# pred_img = pred * std + mean (std and mean themselves are accurate to a few U, relative): term = |pred| std + |mean| + |out|.
C_PI = 2.0        # measured worst 1.59 (per-sample form, T = 29), 1.52 (row form)
# Row losses mask * mean(diff^2): rterm = mask * 2 mean(|diff| (dt + |diff|)) + rowloss.  A partial sum (few rows, the worst
# case is within reach): term = sum rterm + sqrt(chain) sum rowloss, chain = the fp32 additions behind one partial (loss_chain).
# The scalar adds hundreds of independent row errors in double: (sqrt(sum rterm^2) + sqrt(chain) sum rowloss) / sum_mask + |loss|.
C_LOSS = 2.0      # measured worst 1.22 (partial, row form), 1.12 (loss and partial, per-sample form at T = 1)
# AdamW, every rounding counted: m: 2 |g - m| (1 - b1) + |m'|;  v: |v| b2 + 2 g^2 (1 - b2) + |v'|;
# p: 2 |p decayed| + |p'| + lr inv_bc1 / denom * (term of m + 8 |m'|)  (denom: root, scaling, + eps and v's own error: < 5 U).
C_ADAM = 1.0      # measured worst 0.99 (v), 0.87 (m), 0.70 (p), the same at steps 1, 2, 3 and 1000
# AGG pooling: term = sqrt(L) mean_l |latent| + |pooled|.
C_POOL = 2.0      # measured worst 1.05 (33 x 16 x 6 x 9 x 128); 0.39 .. 0.73 on the other shapes, 0 at L = 1
# Head backward: gw: sqrt(N) sum_n |g| |pooled|;  gb: sqrt(N) sum_n |g|;  dlatent: (sqrt(C) sum_j |g| |w|) / L + |dlatent|.
C_HEAD = 1.0      # measured worst 0.88 (gw at N = 1: one product, one rounding), gb 0.70, dlatent 0.76

F32_1E6 = float(np.float32(1e-6))
LOSS_ROWS_PER_WG = 32            # csrc/plan.h
DET_SCALE = 2.0 ** 44            # csrc/common.h HS_DET_SCALE


class Out:
    """One output's reference: ref (fp64), fixed and term (broadcastable to ref), and the name of its constant."""

    def __init__(self, ref, cname=None, term=0.0, fixed=0.0):
        self.ref = torch.as_tensor(ref, dtype=torch.float64)
        self.term = torch.as_tensor(term, dtype=torch.float64).expand_as(self.ref) if cname else torch.zeros_like(self.ref)
        self.fixed = torch.as_tensor(fixed, dtype=torch.float64).expand_as(self.ref)
        self.cname = cname

    def bound(self):
        c = globals()[self.cname] if self.cname else 0.0
        return self.fixed + c * U * self.term

    def _err(self, got):
        got = torch.as_tensor(got).double().reshape(self.ref.shape)
        if not bool(torch.isfinite(got).all()):
            return None
        return (got - self.ref).abs()

    def ratio(self, got):
        """Worst |got - ref| / bound (inf: not finite, or off where the bound is 0)."""
        err = self._err(got)
        if err is None:
            return math.inf
        if err.numel() == 0:
            return 0.0
        b = self.bound()
        if bool(((b <= 0) & (err > 0)).any()):
            return math.inf
        return float(torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err)).max())

    def need(self, got):
        """The constant this result asks for: worst (|got - ref| - fixed) / (U term)."""
        err = self._err(got)
        if err is None:
            return math.inf
        if err.numel() == 0:
            return 0.0
        ex = (err - self.fixed).clamp_min(0.0)
        if bool(((self.term <= 0) & (ex > 0)).any()):
            return math.inf
        return float(torch.where(ex > 0, ex / (U * self.term).clamp_min(1e-300), torch.zeros_like(ex)).max())


def bf16_out(ref, cname, term):
    return Out(ref, cname, (1 + UB) * term, UB * ref.abs())


# ------------------------------------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def skew(shape, g, off=0.5, scale=1.0):
    """Asymmetric data with a mean offset: off + scale * (3 r^2 - 0.5), r uniform: mean off + scale / 2, skewed to the right."""
    return (off + scale * (3.0 * torch.rand(shape, generator=g) ** 2 - 0.5)).float()


def rup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_tpr(d):
    return 8 if d <= 64 else 16 if d <= 128 else 32 if d <= 256 else 64      # hs_ln_bwd's dispatch


def ln_rows_per_wg(d):
    return (256 // ln_tpr(d)) * 8


LN_BWD_D = [8, 64, 72, 128, 144, 256, 264, 512]      # both ends and the inside of each TPR class (72, 144, 264: idle lanes)
LN_FWD_D = [8, 40, 64, 72, 200, 512]
LN_FWD_M = [1, 3, 4, 5, 257]


def ln_bwd_cases(d):
    """(ld, M, accumulate, dres, dgdb) for width d: ld in {0, rup(d, 32), d + 8} x M around one workgroup's rows, the three
    flags running through all eight combinations."""
    rp = ln_rows_per_wg(d)
    out, i = [], LN_BWD_D.index(d)
    for ld in (0, rup(d, 32), d + 8):
        for M in (1, rp - 1, rp, rp + 1, 3 * rp + 5):
            out.append((ld, M, i & 1, (i >> 1) & 1, (i >> 2) & 1))
            i += 1
    return out


def ln_inputs(M, d, seed):
    """x with a row offset (kappa well above 1 on some rows), gamma around 1, skewed du with a zero row, dres, previous dx,
    and what dgamma / dbeta hold before the call."""
    g = gen(seed)
    x = skew((M, d), g, 0.5, 2.0) + 3.0 * torch.rand((M, 1), generator=g)
    gamma = skew((d,), g, 1.0, 0.2)
    beta = skew((d,), g, -0.3, 0.5)
    du = skew((M, d), g, 0.25, 1.0)
    du[M // 2] = 0.0
    dres = skew((M, d), g, -0.5, 1.0)
    prev = skew((M, d), g, 0.3, 2.0)
    g0, b0 = skew((d,), g, 0.4, 1.0), skew((d,), g, -0.2, 1.0)
    return dict(x=x, gamma=gamma, beta=beta, du=du, dres=dres, prev=prev, g0=g0, b0=b0)


def ln_fwd_ref(x, gamma, beta):
    y, xhat, _, kappa = ln64(x, gamma, beta)
    term = (1 + kappa) * gamma.double().abs() * (xhat.abs() + 1) + beta.double().abs() + y.abs()
    return {"out": Out(y, "C_LNF", term)}


def ln_bwd_ref(du, x, gamma, dres=None, prev=None, g0=None, b0=None, workgroups=0):
    """dx = dres + prev + rstd (g du - mean(g du) - xhat mean(g du xhat));  dgamma = g0 + sum_r du xhat;  dbeta = b0 + sum_r du.
    workgroups > 0: deterministic mode, each workgroup's column sum is rounded to a multiple of 2^-44."""
    M, d = x.shape
    dx0, dg, db, xhat, rstd, kappa = GR.ln_bwd64(du, x, gamma, d)
    du64 = du.double()
    stat = GR.ln_bwd_bound(torch.zeros_like(dx0), du64, xhat, rstd, kappa, gamma) / (GR.C_LN * U)
    dx, term = dx0.clone(), stat.clone()
    for a in (dres, prev):
        if a is not None:
            dx = dx + a.double()
            term = term + a.double().abs()
    if dres is not None or prev is not None:
        term = term + dx.abs()
    z = torch.zeros(d, dtype=torch.float64)
    g0 = z if g0 is None else g0.double()
    b0 = z if b0 is None else b0.double()
    q = workgroups * 0.5 / DET_SCALE
    tg = math.sqrt(M) * (du64 * xhat).abs().sum(0) + (du64.abs() * (1 + kappa) * (xhat.abs() + 1)).sum(0) + g0.abs() + (g0 + dg).abs()
    tb = math.sqrt(M) * du64.abs().sum(0) + b0.abs() + (b0 + db).abs()
    return {"dx": Out(dx, "C_LNB", term), "dgamma": Out(g0 + dg, "C_LNG", tg, q), "dbeta": Out(b0 + db, "C_LNG", tb, q)}


# ------------------------------------------------------------------------------------------------ assembly
# (kernel, Dd, ld, T, len_t, len_l): hs_assemble_* takes the float4 kernels for Dd = 64 / 32 stored densely with TL <= 512, the
# generic pair otherwise.  TL = 9 T: 504 is the last fast size on the 9-grid, 513 the first generic one.
ASSEMBLE_CONFIGS = [
    ("fast16", 64, 0, 6, 2, 7), ("fast16", 64, 64, 6, 2, 7), ("fast8", 32, 0, 6, 2, 7), ("fast8", 32, 32, 4, 3, 2),
    ("generic", 48, 64, 6, 2, 7), ("generic", 64, 96, 6, 2, 7), ("generic", 128, 0, 4, 2, 5), ("generic", 512, 0, 2, 1, 4),
    ("fast16", 64, 0, 56, 5, 3), ("generic", 64, 0, 57, 5, 3),
]


def assemble_kernel(Dd, ld, TL):
    """Which kernel pair the launcher takes (restated from hs_assemble_fwd / _bwd)."""
    if TL <= 512 and Dd == 64 and ld in (0, 64):
        return "fast16"
    if TL <= 512 and Dd == 32 and ld in (0, 32):
        return "fast8"
    return "generic"


def assemble_cases():
    """(kernel, Dd, ld, T, len_t, len_l, N): every configuration at K = 1, K = len_t * len_l and K = TL, N alternating 1 / 5."""
    out = []
    for i, (kern, Dd, ld, T, lt, ll) in enumerate(ASSEMBLE_CONFIGS):
        for j, (a, b) in enumerate(((1, 1), (lt, ll), (T, 9))):
            out.append((kern, Dd, ld, T, a, b, 1 if (i + j) % 2 else 5))
    return out


def assemble_inputs(N, T, lt, ll, Dd, seed):
    from oracle import hsimae_oracle as O
    g = gen(seed)
    n1, n2 = torch.rand(N, T, generator=g), torch.rand(N, 9, generator=g)
    _, rest, _ = O.mask_from_noise(n1.numpy(), n2.numpy(), lt, ll)
    K, TL = lt * ll, T * 9
    return dict(rest=torch.from_numpy(rest), y=skew((N, K, Dd), g, 0.5, 1.0), pos=skew((TL, Dd), g, -0.25, 1.0),
                dyf=skew((N, TL, Dd), g, 0.5, 1.0), K=K, TL=TL)


def assemble_fwd_ref(y, pos, rest, K):
    """yfull[n, i] = (rest[n, i] < K ? y[n, rest[n, i]] : mean_k y[n, k]) + pos[i].  Kept rows are one fp32 addition: exact."""
    N, _, Dd = y.shape
    TL = rest.shape[1]
    y64 = y.double()
    mean = y64.mean(1, keepdim=True)
    mabs = y64.abs().mean(1, keepdim=True)
    idx = rest.unsqueeze(-1).expand(-1, -1, Dd)
    pad = TL - K
    ref = torch.gather(torch.cat([y64, mean.expand(N, pad, Dd)], 1), 1, idx) + pos.double()
    exact = (torch.gather(torch.cat([y, torch.zeros(N, pad, Dd)], 1), 1, idx) + pos).double()     # fp32 add, then widened
    kept = (rest < K).unsqueeze(-1)
    ref = torch.where(kept, exact, ref)
    term = math.sqrt(K) * mabs + mean.abs() + pos.double().abs() + ref.abs()
    return {"yfull": Out(ref, "C_ASF", torch.where(kept, torch.zeros_like(term), term))}


def assemble_bwd_ref(dyf, rest, K):
    """dy[n, k] = dyfull[n, slot(k)] + (1 / K) sum_{masked i} dyfull[n, i], bf16."""
    N, TL, Dd = dyf.shape
    d64 = dyf.double()
    masked = (rest >= K).unsqueeze(-1).double()
    msum = (d64 * masked).sum(1, keepdim=True) / K
    mabs = (d64.abs() * masked).sum(1, keepdim=True) / K
    slot = torch.argsort(rest, dim=1)[:, :K]
    dk = torch.gather(d64, 1, slot.unsqueeze(-1).expand(-1, -1, Dd))
    ref = dk + msum
    term = math.sqrt(max(TL - K, 1)) * mabs + msum.abs() + dk.abs() + ref.abs()
    return {"dy": bf16_out(ref, "C_ASB", term)}


# ------------------------------------------------------------------------------------------------ loss
def patch_tokens(x):
    """[N, B, 9, 9] -> [N, T * 9, 72]: token 9 tau + 3 i + j, feature 9 u + 3 p + q holds x[n, 8 tau + u, 3 i + p, 3 j + q]."""
    N, B = x.shape[:2]
    return x.reshape(N, B // 8, 8, 3, 3, 3, 3).permute(0, 1, 3, 5, 2, 4, 6).reshape(N, B // 8 * 9, 72)


def unpatch_tokens(t):
    N, TL = t.shape[:2]
    return t.reshape(N, TL // 9, 3, 3, 8, 3, 3).permute(0, 1, 4, 2, 5, 3, 6).reshape(N, TL // 9 * 8, 9, 9)


def loss_lds_bytes(T, images):
    """What hs_loss compares with 150 KiB: the cube image (twice with reconstruction images) and the mask row."""
    return (T * 8 * 81 * (2 if images else 1) + T * 9) * 4


def loss_chain(TL, form):
    """Length of the longest chain of fp32 additions behind one partial sum: a wave of the per-sample form adds its ceil(TL / 16)
    rows, then one thread the 16 waves; in the row form a wave adds 8 rows, then one thread the 4 waves."""
    return (TL + 15) // 16 + 16 if form == "sample" else LOSS_ROWS_PER_WG // 4 + 4


def loss_form(T, images):
    return "sample" if loss_lds_bytes(T, images) <= 150 * 1024 else "row"


# 150 KiB = 153600 bytes: T * (648 k + 9) * 4 <= 153600  <=>  T <= 29 with images (k = 2: 29 -> 151380, 30 -> 156600) and
# T <= 58 without (k = 1: 58 -> 152424, 59 -> 155052).
assert [loss_form(t, 1) for t in (29, 30)] == ["sample", "row"] and [loss_form(t, 0) for t in (58, 59)] == ["sample", "row"]

LAYOUTS = ["contig", "band", "perm", "off1", "sn1"]       # float4 staging; band-fastest; generic three ways
# the staging branch of loss_sample_kernel each layout takes, as the test ids name it (loss_kernel reads through the strides)
STAGING = {"contig": "float4", "band": "bandfastest", "perm": "generic_permuted", "off1": "generic_x_plus_one_float",
           "sn1": "generic_sn_E_plus_1"}
# (T, N, layout, norm_pix, images, dpred)
LOSS_CASES = ([(T, 3, lay, 1, 1, 1) for T in (1, 6, 29) for lay in LAYOUTS] +
              [(6, 3, "contig", 0, 1, 1), (6, 2, "band", 0, 1, 0), (6, 3, "perm", 1, 0, 1), (6, 3, "contig", 1, 0, 0),
               (6, 2, "band", 1, 0, 1), (1, 1, "sn1", 0, 0, 1),
               (58, 2, "contig", 1, 0, 1), (58, 2, "band", 1, 0, 1), (58, 1, "perm", 0, 0, 1), (58, 2, "off1", 1, 0, 0),
               (30, 1, "contig", 1, 1, 1), (30, 2, "band", 1, 1, 1), (30, 2, "perm", 0, 1, 1), (30, 1, "sn1", 1, 1, 0),
               (59, 1, "contig", 1, 0, 1), (59, 2, "band", 0, 0, 1), (59, 2, "off1", 1, 0, 1)])


def loss_case_id(c):
    T, N, lay, npx, img, dp = c
    form = loss_form(T, img)
    return f"{form}-T{T}-N{N}-{STAGING[lay] if form == 'sample' else lay}-{'norm' if npx else 'raw'}-{'img' if img else 'noimg'}-{'dpred' if dp else 'nodpred'}"


def loss_inputs(T, N, seed):
    """A cube with a band ramp and an offset, one flat patch per sample (std = 1e-3 under norm_pix), predictions, and a
    structured mask that keeps some rows."""
    from oracle import hsimae_oracle as O
    g = gen(seed)
    B = T * 8
    x = skew((N, B, 9, 9), g, 0.3, 0.4) + torch.linspace(0.0, 0.5, B).reshape(1, B, 1, 1)
    for n in range(N):
        tau, i, j = (n * 5) % T, n % 3, (n + 1) % 3
        x[n, 8 * tau:8 * tau + 8, 3 * i:3 * i + 3, 3 * j:3 * j + 3] = 0.7 + 0.1 * n
    pred = skew((N, T * 9, 72), g, 0.2, 1.0)
    lt, ll = max(1, T // 3), 5
    _, _, mask = O.mask_from_noise(torch.rand(N, T, generator=g).numpy(), torch.rand(N, 9, generator=g).numpy(), lt, ll)
    mask = torch.from_numpy(mask)
    for n in range(N):                                         # the flat patch is a masked row: it enters dpred and the loss
        mask[n, 9 * ((n * 5) % T) + 3 * (n % 3) + (n + 1) % 3] = 1.0
    sm = float(np.float32(mask.sum().item()))
    return dict(x=x.float(), pred=pred, mask=mask, sum_mask=sm, inv_scale=float(np.float32(0.5 / (72 * sm))))


def loss_ref(x, pred, mask, norm_pix, inv_scale, sum_mask, form):
    """target = patch tokens, under norm_pix (t - mean) / sqrt(var_unbiased + 1e-6);  rowloss = mask mean((pred - target)^2);
    loss = sum rowloss / sum_mask;  dpred = 2 mask (pred - target) inv_scale (bf16, 72 of 96 columns);
    pred_img = unpatch(pred std + mean), mask_img = unpatch(mask)."""
    N, B = x.shape[:2]
    TL = B // 8 * 9
    t, pr, mk = patch_tokens(x.double()), pred.double(), mask.double().unsqueeze(-1)
    if norm_pix:
        mean = t.mean(-1, keepdim=True)
        std = torch.sqrt(((t - mean) ** 2).sum(-1, keepdim=True) / 71 + F32_1E6)
        tg = (t - mean) / std
        dt = t.abs().mean(-1, keepdim=True) / std + tg.abs()
        pimg = pr * std + mean
        pterm = pr.abs() * std + mean.abs() + pimg.abs()
    else:
        tg, dt, pimg, pterm = t, torch.zeros_like(t), pr, torch.zeros_like(pr)
    diff = pr - tg
    s = 2 * mk * inv_scale
    dp = torch.zeros(N * TL, 96, dtype=torch.float64)
    dpt = torch.zeros_like(dp)
    dp[:, :72] = (s * diff).reshape(N * TL, 72)
    dpt[:, :72] = (s * (dt + diff.abs())).reshape(N * TL, 72)
    rowl = (mk * diff ** 2).mean(-1).reshape(-1)
    rterm = (mk * 2 * diff.abs() * (dt + diff.abs())).mean(-1).reshape(-1) + rowl
    P = TL if form == "sample" else LOSS_ROWS_PER_WG
    depth = loss_chain(TL, form)
    nparts = N if form == "sample" else (N * TL + P - 1) // P
    padded = torch.zeros(2, nparts * P, dtype=torch.float64)
    padded[0, :N * TL], padded[1, :N * TL] = rowl, rterm
    parts = padded[0].reshape(nparts, P).sum(1)
    pterms = padded[1].reshape(nparts, P).sum(1) + math.sqrt(depth) * parts
    loss = rowl.sum() / sum_mask
    lterm = (rterm.pow(2).sum().sqrt() + math.sqrt(depth) * rowl.sum()) / sum_mask + loss.abs()
    return {"loss": Out(loss, "C_LOSS", lterm), "partial": Out(parts, "C_LOSS", pterms), "dpred": bf16_out(dp, "C_DP", dpt),
            "pred_img": Out(unpatch_tokens(pimg), "C_PI", unpatch_tokens(pterm)),
            "mask_img": Out(unpatch_tokens(mk.expand(-1, -1, 72).contiguous()))}


# ------------------------------------------------------------------------------------------------ patch gather (exact)
def patch_gather_ref(x, ids_keep):
    """bf16 (round to nearest even) of the kept tokens' pixels, [N * K, 96] with the columns 72.. zero."""
    N, K = ids_keep.shape
    tok = torch.gather(patch_tokens(x), 1, ids_keep.long().unsqueeze(-1).expand(-1, -1, 72)).reshape(N * K, 72)
    out = torch.zeros(N * K, 96, dtype=torch.bfloat16)
    out[:, :72] = tok.to(torch.bfloat16)
    return out


# ------------------------------------------------------------------------------------------------ AdamW
ADAMW_N = 4 * (2048 * 256) + 4 * 37          # one float4 per thread of the full grid (2048 x 256), then 37 more: the loop's tail
ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)


def adamw_inputs(n, seed):
    """p, g, m, v and the groups: random per element (so most float4 are mixed), a run of all-frozen float4, a run of
    all-decayed ones, NaN gradients under every frozen element, elements with m = v = g = 0 and with v = g = 0 alone."""
    g = gen(seed)
    p = skew((n,), g, 0.1, 0.5)
    grad = skew((n,), g, 0.01, 0.05)
    m = skew((n,), g, 0.005, 0.02)
    v = (skew((n,), g, 0.3, 0.5) ** 2 * 1e-3).float()
    group = torch.randint(0, 3, (n,), generator=g, dtype=torch.uint8)
    group[4000:4400] = 2
    group[8000:8400] = 0
    group[n - 8:n - 4] = 2                                     # an all-frozen float4 in the tail, then a mixed one
    group[n - 4:] = torch.tensor([2, 0, 1, 2], dtype=torch.uint8)
    grad[100:140] = 0.0
    v[100:140] = 0.0
    m[100:120] = 0.0
    grad[group == 2] = float("nan")
    return dict(p=p, g=grad, m=m, v=v, group=group)


def adamw_ref(p, g, m, v, group, step, lr, b1, b2, eps, wd):
    """torch.optim.AdamW (decoupled decay on group 0, none on group 1, group 2 frozen) in fp64 from the fp32 values the ABI
    receives; inv_bc1 and inv_sqrt_bc2 rounded to fp32 as the launcher passes them."""
    def f(a):
        return float(np.float32(a))
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    inv_bc1, isb = f(1.0 / (1.0 - b1 ** step)), f(1.0 / math.sqrt(1.0 - b2 ** step))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    frozen = group == 2
    g = torch.where(frozen, torch.zeros_like(g), g)            # never read
    x = torch.where(group == 0, p * (1 - lr * wd), p)
    mn = m + (g - m) * (1 - b1)
    vn = v * b2 + g * g * (1 - b2)
    den = torch.sqrt(vn) * isb + eps
    pn = x - lr * inv_bc1 * mn / den
    tm = 2 * (g - m).abs() * (1 - b1) + mn.abs()
    tv = v.abs() * b2 + 2 * g * g * (1 - b2) + vn.abs()
    tp = 2 * x.abs() + pn.abs() + lr * inv_bc1 / den * (tm + 8 * mn.abs())
    zero = torch.zeros_like(p)
    return {"p": Out(torch.where(frozen, p, pn), "C_ADAM", torch.where(frozen, zero, tp)),
            "m": Out(torch.where(frozen, m, mn), "C_ADAM", torch.where(frozen, zero, tm)),
            "v": Out(torch.where(frozen, v, vn), "C_ADAM", torch.where(frozen, zero, tv))}


# ------------------------------------------------------------------------------------------------ fine-tuning head
# (N, C, T, L, D).  3 x 5: C T D = 480 and N T D = 288 leave both last workgroups partly filled; 7 x 256: every thread of block 0
# writes gb and C T D = 10240 fills its workgroups exactly; 33 x 16: both counts are whole workgroups; 2 x 3 x 3 x 2 x 7: D is
# no multiple of 4.
HEAD_SHAPES = [(3, 5, 4, 9, 24), (1, 1, 1, 1, 8), (7, 256, 2, 9, 20), (33, 16, 6, 9, 128), (2, 3, 3, 2, 7)]


def head_inputs(N, C, T, L, D, seed):
    g = gen(seed)
    return dict(latent=skew((N, T * L, D), g, 0.3, 1.0), g=skew((N, C), g, -0.1, 0.5), w=skew((C, T * D), g, 0.05, 0.3))


def agg_pool_ref(latent, T, L):
    """pooled[n, t D + c] = mean_l latent[n, t L + l, c]."""
    N, _, D = latent.shape
    l64 = latent.double().reshape(N, T, L, D)
    ref = l64.mean(2).reshape(N, T * D)
    term = math.sqrt(L) * l64.abs().mean(2).reshape(N, T * D) + ref.abs()
    return {"pooled": Out(ref, "C_POOL", term)}


def head_bwd_ref(g, pooled, w, T, L, D):
    """class_pred = pooled W^T + b:  gw = g^T pooled, gb = column sums of g, dlatent[n, t L + l, c] = (g W)[n, t D + c] / L."""
    N, C = g.shape
    g64, p64, w64 = g.double(), pooled.double(), w.double()
    gw, gwt = g64.t() @ p64, math.sqrt(N) * (g64.abs().t() @ p64.abs())
    gb, gbt = g64.sum(0), math.sqrt(N) * g64.abs().sum(0)
    dl = (g64 @ w64) / L
    dlt = math.sqrt(C) * (g64.abs() @ w64.abs()) / L + dl.abs()

    def spread(a):
        return a.reshape(N, T, 1, D).expand(N, T, L, D).reshape(N, T * L, D)
    return {"gw": Out(gw, "C_HEAD", gwt), "gb": Out(gb, "C_HEAD", gbt), "dlatent": Out(spread(dl), "C_HEAD", spread(dlt))}


# ------------------------------------------------------------------------------------------------ masking (exact)
MASK_SHAPES = [(64, 9, 64, 9), (64, 9, 1, 1), (64, 64, 17, 5), (1, 1, 1, 1), (12, 9, 3, 9)]     # (T, L, len_t, len_l)
MASK_N = [1, 63, 64, 65]                                                                       # around one workgroup of 64 samples


def mask_inputs(N, T, L, seed):
    """Noise with exact ties: a quantised noise_1 (many equal values, also across the keep threshold) and a constant noise_2
    on every other sample."""
    g = gen(seed)
    n1 = (torch.rand(N, T, generator=g) * 8).floor() / 8
    n2 = torch.rand(N, L, generator=g)
    n2[::2] = 0.25
    if T > 1:
        n1[:, T - 1] = n1[:, 0]
    return n1.float(), n2.float()
