"""csrc/elem.hip without a GPU: the bounds of tests/elem_ref.py tell right from wrong.  For every operation an fp32 emulation
in the kernel's order of operations (fp32 sums, `* (1 / 72.f)`, bf16 outputs), written apart from the fp64 restatement, lies
inside the bound on the shapes of the GPU matrix, and each planted fault lies outside it.  The exact restatements (patch maps)
are pinned to the oracle's."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import elem_ref as R  # noqa: E402

F = torch.float32


def worst(ref, got, what=None):
    """Worst err / bound over the outputs both dicts have; prints what each asks of its constant."""
    r = {k: ref[k].ratio(v) for k, v in got.items()}
    if what:
        print(f"[{what}] " + ", ".join(f"{k} {v:.3g} (asks C = {ref[k].need(got[k]):.3g})" for k, v in r.items()))
    return max(r.values())


# ------------------------------------------------------------------------------------------------ LayerNorm
def emu_ln_fwd(inp, fault=None):
    x, d = inp["x"], inp["x"].shape[1]
    mean = x.sum(1, keepdim=True) / d
    dl = x - mean
    var = (dl * dl).sum(1, keepdim=True) / (d - 1 if fault == "var_over_d_minus_1" else d)
    return {"out": dl * torch.rsqrt(var + 1e-5) * inp["gamma"] + inp["beta"]}


def emu_ln_bwd(inp, acc, use_dres, fault=None, ld=0):
    x, du, gamma = inp["x"], inp["du"], inp["gamma"]
    M, d = x.shape
    xs, n = x, d
    if fault == "stats_over_ld":                               # finite pad columns: the fault shows without a NaN canary
        xs, n = torch.cat([x, torch.full((M, ld - d), 4.0)], 1), ld
    mean = xs.sum(1, keepdim=True) / n
    var = ((xs - mean) ** 2).sum(1, keepdim=True) / n
    rstd = torch.rsqrt(var + 1e-5)
    xhat = (x - mean) * rstd
    t = du * gamma
    a = t.sum(1, keepdim=True) / d
    b = torch.zeros_like(a) if fault == "xhat_term_dropped" else (t * xhat).sum(1, keepdim=True) / d
    dx = rstd * (t - a - xhat * b)
    if use_dres:
        dx = dx + inp["dres"] * (2 if fault == "dres_twice" and acc else 1)
    if acc:
        dx = dx + inp["prev"]
    rows = torch.ones(M, dtype=torch.bool)
    G, rp = 256 // R.ln_tpr(d), R.ln_rows_per_wg(d)
    if fault == "row_group_left_out":
        rows[torch.arange(M) % G == 1] = False
    if fault == "last_workgroup_left_out":
        rows[(M // rp) * rp:] = False
    return {"dx": dx, "dgamma": inp["g0"] + (du * xhat)[rows].sum(0), "dbeta": inp["b0"] + du[rows].sum(0)}


def ln_bwd_reference(inp, acc, use_dres):
    return R.ln_bwd_ref(inp["du"], inp["x"], inp["gamma"], inp["dres"] if use_dres else None, inp["prev"] if acc else None,
                        inp["g0"], inp["b0"])


@pytest.mark.parametrize("d", R.LN_BWD_D)
def test_ln_bwd_fp32_emulation_is_inside_the_bound(d):
    w = 0.0
    for k, (ld, M, acc, use_dres, _) in enumerate(R.ln_bwd_cases(d)):
        inp = R.ln_inputs(M, d, seed=1000 + 31 * d + k)
        w = max(w, worst(ln_bwd_reference(inp, acc, use_dres), emu_ln_bwd(inp, acc, use_dres)))
    print(f"ln_bwd d={d}: fp32 emulation err / bound {w:.3f}")
    assert w <= 1.0


@pytest.mark.parametrize("fault", ["xhat_term_dropped", "row_group_left_out", "last_workgroup_left_out", "stats_over_ld", "dres_twice"])
@pytest.mark.parametrize("d", [72, 264])
def test_ln_bwd_bound_rejects_planted_faults(d, fault):
    M, ld = 3 * R.ln_rows_per_wg(d) + 5, d + 8
    inp = R.ln_inputs(M, d, seed=11 + d)
    ref = ln_bwd_reference(inp, 1, 1)
    assert worst(ref, emu_ln_bwd(inp, 1, 1)) <= 1.0
    w = worst(ref, emu_ln_bwd(inp, 1, 1, fault, ld), f"ln_bwd d={d} {fault}")
    assert w > 1.0


@pytest.mark.parametrize("d", R.LN_FWD_D)
def test_ln_fwd_fp32_emulation_inside_and_variance_fault_outside(d):
    w = 0.0
    for M in R.LN_FWD_M:
        inp = R.ln_inputs(M, d, seed=2000 + 7 * d + M)
        ref = R.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"])
        w = max(w, worst(ref, emu_ln_fwd(inp)))
        assert worst(ref, emu_ln_fwd(inp, "var_over_d_minus_1"), f"ln_fwd d={d} M={M} var / (d - 1)") > 1.0
    print(f"ln_fwd d={d}: fp32 emulation err / bound {w:.3f}")
    assert w <= 1.0


# ------------------------------------------------------------------------------------------------ assembly
def emu_assemble(inp, fault=None):
    y, pos, rest, dyf, K, TL = inp["y"], inp["pos"], inp["rest"], inp["dyf"], inp["K"], inp["TL"]
    N, _, Dd = y.shape
    mean = y.sum(1, keepdim=True) / (TL - K if fault == "mean_over_TL_minus_K" else K)
    src = y
    if fault == "column_group_shifted":                        # one float4 column group reads its neighbour's columns
        src = y.clone()
        src[..., 4:8] = y[..., 8:12]
    idx = rest.unsqueeze(-1).expand(-1, -1, Dd)
    yfull = torch.gather(torch.cat([src, mean.expand(N, TL - K, Dd)], 1), 1, idx) + pos
    masked = (rest >= K).unsqueeze(-1)
    sel = ~masked if fault == "gradient_over_kept_rows" else masked
    msum = (dyf * sel).sum(1, keepdim=True) / K
    if fault == "mean_gradient_not_added":
        msum = torch.zeros_like(msum)
    slot = torch.argsort(rest, dim=1)[:, :K]
    dy = R.bf(torch.gather(dyf, 1, slot.unsqueeze(-1).expand(-1, -1, Dd)) + msum)
    return {"yfull": yfull, "dy": dy}


def assemble_reference(inp):
    ref = R.assemble_fwd_ref(inp["y"], inp["pos"], inp["rest"], inp["K"])
    ref.update(R.assemble_bwd_ref(inp["dyf"], inp["rest"], inp["K"]))
    return ref


def test_assembly_fp32_emulation_is_inside_the_bound():
    w = 0.0
    for kern, Dd, ld, T, lt, ll, N in R.assemble_cases():
        assert R.assemble_kernel(Dd, ld, 9 * T) == kern
        inp = R.assemble_inputs(N, T, lt, ll, Dd, seed=3000 + 13 * Dd + T + lt)
        w = max(w, worst(assemble_reference(inp), emu_assemble(inp)))
    print(f"assembly: fp32 emulation err / bound {w:.3f}")
    assert w <= 1.0
    assert {c[0] for c in R.assemble_cases()} == {"fast16", "fast8", "generic"}


@pytest.mark.parametrize("fault", ["mean_over_TL_minus_K", "gradient_over_kept_rows", "mean_gradient_not_added", "column_group_shifted"])
def test_assembly_bound_rejects_planted_faults(fault):
    inp = R.assemble_inputs(5, 6, 2, 7, 64, seed=12)
    ref = assemble_reference(inp)
    assert worst(ref, emu_assemble(inp)) <= 1.0
    assert worst(ref, emu_assemble(inp, fault), f"assembly {fault}") > 1.0


# ------------------------------------------------------------------------------------------------ loss
def wave_sum72(v):
    """Sum over the 72 features as a wave does it: lane f adds features f and f + 64, then a balanced tree over the 64 lanes."""
    a = v[..., :64].clone()
    a[..., :8] = a[..., :8] + v[..., 64:72]
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a


def emu_loss(inp, norm_pix, form, fault=None):
    x, pr, mk = inp["x"], inp["pred"], inp["mask"].unsqueeze(-1)
    N, TL = pr.shape[:2]
    t = R.patch_tokens(x)
    if fault == "u_and_pq_swapped":                            # feature index 8 (3 p + q) + u in place of 9 u + 3 p + q
        t = t.reshape(N, TL, 8, 9).transpose(2, 3).reshape(N, TL, 72)
    i72, i71 = torch.tensor(1.0, dtype=F) / 72, torch.tensor(1.0, dtype=F) / 71
    if norm_pix:
        mean = wave_sum72(t) * i72
        dl = t - mean
        var = wave_sum72(dl * dl) * (i72 if fault == "biased_variance" else i71)
        std = torch.sqrt(var) + 1e-6 if fault == "eps_outside_the_root" else torch.sqrt(var + 1e-6)
        tg = dl / std
    else:
        mean, std, tg = torch.zeros_like(t[..., :1]), torch.ones_like(t[..., :1]), t
    diff = pr - tg
    rowl = (wave_sum72(diff * diff)[..., 0] * i72 * inp["mask"]).reshape(-1)
    dmk = torch.ones_like(mk) if fault == "mask_not_applied" else mk
    dpred = torch.zeros(N * TL, 96)
    dpred[:, :72] = R.bf(2.0 * dmk * diff * torch.tensor(inp["inv_scale"], dtype=F)).reshape(N * TL, 72)
    if fault == "neighbour_statistics":
        mean, std = torch.roll(mean, 1, 1), torch.roll(std, 1, 1)
    # pred * std + mean is one fused multiply-add in the kernel (hipcc contracts it): one rounding
    pimg = R.unpatch_tokens((pr.double() * std.double() + mean.double()).float() if norm_pix else pr)
    P = TL if form == "sample" else R.LOSS_ROWS_PER_WG
    nparts = N if form == "sample" else (N * TL + P - 1) // P
    padded = torch.zeros(nparts * P)
    padded[:N * TL] = rowl
    parts = padded.reshape(nparts, P).sum(1)
    used = parts[:-1] if fault == "last_partial_dropped" else parts
    loss = (used.double().sum() / inp["sum_mask"]).float()
    return {"loss": loss, "partial": parts, "dpred": dpred, "pred_img": pimg,
            "mask_img": R.unpatch_tokens(mk.expand(-1, -1, 72).contiguous())}


def loss_reference(inp, norm_pix, form):
    return R.loss_ref(inp["x"], inp["pred"], inp["mask"], norm_pix, inp["inv_scale"], inp["sum_mask"], form)


def test_loss_fp32_emulation_is_inside_the_bound_on_every_case():
    w, seen = 0.0, set()
    for T, N, lay, norm_pix, images, dp in R.LOSS_CASES:
        form = R.loss_form(T, images)
        if (T, N, norm_pix, form) in seen:                     # the layout does not change the arithmetic
            continue
        seen.add((T, N, norm_pix, form))
        inp = R.loss_inputs(T, N, seed=4000 + T + N)
        w = max(w, worst(loss_reference(inp, norm_pix, form), emu_loss(inp, norm_pix, form)))
    print(f"loss: fp32 emulation err / bound {w:.3f}")
    assert w <= 1.0
    ids = [R.loss_case_id(c) for c in R.LOSS_CASES]
    for lay in R.LAYOUTS:                                      # every staging branch with and without images, and the row form
        assert any(i.startswith("sample") and f"-{R.STAGING[lay]}-" in i and "-img-" in i for i in ids)
    for lay in ("contig", "band", "perm"):
        assert any(i.startswith("sample") and f"-{R.STAGING[lay]}-" in i and "-noimg-" in i for i in ids)
    assert any(i.startswith("row-T30") for i in ids) and any(i.startswith("row-T59") for i in ids)


def test_loss_switch_points_are_where_150_kib_puts_them():
    assert R.loss_lds_bytes(29, 1) <= 150 * 1024 < R.loss_lds_bytes(30, 1)
    assert R.loss_lds_bytes(58, 0) <= 150 * 1024 < R.loss_lds_bytes(59, 0)
    src = open(os.path.join(ROOT, "hsimae_amd", "csrc", "elem.hip")).read()
    assert "T <= 29 with images, T <= 58 without" in src and "lds <= 150 * 1024" in src


@pytest.mark.parametrize("fault", ["biased_variance", "eps_outside_the_root", "mask_not_applied", "last_partial_dropped",
                                   "neighbour_statistics", "u_and_pq_swapped"])
@pytest.mark.parametrize("T,form", [(6, "sample"), (30, "row")])
def test_loss_bound_rejects_planted_faults(T, form, fault):
    inp = R.loss_inputs(T, 2, seed=13)
    ref = loss_reference(inp, 1, form)
    assert worst(ref, emu_loss(inp, 1, form)) <= 1.0
    assert worst(ref, emu_loss(inp, 1, form, fault), f"loss T={T} {fault}") > 1.0


def test_flat_patch_needs_the_per_token_factor():
    """On the flat patch (std = 1e-3) the fp32 mean's rounding is amplified about 1000 |t| times in the target: the emulation's
    error there is far above a bound without the factor A, and inside the bound with it."""
    inp = R.loss_inputs(6, 2, seed=13)
    ref = loss_reference(inp, 1, "sample")["dpred"]
    got = emu_loss(inp, 1, "sample")["dpred"]
    flat = 9 * 0 + 3 * 0 + 1                                   # sample 0's flat token (loss_inputs: tau 0, i 0, j 1)
    t = R.patch_tokens(inp["x"])[0, flat]
    assert float(t.max() - t.min()) == 0.0
    err = (got[flat, :72].double() - ref.ref[flat, :72]).abs().max()
    scale = 2 * inp["inv_scale"]
    assert err > 100 * R.U * scale and ref.ratio(got) <= 1.0


# ------------------------------------------------------------------------------------------------ patch maps (exact)
def test_patch_maps_equal_the_oracles():
    from oracle import hsimae_oracle as O
    g = R.gen(1)                                               # (the global generators stay as the other tests left them)
    x = torch.rand(3, 1, 48, 9, 9, generator=g)
    cfg = O.OracleConfig(bands=48)
    tok = O.patchify(x, cfg)
    assert torch.equal(R.patch_tokens(x[:, 0]), tok) and torch.equal(R.unpatch_tokens(tok), x[:, 0])
    keep, _, _ = O.mask_from_noise(torch.rand(3, 6, generator=g).numpy(), torch.rand(3, 9, generator=g).numpy(), 2, 7)
    out = R.patch_gather_ref(x[:, 0], torch.from_numpy(keep))
    want = torch.gather(tok, 1, torch.from_numpy(keep).unsqueeze(-1).expand(-1, -1, 72)).reshape(-1, 72)
    assert torch.equal(out[:, :72].float(), R.bf(want)) and not out[:, 72:].any()


# ------------------------------------------------------------------------------------------------ AdamW
def emu_adamw(st, inp, step, hp, fault=None):
    f = lambda a: torch.tensor(a, dtype=F)                     # noqa: E731
    lr, b1, b2, eps, wd = (f(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    s = step - 1 if fault == "bias_correction_step_minus_1" else step
    inv_bc1 = f(1.0 / (1.0 - float(b1) ** s))
    isb = f(1.0 / math.sqrt(1.0 - float(b2) ** s))
    p, m, v, group = st["p"], st["m"], st["v"], inp["group"]
    frozen = group == 2
    g = torch.where(frozen, torch.zeros_like(inp["g"]), inp["g"])
    decay = (group == 0) | ((group == 1) if fault == "decay_on_group_1" else torch.zeros_like(frozen))
    x = torch.where(decay, p * (1.0 - lr * wd), p)
    mn = m + (g - m) * (1.0 - b1)
    vn = v * b2 + g * g * (1.0 - b2)
    den = torch.sqrt(vn + eps) * isb if fault == "eps_inside_the_root" else torch.sqrt(vn) * isb + eps
    pn = x - lr * inv_bc1 * (mn / den)
    if fault == "frozen_lane_updated":                         # a frozen lane of a mixed float4 is updated with the others
        i4 = torch.arange(p.numel()) // 4
        live = torch.zeros(int(i4.max()) + 1, dtype=torch.bool).index_put_((i4,), ~frozen, accumulate=True)
        frozen = frozen & ~live[i4]
    return {"p": torch.where(frozen, p, pn), "m": torch.where(frozen, m, mn), "v": torch.where(frozen, v, vn)}


def test_adamw_fp32_emulation_three_steps_and_step_1000():
    inp = R.adamw_inputs(R.ADAMW_N, seed=5)
    st = {k: inp[k] for k in "pmv"}
    w = 0.0
    for step in (1, 2, 3, 1000):
        ref = R.adamw_ref(st["p"], inp["g"], st["m"], st["v"], inp["group"], step, **R.ADAMW_HP)
        st = emu_adamw(st, inp, step, R.ADAMW_HP)
        w = max(w, worst(ref, st))
        for k in "pmv":
            assert torch.equal(st[k][inp["group"] == 2], inp[k][inp["group"] == 2])
    print(f"adamw: fp32 emulation err / bound {w:.3f}")
    assert w <= 1.0


@pytest.mark.parametrize("fault,step", [("decay_on_group_1", 1), ("bias_correction_step_minus_1", 2), ("bias_correction_step_minus_1", 1000),
                                        ("eps_inside_the_root", 1), ("frozen_lane_updated", 1)])
def test_adamw_bound_rejects_planted_faults(fault, step):
    inp = R.adamw_inputs(4096 * 4, seed=6)
    if fault == "frozen_lane_updated":
        inp["g"] = torch.where(inp["group"] == 2, torch.full_like(inp["g"], 0.01), inp["g"])     # finite: the fault must show without NaN
    st = {k: inp[k] for k in "pmv"}
    ref = R.adamw_ref(st["p"], inp["g"], st["m"], st["v"], inp["group"], step, **R.ADAMW_HP)
    assert worst(ref, emu_adamw(st, inp, step, R.ADAMW_HP)) <= 1.0
    assert worst(ref, emu_adamw(st, inp, step, R.ADAMW_HP, fault), f"adamw {fault} step {step}") > 1.0


# ------------------------------------------------------------------------------------------------ fine-tuning head
def fma_chain(a, b):
    """sum_k a[:, k] b[k, :] as the kernel's chain of fmaf: the product is exact in fp64, one fp32 rounding per step."""
    acc = torch.zeros(a.shape[0], b.shape[1])
    for k in range(a.shape[1]):
        acc = (a[:, k:k + 1].double() * b[k:k + 1].double() + acc.double()).float()
    return acc


def emu_head(inp, T, L, D, fault=None):
    lat, g, w = inp["latent"], inp["g"], inp["w"]
    N, C = g.shape
    pooled = torch.zeros(N, T, D)
    for l in range(L):                                         # one serial chain per element, as the kernel's loop over l
        pooled = pooled + lat.reshape(N, T, L, D)[:, :, l]
    pooled = pooled.reshape(N, T * D) / L
    gw = fma_chain(g.t().contiguous(), pooled)
    if fault == "gw_transposed":
        gw = fma_chain(pooled.t().contiguous(), g).reshape(C, T * D)
    gb = torch.zeros(C)
    for n in range(N - 1 if fault == "gb_over_N_minus_1" else N):
        gb = gb + g[n]
    dl = fma_chain(g, w)
    if fault != "dlatent_not_divided_by_L":
        dl = dl / L
    return {"pooled": pooled, "gw": gw, "gb": gb, "dlatent": dl.reshape(N, T, 1, D).expand(N, T, L, D).reshape(N, T * L, D)}


def head_reference(inp, T, L, D):
    """The backward's reference takes the fp32 pooled features the (clean) emulation produced, as the GPU test takes the kernel's."""
    ref = R.agg_pool_ref(inp["latent"], T, L)
    ref.update(R.head_bwd_ref(inp["g"], emu_head(inp, T, L, D)["pooled"], inp["w"], T, L, D))
    return ref


@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_fp32_emulation_is_inside_the_bound(shape):
    N, C, T, L, D = shape
    inp = R.head_inputs(N, C, T, L, D, seed=6000 + N + C)
    w = worst(head_reference(inp, T, L, D), emu_head(inp, T, L, D), f"head {shape}")
    assert w <= 1.0


@pytest.mark.parametrize("fault", ["dlatent_not_divided_by_L", "gb_over_N_minus_1", "gw_transposed"])
def test_head_bound_rejects_planted_faults(fault):
    N, C, T, L, D = 3, 5, 4, 9, 24
    inp = R.head_inputs(N, C, T, L, D, seed=14)
    ref = head_reference(inp, T, L, D)
    assert worst(ref, emu_head(inp, T, L, D)) <= 1.0
    assert worst(ref, emu_head(inp, T, L, D, fault), f"head {fault}") > 1.0


# ------------------------------------------------------------------------------------------------ masking inputs
@pytest.mark.parametrize("shape", R.MASK_SHAPES, ids=lambda s: "T{}-L{}-lt{}-ll{}".format(*s))
def test_masking_inputs_hold_exact_ties_across_the_keep_threshold(shape):
    """The noise of the GPU matrix has equal values on both sides of the rank threshold, so "ties: lower index wins" decides."""
    T, L, lt, ll = shape
    n1, n2 = R.mask_inputs(65, T, L, seed=7065 + T)
    if T > 1:
        assert bool((n1[:, T - 1] == n1[:, 0]).all())
    if 1 <= lt < T:
        srt = n1.sort(1).values
        assert bool((srt[:, lt - 1] == srt[:, lt]).any())
    if 1 <= ll < L:
        assert bool((n2[::2] == 0.25).all())
