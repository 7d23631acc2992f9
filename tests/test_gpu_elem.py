"""csrc/elem.hip on the GPU: every kernel and every dispatch branch of its launchers against the fp64 restatements and
element-wise bounds of tests/elem_ref.py.  Every output sits in a canary frame, every input is compared bit for bit after the
call, no element is left out of a comparison, and each test prints the worst err / bound it saw (and the constant the result
asks for: how the C_* of elem_ref.py were measured)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import elem_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
I32_CANARY = -(1 << 30) + 12345
I64_CANARY = -(1 << 62) + 12345
GUARD = 64                     # elements on either side of a flat output (256 bytes of fp32: the 16-byte alignment is kept)
OK, EDIMS, EUNSUPPORTED, ENULL = 0, -1, -2, -4


def libs():
    from hsimae_amd import _lib
    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Inputs:
    """Device inputs with a bit image taken before the call."""

    def __init__(self, **kw):
        self.t = {k: v.to(DEV) for k, v in kw.items() if v is not None}
        self.image = {k: bits(v).clone() for k, v in self.t.items()}

    def __getitem__(self, k):
        return self.t[k]

    def ptr(self, k, off_bytes=0):
        return self.t[k].data_ptr() + off_bytes if k in self.t else None

    def unchanged(self):
        for k, v in self.t.items():
            assert torch.equal(bits(v), self.image[k]), f"input {k} was written"


def flat_out(n, dtype=torch.float32, fill=NAN):
    """(whole buffer, device pointer of the n payload elements, payload view) with GUARD canary elements on either side."""
    full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return full, full.data_ptr() + GUARD * full.element_size(), full[GUARD:GUARD + n]


def flat_frame_intact(full, n, fill=NAN):
    g = torch.cat([full[:GUARD], full[GUARD + n:]])
    return bool(g.isnan().all()) if fill != fill else bool((g == fill).all())


def rows_out(rows, ld, dtype=torch.float32):
    """[rows + 2, ld] of NaN: a canary row above and below; returns (buffer, pointer of row 1)."""
    full = torch.full((rows + 2, ld), NAN, dtype=dtype, device=DEV)
    return full, full.data_ptr() + ld * full.element_size()


def rows_frame_intact(full, rows, width):
    return bool(full[0].isnan().all() and full[rows + 1].isnan().all() and full[1:rows + 1, width:].isnan().all())


def pad_cols(a, ld):
    """[M, d] -> [M, ld] with NaN in the columns the kernel must not read."""
    out = torch.full((a.shape[0], ld), NAN)
    out[:, :a.shape[1]] = a
    return out


class Worst:
    def __init__(self, what):
        self.what, self.r, self.c = what, {}, {}

    def add(self, name, out, got):
        r, c = out.ratio(got), out.need(got)
        self.r[name], self.c[name] = max(self.r.get(name, 0.0), r), max(self.c.get(name, 0.0), c)
        return r

    def report(self):
        print(f"[elem {self.what}] worst err / bound: " +
              ", ".join(f"{k} {v:.3f} (asks C = {self.c[k]:.3g})" for k, v in self.r.items()))
        bad = {k: v for k, v in self.r.items() if not v <= 1.0}
        assert not bad, bad


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def run_ln_bwd(inp, M, d, ld, acc, use_dres, use_dg, det=False):
    """One hsimae_ln_bwd call -> (dx [M, d], dgamma, dbeta, (flat, acc64)); frames and inputs are checked here."""
    _lib, lib = libs()
    LD = ld or d
    ins = Inputs(x=pad_cols(inp["x"], LD), du=pad_cols(inp["du"], LD), dres=pad_cols(inp["dres"], LD) if use_dres else None,
                 gamma=inp["gamma"])
    dxf, dxp = rows_out(M, LD)
    if acc:
        dxf[1:M + 1, :d] = inp["prev"].to(DEV)
    flat = torch.full((3 * d + 40,), NAN, device=DEV)          # dgamma at 8, dbeta at d + 24: slots of a flat gradient buffer
    gs, bs = slice(8, 8 + d), slice(d + 24, 2 * d + 24)
    flat[gs], flat[bs] = (0.0, 0.0) if det else (inp["g0"].to(DEV), inp["b0"].to(DEV))
    acc64 = None
    if det:
        acc64 = torch.full((flat.numel(),), I64_CANARY, dtype=torch.int64, device=DEV)
        acc64[gs], acc64[bs] = 0, 0
    before = flat.clone()
    p = _lib.LnBwdParams(du=ins.ptr("du"), x=ins.ptr("x"), stats=None, gamma=ins.ptr("gamma"), dres=ins.ptr("dres"), dx=dxp,
                         accumulate=acc, dgamma=flat.data_ptr() + 32 if use_dg else None,
                         dbeta=flat.data_ptr() + 4 * (d + 24) if use_dg else None, M=M, d=d, ld=ld,
                         det_base=flat.data_ptr() if det else None, det_acc=acc64.data_ptr() if det else None)
    assert lib.hsimae_ln_bwd(C.byref(p), stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged()
    assert rows_frame_intact(dxf, M, d), "dx: a frame row or a column in [d, ld) was written"
    guard = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
    guard[gs], guard[bs] = False, False
    assert bool(flat[guard].isnan().all()), "dgamma / dbeta: written outside their slots"
    if det:
        assert bool((acc64[guard] == I64_CANARY).all()), "det_acc: written outside the slots"
    if not use_dg:
        assert torch.equal(bits(flat), bits(before)), "dgamma / dbeta NULL, yet the slots changed"
    return dxf[1:M + 1, :d].cpu(), flat[gs].cpu(), flat[bs].cpu(), (flat, acc64)


@pytest.mark.parametrize("d", R.LN_BWD_D, ids=lambda d: f"tpr{R.ln_tpr(d)}-d{d}")
def test_ln_bwd_every_width_class_stride_and_row_count(d):
    """ln_bwd_kernel<TPR>: TPR = 8 for d <= 64, 16 for d <= 128, 32 for d <= 256, 64 above (hs_ln_bwd); one workgroup owns
    (256 / TPR) * 8 rows.  d = 8, 72, 144, 264 leave lanes of every row idle."""
    w = Worst(f"ln_bwd<{R.ln_tpr(d)}> d={d}")
    for k, (ld, M, acc, use_dres, use_dg) in enumerate(R.ln_bwd_cases(d)):
        inp = R.ln_inputs(M, d, seed=1000 + 31 * d + k)
        dx, dg, db, _ = run_ln_bwd(inp, M, d, ld, acc, use_dres, use_dg)
        ref = R.ln_bwd_ref(inp["du"], inp["x"], inp["gamma"], inp["dres"] if use_dres else None, inp["prev"] if acc else None,
                           inp["g0"], inp["b0"])
        w.add("dx", ref["dx"], dx)
        if use_dg:
            w.add("dgamma", ref["dgamma"], dg)
            w.add("dbeta", ref["dbeta"], db)
        zr = M // 2                                             # the zero row of du: dx is what was added, exactly
        want = (inp["dres"][zr].double() if use_dres else 0) + (inp["prev"][zr].double() if acc else 0)
        assert torch.equal(dx[zr].double(), (torch.zeros(d, dtype=torch.float64) + want).float().double())
    w.report()


@pytest.mark.parametrize("d", [8, 72, 144, 512], ids=lambda d: f"tpr{R.ln_tpr(d)}-d{d}")
def test_ln_bwd_deterministic_commits(d):
    """det_base / det_acc: bit-identical on a second call, det_acc / 2^44 within the bound, the fp32 slots left alone, and a
    non-finite addend poisons its fp32 slot with NaN."""
    rp = R.ln_rows_per_wg(d)
    M, ld = 3 * rp + 5, d + 8
    inp = R.ln_inputs(M, d, seed=77 + d)
    a = run_ln_bwd(inp, M, d, ld, 0, 1, 1, det=True)
    b = run_ln_bwd(inp, M, d, ld, 0, 1, 1, det=True)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[3][1], b[3][1]) and torch.equal(bits(a[3][0]), bits(b[3][0]))
    assert not a[1].any() and not a[2].any()                    # the sums are in det_acc, the fp32 slots still hold their zeros
    ref = R.ln_bwd_ref(inp["du"], inp["x"], inp["gamma"], inp["dres"], None, None, None, workgroups=(M + rp - 1) // rp)
    acc = a[3][1].cpu().double() / R.DET_SCALE
    w = Worst(f"ln_bwd<{R.ln_tpr(d)}> d={d} deterministic")
    w.add("dx", ref["dx"], a[0])
    w.add("dgamma", ref["dgamma"], acc[8:8 + d])
    w.add("dbeta", ref["dbeta"], acc[d + 24:2 * d + 24])
    w.report()
    bad = dict(inp)
    bad["du"] = inp["du"].clone()
    c = d - 3
    bad["du"][rp + 1, c] = float("inf")                         # one addend of column c is not finite
    _, dg, db, _ = run_ln_bwd(bad, M, d, ld, 0, 1, 1, det=True)
    others = torch.arange(d) != c
    assert bool(dg[c].isnan()) and bool(db[c].isnan()) and not dg[others].any() and not db[others].any()


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@pytest.mark.parametrize("d", R.LN_FWD_D)
def test_ln_fwd_every_width_and_row_count(d):
    """ln_fwd_kernel: one wave per row, four rows per workgroup (M = 3, 4, 5, 257 around it), lanes own columns lane + 64 i."""
    _lib, lib = libs()
    w = Worst(f"ln_fwd d={d}")
    for M in R.LN_FWD_M:
        inp = R.ln_inputs(M, d, seed=2000 + 7 * d + M)
        ins = Inputs(x=inp["x"], gamma=inp["gamma"], beta=inp["beta"])
        full, ptr = rows_out(M, d)
        assert lib.hsimae_ln_fwd(ins.ptr("x"), ins.ptr("gamma"), ins.ptr("beta"), ptr, M, d, stream()) == OK
        torch.cuda.synchronize()
        ins.unchanged()
        assert rows_frame_intact(full, M, d)
        w.add("out", R.ln_fwd_ref(inp["x"], inp["gamma"], inp["beta"])["out"], full[1:M + 1].cpu())
    w.report()


# ------------------------------------------------------------------------------------------------ assembly
def asm_id(c):
    kern, Dd, ld, T, lt, ll, N = c
    return f"{kern}-Dd{Dd}-ld{ld}-TL{9 * T}-K{lt * ll}-N{N}"


@pytest.mark.parametrize("case", R.assemble_cases(), ids=asm_id)
def test_assembly_forward_backward_every_kernel_pair(case):
    """hs_assemble_fwd / _bwd: assemble_*_fast_kernel<16> at Dd = 64 and <8> at Dd = 32 when the rows are dense (ld 0 or Dd) and
    TL <= 512 (TL = 504 fast, 513 generic), the generic pair otherwise (Dd = 48 at ld = 64, Dd = 64 at ld = 96, 128, 512)."""
    _lib, lib = libs()
    kern, Dd, ld, T, lt, ll, N = case
    inp = R.assemble_inputs(N, T, lt, ll, Dd, seed=3000 + 13 * Dd + T + lt)
    K, TL, LD = inp["K"], inp["TL"], ld or Dd
    assert R.assemble_kernel(Dd, ld, TL) == kern
    ins = Inputs(y=pad_cols(inp["y"].reshape(N * K, Dd), LD), pos=inp["pos"], rest=inp["rest"].int(),
                 dyf=pad_cols(inp["dyf"].reshape(N * TL, Dd), LD))
    yf, yfp = rows_out(N * TL, LD)
    dy, dyp = rows_out(N * K, LD, torch.bfloat16)
    p = _lib.AssembleParams(y=ins.ptr("y"), N=N, K=K, TL=TL, Dd=Dd, ids_restore=ins.ptr("rest"), pos=ins.ptr("pos"), yfull=yfp,
                            dyfull=ins.ptr("dyf"), dy=dyp, ld=ld)
    assert lib.hsimae_assemble_fwd(C.byref(p), stream()) == OK
    assert lib.hsimae_assemble_bwd(C.byref(p), stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged()
    assert rows_frame_intact(yf, N * TL, Dd), "yfull: a frame row or a column in [Dd, ld) was written"
    assert rows_frame_intact(dy, N * K, Dd), "dy: a frame row or a column in [Dd, ld) was written"
    w = Worst(f"assemble {asm_id(case)}")
    w.add("yfull", R.assemble_fwd_ref(inp["y"], inp["pos"], inp["rest"], K)["yfull"], yf[1:N * TL + 1, :Dd].cpu().reshape(N, TL, Dd))
    w.add("dy", R.assemble_bwd_ref(inp["dyf"], inp["rest"], K)["dy"], dy[1:N * K + 1, :Dd].float().cpu().reshape(N, K, Dd))
    w.report()


# ------------------------------------------------------------------------------------------------ loss
def place_cube(x, layout):
    """The logical cube [N, B, 9, 9] in one of the layouts -> (buffer, pointer, sn, sb, sh, sw)."""
    N, B = x.shape[:2]
    E = B * 81
    if layout == "contig":                                     # sw 1, sh 9, sb 81, sn % 4 == 0, aligned: the float4 staging
        buf = x.contiguous().to(DEV)
        return buf, buf.data_ptr(), E, 81, 9, 1
    if layout == "band":                                       # [N, 9, 9, B]: sb == 1
        buf = x.permute(0, 2, 3, 1).contiguous().to(DEV)
        return buf, buf.data_ptr(), E, 1, 9 * B, B
    if layout == "perm":                                       # [N, B, w, h]: generic strides
        buf = x.permute(0, 1, 3, 2).contiguous().to(DEV)
        return buf, buf.data_ptr(), E, 81, 1, 9
    if layout == "off1":                                       # contiguous strides, x one float past a 16-byte boundary: generic
        buf = torch.full((N * E + 8,), NAN)
        buf[1:1 + N * E] = x.reshape(-1)
        buf = buf.to(DEV)
        return buf, buf.data_ptr() + 4, E, 81, 9, 1
    assert layout == "sn1"                                     # contiguous samples E + 1 apart: sn % 4 != 0, generic
    buf = torch.full((N, E + 1), NAN)
    buf[:, :E] = x.reshape(N, E)
    buf = buf.to(DEV)
    return buf, buf.data_ptr(), E + 1, 81, 9, 1


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=R.loss_case_id)
def test_loss_every_form_staging_branch_and_optional_output(case):
    """hs_loss: loss_sample_kernel while (T 8 81 (2 with images, else 1) + 9 T) 4 bytes <= 150 KiB, i.e. T <= 29 with images
    and T <= 58 without; loss_kernel (32 rows per workgroup) from T = 30 / 59.  The per-sample form writes N partial sums,
    the row form ceil(N T 9 / 32): which of the two ran is read off the partial buffer's canaries."""
    _lib, lib = libs()
    T, N, layout, norm_pix, images, want_dpred = case
    B, TL, M, E = T * 8, T * 9, N * T * 9, T * 8 * 81
    form = R.loss_form(T, images)
    assert form == ("sample" if T <= (29 if images else 58) else "row")
    inp = R.loss_inputs(T, N, seed=4000 + T + N)
    buf, xp, sn, sb, sh, sw = place_cube(inp["x"], layout)
    ximg = bits(buf).clone()
    ins = Inputs(pred=inp["pred"].reshape(M, 72), mask=inp["mask"].reshape(M))
    nparts = lib.hsimae_loss_partials(N, T)
    assert nparts == max((M + 31) // 32, N)
    written = N if form == "sample" else (M + 31) // 32
    pf, pp, pv = flat_out(nparts)
    lf, lp, lv = flat_out(1)
    df, dp = rows_out(M, 96, torch.bfloat16)
    imf, imp, imv = flat_out(N * E)
    mmf, mmp, mmv = flat_out(N * E)
    p = _lib.LossParams(x=xp, sn=sn, sb=sb, sh=sh, sw=sw, N=N, T=T, pred=ins.ptr("pred"), mask=ins.ptr("mask"), norm_pix=norm_pix,
                        inv_scale=inp["inv_scale"], partial=pp, loss=lp, sum_mask=inp["sum_mask"], dpred=dp if want_dpred else None,
                        pred_img=imp if images else None, mask_img=mmp if images else None)
    assert lib.hsimae_loss(C.byref(p), stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged()
    assert torch.equal(bits(buf), ximg), "the cube was written"
    assert flat_frame_intact(pf, nparts) and flat_frame_intact(lf, 1) and flat_frame_intact(imf, N * E) and flat_frame_intact(mmf, N * E)
    assert bool(pv[written:].isnan().all()) and not bool(pv[:written].isnan().any()), f"not the {form} form's partial sums"
    ref = R.loss_ref(inp["x"], inp["pred"], inp["mask"], norm_pix, inp["inv_scale"], inp["sum_mask"], form)
    w = Worst(f"loss {R.loss_case_id(case)}")
    w.add("loss", ref["loss"], lv.cpu())
    w.add("partial", ref["partial"], pv[:written].cpu())
    if want_dpred:
        assert rows_frame_intact(df, M, 96)
        w.add("dpred", ref["dpred"], df[1:M + 1].float().cpu())
        assert not df[1:M + 1, 72:].any(), "dpred's padding columns 72..95 are not zero"
    else:
        assert bool(df.isnan().all())
    if images:
        w.add("pred_img", ref["pred_img"], imv.cpu().reshape(N, B, 9, 9))
        assert torch.equal(mmv.cpu().reshape(N, B, 9, 9).double(), ref["mask_img"].ref), "mask_img"
    else:
        assert bool(imv.isnan().all() and mmv.isnan().all())
    w.report()


# ------------------------------------------------------------------------------------------------ AdamW
def test_adamw_mixed_groups_frozen_lanes_tail_and_three_steps():
    """adamw_kernel over n / 4 = 2048 * 256 + 37 float4 (the grid is capped at 2048 workgroups: the last 37 are the loop's
    second trip), steps 1, 2, 3 in a row, each compared with the fp64 update of the kernel's own previous state, then step 1000."""
    _lib, lib = libs()
    n = R.ADAMW_N
    assert n // 4 > 2048 * 256 and n % 4 == 0
    inp = R.adamw_inputs(n, seed=5)
    hp = R.ADAMW_HP
    ins = Inputs(g=inp["g"], group=inp["group"])
    frozen = inp["group"] == 2
    st = {k: flat_out(n) for k in "pmv"}
    for k in "pmv":
        st[k][2].copy_(inp[k])
    w = Worst("adamw")
    for step in (1, 2, 3, 1000):
        prev = {k: st[k][2].cpu() for k in "pmv"}
        rc = lib.hsimae_adamw_step(st["p"][1], ins.ptr("g"), st["m"][1], st["v"][1], ins.ptr("group"), n, hp["lr"], hp["b1"], hp["b2"],
                                   hp["eps"], hp["wd"], step, stream())
        assert rc == OK
        torch.cuda.synchronize()
        ins.unchanged()
        ref = R.adamw_ref(prev["p"], inp["g"], prev["m"], prev["v"], inp["group"], step, **hp)
        for k in "pmv":
            got = st[k][2].cpu()
            assert flat_frame_intact(st[k][0], n)
            assert torch.equal(bits(got[frozen]), bits(prev[k][frozen])), f"{k}: a frozen element changed (NaN gradient under it)"
            w.add(f"{k}@{step}", ref[k], got)
    w.report()


# ------------------------------------------------------------------------------------------------ fine-tuning head
@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_agg_pool_and_head_backward(shape):
    _lib, lib = libs()
    N, C_, T, L, D = shape
    TD = T * D
    inp = R.head_inputs(N, C_, T, L, D, seed=6000 + N + C_)
    ins = Inputs(latent=inp["latent"], g=inp["g"], w=inp["w"])
    pf, pp, pv = flat_out(N * TD)
    assert lib.hsimae_agg_pool(ins.ptr("latent"), pp, N, T, L, D, stream()) == OK
    gwf, gwp, gwv = flat_out(C_ * TD)                          # assigned, not accumulated: NaN before the call
    gbf, gbp, gbv = flat_out(C_)
    dlf, dlp, dlv = flat_out(N * T * L * D)
    assert lib.hsimae_head_bwd(ins.ptr("g"), pp, ins.ptr("w"), gwp, gbp, dlp, N, C_, T, L, D, stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged()
    assert flat_frame_intact(pf, N * TD) and flat_frame_intact(gwf, C_ * TD) and flat_frame_intact(gbf, C_) and flat_frame_intact(dlf, N * T * L * D)
    pooled = pv.cpu().reshape(N, TD)
    w = Worst(f"head {shape}")
    w.add("pooled", R.agg_pool_ref(inp["latent"], T, L)["pooled"], pooled)
    ref = R.head_bwd_ref(inp["g"], pooled, inp["w"], T, L, D)
    w.add("gw", ref["gw"], gwv.cpu().reshape(C_, TD))
    w.add("gb", ref["gb"], gbv.cpu())
    w.add("dlatent", ref["dlatent"], dlv.cpu().reshape(N, T * L, D))
    w.report()


# ------------------------------------------------------------------------------------------------ masking
def run_mask(n1, n2, lt, ll):
    _lib, lib = libs()
    N, T = n1.shape
    L = n2.shape[1]
    K, TL = lt * ll, T * L
    ins = Inputs(n1=n1, n2=n2)
    kf, kp, kv = flat_out(N * K, torch.int32, I32_CANARY)
    rf, rp, rv = flat_out(N * TL, torch.int32, I32_CANARY)
    mf, mp, mv = flat_out(N * TL)
    p = _lib.MaskParams(noise1=ins.ptr("n1"), noise2=ins.ptr("n2"), N=N, T=T, L=L, len_t=lt, len_l=ll, ids_keep=kp, ids_restore=rp,
                        mask=mp)
    assert lib.hsimae_mask_from_noise(C.byref(p), stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged()
    assert flat_frame_intact(kf, N * K, I32_CANARY) and flat_frame_intact(rf, N * TL, I32_CANARY) and flat_frame_intact(mf, N * TL)
    return kv.cpu().numpy().reshape(N, K), rv.cpu().numpy().reshape(N, TL), mv.cpu().numpy().reshape(N, TL)


@pytest.mark.parametrize("shape", R.MASK_SHAPES, ids=lambda s: "T{}-L{}-lt{}-ll{}".format(*s))
def test_masking_bit_exact_with_ties_up_to_64_groups(shape):
    """T = 64 sets bit 63 of the keep mask; L = 64 likewise for the positions; one workgroup holds 64 samples."""
    from oracle import hsimae_oracle as O
    T, L, lt, ll = shape
    for N in R.MASK_N:
        n1, n2 = R.mask_inputs(N, T, L, seed=7000 + N + T)
        keep, rest, mask = run_mask(n1, n2, lt, ll)
        k2, r2, m2 = O.mask_from_noise(n1.numpy(), n2.numpy(), lt, ll)
        assert np.array_equal(keep, k2) and np.array_equal(rest, r2) and mask.tobytes() == m2.tobytes(), (shape, N)


# ------------------------------------------------------------------------------------------------ patch gather
@pytest.mark.parametrize("layout", ["contig", "band"])
def test_patch_gather_grid_stride_loop_bit_exact(layout):
    """N K 12 = 1048656 octets: 80 more than the 4096 x 256 threads of the capped grid, which take a second trip."""
    from oracle import hsimae_oracle as O
    _lib, lib = libs()
    N, T, lt, ll = 6242, 2, 2, 7
    K = lt * ll
    assert N * K * 12 > 4096 * 256 >= (N - 1) * K * 12
    g = R.gen(8)
    x = R.skew((N, 16, 9, 9), g, 0.3, 0.5)
    x[:, :, 0, 0], x[:, :, 0, 1] = 1.00390625, 1.01171875      # exact bf16 ties: to even, down and up
    keep, _, _ = O.mask_from_noise(torch.rand(N, T, generator=g).numpy(), torch.rand(N, 9, generator=g).numpy(), lt, ll)
    buf, xp, sn, sb, sh, sw = place_cube(x, layout)
    ximg = bits(buf).clone()
    ins = Inputs(ids=torch.from_numpy(keep).int())
    of, op = rows_out(N * K, 96, torch.bfloat16)
    p = _lib.PatchParams(x=xp, sn=sn, sb=sb, sh=sh, sw=sw, N=N, T=T, K=K, ids_keep=ins.ptr("ids"), out=op, pos_ids=None)
    assert lib.hsimae_patch_gather(C.byref(p), stream()) == OK
    torch.cuda.synchronize()
    ins.unchanged()
    assert torch.equal(bits(buf), ximg) and rows_frame_intact(of, N * K, 96)
    ref = R.patch_gather_ref(x, torch.from_numpy(keep))
    assert torch.equal(bits(of[1:N * K + 1].cpu()), bits(ref))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_their_code_and_write_nothing():
    """Every check below precedes its launch in the launcher (hs_ln_bwd, hs_ln_fwd, hs_assemble_*, hs_mask, hs_head_bwd, hs_adamw),
    so the buffers a refused call names keep their canaries."""
    _lib, lib = libs()
    t = torch.full((1 << 16,), NAN, device=DEV)
    a, s = t.data_ptr(), stream()

    def at(k):
        return a + 4096 * k
    ln = dict(du=at(0), x=at(1), gamma=at(2), dres=at(3), dx=at(4), accumulate=0, dgamma=at(5), dbeta=at(6), M=4, d=64, ld=0)

    def ln_rc(**kw):
        d = dict(ln); d.update(kw)
        return lib.hsimae_ln_bwd(C.byref(_lib.LnBwdParams(**d)), s)
    assert ln_rc(d=520) == EUNSUPPORTED and ln_rc(d=12) == EUNSUPPORTED and ln_rc(M=0) == OK and ln_rc(M=-3) == OK
    assert lib.hsimae_ln_bwd(None, s) == ENULL
    assert lib.hsimae_ln_fwd(at(0), at(1), at(2), at(3), 4, 520, s) == EUNSUPPORTED
    assert lib.hsimae_ln_fwd(at(0), at(1), at(2), at(3), 0, 64, s) == OK and lib.hsimae_ln_fwd(None, at(1), at(2), at(3), 4, 64, s) == ENULL
    asm = dict(y=at(0), N=2, K=4, TL=18, Dd=64, ids_restore=at(1), pos=at(2), yfull=at(3), dyfull=at(4), dy=at(5), ld=0)
    for fn in (lib.hsimae_assemble_fwd, lib.hsimae_assemble_bwd):
        assert fn(C.byref(_lib.AssembleParams(**dict(asm, Dd=520))), s) == EUNSUPPORTED
        assert fn(C.byref(_lib.AssembleParams(**dict(asm, N=0))), s) == OK and fn(None, s) == ENULL
    mk = dict(noise1=at(0), noise2=at(1), N=2, T=12, L=9, len_t=3, len_l=9, ids_keep=at(2), ids_restore=at(3), mask=at(4))

    def mk_rc(**kw):
        return lib.hsimae_mask_from_noise(C.byref(_lib.MaskParams(**dict(mk, **kw))), s)
    assert mk_rc(T=65) == EDIMS and mk_rc(len_t=0) == EDIMS and mk_rc(len_t=13) == EDIMS and mk_rc(L=65) == EDIMS
    assert mk_rc(len_l=0) == EDIMS and mk_rc(len_l=10) == EDIMS and mk_rc(N=0) == OK
    hb = lib.hsimae_head_bwd
    assert hb(at(0), at(1), at(2), at(3), at(4), at(5), 2, 257, 2, 9, 8, s) == EDIMS
    assert hb(at(0), at(1), at(2), at(3), at(4), at(5), 2, 0, 2, 9, 8, s) == EDIMS
    assert hb(at(0), at(1), at(2), at(3), at(4), at(5), 0, 4, 2, 9, 8, s) == OK
    assert lib.hsimae_agg_pool(at(0), at(1), 0, 2, 9, 8, s) == OK
    ad = lib.hsimae_adamw_step
    assert ad(at(0), at(1), at(2), at(3), at(4), 10, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1, s) == EDIMS
    assert ad(at(0), at(1), at(2), at(3), at(4), 8, 1e-3, 0.9, 0.999, 1e-8, 0.05, 0, s) == EDIMS
    assert ad(at(0), at(1), at(2), at(3), at(4), 0, 1e-3, 0.9, 0.999, 1e-8, 0.05, 1, s) == OK
    ls = dict(x=at(0), sn=648, sb=81, sh=9, sw=1, N=0, T=1, pred=at(1), mask=at(2), norm_pix=1, inv_scale=1.0, partial=at(3), loss=at(4),
              sum_mask=1.0, dpred=at(5), pred_img=at(6), mask_img=at(7))
    assert lib.hsimae_loss(C.byref(_lib.LossParams(**ls)), s) == OK and lib.hsimae_loss(None, s) == ENULL
    pg = dict(x=at(0), sn=648, sb=81, sh=9, sw=1, N=0, T=1, K=4, ids_keep=at(1), out=at(2), pos_ids=None)
    assert lib.hsimae_patch_gather(C.byref(_lib.PatchParams(**pg)), s) == OK
    torch.cuda.synchronize()
    assert bool(t.isnan().all()), "a refused or empty call wrote something"
