"""The fused MLP half (csrc/fused_enc.hip), instantiation by instantiation, against a float64 reference (tests/mlp_ref.py) on a
real MI355X.  Every call goes through hsimae_enc_mlp_fwd / hsimae_enc_mlp_bwd.

The library launches seven instantiations: enc_mlp_fwd_kernel<D, HP> and enc_mlp_bwd_kernel<D, HP, false> for (D, HP) = (128, 352),
(256, 704), (64, 192), and enc_mlp_bwd_kernel<256, 704, true>, the late-store form for planar operands.  mlp_ref.expected restates
the rule; the first test proves that the cases below reach all seven.

One helper builds every case.  Every input carries 3 guard rows of NaN past M (x1, dy, res2, the row factors), b1 / b3 hold NaN
past `hidden`, every non-atomic output sits in a NaN-filled buffer with guard rows that must be bit-identical afterwards, and
g_n2w / g_n2b start from random values between finite sentinels (NaN cannot be a canary under an atomic add).  Every compared
element is held to its own derived bound (never max-over-max); the worst err / bound per case is printed ("RATIO ...", run
with -s).  The bounds are derived in mlp_ref.py and not adjusted to what is measured here.

Worst err / bound seen on MI355X per instantiation and output (dyb and dx1b are compared for bit equality):

    instantiation                          x2      u2      g       dh1     dh3     dx1     g_n2w   g_n2b
    enc_mlp_fwd_kernel<128, 352>           0.997
    enc_mlp_fwd_kernel<256, 704>           0.984
    enc_mlp_fwd_kernel<64, 192>            0.979
    enc_mlp_bwd_kernel<128, 352, false>            0.995   0.995   0.991   0.992   0.128   0.160   0.242
    enc_mlp_bwd_kernel<256, 704, false>            0.995   0.994   0.991   0.992   0.129   0.171   0.202
    enc_mlp_bwd_kernel<256, 704, true>             0.991   0.991   0.986   0.991   0.083   0.016   0.010
    enc_mlp_bwd_kernel<64, 192, false>             0.995   0.995   0.991   0.991   0.099   0.223   0.269

u2, g, dh1 and dh3 sit just under 1 because their bound is dominated by the half ulp of their own bf16 rounding, which some
element of a few thousand always comes close to.  x2 reaches its bound where an operand did round the other way (a flip of
mlp_ref: the error is then one bf16 ulp of that operand times its weight, which is the bound's own term); where none did it is
0.002 - 0.5.  The LayerNorm-2 gradients are largest at M = 1 (one addend per element); at M = 113 they are near 0.01 and
at M = 1000 near 0.004: their bound adds the rows' worst cases (the propagated accumulation bound of du2 and the error of xhat),
the errors themselves add like a random walk.  With the extreme pre-activations x2 is at 0.39 - 0.63.
"""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

from hsimae_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EDIMS, EUNSUP, ENULL = 0, -1, -2, -4
GUARD = 3
SENT = -7777.25                        # guard value around g_n2w / g_n2b
BF, F32 = torch.bfloat16, torch.float32
WIDTHS = [128, 256, 64]
SHAPE_CASES = [(d, h) for d in WIDTHS for h in (R.SHAPES[d][0], R.SHAPES[d][0] - 31, R.MODEL_HIDDEN[d])]


def row_counts(d):
    r = R.SHAPES[d][1]
    return [1, r - 1, r, r + 1, 2 * r + 17, 1000]


def test_cases_reach_every_instantiation():
    reached = set()
    for d, h in SHAPE_CASES:
        e = R.expected(d, h, 0, True)
        assert e[:3] == (d,) + R.SHAPES[d]
        reached |= {R.fwd_name(e), R.bwd_name(e)}
    for d in WIDTHS:                                          # the planar test: late stores at D = 256 and nowhere else
        e = R.expected(d, R.MODEL_HIDDEN[d], 2 * R.SHAPES[d][1] + 17, True)
        assert e[3] == (d == 256)
        reached.add(R.bwd_name(e))
        assert not R.expected(d, R.MODEL_HIDDEN[d], 200, False)[3]      # {dh13, g} NULL: nothing to store late
    print("\n".join(sorted(reached)))
    assert reached == R.INSTANTIATIONS and len(reached) == 7


# ------------------------------------------------------------------------------------------------ plumbing
def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(sources, N_img, K_img):
    """sources: [(fp32 matrix [rows, cols], transpose, n_off, k_off)] -> packed bf16 image (hsimae_pack_matrix), zero elsewhere."""
    img = torch.zeros(N_img * K_img, dtype=BF, device=DEV)
    descs = (_lib.PackDesc * len(sources))()
    keep = []
    for i, (w, tr, n_off, k_off) in enumerate(sources):
        w = w.contiguous().float()
        keep.append(w)
        descs[i] = _lib.PackDesc(src=w.data_ptr(), rows=w.shape[0], cols=w.shape[1], transpose=tr, n_off=n_off, k_off=k_off,
                                 KS=K_img // 32, dst=img.data_ptr())
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).clone().to(DEV)
    _lib.check(_lib.load().hsimae_pack_matrix(table.data_ptr(), len(sources), max(w.numel() for w in keep), stream()))
    torch.cuda.synchronize()
    return img


@functools.lru_cache(maxsize=None)
def weights(d, hidden, seed=1, extreme=False):
    """(mlp_ref.Mlp on the device, the hsimae_mlp_weights struct, the tensors it points into)."""
    p = R.Mlp(d, hidden, seed, DEV, w1_scale=(slice(3, 40, 4), 60.0) if extreme else None)
    hp = p.HP
    b1, b3 = torch.full((hp,), float("nan"), device=DEV), torch.full((hp,), float("nan"), device=DEV)
    b1[:hidden], b3[:hidden] = p.b1, p.b3                    # NaN past `hidden`: the kernels must not use what lies there
    imgs = [pack([(p.W1, 0, 0, 0)], hp, d), pack([(p.W3, 0, 0, 0)], hp, d), pack([(p.W2, 0, 0, 0)], d, hp),
            pack([(p.W2, 1, 0, 0)], hp, d), pack([(p.W1, 1, 0, 0), (p.W3, 1, 0, hp)], d, 2 * hp)]
    w = _lib.MlpWeights(n2w=p.gamma.data_ptr(), n2b=p.beta.data_ptr(), w1b=b1.data_ptr(), w3b=b3.data_ptr(), w2b=p.b2.data_ptr(),
                        w1=imgs[0].data_ptr(), w3=imgs[1].data_ptr(), w2=imgs[2].data_ptr(), w2T=imgs[3].data_ptr(),
                        w13T=imgs[4].data_ptr(), hidden=hidden)
    return p, w, (b1, b3, imgs)


def guarded(t, dtype=F32):
    """t [M, ...] followed by GUARD rows of NaN."""
    o = torch.full((t.shape[0] + GUARD,) + tuple(t.shape[1:]), float("nan"), dtype=dtype, device=DEV)
    o[:t.shape[0]] = t
    return o


def nan_buf(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def untouched(buf, before, mask, what):
    assert torch.equal(bits(buf)[mask], bits(before)[mask]), f"{what}: canary region written"


def make_case(d, hidden, M, seed, factors=True, extreme=False):
    p, w, _ = weights(d, hidden, 9 if extreme else 1, extreme)
    inp = R.make_inputs(p, M, seed, DEV)
    if not factors:
        inp["rs"] = inp["rs_mlp"] = inp["rs_attn"] = None
    dev = {k: (guarded(v) if v is not None and k not in ("g0w", "g0b") else v) for k, v in inp.items()}
    return dict(p=p, w=w, M=M, inp=inp, dev=dev)


def run_fwd(c, res2=True, M=None):
    """x2 [M, d] of one forward call; the guard rows of the output buffer are checked here."""
    M = c["M"] if M is None else M
    d, dev = c["p"].d, c["dev"]
    x2 = nan_buf(c["M"] + GUARD, d)
    rc = _lib.load().hsimae_enc_mlp_fwd(dev["x1"].data_ptr(), dev["res2"].data_ptr() if res2 else None, x2.data_ptr(), M, d,
                                        C.byref(c["w"]), _lib.ptr(dev["rs"]), stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    assert bool(x2[M:].isnan().all()), "x2: rows past M written"
    return x2[:M]


def run_bwd(c, groups=("u2", "dh13", "dx1b"), plane_rows=0, M=None):
    """One backward call.  groups: which optional outputs are passed ({u2, dyb}, {dh13, g}, dx1b).  Returns the outputs as
    mlp_ref.bwd_ratios takes them (row-major views of planar operands), None for a group that was not passed; every canary of
    every buffer is checked here."""
    M = c["M"] if M is None else M
    p, dev, inp = c["p"], c["dev"], c["inp"]
    d, hp, h = p.d, p.HP, p.hidden
    P = R.cdiv(hp, 64)
    rows = c["M"] + GUARD
    dx1 = nan_buf(rows, d)
    u2, dyb = (nan_buf(rows, d, dtype=BF), nan_buf(rows, d, dtype=BF)) if "u2" in groups else (None, None)
    dx1b = nan_buf(rows, d, dtype=BF) if "dx1b" in groups else None
    g = dh13 = None
    if "dh13" in groups:
        if plane_rows:
            g, dh13 = nan_buf(P * plane_rows * 64 + 192, dtype=BF), nan_buf(2 * P * plane_rows * 64 + 192, dtype=BF)
        else:
            g, dh13 = nan_buf(rows, hp, dtype=BF), nan_buf(rows, 2 * hp, dtype=BF)
    flat = torch.full((2 * d + 24,), SENT, device=DEV)       # g_n2w at 8, g_n2b at d + 16, sentinels around and between
    gw, gb = flat[8:8 + d], flat[d + 16:2 * d + 16]
    gw.copy_(inp["g0w"]), gb.copy_(inp["g0b"])
    before = {k: v.clone() for k, v in (("g", g), ("dh13", dh13)) if v is not None}
    rc = _lib.load().hsimae_enc_mlp_bwd(dev["x1"].data_ptr(), dev["dy"].data_ptr(), dx1.data_ptr(), _lib.ptr(u2), _lib.ptr(dh13),
                                        _lib.ptr(g), _lib.ptr(dyb), _lib.ptr(dx1b), M, d, C.byref(c["w"]), gw.data_ptr(),
                                        gb.data_ptr(), _lib.ptr(dev["rs_mlp"]), _lib.ptr(dev["rs_attn"]), plane_rows, stream())
    torch.cuda.synchronize()
    assert rc == OK, rc
    for name, t in (("dx1", dx1), ("u2", u2), ("dyb", dyb), ("dx1b", dx1b)):
        assert t is None or bool(t[M:].isnan().all()), f"{name}: rows past M written"
    assert bool((flat[:8] == SENT).all() and (flat[8 + d:d + 16] == SENT).all() and (flat[2 * d + 16:] == SENT).all()), "g_n2w / g_n2b guards"
    out = dict(dx1=dx1[:M], u2=None if u2 is None else u2[:M], dyb=None if dyb is None else dyb[:M],
               dx1b=None if dx1b is None else dx1b[:M], gw=gw.clone(), gb=gb.clone(), g=None, dh1=None, dh3=None)
    if g is not None and not plane_rows:
        assert bool(g[M:].isnan().all()) and bool(dh13[M:].isnan().all()), "g / dh13: rows past M written"
        out.update(g=g[:M], dh1=dh13[:M, :hp], dh3=dh13[:M, hp:])
    elif g is not None:
        # planes [plane][plane_rows][64]: rows past M of every plane, the columns past hp of the last plane and the tail stay NaN
        gp = g[:P * plane_rows * 64].view(P, plane_rows, 64)
        dp = dh13[:2 * P * plane_rows * 64].view(2 * P, plane_rows, 64)
        live_g = torch.zeros(P, plane_rows, 64, dtype=torch.bool, device=DEV)
        for cc in range(P):
            live_g[cc, :M, :min(64, hp - 64 * cc)] = True
        for name, buf, live in (("g", g, live_g), ("dh13", dh13, torch.cat([live_g, live_g]))):
            mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
            mask[:live.numel()] = ~live.reshape(-1)
            untouched(buf, before[name], mask, name + " (planar)")
        rm = lambda planes: torch.cat([planes[cc, :M] for cc in range(P)], 1)[:, :hp].contiguous()      # noqa: E731
        out.update(g=rm(gp), dh1=rm(dp[:P]), dh3=rm(dp[P:]), planes=(g, dh13))
        assert not bool(out["g"].isnan().any() | out["dh1"].isnan().any() | out["dh3"].isnan().any()), "planar operands: a live element was not written"
    return out


WORST = {}


def report(inst, what, r, note=""):
    print(f"RATIO {inst:<36s} {what:<6s} {r:8.4f}  {note}")
    WORST[(inst, what)] = max(WORST.get((inst, what), 0.0), r)
    return r


def check_fwd(c, x2, res2, note, M=None):
    M = c["M"] if M is None else M
    p, inp = c["p"], c["inp"]
    e = R.expected(p.d, p.hidden)
    r = report(R.fwd_name(e), "x2", R.fwd_ratio(p, x2, inp["x1"][:M], inp["res2"][:M] if res2 else None,
                                                None if inp["rs"] is None else inp["rs"][:M]), note)
    assert r <= 1.0, f"x2: err / bound = {r:.3g} ({note})"


def check_bwd(c, out, note, plane_rows=0, full=None):
    p = c["p"]
    e = R.expected(p.d, p.hidden, plane_rows, out["g"] is not None)
    rr = R.bwd_ratios(p, c["inp"], out, full)
    for k, v in rr.items():
        report(R.bwd_name(e), k, v, note)
    assert all(v <= 1.0 for v in rr.values()), f"{note}: {rr}"
    return rr


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("d,hidden", SHAPE_CASES, ids=lambda v: str(v))
def test_forward_and_backward(d, hidden):
    for i, M in enumerate(row_counts(d)):
        c = make_case(d, hidden, M, seed=17 * i + hidden, factors=i != 2)       # M = R: without row factors (NULL pointers)
        note = f"hidden={hidden} M={M}" + ("" if i != 2 else " no-factors")
        res2 = i % 2 == 0
        check_fwd(c, run_fwd(c, res2), res2, note + (" res2" if res2 else ""))
        rr = check_bwd(c, run_bwd(c), note)
        assert len(rr) == 9


@pytest.mark.parametrize("d", WIDTHS)
def test_optional_output_groups(d):
    """{u2, dyb}, {dh13, g} and dx1b are optional: dx1 does not depend on which are passed, the LayerNorm-2 gradients stay inside
    their bound, and the outputs that are present are checked as usual."""
    c = make_case(d, R.MODEL_HIDDEN[d], 2 * R.SHAPES[d][1] + 17, seed=23)
    full = run_bwd(c)
    check_bwd(c, full, "all groups")
    for groups in (("dh13", "dx1b"), ("u2", "dx1b"), ("u2", "dh13"), ()):
        out = run_bwd(c, groups)
        missing = sorted({"u2", "dh13", "dx1b"} - set(groups))
        assert torch.equal(bits(out["dx1"]), bits(full["dx1"])), f"dx1 changes without {missing}"
        rr = check_bwd(c, out, "without " + "+".join(missing), full=full)
        assert ("u2" in rr) == ("u2" in groups) and ("g" in rr) == ("dh13" in groups) and ("dx1b" in rr) == ("dx1b" in groups)


@pytest.mark.parametrize("pad", [0, 48])
@pytest.mark.parametrize("d", WIDTHS)
def test_planar_operands(d, pad):
    """g / dh1 / dh3 as 64-column planes of plane_rows = M + pad rows: exactly the row-major run's values plane by plane, nothing
    else of the buffers written (run_bwd checks it), dx1 bit-identical.  At D = 256 this is the late-store kernel."""
    c = make_case(d, R.MODEL_HIDDEN[d], 2 * R.SHAPES[d][1] + 17, seed=29)
    M = c["M"]
    assert R.expected(d, c["p"].hidden, M + pad, True)[3] == (d == 256)
    rowmajor = run_bwd(c)
    planar = run_bwd(c, plane_rows=M + pad)
    for k in ("g", "dh1", "dh3", "dx1", "u2", "dyb", "dx1b"):
        assert torch.equal(bits(planar[k]), bits(rowmajor[k])), f"{k}: planar run differs from the row-major run"
    check_bwd(c, planar, f"planar plane_rows=M+{pad}", plane_rows=M + pad)


@pytest.mark.parametrize("d", WIDTHS)
def test_a_longer_launch_leaves_the_prefix_unchanged(d):
    r = R.SHAPES[d][1]
    c = make_case(d, R.MODEL_HIDDEN[d], 2 * r + 17, seed=31)
    M1 = r + 5
    assert torch.equal(bits(run_fwd(c, True, M=M1)), bits(run_fwd(c, True)[:M1]))
    assert torch.equal(bits(run_bwd(c, M=M1)["dx1"]), bits(run_bwd(c)["dx1"][:M1]))


@pytest.mark.parametrize("d", WIDTHS)
def test_extreme_gate_preactivations(d):
    """Some rows of W1 scaled until h1 passes -95 and +95 (asserted from the reference): below -88.72 the exponential of the
    forward SiLU overflows.  x2 must be finite and inside the same bound as everywhere."""
    c = make_case(d, R.MODEL_HIDDEN[d], 50, seed=2, extreme=True)
    h1 = R.fwd_ref(c["p"], c["inp"]["x1"], c["inp"]["res2"], c["inp"]["rs"])[2]
    assert float(h1.min()) < -95 and float(h1.max()) > 95, (float(h1.min()), float(h1.max()))
    x2 = run_fwd(c, True)
    bad = int((~torch.isfinite(x2)).sum())
    print(f"EXTREMES d={d}: h1 in [{float(h1.min()):.1f}, {float(h1.max()):.1f}], {bad} of {x2.numel()} x2 elements not finite")
    assert bad == 0
    check_fwd(c, x2, True, "extremes")


# ------------------------------------------------------------------------------------------------ refusals
def call_fwd(c, **over):
    a = dict(x1=c["dev"]["x1"].data_ptr(), x2=c["x2"].data_ptr(), M=c["M"], d=c["p"].d, w=C.byref(c["w"]))
    a.update(over)
    rc = _lib.load().hsimae_enc_mlp_fwd(a["x1"], None, a["x2"], a["M"], a["d"], a["w"], None, stream())
    torch.cuda.synchronize()
    return rc


def call_bwd(c, **over):
    dev, o = c["dev"], c["outs"]
    a = dict(x1=dev["x1"].data_ptr(), dy=dev["dy"].data_ptr(), dx1=o["dx1"].data_ptr(), u2=o["u2"].data_ptr(), dh13=o["dh13"].data_ptr(),
             g=o["g"].data_ptr(), dyb=o["dyb"].data_ptr(), dx1b=o["dx1b"].data_ptr(), M=c["M"], d=c["p"].d, w=C.byref(c["w"]),
             g_n2w=o["gw"].data_ptr(), g_n2b=o["gb"].data_ptr(), plane_rows=0)
    a.update(over)
    rc = _lib.load().hsimae_enc_mlp_bwd(a["x1"], a["dy"], a["dx1"], a["u2"], a["dh13"], a["g"], a["dyb"], a["dx1b"], a["M"], a["d"], a["w"],
                                        a["g_n2w"], a["g_n2b"], None, None, a["plane_rows"], stream())
    torch.cuda.synchronize()
    return rc


def refusal_case(d=128):
    c = make_case(d, R.MODEL_HIDDEN[d], 40, seed=1, factors=False)
    hp = c["p"].HP
    c["x2"] = nan_buf(43, d)
    c["outs"] = dict(dx1=nan_buf(43, d), u2=nan_buf(43, d, dtype=BF), dyb=nan_buf(43, d, dtype=BF), dx1b=nan_buf(43, d, dtype=BF),
                     dh13=nan_buf(43, 2 * hp, dtype=BF), g=nan_buf(43, hp, dtype=BF), gw=torch.full((d,), SENT, device=DEV),
                     gb=torch.full((d,), SENT, device=DEV))
    return c


def nothing_written(c):
    o = c["outs"]
    return bool(c["x2"].isnan().all()) and all(bool(o[k].isnan().all()) for k in ("dx1", "u2", "dyb", "dx1b", "dh13", "g")) and \
        bool((o["gw"] == SENT).all() and (o["gb"] == SENT).all())


def with_hidden(w, hidden):
    w2 = _lib.MlpWeights()
    C.memmove(C.byref(w2), C.byref(w), C.sizeof(w))
    w2.hidden = hidden
    return w2


def test_refusals():
    c = refusal_case()
    assert call_fwd(c, d=96) == EUNSUP and call_bwd(c, d=96) == EUNSUP
    for d in WIDTHS:
        cd = refusal_case(d)
        for hidden in (cd["p"].HP - 32, cd["p"].HP + 1):
            w2 = with_hidden(cd["w"], hidden)
            assert R.expected(d, hidden) is None
            assert call_fwd(cd, w=C.byref(w2)) == EUNSUP and call_bwd(cd, w=C.byref(w2)) == EUNSUP, (d, hidden)
        assert nothing_written(cd)
    for pr in (1, 39):
        assert call_bwd(c, plane_rows=pr) == EDIMS
    for k in ("x1", "x2", "w"):
        assert call_fwd(c, **{k: None}) == ENULL, k
    for k in ("x1", "dy", "dx1", "w", "g_n2w", "g_n2b"):
        assert call_bwd(c, **{k: None}) == ENULL, k
    for k in ("u2", "dyb", "dh13", "g"):                      # a group passed by half
        assert call_bwd(c, **{k: None}) == ENULL, k
    assert nothing_written(c)


def test_zero_rows_is_a_no_op():
    c = refusal_case()
    assert call_fwd(c, M=0) == OK and call_bwd(c, M=0) == OK and nothing_written(c)
