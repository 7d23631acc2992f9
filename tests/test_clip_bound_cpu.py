"""csrc/clip.hip without a GPU: the fp64 restatement (tests/clip_ref.py) against torch's clip_grad_norm_ + AdamW in fp64, an
fp32 emulation of the two kernels inside the bound, the bound against planted faults, the skip bookkeeping over a sequence of
steps, and the library's two new symbols under ABI 108 with the refusals that precede every launch."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_ref as R  # noqa: E402

N = R.STEP_N
HP = R.ADAMW_HP
INF = float("inf")


@pytest.fixture(autouse=True)
def rng_state_left_as_found():
    """Tests that run after this file and draw from the global generators without seeding find them as they would have without it."""
    import random
    saved = random.getstate(), np.random.get_state(), torch.get_rng_state()
    yield
    random.setstate(saved[0])
    np.random.set_state(saved[1])
    torch.set_rng_state(saved[2])


def clean_inputs(seed=5, n=N):
    """adamw_inputs with finite values under the frozen lanes too (a fault that counts or steps them shows as a number)."""
    inp = R.adamw_inputs(n, seed)
    frozen = inp["group"] == 2
    inp["g"][frozen] = 0.75
    return inp


def measured_norm(inp):
    s, n, _ = R.sumsq_ref([(inp["g"], inp["group"])])
    return math.sqrt(s)


# ------------------------------------------------------------------------------------------------ against torch, fp64
@pytest.mark.parametrize("case", ["below", "equal", "above", "inf"])
def test_restatement_equals_torch_clip_grad_norm_and_adamw_in_fp64(case):
    """Hyper-parameters that are exact in fp32 and whose bias corrections at step 1 are exact too (b1 = 1/2, b2 = 3/4: both
    factors are 2), so that the restatement's fp32 roundings of them change nothing and 1e-12 can be asked."""
    hp = dict(lr=2.0 ** -7, b1=0.5, b2=0.75, eps=2.0 ** -20, wd=2.0 ** -4)
    inp = R.adamw_inputs(N, 7)
    live = inp["group"] != 2
    norm = measured_norm(inp)
    max_norm = {"below": R.f32(0.3 * norm), "equal": R.f32(norm), "above": R.f32(3.0 * norm), "inf": INF}[case]
    idx = [torch.nonzero(inp["group"] == k).reshape(-1) for k in (0, 1)]
    params = [torch.nn.Parameter(inp["p"][i].double()) for i in idx]
    for q, i in zip(params, idx):
        q.grad = inp["g"][i].double()
    opt = torch.optim.AdamW([dict(params=[params[0]], weight_decay=hp["wd"]), dict(params=[params[1]], weight_decay=0.0)],
                            lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"])
    for q, i in zip(params, idx):                              # moments that are not zero
        opt.state[q] = dict(step=torch.tensor(0.0), exp_avg=inp["m"][i].double().clone(), exp_avg_sq=inp["v"][i].double().clone())
    t_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    j = int(inp["g"][idx[0]].abs().argmax())
    t_coef = float(params[0].grad[j] / inp["g"][idx[0][j]].double())
    opt.step()

    s, n, _ = R.sumsq_ref([(inp["g"], inp["group"])])
    ctl = R.ctl_ref(s, n, max_norm, 0, 1, 0, hp["b1"], hp["b2"])
    assert n == int(live.sum()) and ctl["finite"] == 1 and ctl["apply"] == 1 and ctl["t"] == 1
    assert abs(float(ctl["norm"].ref) - t_norm) <= 1e-12 * t_norm
    assert abs(float(ctl["coef"].ref) - t_coef) <= 1e-12
    assert (float(ctl["coef"].ref) == 1.0) == (case in ("above", "inf")) and (case != "equal" or 1 - 2e-6 < float(ctl["coef"].ref) < 1)
    ref = R.adamw_ctl_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["group"], float(ctl["coef"].ref), 1, 1, **hp)
    for k, (q, i) in enumerate(zip(params, idx)):
        st = opt.state[q]
        for name, got in (("p", q.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            err = float((got - ref[name].ref[i]).abs().max())
            assert err <= 1e-12, (case, k, name, err)


# ------------------------------------------------------------------------------------------------ fp32 emulation and faults
def emulate(state, g, group, max_norm, skip, step, skipped_before, hp, fault=None, norm_max_before=0.0):
    """The two kernels as they compute: fp64 squares added in another order than the reference's (sequentially), the control
    block in fp64 with one fp32 rounding per field, the step in fp32.  `fault` plants one mistake."""
    c = torch.ones_like(group, dtype=torch.bool) if fault == "frozen_counted" else R.counted(g, group)
    with np.errstate(all="ignore"):
        sq = (g[c] * g[c]).double() if fault == "fp32_squares" else g[c].double() ** 2
        sumsq = float(np.add.accumulate(sq.numpy())[-1]) if sq.numel() else 0.0
    finite = int(math.isfinite(sumsq))
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64(sumsq)))
        cc = float(np.float64(R.f32(max_norm)) / (np.float64(norm) + (0.0 if fault == "no_1e-6" else 1e-6)))
    coef = cc if (fault == "no_clamp" or not cc > 1.0) else 1.0
    apply_ = int(not (skip and not finite))
    skipped = skipped_before + (1 - apply_)
    t = step if fault == "skip_advances_t" else step - skipped
    i1, i2 = R.bias_corrections(t, hp["b1"], hp["b2"])
    out = dict(sumsq=sumsq, norm=R.f32(norm), coef=R.f32(coef), finite=finite, apply=apply_, skipped=skipped, inv_bc1=R.f32(i1),
               inv_sqrt_bc2=R.f32(i2), norm_max=max(R.f32(norm_max_before), R.f32(norm)) if finite else R.f32(norm_max_before))
    f = np.float32
    lr, b1, b2, eps, wd = (f(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    p, m, v = state["p"], state["m"], state["v"]
    frozen = group == 2
    decayed = torch.where(group == 0, p * float(f(1) - lr * wd), p)
    if not apply_:
        out.update(p=torch.where(frozen, p, decayed) if fault == "skip_decays" else p.clone(), m=m.clone(), v=v.clone())
        return out
    gz = torch.where(frozen, torch.zeros_like(g), g)
    gc = gz * out["coef"]
    gm = gz if fault == "coef_not_applied" else gc
    gv = gz if fault in ("coef_not_applied", "coef_m_only") else gc
    mn = m + (gm - m) * float(f(1) - b1)
    vn = v * float(b2) + gv * gv * float(f(1) - b2)
    den = torch.sqrt(vn) * out["inv_sqrt_bc2"] + float(eps)
    pn = decayed - float(lr * f(out["inv_bc1"])) * (mn / den)
    out.update(p=torch.where(frozen, p, pn), m=torch.where(frozen, m, mn), v=torch.where(frozen, v, vn))
    return out


def judge(got, state, g, group, max_norm, skip, step, skipped_before, hp, norm_max_before=0.0):
    """Worst err / bound of one emulated (or faulty) step against the restatement; inf for a wrong exact field."""
    s, n, _ = R.sumsq_ref([(g, group)])
    ctl = R.ctl_ref(s, n, max_norm, skip, step, skipped_before, hp["b1"], hp["b2"], norm_max_before)
    worst = 0.0
    for k in ("finite", "apply", "skipped"):
        if got[k] != ctl[k]:
            return math.inf
    for k in ("sumsq", "norm", "coef", "norm_max", "inv_bc1", "inv_sqrt_bc2"):
        ref = float(ctl[k].ref)
        if math.isfinite(ref):
            worst = max(worst, ctl[k].ratio(torch.tensor(got[k], dtype=torch.float64)))
        elif not R.same_nonfinite(got[k], ref):
            return math.inf
    ref = R.adamw_ctl_ref(state["p"], g, state["m"], state["v"], group, got["coef"], ctl["apply"], ctl["t"], **hp)
    for k in "pmv":
        worst = max(worst, ref[k].ratio(got[k]))
    return worst


def state_of(inp):
    return {k: inp[k].clone() for k in "pmv"}


@pytest.mark.parametrize("factor", [0.3, 1.0, 3.0, INF])
def test_fp32_emulation_stays_within_the_bound_over_three_steps(factor):
    inp = clean_inputs()
    g, group = inp["g"], inp["group"]
    max_norm = INF if factor == INF else R.f32(factor * measured_norm(inp))
    st, nm = state_of(inp), 0.0
    for step in (1, 2, 3):
        got = emulate(st, g, group, max_norm, 1, step, 0, HP, None, nm)
        w = judge(got, st, g, group, max_norm, 1, step, 0, HP, nm)
        print(f"factor {factor} step {step}: worst err / bound {w:.3f}, coef {got['coef']:.6f}")
        assert w <= 1.0
        st, nm = {k: got[k] for k in "pmv"}, got["norm_max"]


FAULTS = ["coef_not_applied", "coef_m_only", "frozen_counted", "no_1e-6", "no_clamp", "skip_decays", "skip_advances_t", "fp32_squares"]


@pytest.mark.parametrize("fault", FAULTS)
def test_bound_rejects_planted_faults(fault):
    inp = clean_inputs()
    g, group = inp["g"].clone(), inp["group"]
    skip, step, before = 1, 1, 0
    if fault == "no_1e-6":
        g *= 1e-3                                              # a small norm: 1e-6 is a visible part of the denominator
    if fault == "fp32_squares":
        g[group != 2] = 0.0
        g[torch.nonzero(group != 2)[:3].reshape(-1)] = torch.tensor([1e30, -1e30, 1e30])
    norm = measured_norm(dict(g=g, group=group))
    max_norm = R.f32((3.0 if fault == "no_clamp" else 0.3) * norm)
    if fault == "fp32_squares":
        assert math.isfinite(norm) and abs(norm - math.sqrt(3) * 1e30) < 1e24        # (fp32's 1e30 is 1.00000002e30)
        max_norm = 1.0                                         # clipped to 1: the step itself stays inside fp32
    if fault == "skip_decays":
        g[torch.nonzero(group != 2)[-1]] = float("nan")        # this step is skipped
    if fault == "skip_advances_t":
        step, before = 3, 1                                    # a clean step after one skipped step: t = 2, not 3
    st = state_of(inp)
    args = (st, g, group, max_norm, skip, step, before, HP)
    assert judge(emulate(*args), *args) <= 1.0                 # the harness itself is clean on this very input
    w = judge(emulate(*args, fault=fault), *args)
    print(f"{fault}: worst err / bound = {w:.3g}")
    assert w > 10.0, w


def test_skip_bookkeeping_over_five_steps_with_steps_2_and_3_not_finite():
    inp = clean_inputs()
    group = inp["group"]
    last = int(torch.nonzero(group != 2)[-1])
    max_norm = R.f32(0.3 * measured_norm(inp))
    st, skipped, nm = state_of(inp), 0, 0.0
    seen_skipped, seen_t = [], []
    for step in (1, 2, 3, 4, 5):
        g = inp["g"].clone()
        if step == 2:
            g[last] = INF
        if step == 3:
            g[last] = float("nan")
        got = emulate(st, g, group, max_norm, 1, step, skipped, HP, None, nm)
        assert judge(got, st, g, group, max_norm, 1, step, skipped, HP, nm) <= 1.0
        if step in (2, 3):
            assert got["apply"] == 0 and all(torch.equal(got[k], st[k]) for k in "pmv")
        s, n, _ = R.sumsq_ref([(g, group)])
        seen_t.append(R.ctl_ref(s, n, max_norm, 1, step, skipped, HP["b1"], HP["b2"])["t"])
        skipped, nm = got["skipped"], got["norm_max"]
        seen_skipped.append(skipped)
        st = {k: got[k] for k in "pmv"}
    assert seen_skipped == [0, 1, 2, 2, 2] and seen_t == [1, 1, 1, 2, 3]
    # without skip_nonfinite the same gradients are applied, with the coefficient IEEE arithmetic gives (torch does the same)
    g = inp["g"].clone(); g[last] = INF
    s, n, _ = R.sumsq_ref([(g, group)])
    c = R.ctl_ref(s, n, max_norm, 0, 1, 0, HP["b1"], HP["b2"])
    assert c["apply"] == 1 and c["finite"] == 0 and c["coef_value"] == 0.0 and c["norm_value"] == INF
    g[last] = float("nan")
    s, n, _ = R.sumsq_ref([(g, group)])
    assert math.isnan(R.ctl_ref(s, n, max_norm, 0, 1, 0, HP["b1"], HP["b2"])["coef_value"])


# ------------------------------------------------------------------------------------------------ ABI
def test_library_exports_the_clip_entry_points_under_abi_108():
    from hsimae_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    for name in ("hsimae_grad_norm", "hsimae_adamw_step_ctl"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    declared = set(re.findall(r"\b(hsimae_[a-z0-9_]+)\s*\(", hdr)) - {"hsimae_bucket_cb"}
    assert declared == set(_lib.SYMBOLS.keys())
    # the struct in _lib.py against the header's: the same fields in the same order, and the size the header states
    body = re.search(r"typedef struct hsimae_clip_ctl \{(.*?)\} hsimae_clip_ctl;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": C.c_double, "float": C.c_float, "int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            fields += [(nm.strip(), ctype[ty]) for nm in names.split(",")]

    class FromHeader(C.Structure):
        _fields_ = fields
    assert fields == list(_lib.ClipCtl._fields_)
    assert C.sizeof(FromHeader) == C.sizeof(_lib.ClipCtl) == 48 == int(re.search(r"hsimae_adamw_step_ctl; (\d+) bytes", hdr).group(1))
    assert int(re.search(r"#define HSIMAE_CLIP_GRID (\d+)", hdr).group(1)) == _lib.CLIP_GRID == R.GRID
    assert int(re.search(r"#define HSIMAE_CLIP_MAX_SEGS (\d+)", hdr).group(1)) == _lib.CLIP_MAX_SEGS == 8
    assert C.sizeof(_lib.GradSeg) == 24

    # the refusals that are decided before anything is launched
    def segs(*ns):
        a = (_lib.GradSeg * max(len(ns), 1))()
        for k, n in enumerate(ns):
            a[k] = _lib.GradSeg(1 << 20, None, n)
        return a

    def gn(s=None, nseg=1, max_norm=1.0, step=1, partials=1 << 21, ctl=1 << 22):
        return lib.hsimae_grad_norm(segs(4) if s is None else s, nseg, max_norm, 1, step, 0.9, 0.95, partials, ctl, None)
    assert gn(nseg=0) == -1 and gn(s=segs(*([4] * 9)), nseg=9) == -1 and gn(s=segs(4, -1), nseg=2) == -1 and gn(step=0) == -1
    assert gn(ctl=None) == -1 and gn(partials=None) == -1
    assert gn(max_norm=0.0) == -1 and gn(max_norm=-1.0) == -1 and gn(max_norm=float("nan")) == -1
    bad = segs(4); bad[0].g = None
    assert gn(s=bad) == -4
    bad[0].g = (1 << 20) + 2
    assert gn(s=bad) == -3 and gn(partials=(1 << 21) + 4) == -3 and gn(ctl=(1 << 22) + 4) == -3

    def st(p=1 << 20, g=1 << 21, m=1 << 22, v=1 << 23, group=None, gu=0, n=17, ctl=1 << 24):
        return lib.hsimae_adamw_step_ctl(p, g, m, v, group, gu, n, 1e-3, 0.9, 0.95, 1e-8, 0.05, ctl, None)
    assert st(n=-1) == -1 and st(gu=3) == -1 and st(gu=-1) == -1
    assert st(n=0) == 0 and st(gu=2) == 0
    assert st(p=None) == -4 and st(g=None) == -4 and st(m=None) == -4 and st(v=None) == -4 and st(ctl=None) == -4
    assert st(p=(1 << 20) + 2) == -3 and st(ctl=(1 << 24) + 4) == -3


def test_fused_adamw_takes_the_new_arguments_and_leaves_the_default_alone():
    from hsimae_amd import FusedAdamW
    lin = torch.nn.Linear(3, 2)
    plain = FusedAdamW(lin, lr=1e-3)
    assert plain._clip is False and plain._extra is None and plain.max_grad_norm is None
    with pytest.raises(AttributeError, match="without max_grad_norm"):
        plain.grad_norm
    assert FusedAdamW(lin, max_grad_norm=1.0)._clip and FusedAdamW(lin, skip_nonfinite=True)._clip
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="greater than 0"):
            FusedAdamW(lin, max_grad_norm=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAdamW(lin, max_grad_norm=1.0).grad_norm
