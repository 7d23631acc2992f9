"""csrc/clip.hip on the GPU against the fp64 restatement of tests/clip_ref.py: the gradient norm and its control block through the
C ABI at every size where the kernel takes another path, the step that reads the control block, the refusals, and the Python
layer: FusedAdamW(max_grad_norm=, skip_nonfinite=) on HSIMAE and DualViT, its state_dict, and the fine-tuning loop."""
import contextlib
import copy
import ctypes as C
import io
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
GUARD = 64
OK, EDIMS, EALIGN, ENULL = 0, -1, -3, -4
B1, B2 = 0.9, 0.95
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_loop_default.json")


@pytest.fixture(autouse=True)
def rng_state_left_as_found():
    """These tests seed the global generators (model initialisation, the loop's split); tests that run after this file and draw
    from them without seeding must find them as they would have without it."""
    import random
    saved = random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state_all()
    yield
    random.setstate(saved[0])
    np.random.set_state(saved[1])
    torch.set_rng_state(saved[2])
    torch.cuda.set_rng_state_all(saved[3])


def libs():
    from hsimae_amd import _lib
    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Ctl:
    """A control block and the partials in device memory, each between canaries."""

    def __init__(self, skipped=0, norm_max=0.0):
        _lib, _ = libs()
        self.size = C.sizeof(_lib.ClipCtl)
        host = torch.full((self.size + 2 * GUARD,), 0xA5, dtype=torch.uint8)
        c = _lib.ClipCtl(skipped=skipped, norm_max=norm_max)
        host[GUARD:GUARD + self.size] = torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8)
        self.buf = host.to(DEV)
        self.part = torch.full((R.GRID + 2 * GUARD,), NAN, dtype=torch.float64, device=DEV)
        self.ptr = self.buf.data_ptr() + GUARD
        self.part_ptr = self.part.data_ptr() + GUARD * 8

    def raw(self):
        return self.buf[GUARD:GUARD + self.size].cpu()

    def read(self):
        _lib, _ = libs()
        c = _lib.ClipCtl.from_buffer_copy(self.raw().numpy().tobytes())
        return {f: getattr(c, f) for f, _ in _lib.ClipCtl._fields_}

    def partials(self):
        return self.part[GUARD:GUARD + R.GRID].cpu()

    def frame_intact(self):
        b, p = self.buf.cpu(), self.part.cpu()
        return (bool((b[:GUARD] == 0xA5).all() and (b[GUARD + self.size:] == 0xA5).all()) and
                bool(p[:GUARD].isnan().all() and p[GUARD + R.GRID:].isnan().all()))


def device_segs(segs, g_off=None, grp_off=None):
    """[(g, group)] on the host -> the ctypes array and the device tensors that back it.  g_off / grp_off: elements by which
    segment 0's arrays start behind a 256-byte boundary."""
    _lib, _ = libs()
    arr, keep = (_lib.GradSeg * len(segs))(), []
    for k, (g, group) in enumerate(segs):
        go, ro = (g_off or 0, grp_off or 0) if k == 0 else (0, 0)
        gd = torch.full((g.numel() + go,), NAN, device=DEV)
        gd[go:] = g.to(DEV)
        rd = None
        if group is not None:
            rd = torch.full((g.numel() + ro,), 2, dtype=torch.uint8, device=DEV)
            rd[ro:] = group.to(DEV)
        keep += [gd, rd]
        arr[k] = _lib.GradSeg(gd.data_ptr() + 4 * go, None if rd is None else rd.data_ptr() + ro, g.numel())
    return arr, keep


def run_norm(segs, max_norm, skip, step, skipped=0, norm_max=0.0, **off):
    _, lib = libs()
    arr, keep = device_segs(segs, **off)
    images = [None if t is None else bits(t).clone() for t in keep]
    ctl = Ctl(skipped, norm_max)
    rc = lib.hsimae_grad_norm(arr, len(segs), max_norm, skip, step, B1, B2, ctl.part_ptr, ctl.ptr, stream())
    assert rc == OK
    torch.cuda.synchronize()
    assert ctl.frame_intact(), "a canary behind partials or ctl was written"
    for t, im in zip(keep, images):
        assert t is None or torch.equal(bits(t), im), "an input was written"
    return ctl


def check_ctl(got, segs, max_norm, skip, step, skipped=0, norm_max=0.0, what=""):
    s, n, _ = R.sumsq_ref(segs)
    ref = R.ctl_ref(s, n, max_norm, skip, step, skipped, B1, B2, norm_max)
    for k in ("finite", "apply", "skipped"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    worst = {}
    for k in ("sumsq", "norm", "coef", "norm_max", "inv_bc1", "inv_sqrt_bc2"):
        r = float(ref[k].ref)
        if math.isfinite(r):
            worst[k] = ref[k].ratio(torch.tensor(got[k], dtype=torch.float64))
        else:
            assert R.same_nonfinite(got[k], r), (what, k, got[k], r)
    print(f"[clip norm {what}] n counted {n}, norm {got['norm']:.6g}, coef {got['coef']:.6g}; err / bound: " +
          ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return ref


# ------------------------------------------------------------------------------------------------ the norm, through the C ABI
def norm_cases():
    sizes8 = [1, 3, 4, 5, 255, 1021, 4099, 70001]
    cases = {f"n{n}-group": dict(segs=[(n, True)]) for n in R.NORM_N}
    cases["n5-nogroup"] = dict(segs=[(5, False)])
    cases["n1021-nogroup"] = dict(segs=[(1021, False)])
    cases["g-4-bytes-off-ids-unaligned"] = dict(segs=[(1021, True)], g_off=1, grp_off=0)     # ids start 3 before a 4-byte boundary
    cases["g-4-bytes-off-ids-aligned"] = dict(segs=[(1021, True)], g_off=1, grp_off=1)
    cases["g-12-bytes-off-nogroup"] = dict(segs=[(258, False)], g_off=3)
    cases["2-segments"] = dict(segs=[(1021, True), (255, False)])
    cases["8-segments"] = dict(segs=[(n, k % 2 == 0) for k, n in enumerate(sizes8)])
    return cases


NORM_CASES = norm_cases()


@pytest.mark.parametrize("name", list(NORM_CASES))
def test_norm_every_size_alignment_and_segment_count(name):
    """sumsq, norm, coef and the bias corrections within the restatement's bound, the integer fields exact, NaN under every
    id-2 element, canaries intact, and a second run bit-identical (control block and all 1024 partials).  Called as step 3 with
    one step skipped before: t = 2."""
    case = NORM_CASES[name]
    assert R.NORM_N_FULL == 4 * 256 * R.GRID + 4 * 37 + 3
    segs = [R.norm_segment(n, 11 + k, wg) for k, (n, wg) in enumerate(case["segs"])]
    off = {k: v for k, v in case.items() if k != "segs"}
    s, _, _ = R.sumsq_ref(segs)
    max_norm = R.f32(0.3 * math.sqrt(s)) if s > 0 else 1.0
    a = run_norm(segs, max_norm, 1, 3, skipped=1, norm_max=0.001, **off)
    b = run_norm(segs, max_norm, 1, 3, skipped=1, norm_max=0.001, **off)
    assert torch.equal(a.raw(), b.raw()) and torch.equal(bits(a.partials()), bits(b.partials())), "two runs differ"
    ref = check_ctl(a.read(), segs, max_norm, 1, 3, 1, 0.001, name)
    assert ref["t"] == 2 and ref["apply"] == 1
    if s > 0:
        assert 0.29 < a.read()["coef"] < 0.31
    # report only: +inf never clips
    c = run_norm(segs, INF, 0, 1).read()
    assert c["coef"] == 1.0 and c["apply"] == 1 and c["skipped"] == 0


def test_norm_of_1e30_is_finite_and_inf_or_nan_in_the_last_tail_is_not():
    segs = [R.norm_segment(255, 3, True), R.norm_segment(4 * 300 + 3, 4, True)]
    g, group = segs[1]
    n = g.numel()
    group[n - 3:] = torch.tensor([0, 2, 1], dtype=torch.uint8)
    g[n - 3:] = torch.tensor([0.5, NAN, -0.25])                # the tail: counted, frozen (NaN under it), counted
    big = [(segs[0][0], segs[0][1]), (g.clone(), group)]
    live = torch.nonzero(group != 2).reshape(-1)
    big[1][0][live[:2]] = torch.tensor([1e30, -1e30])
    big[1][0][n - 1] = 1e30
    got = run_norm(big, 1.0, 1, 1).read()
    check_ctl(got, big, 1.0, 1, 1, what="1e30")
    assert got["finite"] == 1 and math.isfinite(got["norm"]) and got["norm"] > 1.7e30 and 0 < got["coef"] < 1e-30
    for bad in (INF, NAN):
        g2 = g.clone()
        g2[n - 1] = bad
        s2 = [segs[0], (g2, group)]
        skipped = run_norm(s2, 1.0, 1, 2, skipped=0, norm_max=0.5).read()
        ref = check_ctl(skipped, s2, 1.0, 1, 2, 0, 0.5, what=f"{bad} skip")
        assert skipped["finite"] == 0 and skipped["apply"] == 0 and skipped["skipped"] == 1 and ref["t"] == 1
        assert skipped["norm_max"] == 0.5                       # a norm that is not finite does not enter the running maximum
        applied = run_norm(s2, 1.0, 0, 2).read()
        check_ctl(applied, s2, 1.0, 0, 2, what=f"{bad} no skip")
        assert applied["finite"] == 0 and applied["apply"] == 1 and applied["skipped"] == 0
        assert applied["coef"] == 0.0 if bad == INF else math.isnan(applied["coef"])


# ------------------------------------------------------------------------------------------------ the step, through the C ABI
class State:
    def __init__(self, inp):
        n = inp["p"].numel()
        self.n = n
        self.full = {k: torch.full((n + 2 * GUARD,), NAN, device=DEV) for k in "pmv"}
        for k in "pmv":
            self.full[k][GUARD:GUARD + n] = inp[k].to(DEV)

    def ptr(self, k):
        return self.full[k].data_ptr() + 4 * GUARD

    def host(self):
        return {k: self.full[k][GUARD:GUARD + self.n].cpu() for k in "pmv"}

    def frame_intact(self):
        return all(bool(f[:GUARD].isnan().all() and f[GUARD + self.n:].isnan().all()) for f in self.full.values())


def run_step(st, g_dev, group_dev, gu, ctl, hp):
    _, lib = libs()
    rc = lib.hsimae_adamw_step_ctl(st.ptr("p"), g_dev.data_ptr(), st.ptr("m"), st.ptr("v"),
                                   None if group_dev is None else group_dev.data_ptr(), gu, st.n, hp["lr"], hp["b1"], hp["b2"],
                                   hp["eps"], hp["wd"], ctl.ptr, stream())
    assert rc == OK
    torch.cuda.synchronize()


def clipped_step(st, inp_g, group, gu, max_norm, skip, step, ctl, hp, worst, tag):
    """One hsimae_grad_norm + hsimae_adamw_step_ctl on the running state; compared with the restatement fed the state before it."""
    _lib, lib = libs()
    group_h = group if group is not None else R.uniform_group(st.n, gu)
    prev = st.host()
    before = ctl.read()
    g_dev = inp_g.to(DEV)
    g_img = bits(g_dev).clone()
    group_dev = None if group is None else group.to(DEV)
    arr = (_lib.GradSeg * 1)(_lib.GradSeg(g_dev.data_ptr(), None if group is None else group_dev.data_ptr(), st.n))
    assert lib.hsimae_grad_norm(arr, 1, max_norm, skip, step, hp["b1"], hp["b2"], ctl.part_ptr, ctl.ptr, stream()) == OK
    run_step(st, g_dev, group_dev, gu, ctl, hp)
    assert torch.equal(bits(g_dev), g_img), "the gradient was modified: the clip belongs inside the step"
    got, now = st.host(), ctl.read()
    s, n, _ = R.sumsq_ref([(inp_g, group)])
    cref = R.ctl_ref(s, n, max_norm, skip, step, before["skipped"], hp["b1"], hp["b2"], before["norm_max"])
    assert (now["finite"], now["apply"], now["skipped"]) == (cref["finite"], cref["apply"], cref["skipped"]), (tag, now)
    for k in ("inv_bc1", "inv_sqrt_bc2"):
        assert cref[k].ratio(torch.tensor(now[k], dtype=torch.float64)) <= 1.0, (tag, k)
    if cref["finite"]:
        assert cref["coef"].ratio(torch.tensor(now["coef"], dtype=torch.float64)) <= 1.0, (tag, now["coef"])
    ref = R.adamw_ctl_ref(prev["p"], inp_g, prev["m"], prev["v"], group_h, now["coef"], cref["apply"], cref["t"],
                          hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"])
    frozen = group_h == 2
    assert st.frame_intact() and ctl.frame_intact()
    for k in "pmv":
        assert torch.equal(bits(got[k][frozen]), bits(prev[k][frozen])), f"{tag} {k}: a frozen element changed"
        if not cref["apply"]:
            assert torch.equal(bits(got[k]), bits(prev[k])), f"{tag} {k}: a skipped step wrote"
        worst[f"{k}@{tag}"] = ref[k].ratio(got[k])
    return now, cref


def test_step_clipped_unclipped_skipped_and_resumed():
    """n = 4 (256 + 37) + 3 on adamw_inputs (mixed ids, NaN under the frozen ones): steps 1-3 clipped to about 0.3, steps 4-6 with
    +inf, step 7 with a NaN planted and skipped (bit-identical, skipped = 1), step 8 clean with t = 7."""
    n = R.STEP_N
    assert n == 4 * (256 + 37) + 3
    inp = R.adamw_inputs(n, seed=5)
    hp = R.ADAMW_HP
    s, _, _ = R.sumsq_ref([(inp["g"], inp["group"])])
    clip = R.f32(0.3 * math.sqrt(s))
    st, ctl, worst = State(inp), Ctl(), {}
    for step in (1, 2, 3):
        now, _ = clipped_step(st, inp["g"], inp["group"], 0, clip, 1, step, ctl, hp, worst, f"clip{step}")
        assert 0.29 < now["coef"] < 0.31
    for step in (4, 5, 6):
        now, _ = clipped_step(st, inp["g"], inp["group"], 0, INF, 1, step, ctl, hp, worst, f"inf{step}")
        assert now["coef"] == 1.0
    bad = inp["g"].clone()
    bad[int(torch.nonzero(inp["group"] != 2)[-1])] = NAN       # a counted element of the tail
    now, cref = clipped_step(st, bad, inp["group"], 0, clip, 1, 7, ctl, hp, worst, "nan7")
    assert now["apply"] == 0 and now["skipped"] == 1
    now, cref = clipped_step(st, inp["g"], inp["group"], 0, clip, 1, 8, ctl, hp, worst, "clean8")
    assert now["apply"] == 1 and now["skipped"] == 1 and cref["t"] == 7
    print("[clip step] worst err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}


@pytest.mark.parametrize("n", [17, 1])
@pytest.mark.parametrize("gu", [0, 1])
def test_step_with_one_group_for_every_element(n, gu):
    """group = NULL: 17 elements (cls_head.bias with 17 classes: four float4 and one more) and a single one."""
    inp = R.adamw_inputs(64, seed=9)
    inp = {k: v[:n].clone() for k, v in inp.items()}
    inp["g"] = torch.where(inp["g"].isnan(), torch.full_like(inp["g"], 0.02), inp["g"])
    hp = R.ADAMW_HP
    s, _, _ = R.sumsq_ref([(inp["g"], None)])
    st, ctl, worst = State(inp), Ctl(), {}
    for step in (1, 2):
        clipped_step(st, inp["g"], None, gu, R.f32(0.3 * math.sqrt(s)), 0, step, ctl, hp, worst, f"u{gu}s{step}")
    assert all(v <= 1.0 for v in worst.values()), worst
    before = st.host()                                         # id 2 for every element: nothing moves
    g_dev = inp["g"].to(DEV)
    run_step(st, g_dev, None, 2, ctl, hp)
    assert all(torch.equal(bits(before[k]), bits(st.host()[k])) for k in "pmv")


def test_refusals_return_their_code_and_write_nothing():
    _lib, lib = libs()
    n = 64
    inp = {k: v[:n].clone() for k, v in R.adamw_inputs(256, seed=2).items()}
    st, ctl = State(inp), Ctl(skipped=3, norm_max=0.25)
    g = torch.rand(n + 4, device=DEV)
    grp = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ctl_img, part_img, st_img = ctl.buf.clone(), bits(ctl.part).clone(), {k: bits(v).clone() for k, v in st.full.items()}

    def segs(*ns, ptr=g.data_ptr()):
        a = (_lib.GradSeg * max(len(ns), 1))()
        for k, m in enumerate(ns):
            a[k] = _lib.GradSeg(ptr, None, m)
        return a

    def gn(s=None, nseg=1, max_norm=1.0, step=1, part=ctl.part_ptr, c=ctl.ptr):
        return lib.hsimae_grad_norm(segs(n) if s is None else s, nseg, max_norm, 1, step, B1, B2, part, c, stream())
    assert gn(nseg=0) == EDIMS and gn(s=segs(*([4] * 9)), nseg=9) == EDIMS and gn(nseg=-1) == EDIMS
    assert gn(s=segs(n, -1), nseg=2) == EDIMS and gn(step=0) == EDIMS
    assert gn(c=None) == EDIMS and gn(part=None) == EDIMS
    assert gn(max_norm=0.0) == EDIMS and gn(max_norm=-2.0) == EDIMS and gn(max_norm=NAN) == EDIMS
    assert gn(s=segs(n, ptr=None)) == ENULL and gn(s=segs(n, ptr=g.data_ptr() + 2)) == EALIGN
    assert gn(part=ctl.part_ptr + 4) == EALIGN and gn(c=ctl.ptr + 4) == EALIGN
    assert lib.hsimae_grad_norm(None, 1, 1.0, 1, 1, B1, B2, ctl.part_ptr, ctl.ptr, stream()) == ENULL

    def step(p=st.ptr("p"), gp=g.data_ptr(), m=st.ptr("m"), v=st.ptr("v"), group=None, gu=0, cnt=n, c=ctl.ptr):
        return lib.hsimae_adamw_step_ctl(p, gp, m, v, group, gu, cnt, 1e-3, B1, B2, 1e-8, 0.05, c, stream())
    assert step(cnt=-1) == EDIMS and step(gu=3) == EDIMS and step(gu=-1) == EDIMS
    assert step(p=None) == ENULL and step(gp=None) == ENULL and step(m=None) == ENULL and step(v=None) == ENULL and step(c=None) == ENULL
    assert step(p=st.ptr("p") + 2) == EALIGN and step(c=ctl.ptr + 4) == EALIGN
    assert step(cnt=0) == OK and step(gu=2) == OK and step(group=grp.data_ptr(), gu=7, cnt=0) == OK
    torch.cuda.synchronize()
    assert torch.equal(ctl.buf, ctl_img) and torch.equal(bits(ctl.part), part_img)
    assert all(torch.equal(bits(v), st_img[k]) for k, v in st.full.items())


# ------------------------------------------------------------------------------------------------ FusedAdamW
def tiny_hsimae(state=None):
    from hsimae_amd import HSIMAE
    from oracle import hsimae_oracle as O
    cfg = O.OracleConfig(bands=48)
    state = O.init_state(cfg, seed=9, std=0.02) if state is None else state
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=cfg.bands, b_patch_size=8, embed_dim=cfg.embed_dim,
                   depth=cfg.depth, num_heads=cfg.num_heads, s_depth=cfg.s_depth, decoder_embed_dim=cfg.decoder_embed_dim,
                   decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads, norm_pix_loss=cfg.norm_pix_loss,
                   trunc_init=True)
    m.load_state_dict(state)
    return m.to(DEV), state


def hsimae_batch(seed=31):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(16, 1, 48, 9, 9, generator=g).to(DEV)
    return x, (torch.rand(16, 6, generator=g), torch.rand(16, 9, generator=g))


def fp64_grad_norm(params):
    gs = [p.grad for p in params if p.grad is not None]
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs)), sum(g.numel() for g in gs)


def test_fused_adamw_clipped_matches_clip_grad_norm_and_torch_adamw():
    """Identical gradients in two tiny HSIMAE; clip_grad_norm_ + torch.optim.AdamW (the reference's two groups) on one,
    FusedAdamW(max_grad_norm = half the measured norm) on the other: after one step max |delta flat| <= 1e-6."""
    from hsimae_amd import FusedAdamW
    mc, state = tiny_hsimae()
    md, _ = tiny_hsimae(state)
    x, noise = hsimae_batch()
    for m_ in (mc, md):
        m_(x, 0.75, noise=noise, grid=(2, 7))[0].backward()
    md._flat_grad.copy_(mc._flat_grad)
    measured, _ = fp64_grad_norm(list(mc.parameters()))
    max_norm = 0.5 * measured
    nd = ["bias", "norm"]
    groups = [{"params": [p for n_, p in mc.named_parameters() if not any(k in n_ for k in nd)], "weight_decay": 5e-2},
              {"params": [p for n_, p in mc.named_parameters() if any(k in n_ for k in nd)], "weight_decay": 0.0}]
    ref = torch.optim.AdamW(groups, lr=5e-3, weight_decay=5e-2, betas=(0.9, 0.95))
    g_before = md._flat_grad.clone()
    t_norm = float(torch.nn.utils.clip_grad_norm_([p for p in mc.parameters() if p.grad is not None], max_norm))
    ref.step()
    fused = FusedAdamW(md, lr=5e-3, weight_decay=5e-2, betas=(0.9, 0.95), max_grad_norm=max_norm)
    fused.step()
    torch.cuda.synchronize()
    delta = float((mc._flat - md._flat).abs().max())
    norm, coef = float(fused.grad_norm), float(fused.clip_coef)
    print(f"[clip fused] norm {norm:.6f} (torch {t_norm:.6f}, fp64 {measured:.6f}), coef {coef:.6f}, max |delta flat| {delta:.3g}")
    assert delta <= 1e-6
    assert abs(norm - t_norm) <= 1e-6 * t_norm
    assert 0.49 < coef < 0.51 and int(fused.skipped_steps) == 0
    assert torch.equal(bits(md._flat_grad), bits(g_before)), ".grad was modified"
    assert set(fused.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "param_groups", "extra", "skipped", "outside_exp_avg",
                                       "outside_exp_avg_sq"}
    assert set(FusedAdamW(md, lr=5e-3).state_dict()) == {"step", "exp_avg", "exp_avg_sq", "param_groups", "extra"}


def test_clipped_step_issues_no_torch_op_and_no_host_wait():
    """After the first step (which allocates the control block) the clipped step() of an HSIMAE is three library launches and no
    ATen op at all -- so no _local_scalar_dense, no copy to the host -- also with torch's sync debug mode set to "error"."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from hsimae_amd import FusedAdamW

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    m, _ = tiny_hsimae()
    x, noise = hsimae_batch()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=5e-2, betas=(0.9, 0.95), max_grad_norm=1.0, skip_nonfinite=True)
    for k in range(2):
        opt.zero_grad()
        m(x, 0.75, noise=noise, grid=(2, 7))[0].backward()
        if k == 0:
            opt.step()
            continue
        before = m._flat.clone()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with Count() as c:
                opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        moving = [o for o in c.ops if "_local_scalar_dense" in o or "_to_copy" in o or "copy_" in o or "item" in o]
        assert not moving, moving
        assert c.ops == [], c.ops[:8]
        assert not torch.equal(before, m._flat) and float(opt.grad_norm) > 0


def tiny_dualvit():
    from hsimae_amd import DualViT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = DualViT(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=64, depth=4, s_depth=2,
                    num_heads=4, num_class=4, trunc_init=True, drop_path=0.0, decoder_embed_dim=32, decoder_depth=1,
                    decoder_num_heads=4, norm_pix_loss=True)
    with torch.no_grad():
        m.cls_head.weight.normal_(0, 0.5)
    return m.to(DEV).train()


def dualvit_backward(m, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(16, 1, 32, 9, 9, generator=g).to(DEV)
    xu = torch.rand(16, 1, 32, 9, 9, generator=g).to(DEV)
    y = torch.tensor([0, 1, 2, 3, 1, 0, 2, 3, 3, 1, 0, 2, 1, 2, 3, 1], device=DEV)
    torch.manual_seed(seed)
    loss_rec, _, _, out = m(x, xu, mask_ratio=0.5)
    (5 * loss_rec + torch.nn.functional.cross_entropy(out, y, ignore_index=0)).backward()


def test_dualvit_norm_covers_the_head_and_a_nan_in_the_head_skips_everything():
    from hsimae_amd import FusedAdamW
    m = tiny_dualvit()
    opt = FusedAdamW(m, lr=1e-3, weight_decay=5e-3, max_grad_norm=INF, skip_nonfinite=True)
    assert opt._extra is None and len(opt._outside) == 2       # no host-side optimizer for the head in this mode
    opt.zero_grad()
    dualvit_backward(m, 1)
    assert m.cls_head.weight.grad is not None and m.cls_head.bias.grad is not None
    norm64, n = fp64_grad_norm(list(m.parameters()))
    head64, _ = fp64_grad_norm([m.cls_head.weight, m.cls_head.bias])
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    ref = R.ctl_ref(norm64 ** 2, n, INF, 1, 1, 0, 0.9, 0.999)
    r = ref["norm"].ratio(opt.grad_norm.double().cpu())
    print(f"[clip dualvit] norm {float(opt.grad_norm):.6f}, fp64 {norm64:.6f} (head alone {head64:.6f}), err / bound {r:.3f}")
    assert r <= 1.0
    # the head is a visible part of it: the norm without the head lies outside the bound
    assert abs(math.sqrt(norm64 ** 2 - head64 ** 2) - norm64) > 4 * float(ref["norm"].bound())
    assert float(opt.clip_coef) == 1.0 and int(opt.skipped_steps) == 0
    moved = [k for k, p in m.named_parameters() if p.grad is not None and not torch.equal(p.detach(), before[k])]
    assert "cls_head.weight" in moved and "cls_head.bias" in moved and len(moved) > 50
    # a NaN in the head's bias gradient: nothing moves anywhere
    opt.zero_grad()
    dualvit_backward(m, 2)
    m.cls_head.bias.grad[1] = NAN
    before = {k: bits(p.detach()).clone() for k, p in m.named_parameters()}
    moments = [bits(t).clone() for t in (opt.exp_avg, opt.exp_avg_sq, *opt._out_m, *opt._out_v)]
    opt.step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.equal(bits(p.detach()), before[k]), f"{k} moved in a skipped step"
    for t, im in zip((opt.exp_avg, opt.exp_avg_sq, *opt._out_m, *opt._out_v), moments):
        assert torch.equal(bits(t), im)
    assert int(opt.skipped_steps) == 1 and math.isnan(float(opt.grad_norm))


def test_state_dict_after_a_skipped_step_resumes_bit_for_bit():
    """Two identical deterministic models take a clean step and a skipped one; the second model then gets a FRESH optimizer
    loaded from the first one's state_dict (through torch.save, as checkpoint.save_resume writes it): step 3 is bit-identical."""
    from hsimae_amd import FusedAdamW
    ma, state = tiny_hsimae()
    mb, _ = tiny_hsimae(state)
    kw = dict(lr=5e-3, weight_decay=5e-2, betas=(0.9, 0.95), max_grad_norm=1e-3, skip_nonfinite=True)
    opts = []
    for m in (ma, mb):
        m.deterministic = True
        opt = FusedAdamW(m, **kw)
        for step in (1, 2):
            x, noise = hsimae_batch(40 + step)
            opt.zero_grad()
            m(x, 0.75, noise=noise, grid=(2, 7))[0].backward()
            if step == 2:
                m.blocks[0].mlp.w1.weight.grad.view(-1)[5] = NAN
            opt.step()
        opts.append(opt)
    torch.cuda.synchronize()
    assert torch.equal(bits(ma._flat), bits(mb._flat)) and int(opts[0].skipped_steps) == 1
    blob = io.BytesIO()
    torch.save(opts[0].state_dict(), blob)
    blob.seek(0)
    fresh = FusedAdamW(mb, **kw)
    fresh.load_state_dict(torch.load(blob, map_location=DEV))
    assert fresh.step_count == 2
    for m, opt in ((ma, opts[0]), (mb, fresh)):
        x, noise = hsimae_batch(43)
        opt.zero_grad()
        m(x, 0.75, noise=noise, grid=(2, 7))[0].backward()
        opt.step()
    torch.cuda.synchronize()
    assert int(fresh.skipped_steps) == 1 and float(fresh.clip_coef) < 1.0
    assert torch.equal(bits(ma._flat), bits(mb._flat))
    assert torch.equal(bits(opts[0].exp_avg), bits(fresh.exp_avg)) and torch.equal(bits(opts[0].exp_avg_sq), bits(fresh.exp_avg_sq))
    # a checkpoint written without the feature loads as before, into either kind of optimizer
    plain = FusedAdamW(ma, lr=5e-3)
    plain._bind()
    sd = copy.deepcopy(plain.state_dict())
    FusedAdamW(ma, lr=5e-3).load_state_dict(sd)
    late = FusedAdamW(ma, **kw)
    late.load_state_dict(sd)
    assert int(late.skipped_steps) == 0


# ------------------------------------------------------------------------------------------------ the loop
def toy_set():
    """The toy set of tests/test_gpu_cls.py, halved."""
    rng = np.random.default_rng(0)
    n_lab, n_unl, bands, classes = 48, 64, 32, 3
    gt = np.tile(np.arange(1, classes + 1), n_lab // classes)
    ramp = np.linspace(0, 1, bands, dtype=np.float32)

    def cube(c):
        spectrum = 0.25 + 0.2 * c * ramp if c % 2 else 0.75 - 0.2 * c * ramp
        return np.clip(spectrum[None, None, :] + 0.05 * rng.standard_normal((9, 9, bands)).astype(np.float32), 0, 1)

    data_list = [cube(int(c)) for c in gt]
    unlabeled = [cube(int(rng.integers(1, classes + 1))) for _ in range(n_unl)]
    return data_list, list(range(n_lab)), unlabeled, gt


LOOP_KW = dict(lr=2e-3, wd=5e-3, depth=4, dim=64, dec_depth=1, dec_dim=32, s_depth=2, epochs=2, mask_ratio=0.5, lamda=5, batch_size=16)


def run_loop(tmp, **kw):
    import random
    from hsimae_amd import dual_branch_finetuning
    lines = []
    random.seed(0); np.random.seed(0); torch.manual_seed(0)    # the model's initialisation and the split draw from these
    with contextlib.redirect_stdout(io.StringIO()):
        out = dual_branch_finetuning(*toy_set(), str(tmp), "ft.pkl", log=lambda *a: lines.append(" ".join(map(str, a))), **LOOP_KW, **kw)
    return out, lines


def loop_record(out):
    val_value, tr, va = out
    return dict(val=[np.asarray(v, dtype=np.float64).reshape(-1).tolist() for v in val_value], train_loss=list(tr), val_loss=list(va))


def test_finetuning_loop_logs_the_norm_and_the_skip_count(tmp_path):
    import re
    out, lines = run_loop(tmp_path, max_grad_norm=1.0, skip_nonfinite=True)
    logged = [re.search(r"largest gradient norm (\S+), (\d+) steps skipped", ln) for ln in lines]
    logged = [m for m in logged if m]
    assert len(logged) == 2, lines
    for m in logged:
        assert math.isfinite(float(m.group(1))) and float(m.group(1)) > 0 and int(m.group(2)) == 0
    assert len(out[1]) == 2 and all(math.isfinite(v) for v in out[1] + out[2])


def test_finetuning_loop_without_the_arguments_is_the_loop_as_it_was(tmp_path, monkeypatch):
    """The default path is guarded by values the loop returned BEFORE the feature existed (tests/golden/clip_loop_default.json:
    this toy set, HSIMAE_DETERMINISTIC=1): the same losses and scores, to the last bit, and no new log line."""
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    out, lines = run_loop(tmp_path)
    assert not any("gradient norm" in ln for ln in lines)
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = loop_record(out)
    print(f"[clip loop default] train loss {got['train_loss']}, recorded {want['train_loss']}")
    assert got == want
