"""The grouped AdamW step (hsimae_adamw_step_groups, csrc/clip.hip) on the GPU against the fp64 restatement of tests/groups_ref.py:
through the C ABI at every size, alignment, table size and control-block mode, against the entry point it replaces, the refusals,
and the Python layer: FusedAdamW(layer_decay=, freeze=) and hand-written param_groups on HSIMAE and DualViT, the state_dict and
the fine-tuning loop."""
import contextlib
import ctypes as C
import io
import math
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import groups_ref as G  # noqa: E402
import clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
GUARD = 64
OK, EDIMS, EALIGN, ENULL = 0, -1, -3, -4
HP = G.ADAMW_HP
SMALL_N = [0, 1, 3, 5, G.STEP_N]
MODES = ["noctl", "clipped", "unclipped", "apply0"]
T_STEP = 2                                                     # the step of the bias corrections in the ABI tests


@pytest.fixture(autouse=True)
def rng_state_left_as_found():
    """These tests seed the global generators (model initialisation, the loop's split); tests that run after this file and draw
    from them without seeding must find them as they would have without it."""
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


# ------------------------------------------------------------------------------------------------ device state between canaries
class Arrays:
    """p, g, m, v (NaN canaries) and the ids (canary 0: a live id, so a read past the end would step a canary) in device memory.
    off: floats by which every fp32 array starts behind a 256-byte boundary (1: the scalar path)."""

    def __init__(self, inp, off=0, with_ids=True):
        n = inp["p"].numel()
        self.n, self.off = n, off
        self.full = {k: torch.full((n + 2 * GUARD + off,), NAN, device=DEV) for k in "pgmv"}
        for k in "pgmv":
            self.full[k][GUARD + off:GUARD + off + n] = inp[k].to(DEV)
        self.ids = None
        if with_ids:
            self.ids = torch.zeros(n + 2 * GUARD, dtype=torch.uint8, device=DEV)
            self.ids[GUARD:GUARD + n] = inp["ids"].to(DEV)
        self.image = {k: bits(v).clone() for k, v in self.full.items()}

    def ptr(self, k):
        return self.full[k].data_ptr() + 4 * (GUARD + self.off)

    def ids_ptr(self):
        return None if self.ids is None else self.ids.data_ptr() + GUARD

    def host(self):
        lo = GUARD + self.off
        return {k: self.full[k][lo:lo + self.n].cpu() for k in "pmv"}

    def frame_intact(self):
        lo = GUARD + self.off
        for k, f in self.full.items():
            im = self.image[k]
            if not (torch.equal(bits(f)[:lo], im[:lo]) and torch.equal(bits(f)[lo + self.n:], im[lo + self.n:])):
                return False
        return torch.equal(bits(self.full["g"]), self.image["g"])              # the gradient is never written

    def unchanged(self):
        return all(torch.equal(bits(f), self.image[k]) for k, f in self.full.items())


def ctl_block(mode, hp=HP, t=T_STEP):
    """(device tensor or None, pointer or None, coef, apply): a control block as hsimae_grad_norm would have left it."""
    if mode == "noctl":
        return None, None, 1.0, 1
    _lib, _ = libs()
    coef = R.f32(0.3) if mode == "clipped" else 1.0
    apply_ = 0 if mode == "apply0" else 1
    i1, i2 = R.bias_corrections(t, hp["b1"], hp["b2"])
    c = _lib.ClipCtl(sumsq=1.0, norm=1.0, coef=coef, finite=1, apply=apply_, skipped=0, inv_bc1=i1, inv_sqrt_bc2=i2, norm_max=1.0)
    host = torch.full((C.sizeof(c) + 2 * GUARD,), 0xA5, dtype=torch.uint8)
    host[GUARD:GUARD + C.sizeof(c)] = torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8)
    buf = host.to(DEV)
    return buf, buf.data_ptr() + GUARD, coef, apply_


def c_table(table):
    _lib, _ = libs()
    return (_lib.AdamWGroup * len(table))(*[_lib.AdamWGroup(a, b) for a, b in table])


def call_groups(arr, table, gu, ctl_ptr, hp=HP, step=T_STEP, ids=True):
    _, lib = libs()
    return lib.hsimae_adamw_step_groups(arr.ptr("p"), arr.ptr("g"), arr.ptr("m"), arr.ptr("v"), arr.ids_ptr() if ids else None, gu,
                                        arr.n, c_table(table), len(table), hp["b1"], hp["b2"], hp["eps"], step, ctl_ptr, stream())


def check_step(inp, table, mode, off, tag, worst, uniform=None):
    """One launch on fresh arrays, twice; the result against the restatement, everything else against its image."""
    ids_h = inp["ids"] if uniform is None else torch.full((inp["p"].numel(),), uniform, dtype=torch.uint8)
    runs = []
    for _ in range(2):
        arr = Arrays(inp, off, with_ids=uniform is None)
        buf, ctl_ptr, coef, apply_ = ctl_block(mode)
        ctl_img = None if buf is None else buf.clone()
        assert call_groups(arr, table, 0 if uniform is None else uniform, ctl_ptr) == OK, tag
        torch.cuda.synchronize()
        assert arr.frame_intact(), f"{tag}: a canary or the gradient was written"
        assert buf is None or torch.equal(buf, ctl_img), f"{tag}: the control block was written"
        runs.append(arr)
    a, b = runs
    assert all(torch.equal(bits(a.full[k]), bits(b.full[k])) for k in "pmv"), f"{tag}: two runs differ"
    if not apply_:
        assert a.unchanged(), f"{tag}: apply = 0 wrote"
    got = a.host()
    ref = G.adamw_groups_ref(inp["p"], inp["g"], inp["m"], inp["v"], ids_h, table, coef, apply_, T_STEP, HP["b1"], HP["b2"], HP["eps"])
    dead = ~G.live_mask(ids_h, len(table))
    for k in "pmv":
        assert torch.equal(bits(got[k][dead]), bits(inp[k][dead])), f"{tag} {k}: an element that must not be touched changed"
        if a.n:
            worst[f"{k}@{tag}"] = ref[k].ratio(got[k])
    if apply_ and a.n and bool((~dead).any()):
        assert not torch.equal(bits(got["m"]), bits(inp["m"])), f"{tag}: nothing moved"
    return got


# ------------------------------------------------------------------------------------------------ 1. the C ABI against the bound
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ngroups", [1, 3, 29, 64])
def test_step_groups_every_small_size_alignment_and_mode(ngroups, mode):
    """n in {0, 1, 3, 5, 4 (256 + 37) + 3} x {16-byte aligned, one float behind}: ids per element over the table with runs of one
    id, ids 2 and ids >= ngroups planted, NaN under every untouched element, table[2] = (-1, NaN)."""
    assert G.STEP_N == 4 * (256 + 37) + 3 == 1175
    table, worst = G.table_for(ngroups), {}
    for n in SMALL_N:
        inp = G.step_inputs(n, ngroups, 20 + n % 7)
        for off in (0, 1):
            check_step(inp, table, mode, off, f"n{n}-off{off}", worst)
    print(f"[groups abi ng{ngroups} {mode}] worst err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items() if v > 0.5))
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}


@pytest.mark.parametrize("ngroups,mode,off", [(29, "clipped", 0), (64, "noctl", 0), (3, "unclipped", 1)])
def test_step_groups_where_the_stride_loop_runs_twice(ngroups, mode, off):
    """n = 4 * 256 * 2048 + 4 * 37 + 3: one full pass of the capped grid (2048 workgroups), a partial second one, a tail of 3."""
    assert G.N_STRIDE == 4 * 256 * 2048 + 4 * 37 + 3
    worst = {}
    check_step(G.step_inputs(G.N_STRIDE, ngroups, 3), G.table_for(ngroups), mode, off, f"stride-ng{ngroups}-{mode}-off{off}", worst)
    print("[groups abi stride] worst err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("ngroups", [1, 3, 29, 64])
def test_step_groups_with_each_uniform_id(ngroups):
    """group = NULL: 17 elements (cls_head.bias with 17 classes: four float4 and one more) with every id of the table in turn,
    with and without a control block; the uniform id 2 launches nothing."""
    table, worst = G.table_for(ngroups), {}
    inp = G.step_inputs(17, ngroups, 9)
    inp["g"] = torch.full_like(inp["g"], 0.02) + 0.01 * torch.arange(17)
    for gu in range(ngroups):
        for mode in ("noctl", "clipped"):
            got = check_step(inp, table, mode, gu % 2, f"u{gu}-{mode}", worst, uniform=gu)
            assert (gu == 2) == all(torch.equal(bits(got[k]), bits(inp[k])) for k in "pmv")
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}


# ------------------------------------------------------------------------------------------------ 2. the entry point it replaces
def test_two_entry_table_is_hsimae_adamw_step_ctl_bit_for_bit_and_hsimae_adamw_step_within_the_bound():
    _, lib = libs()
    table = [(HP["lr"], HP["wd"]), (HP["lr"], 0.0)]
    for n in SMALL_N + [G.N_STRIDE]:
        inp = G.step_inputs(n, 2, 30 + n % 5)
        inp["ids"] = torch.randint(0, 3, (n,), generator=G.gen(n), dtype=torch.uint8)
        inp["g"] = torch.where(inp["ids"] == 2, torch.full_like(inp["g"], NAN), torch.where(inp["g"].isnan(), torch.full_like(inp["g"], 0.02), inp["g"]))
        for off in (0, 1):
            for mode in ("clipped", "unclipped", "apply0"):
                if n == G.N_STRIDE and (off, mode) not in ((0, "clipped"), (1, "unclipped")):
                    continue
                new, old = Arrays(inp, off), Arrays(inp, off)
                buf, ctl_ptr, _, _ = ctl_block(mode)
                assert call_groups(new, table, 0, ctl_ptr) == OK
                assert lib.hsimae_adamw_step_ctl(old.ptr("p"), old.ptr("g"), old.ptr("m"), old.ptr("v"), old.ids_ptr(), 0, n, HP["lr"],
                                                 HP["b1"], HP["b2"], HP["eps"], HP["wd"], ctl_ptr, stream()) == OK
                torch.cuda.synchronize()
                assert all(torch.equal(bits(new.full[k]), bits(old.full[k])) for k in "pgmv"), (n, off, mode)
    # hsimae_adamw_step: n a multiple of 4, no control block; both results lie within the bound of the one restatement
    for n in (4, 1172, G.N_STRIDE - 3):
        inp = G.step_inputs(n, 2, 41)
        inp["ids"] = torch.randint(0, 3, (n,), generator=G.gen(n), dtype=torch.uint8)
        inp["g"] = torch.where(inp["ids"] == 2, torch.full_like(inp["g"], NAN), torch.where(inp["g"].isnan(), torch.full_like(inp["g"], 0.02), inp["g"]))
        new, old = Arrays(inp), Arrays(inp)
        assert call_groups(new, table, 0, None, step=3) == OK
        assert lib.hsimae_adamw_step(old.ptr("p"), old.ptr("g"), old.ptr("m"), old.ptr("v"), old.ids_ptr(), n, HP["lr"], HP["b1"],
                                     HP["b2"], HP["eps"], HP["wd"], 3, stream()) == OK
        torch.cuda.synchronize()
        ref = G.adamw_groups_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["ids"], table, 1.0, 1, 3, HP["b1"], HP["b2"], HP["eps"])
        gn, go = new.host(), old.host()
        differ = {k: int((bits(gn[k]) != bits(go[k])).sum()) for k in "pmv"}
        ratios = {k: (ref[k].ratio(gn[k]), ref[k].ratio(go[k])) for k in "pmv"}
        print(f"[groups vs adamw_step n {n}] elements that differ {differ}; err / bound (grouped, plain) {ratios}")
        assert all(a <= 1.0 and b <= 1.0 for a, b in ratios.values()), ratios
        assert new.frame_intact() and old.frame_intact()


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_return_their_code_and_write_nothing():
    _lib, lib = libs()
    n = 64
    inp = G.step_inputs(n, 3, 2)
    inp["g"] = torch.full_like(inp["g"], 0.02)
    arr = Arrays(inp)
    buf, ctl_ptr, _, _ = ctl_block("clipped")
    ctl_img = buf.clone()
    good = [(1e-3, 0.05), (1e-3, 0.0), (-1.0, NAN)]

    def step(p=arr.ptr("p"), g=arr.ptr("g"), m=arr.ptr("m"), v=arr.ptr("v"), group=arr.ids_ptr(), gu=0, cnt=n, table=good, ng=None,
             st=1, c=None):
        t = None if table is None else c_table(table)
        ng = (len(table) if table is not None else 2) if ng is None else ng
        return lib.hsimae_adamw_step_groups(p, g, m, v, group, gu, cnt, t, ng, 0.9, 0.95, 1e-8, st, c, stream())
    assert step(cnt=-1) == EDIMS
    assert step(ng=0) == EDIMS and step(ng=-1) == EDIMS and step(table=good + [(1e-3, 0.0)] * 62, ng=65) == EDIMS
    assert step(group=None, gu=-1) == EDIMS and step(group=None, gu=3) == EDIMS and step(group=None, gu=64) == EDIMS
    assert step(st=0) == EDIMS and step(st=-5) == EDIMS and step(st=0, c=ctl_ptr, cnt=0) == OK     # with ctl the step is ignored
    for bad in ([(-1e-3, 0.0)], [(1e-3, -0.5)], [(NAN, 0.0)], [(1e-3, NAN)], good + [(1e-3, 0.0), (-0.0 - 1e-9, 0.0)]):
        assert step(table=bad) == EDIMS, bad
    assert step(p=None) == ENULL and step(g=None) == ENULL and step(m=None) == ENULL and step(v=None) == ENULL
    assert step(table=None) == ENULL
    assert step(p=arr.ptr("p") + 2) == EALIGN and step(g=arr.ptr("g") + 1) == EALIGN and step(m=arr.ptr("m") + 2) == EALIGN
    assert step(v=arr.ptr("v") + 3) == EALIGN and step(c=ctl_ptr + 4) == EALIGN
    assert step(cnt=0) == OK and step(cnt=0, table=None) == OK and step(group=None, gu=2) == OK
    assert step(group=None, gu=2, table=[(1e-3, 0.0)]) == OK                  # id 2 is frozen in a table of any size
    torch.cuda.synchronize()
    assert arr.unchanged() and torch.equal(buf, ctl_img)


# ------------------------------------------------------------------------------------------------ models
MODEL_KW = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=64, depth=4, s_depth=2, num_heads=4,
                decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True, trunc_init=True)
DEPTH, S_DEPTH = 4, 2
OPT_KW = dict(lr=2e-3, weight_decay=5e-3, betas=(0.9, 0.95))
_STATE = {}


def tiny(kind, same_as=None):
    """The shapes of test_gpu_clip.LOOP_KW: depth 4, dim 64, s_depth 2, decoder 1 x 32.  The initial state is drawn once per kind
    and shared: every model of a kind starts from the same parameters."""
    from hsimae_amd import HSIMAE, DualViT
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIMAE(**MODEL_KW) if kind == "HSIMAE" else DualViT(num_class=4, drop_path=0.0, **MODEL_KW)
    if kind == "DualViT":
        with torch.no_grad():
            m.cls_head.weight.normal_(0, 0.5)
    if kind not in _STATE:
        _STATE[kind] = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(_STATE[kind])
    return m.to(DEV).train()


def backward(m, seed=1):
    """One real forward / backward on 16 cubes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(16, 1, 32, 9, 9, generator=g).to(DEV)
    random.seed(seed); torch.manual_seed(seed)
    if hasattr(m, "cls_head"):
        xu = torch.rand(16, 1, 32, 9, 9, generator=g).to(DEV)
        y = torch.tensor([0, 1, 2, 3, 1, 0, 2, 3, 3, 1, 0, 2, 1, 2, 3, 1], device=DEV)
        loss_rec, _, _, out = m(x, xu, mask_ratio=0.5)
        (5 * loss_rec + torch.nn.functional.cross_entropy(out, y, ignore_index=0)).backward()
    else:
        m(x, 0.5)[0].backward()


def everything(m):
    """Every parameter as one fp32 host vector: the flat buffer, then the parameters outside it."""
    names = [n for n, _ in m.named_parameters()]
    outside = [p for n, p in m.named_parameters() if n.startswith("cls_head.")]
    return names, outside


def gather(m, outside, what="p"):
    flat = (m._flat if what == "p" else m._flat_grad).detach().cpu()
    rest = [(p.detach() if what == "p" else p.grad).reshape(-1).cpu() for p in outside]
    return torch.cat([flat] + rest)


def element_ids(m, ids_by_name):
    """One id per element of gather()'s vector, from the test's own table."""
    flat_names = [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
    ids = torch.full((m._flat.numel(),), 2, dtype=torch.uint8)
    for n, off, size in zip(flat_names, m._offs, m._sizes):
        ids[off:off + size] = ids_by_name[n]
    rest = [torch.full((p.numel(),), ids_by_name[n], dtype=torch.uint8) for n, p in m.named_parameters() if n.startswith("cls_head.")]
    return torch.cat([ids] + rest)


class TorchGroups:
    """torch.optim.AdamW in fp64 on copies: one torch group per table entry, holding the elements that carry its id."""

    def __init__(self, p0, ids, ngroups, betas, eps):
        self.idx = {k: torch.nonzero(ids == k).reshape(-1) for k in range(ngroups) if k != 2}
        self.idx = {k: i for k, i in self.idx.items() if i.numel()}
        self.params = {k: torch.nn.Parameter(p0[i].double()) for k, i in self.idx.items()}
        self.opt = torch.optim.AdamW([dict(params=[self.params[k]]) for k in self.idx], lr=1.0, betas=betas, eps=eps)
        self.n = p0.numel()
        self.p0 = p0.double()

    def state(self):
        """(p, m, v) as whole fp64 vectors (the elements no group holds keep their first value, moments 0)."""
        p, m, v = self.p0.clone(), torch.zeros(self.n, dtype=torch.float64), torch.zeros(self.n, dtype=torch.float64)
        for k, i in self.idx.items():
            st = self.opt.state.get(self.params[k], {})
            p[i] = self.params[k].detach()
            if "exp_avg" in st:
                m[i], v[i] = st["exp_avg"], st["exp_avg_sq"]
        return p, m, v

    def step(self, g, table, coef=1.0):
        for grp, k in zip(self.opt.param_groups, self.idx):
            grp["lr"], grp["weight_decay"] = table[k]
            self.params[k].grad = g[self.idx[k]].double() * coef
        self.opt.step()


def frozen_names(m, freeze=()):
    return tuple(n for n, p in m.named_parameters() if not p.requires_grad) + tuple(freeze)


def run_against_torch(kind, clip):
    """3 steps of FusedAdamW(layer_decay = 0.75) with CosineLRScheduler stepping between them, every step fed the gradients of one
    real backward; torch.optim.AdamW in fp64 with the test's own groups beside it.  Returns the worst |p - p64| / summed bound."""
    from hsimae_amd import FusedAdamW, CosineLRScheduler
    m = tiny(kind)
    backward(m)
    names, outside = everything(m)
    if clip == "half":                                         # half the norm of these very gradients: the clip bites
        clip = 0.5 * math.sqrt(float((gather(m, outside, "g").nan_to_num().double() ** 2).sum()))
    kw = dict(max_grad_norm=clip, skip_nonfinite=True) if clip else {}
    opt = FusedAdamW(m, layer_decay=0.75, **OPT_KW, **kw)
    sched = CosineLRScheduler(opt, t_initial=10, lr_min=2e-5, warmup_t=2, warmup_lr_init=2e-4)
    by_name, unit, _ = G.layer_table(names, DEPTH, S_DEPTH, 0.75, 1.0, OPT_KW["weight_decay"], frozen=frozen_names(m))
    ids = element_ids(m, by_name)
    ng = len(unit)                                             # unit: (lr_scale, weight_decay) per table id
    assert ng == 2 * (DEPTH + 2) + 1 == opt._ngroups
    g = gather(m, outside, "g")
    live = G.live_mask(ids, ng)
    assert bool(torch.isfinite(g[live]).all()) and float(g.abs().max()) > 0
    tg = TorchGroups(gather(m, outside), ids, ng, OPT_KW["betas"], 1e-8)
    norm = math.sqrt(float((g[live].double() ** 2).sum()))
    total = torch.zeros(ids.numel(), dtype=torch.float64)
    lrs, coef = [], 1.0
    for t in (1, 2, 3):
        base = opt.param_groups[0]["lr"]
        assert all(gr["lr"] == base for gr in opt.param_groups)
        lrs.append(base)
        table = [(base * scale, wd) for scale, wd in unit]
        opt.step()
        if clip:                                               # the fp32 coefficient the step read
            coef = float(opt.clip_coef)
            assert abs(float(opt.grad_norm) - norm) <= 1e-5 * norm and abs(coef - min(1.0, clip / (norm + 1e-6))) <= 1e-6
        p64, m64, v64 = tg.state()
        step_ref = G.adamw_groups_ref(p64, g, m64, v64, ids, [(R.f32(a), R.f32(b)) for a, b in table], coef, 1, t,
                                      *OPT_KW["betas"], 1e-8)
        total += step_ref["p"].bound()
        tg.step(g, table, coef)
        sched.step(t)
    assert len(set(lrs)) == 3, lrs                             # the schedule moved the rate between the steps
    torch.cuda.synchronize()
    got = gather(m, outside).double()
    p64, _, _ = tg.state()
    err = (got - p64).abs()
    assert torch.equal(got[~live], tg.p0[~live]), "a frozen element moved"
    assert bool((err[live] > 0).any()) and float((got - tg.p0).abs().max()) > 1e-5
    ratio = float((err[live] / total[live].clamp_min(1e-300)).max())
    return ratio, m, opt, outside


# ------------------------------------------------------------------------------------------------ 4. layer decay against torch
@pytest.mark.parametrize("kind", ["HSIMAE", "DualViT"])
def test_layer_decay_three_scheduled_steps_match_torch_adamw_in_fp64(kind):
    ratio, _, _, _ = run_against_torch(kind, clip=False)
    print(f"[groups layer_decay {kind}] worst |p - p64| / summed bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("max_norm", [1.0, "half"])
@pytest.mark.parametrize("kind", ["HSIMAE", "DualViT"])
def test_layer_decay_clipped_matches_torch_and_a_nan_gradient_skips_the_step(kind, max_norm):
    """max_grad_norm = 1.0 (these gradients' norm lies below it: measured, not clipped) and half their norm (clipped to it)."""
    ratio, m, opt, outside = run_against_torch(kind, clip=max_norm)
    print(f"[groups layer_decay clipped {kind} {max_norm}] coef {float(opt.clip_coef):.4f}, worst |p - p64| / summed bound {ratio:.3f}")
    assert ratio <= 1.0 and int(opt.skipped_steps) == 0
    assert max_norm != "half" or 0.49 < float(opt.clip_coef) < 0.51
    before = bits(gather(m, outside)).clone()
    moments = [bits(t).clone() for t in (opt.exp_avg, opt.exp_avg_sq, *opt._out_m, *opt._out_v)]
    m.blocks[0].mlp.w1.weight.grad.view(-1)[5] = NAN
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(gather(m, outside)), before), "a skipped step moved a parameter"
    for t, im in zip((opt.exp_avg, opt.exp_avg_sq, *opt._out_m, *opt._out_v), moments):
        assert torch.equal(bits(t), im)
    assert int(opt.skipped_steps) == 1


# ------------------------------------------------------------------------------------------------ 5. param_groups is honoured
class Spy:
    """Stands where _lib.load() stands and records which entry points are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("hsimae_"):
            return fn

        def wrapped(*a):
            self.calls.append(name)
            return fn(*a)
        return wrapped


@pytest.mark.parametrize("kind", ["HSIMAE", "DualViT"])
def test_param_groups_written_by_hand_are_honoured(kind, monkeypatch):
    """A default-built FusedAdamW with param_groups[1]["lr"] = 3 x group 0's: the parameters without decay move as torch's do
    with that rate (on the commit before this feature they were stepped with group 0's).  With the groups left equal the step is
    the one hsimae_adamw_step launch it always was, to the last bit."""
    from hsimae_amd import FusedAdamW, optim
    m, twin = tiny(kind), tiny(kind)
    backward(m); backward(twin)
    twin._flat_grad.copy_(m._flat_grad)                        # two backward passes differ in the order of their atomic sums
    for a, b in zip(everything(m)[1], everything(twin)[1]):
        b.grad.copy_(a.grad)
    assert torch.equal(bits(m._flat), bits(twin._flat))
    opt = FusedAdamW(m, **OPT_KW)
    opt.param_groups[1]["lr"] = 3 * opt.param_groups[0]["lr"]
    names, outside = everything(m)
    by_name, _, _ = G.layer_table(names, DEPTH, S_DEPTH, None, 1.0, 0.0, frozen=frozen_names(m))
    ids = element_ids(m, by_name)
    assert set(ids.tolist()) == {0, 1, 2}
    table = [(OPT_KW["lr"], OPT_KW["weight_decay"]), (3 * OPT_KW["lr"], 0.0)]
    g = gather(m, outside, "g")
    tg = TorchGroups(gather(m, outside), ids, 2, OPT_KW["betas"], 1e-8)
    p64, m64, v64 = tg.state()
    ref = G.adamw_groups_ref(p64, g, m64, v64, ids, [(R.f32(a), R.f32(b)) for a, b in table], 1.0, 1, 1, *OPT_KW["betas"], 1e-8)
    tg.step(g, table)
    spy = Spy(optim._lib.load())
    monkeypatch.setattr(optim._lib, "load", lambda: spy)
    opt.step()
    torch.cuda.synchronize()
    got, p64 = gather(m, outside).double(), tg.state()[0]
    err, bound = (got - p64).abs(), ref["p"].bound()
    for k in (0, 1):
        sel = ids == k
        print(f"[groups by hand {kind}] id {k}: worst |p - p64| / bound {float((err[sel] / bound[sel].clamp_min(1e-300)).max()):.3f}, "
              f"largest move {float((got - tg.p0)[sel].abs().max()):.3g}")
        assert bool((err[sel] <= bound[sel]).all()), k
    assert spy.calls == ["hsimae_adamw_step_groups"], spy.calls
    # the same step at group 0's rate for everyone lies far outside: the comparison sees the rate
    wrong = TorchGroups(tg.p0, ids, 2, OPT_KW["betas"], 1e-8)
    wrong.step(g, [table[0], (OPT_KW["lr"], 0.0)])
    sel = ids == 1
    assert float(((wrong.state()[0] - p64).abs()[sel] / bound[sel].clamp_min(1e-300)).max()) > 100
    # groups left equal: one hsimae_adamw_step launch, and the result of calling that entry point directly
    plain = FusedAdamW(twin, **OPT_KW)
    spy.calls.clear()
    want_p, want_m, want_v = twin._flat.clone(), torch.zeros_like(twin._flat), torch.zeros_like(twin._flat)
    plain.step()
    assert spy.calls == ["hsimae_adamw_step"], spy.calls
    monkeypatch.undo()
    plain._bind()
    _lib, lib = libs()
    _lib.check(lib.hsimae_adamw_step(want_p.data_ptr(), twin._flat_grad.data_ptr(), want_m.data_ptr(), want_v.data_ptr(),
                                     plain._group.data_ptr(), want_p.numel(), OPT_KW["lr"], 0.9, 0.95, 1e-8, OPT_KW["weight_decay"], 1,
                                     stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(want_p), bits(twin._flat)) and torch.equal(bits(want_m), bits(plain.exp_avg))
    assert torch.equal(bits(want_v), bits(plain.exp_avg_sq))


# ------------------------------------------------------------------------------------------------ 6. freeze
FROZEN = ("patch_embed", "blocks_1.0.", "blocks_2.0.")


@pytest.mark.parametrize("clip", [False, True])
def test_frozen_prefixes_and_their_moments_stay_bit_unchanged(clip):
    from hsimae_amd import FusedAdamW
    m = tiny("HSIMAE")
    kw = dict(max_grad_norm=INF) if clip else {}
    opt = FusedAdamW(m, freeze=FROZEN, **OPT_KW, **kw)
    before = None
    for step in (1, 2, 3):
        opt.zero_grad()
        backward(m, step)
        if before is None:
            before = {n: bits(p.detach()).clone() for n, p in m.named_parameters()}
        for prefix in FROZEN:                                  # the frozen layers do receive gradients: it is the step that leaves them
            assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for n, p in m.named_parameters() if n.startswith(prefix))
        opt.step()
    torch.cuda.synchronize()
    flat_names = [n for n, _ in m.named_parameters()]
    moved = 0
    for n, off, size in zip(flat_names, m._offs, m._sizes):
        p = dict(m.named_parameters())[n]
        if n.startswith(FROZEN):
            assert torch.equal(bits(p.detach()), before[n]), f"{n} moved"
            assert not bool(opt.exp_avg[off:off + size].any()) and not bool(opt.exp_avg_sq[off:off + size].any()), f"{n}: moments"
        elif p.requires_grad and n != "mask_token":
            moved += int(not torch.equal(bits(p.detach()), before[n]) and bool(opt.exp_avg_sq[off:off + size].any()))
    assert moved > 40                                          # (a key bias has no gradient at all: softmax does not see it)
    if clip:                                                   # the norm leaves the frozen gradients out
        rest = [p.grad for n, p in m.named_parameters() if p.grad is not None and not n.startswith(FROZEN) and n != "mask_token"]
        every = [p.grad for n, p in m.named_parameters() if p.grad is not None and n != "mask_token"]
        s, cnt = sum(float((g.double() ** 2).sum()) for g in rest), sum(g.numel() for g in rest)
        ref = R.ctl_ref(s, cnt, INF, 0, 3, 0, *OPT_KW["betas"])
        r = ref["norm"].ratio(opt.grad_norm.double().cpu())
        with_frozen = math.sqrt(sum(float((g.double() ** 2).sum()) for g in every))
        print(f"[groups freeze] norm {float(opt.grad_norm):.6f}, fp64 over the rest {math.sqrt(s):.6f} (with the frozen {with_frozen:.6f}), "
              f"err / bound {r:.3f}")
        assert r <= 1.0
        assert abs(with_frozen - math.sqrt(s)) > 4 * float(ref["norm"].bound())     # the frozen gradients are a visible part


@pytest.mark.parametrize("clip", [False, True])
def test_linear_probe_changes_only_the_head(clip):
    from hsimae_amd import FusedAdamW
    m = tiny("DualViT")
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if clip else {}
    everything_else = tuple(n for n, _ in m.named_parameters() if not n.startswith("cls_head."))
    opt = FusedAdamW(m, freeze=everything_else, **OPT_KW, **kw)
    opt.zero_grad()
    backward(m)
    before = {n: bits(p.detach()).clone() for n, p in m.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    changed = {n for n, p in m.named_parameters() if not torch.equal(bits(p.detach()), before[n])}
    assert changed == {"cls_head.weight", "cls_head.bias"}, changed
    assert not bool(opt.exp_avg.any()) and not bool(opt.exp_avg_sq.any())
    if clip:
        head = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in (m.cls_head.weight, m.cls_head.bias)))
        assert abs(float(opt.grad_norm) - head) <= 1e-5 * head


# ------------------------------------------------------------------------------------------------ 7. no ATen op, no host wait
def test_grouped_clipped_step_issues_no_torch_op_and_no_host_wait():
    from torch.utils._python_dispatch import TorchDispatchMode
    from hsimae_amd import FusedAdamW

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    m = tiny("HSIMAE")
    opt = FusedAdamW(m, layer_decay=0.75, freeze=("patch_embed",), max_grad_norm=1.0, skip_nonfinite=True, **OPT_KW)
    for k in range(2):
        opt.zero_grad()
        backward(m, k)
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
        assert c.ops == [], c.ops[:8]
        assert not torch.equal(before, m._flat) and float(opt.grad_norm) > 0


# ------------------------------------------------------------------------------------------------ 8. state_dict
def test_state_dict_resumes_a_layer_decay_run_bit_for_bit(monkeypatch):
    """2 steps, save, load into a fresh optimizer (and a fresh scheduler position), 2 more steps: bit-identical to 4 uninterrupted
    steps in deterministic mode.  A two-group checkpoint does not load into a layer_decay optimizer."""
    from hsimae_amd import FusedAdamW, CosineLRScheduler
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    kw = dict(layer_decay=0.75, **OPT_KW)

    def steps(m, opt, sched, which):
        for t in which:
            opt.zero_grad()
            backward(m, 50 + t)
            opt.step()
            sched.step(t)

    def schedule(opt):
        return CosineLRScheduler(opt, t_initial=8, lr_min=2e-5, warmup_t=2, warmup_lr_init=2e-4)
    ma, mb = tiny("HSIMAE"), tiny("HSIMAE")
    ma.deterministic = mb.deterministic = True
    oa = FusedAdamW(ma, **kw)
    sa = schedule(oa)
    steps(ma, oa, sa, (0, 1, 2, 3))
    ob = FusedAdamW(mb, **kw)
    sb = schedule(ob)
    steps(mb, ob, sb, (0, 1))
    blob = io.BytesIO()
    torch.save({"opt": ob.state_dict(), "sched": sb.state_dict()}, blob)
    blob.seek(0)
    sd = torch.load(blob, map_location=DEV)
    assert [g["lr_scale"] for g in sd["opt"]["param_groups"]] == [0.75 ** (j // 2) for j in range(12)]
    fresh = FusedAdamW(mb, **kw)
    fs = schedule(fresh)
    fresh.load_state_dict(sd["opt"])
    fs.load_state_dict(sd["sched"])
    assert fresh.step_count == 2 and fresh.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
    steps(mb, fresh, fs, (2, 3))
    torch.cuda.synchronize()
    assert torch.equal(bits(ma._flat), bits(mb._flat))
    assert torch.equal(bits(oa.exp_avg), bits(fresh.exp_avg)) and torch.equal(bits(oa.exp_avg_sq), bits(fresh.exp_avg_sq))
    two = FusedAdamW(mb, **OPT_KW)
    two._bind()
    with pytest.raises(ValueError, match=r"2 parameter groups.*12"):
        FusedAdamW(mb, **kw).load_state_dict(two.state_dict())


# ------------------------------------------------------------------------------------------------ 9. the loop
def test_finetuning_loop_with_layer_decay_logs_the_rate_range_and_writes_the_checkpoint(tmp_path):
    import test_gpu_clip as TC
    from hsimae_amd import dual_branch_finetuning
    lines = []
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        out = dual_branch_finetuning(*TC.toy_set(), str(tmp_path), "ft.pkl", log=lambda *a: lines.append(" ".join(map(str, a))),
                                     **TC.LOOP_KW, layer_decay=0.75, freeze=("patch_embed",))
    logged = [re.search(r"learning rate (\S+) \.\. (\S+) over (\d+) groups", ln) for ln in lines]
    logged = [h for h in logged if h]
    assert len(logged) == 2, lines
    for h in logged:
        lo, hi = float(h.group(1)), float(h.group(2))
        assert 0 < lo < hi and abs(lo / hi - 0.75 ** 4) < 1e-4 and int(h.group(3)) == 10     # layer 0 is frozen: layers 1 .. 5
    assert len(out[1]) == 2 and all(math.isfinite(v) for v in out[1] + out[2])
    saved = torch.load(os.path.join(str(tmp_path), "ft.pkl"), map_location="cpu")
    model_names = {n for n, _ in tiny("DualViT").state_dict().items()}
    assert set(saved) == model_names and all(bool(torch.isfinite(v).all()) for v in saved.values())
