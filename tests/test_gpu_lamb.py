"""The LAMB step (hsimae_lamb_step, csrc/lamb.hip) on the GPU against the fp64 restatement of tests/lamb_ref.py: through the C ABI
on the smallest tensor lists at which its three kernels can go wrong, in every control-block mode, with the refusals and the table
guard; and the Python layer: FusedLAMB on HSIMAE and DualViT, its state_dict, the pretraining loop, and FusedAdamW left as it was."""
import contextlib
import ctypes as C
import gc
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
import lamb_ref as L  # noqa: E402
import groups_ref as G  # noqa: E402
import clip_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
GUARD = 64
OK, EDIMS, EALIGN, ENULL = 0, -1, -3, -4
HP = L.HP
MODES = {"clipped": (0.3, 1), "unclipped": (1.0, 1), "apply0": (0.3, 0)}          # coef, apply
RATIO_CANARY = 3.25                                            # what `ratios` holds before a call
_REFS = {}


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


@pytest.fixture(scope="module", autouse=True)
def models_released_with_the_file():
    """This file builds some twenty models; when it ends they and their device memory are released here, not whenever the collector
    next runs in the middle of a later file."""
    yield
    _REFS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def libs():
    from hsimae_amd import _lib
    return _lib, _lib.load()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------ device state between canaries
class Arrays:
    """p, g, m, v (NaN canaries), the ids (canary 0: a live id, so a read past the end would step a canary), the tensor table, the
    partial sums (NaN canaries), the ratios (a canary value throughout) and the flag, all in device memory.
    off: floats by which every fp32 array starts behind a 256-byte boundary."""

    def __init__(self, inp, off=0, with_ids=True, rows=None, nchunks=None):
        n = inp["p"].numel()
        self.n, self.off = n, off
        self.full = {k: torch.full((n + 2 * GUARD + off,), NAN, device=DEV) for k in "pgmv"}
        for k in "pgmv":
            self.full[k][GUARD + off:GUARD + off + n] = inp[k].to(DEV)
        self.ids = None
        if with_ids:
            self.ids = torch.zeros(n + 2 * GUARD, dtype=torch.uint8, device=DEV)
            self.ids[GUARD:GUARD + n] = inp["ids"].to(DEV)
        if rows is None:
            rows, nchunks = L.chunk_table(inp["tensors"])
        _lib, _ = libs()
        table = (_lib.LambTensor * len(rows))(*[_lib.LambTensor(o, c, c0, 0) for o, c, c0 in rows])
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
        self.nt, self.nchunks = len(rows), nchunks
        self.partials = torch.full((2 * nchunks + 2 * GUARD,), NAN, dtype=torch.float64, device=DEV)
        self.ratios = torch.full((self.nt + 2 * GUARD,), RATIO_CANARY, device=DEV)
        self.bad = torch.zeros(1 + 2 * GUARD, dtype=torch.int32, device=DEV)
        self.image = {k: bits(v).clone() for k, v in self.full.items()}
        self.side = {k: bits(getattr(self, k)).clone() for k in ("partials", "ratios", "bad", "table")}

    def ptr(self, k):
        return self.full[k].data_ptr() + 4 * (GUARD + self.off)

    def ids_ptr(self):
        return None if self.ids is None else self.ids.data_ptr() + GUARD

    def partials_ptr(self):
        return self.partials.data_ptr() + 8 * GUARD

    def ratios_ptr(self):
        return self.ratios.data_ptr() + 4 * GUARD

    def bad_ptr(self):
        return self.bad.data_ptr() + 4 * GUARD

    def host(self):
        lo = GUARD + self.off
        out = {k: self.full[k][lo:lo + self.n].cpu() for k in "pmv"}
        out["r"] = self.ratios[GUARD:GUARD + self.nt].cpu()
        return out

    def flag(self):
        return int(self.bad[GUARD])

    def frame_intact(self):
        lo = GUARD + self.off
        for k, f in self.full.items():
            im = self.image[k]
            if not (torch.equal(bits(f)[:lo], im[:lo]) and torch.equal(bits(f)[lo + self.n:], im[lo + self.n:])):
                return False
        for k, lo, cnt in (("partials", GUARD, 2 * self.nchunks), ("ratios", GUARD, self.nt), ("bad", GUARD, 1)):
            b, im = bits(getattr(self, k)), self.side[k]
            if not (torch.equal(b[:lo], im[:lo]) and torch.equal(b[lo + cnt:], im[lo + cnt:])):
                return False
        return torch.equal(bits(self.table), self.side["table"]) and torch.equal(bits(self.full["g"]), self.image["g"])

    def unchanged(self):
        return (all(torch.equal(bits(f), self.image[k]) for k, f in self.full.items()) and
                all(torch.equal(bits(getattr(self, k)), im) for k, im in self.side.items()))


def ctl_block(mode, hp=HP, t=L.T_STEP):
    """(device tensor, pointer, coef, apply): a control block as hsimae_grad_norm would have left it."""
    _lib, _ = libs()
    coef, apply_ = MODES[mode]
    coef = R.f32(coef)
    i1, i2 = R.bias_corrections(t, hp["b1"], hp["b2"])
    c = _lib.ClipCtl(sumsq=1.0, norm=1.0, coef=coef, finite=1, apply=apply_, skipped=0, inv_bc1=i1, inv_sqrt_bc2=i2, norm_max=1.0)
    host = torch.full((C.sizeof(c) + 2 * GUARD,), 0xA5, dtype=torch.uint8)
    host[GUARD:GUARD + C.sizeof(c)] = torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8)
    buf = host.to(DEV)
    return buf, buf.data_ptr() + GUARD, coef, apply_


def c_table(table):
    _lib, _ = libs()
    return (_lib.AdamWGroup * len(table))(*[_lib.AdamWGroup(a, b) for a, b in table])


def call_lamb(arr, ctl_ptr, trust_clip=None, always_adapt=False, gu=0, table=L.TABLE, hp=HP, **over):
    _, lib = libs()
    if isinstance(table, list):
        table = c_table(table)
    a = dict(p=arr.ptr("p"), g=arr.ptr("g"), m=arr.ptr("m"), v=arr.ptr("v"), group=arr.ids_ptr(), gu=gu, n=arr.n,
             tensors=arr.table.data_ptr(), nt=arr.nt, nch=arr.nchunks, table=table, ng=len(table) if table is not None else 5,
             partials=arr.partials_ptr(), ratios=arr.ratios_ptr(), bad=arr.bad_ptr(), ctl=ctl_ptr)
    a.update(over)
    return lib.hsimae_lamb_step(a["p"], a["g"], a["m"], a["v"], a["group"], a["gu"], a["n"], a["tensors"], a["nt"], a["nch"], a["table"],
                                a["ng"], hp["b1"], hp["b2"], hp["eps"], 0.0 if trust_clip is None else trust_clip, int(always_adapt),
                                a["partials"], a["ratios"], a["bad"], a["ctl"], stream())


def reference(key, inp, ids, coef, trust_clip, always_adapt):
    """One fp64 reference per (inputs, coef, trust_clip, always_adapt), shared by every run that needs it and never changed."""
    k = (key, coef, trust_clip, always_adapt)
    if k not in _REFS:
        _REFS[k] = L.lamb_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["tensors"], ids, L.TABLE, coef, 1, L.T_STEP, HP["b1"], HP["b2"],
                              HP["eps"], trust_clip, always_adapt)
    return _REFS[k]


def check_step(key, inp, mode, trust_clip, always_adapt, off, worst, uniform=None, plants=None):
    """One call on fresh arrays, twice; the result against the restatement, everything else against its image."""
    n = inp["p"].numel()
    ids_h = inp["ids"] if uniform is None else torch.full((n,), uniform, dtype=torch.uint8)
    tag = f"{key}-{mode}-clip{trust_clip}-adapt{int(always_adapt)}-off{off}"
    runs = []
    for _ in range(2):
        arr = Arrays(inp, off, with_ids=uniform is None)
        buf, ctl_ptr, coef, apply_ = ctl_block(mode)
        ctl_img = buf.clone()
        assert call_lamb(arr, ctl_ptr, trust_clip, always_adapt, gu=0 if uniform is None else uniform) == OK, tag
        torch.cuda.synchronize()
        assert arr.frame_intact(), f"{tag}: a canary, the table or the gradient was written"
        assert torch.equal(buf, ctl_img), f"{tag}: the control block was written"
        assert arr.flag() == 0, f"{tag}: the table guard fired"
        runs.append(arr)
    a, b = runs
    assert all(torch.equal(bits(a.full[k]), bits(b.full[k])) for k in "pmv"), f"{tag}: two runs differ"
    assert torch.equal(bits(a.ratios), bits(b.ratios)) and torch.equal(bits(a.partials), bits(b.partials)), f"{tag}: two runs differ"
    got = a.host()
    if not apply_:
        assert a.unchanged(), f"{tag}: apply = 0 wrote"
        return got
    ref = reference(key if uniform is None else f"{key}-u{uniform}", inp, ids_h, coef, trust_clip, always_adapt)
    dead = ~((ids_h != 2) & (ids_h < len(L.TABLE)))
    for k in "pmv":
        assert torch.equal(bits(got[k][dead]), bits(inp[k][dead])), f"{tag} {k}: an element that must not be touched changed"
        worst[f"{k}@{tag}"] = ref[k].ratio(got[k])
    worst[f"r@{tag}"] = ref["r"].ratio(got["r"])
    for T, kind in (plants or {}).items():
        o, cnt = inp["tensors"][T]
        sl = slice(o, o + cnt)
        if kind in ("frozen", "dead", "zero_u", "zero_w"):
            assert float(got["r"][T]) == 1.0, f"{tag}: tensor {T} ({kind}) has ratio {float(got['r'][T])}"
        if kind == "zero_u":
            assert torch.equal(bits(got["p"][sl]), bits(inp["p"][sl])), f"{tag}: u = 0 moved p"
        if kind == "zero_w":
            assert bool((got["p"][sl] != 0).all()) and bool((got["m"][sl] != inp["m"][sl]).any()), f"{tag}: zero weights were not stepped"
    if bool((~dead).any()):
        assert not torch.equal(bits(got["m"]), bits(inp["m"])), f"{tag}: nothing moved"
    return got


# ------------------------------------------------------------------------------------------------ 1. the C ABI against the bound
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(L.CASES))
def test_lamb_step_on_every_list_alignment_and_mode(case, mode):
    """A: sizes 1 .. 8193 packed so that tensor starts hit every alignment mod 4; B: 65 chunks in one tensor (the ratio kernel's lane
    loop runs twice, the last chunk is a 5-element tail), each planted kind on it in turn; C: 700 tensors of 1 .. 9 elements.
    Base offsets 0 and 1 float, trust_clip none and 1.0, always_adapt 0 and 1."""
    assert L.LIST_A == [1, 3, 4, 5, 7, 64, 255, 4095, 4096, 4097, 8193] and L.LIST_B == [1, 64 * 4096 + 5, 1]
    assert len(L.LIST_C) == 700 and set(L.LIST_C) == set(range(1, 10))
    inp = L.case_inputs(case)
    plants = {k: v for k, v in L.CASES[case][1].items() if v}
    assert {int(inp["tensors"][T][0]) % 4 for T in range(len(inp["tensors"]))} == ({0, 1, 2, 3} if case[0] in "AC" else {0, 1, 2})
    worst = {}
    for trust_clip in (None, 1.0):
        for always_adapt in (False, True):
            for off in (0, 1):
                check_step(case, inp, mode, trust_clip, always_adapt, off, worst, plants=plants)
    kinds = {q: max([v for k, v in worst.items() if k.startswith(q + "@")], default=0.0) for q in "pmvr"}
    print(f"[lamb abi {case} {mode}] worst err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in kinds.items()))
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}
    if mode != "apply0" and case in ("A", "C"):                # the ratios fall on both sides of 1
        r = reference(case, inp, inp["ids"], R.f32(MODES[mode][0]), None, True)["r"].ref
        assert float(r.min()) < 0.5 and float(r.max()) > 2.0


@pytest.mark.parametrize("n", [17, 5000])
def test_lamb_step_with_each_uniform_id(n):
    """group = NULL on a one-tensor table: the call FusedLAMB makes for a parameter outside the flat buffer (17: cls_head.bias with
    17 classes; 5000: two chunks).  Every id of the table in turn; the uniform id 2 changes nothing and reports ratio 1."""
    inp = L.inputs([n], 23)
    worst = {}
    for gu in range(len(L.TABLE)):
        for always_adapt in (False, True):
            got = check_step(f"uniform{n}", inp, "clipped", None, always_adapt, gu % 2, worst, uniform=gu)
            assert (gu == 2) == all(torch.equal(bits(got[k]), bits(inp[k])) for k in "pmv")
            adapted = gu != 2 and (always_adapt or L.TABLE[gu][1] != 0.0)
            assert (float(got["r"][0]) != 1.0) == adapted, (gu, always_adapt, float(got["r"][0]))
    assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_refusals_return_their_code_and_write_nothing():
    inp = L.inputs([5, 64, 7], 2)
    arr = Arrays(inp)
    buf, ctl_ptr, _, _ = ctl_block("clipped")
    ctl_img = buf.clone()

    def step(**over):
        return call_lamb(arr, ctl_ptr, **over)
    for k in ("p", "g", "m", "v", "tensors", "table", "partials", "ratios", "bad", "ctl"):
        assert step(**{k: None}) == ENULL, k
    assert step(n=-1) == EDIMS and step(nt=0) == EDIMS and step(nt=-3) == EDIMS and step(nch=0) == EDIMS and step(nch=-1) == EDIMS
    assert step(ng=0) == EDIMS and step(ng=-1) == EDIMS and step(table=c_table([(1e-3, 0.0)] * 65), ng=65) == EDIMS
    assert step(group=None, gu=-1) == EDIMS and step(group=None, gu=5) == EDIMS and step(group=None, gu=64) == EDIMS
    for bad in ((-1e-3, 0.0), (1e-3, -0.5), (NAN, 0.0), (1e-3, NAN)):
        assert step(table=c_table([bad, (1e-3, 0.0)]), ng=2) == EDIMS, bad
    assert step(partials=arr.partials_ptr() + 4) == EALIGN
    assert step(p=arr.ptr("p") + 2) == EALIGN and step(g=arr.ptr("g") + 1) == EALIGN and step(ctl=ctl_ptr + 4) == EALIGN
    assert step(n=0) == OK
    torch.cuda.synchronize()
    assert arr.unchanged() and torch.equal(buf, ctl_img)


# ------------------------------------------------------------------------------------------------ 3. the table guard
@pytest.mark.parametrize("past", [1, 32])
def test_a_tensor_that_reaches_past_the_arrays_sets_the_flag_and_writes_nothing_of_it(past):
    """The last tensor claims `past` floats behind n_total.  Even a missing guard could only reach the test's own guard region of
    64 floats; with the guard the tensor is not touched at all and the canaries stand."""
    assert past <= 32 < GUARD
    inp = L.case_inputs("A")
    rows, _ = L.chunk_table(inp["tensors"])
    o, cnt, c0 = rows[-1]
    rows[-1] = (o, cnt + past, c0)
    nchunks = c0 + -(-(cnt + past) // L.CHUNK)
    arr = Arrays(inp, rows=rows, nchunks=nchunks)
    buf, ctl_ptr, _, _ = ctl_block("clipped")
    assert call_lamb(arr, ctl_ptr) == OK
    torch.cuda.synchronize()
    assert arr.flag() == 1 and arr.frame_intact()
    got = arr.host()
    for k in "pmv":
        assert torch.equal(bits(got[k][o:]), bits(inp[k][o:])), f"{k}: the inconsistent tensor was written"
    assert not torch.equal(bits(got["m"][:o]), bits(inp["m"][:o]))             # the consistent ones were stepped


@pytest.mark.parametrize("which,delta", [(5, 1), (10, -1), (0, 1)])
def test_a_wrong_chunk0_sets_the_flag_and_no_canary_changes(which, delta):
    inp = L.case_inputs("A")
    rows, nchunks = L.chunk_table(inp["tensors"])
    o, cnt, c0 = rows[which]
    rows[which] = (o, cnt, c0 + delta)
    arr = Arrays(inp, rows=rows, nchunks=nchunks)
    buf, ctl_ptr, _, _ = ctl_block("unclipped")
    assert call_lamb(arr, ctl_ptr) == OK
    torch.cuda.synchronize()
    assert arr.flag() == 1 and arr.frame_intact()
    # no half-applied step: the tensor whose chunks no longer end where the next one's begin, and the one in front of it whose
    # chunks no longer meet its own, keep every bit of p, m and v and get no ratio; a tensor away from the fault is stepped
    got = arr.host()
    for T in {which, max(which - 1, 0)}:
        lo, cnt = inp["tensors"][T]
        for k in "pmv":
            assert torch.equal(bits(got[k][lo:lo + cnt]), bits(inp[k][lo:lo + cnt])), f"tensor {T}: {k} was written"
        assert float(got["r"][T]) == RATIO_CANARY, T
    lo, cnt = inp["tensors"][3]
    assert not torch.equal(bits(got["m"][lo:lo + cnt]), bits(inp["m"][lo:lo + cnt])) and float(got["r"][3]) != RATIO_CANARY


# ------------------------------------------------------------------------------------------------ models
MODEL_KW = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=64, depth=4, s_depth=2, num_heads=4,
                decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True, trunc_init=True)
DEPTH, S_DEPTH = 4, 2
OPT_KW = dict(lr=2e-3, weight_decay=5e-3, betas=(0.9, 0.95))
EPS = 1e-6                                                     # FusedLAMB's default
_STATE = {}


def tiny(kind):
    """Depth 4, dim 64, s_depth 2, decoder 1 x 32; every model of a kind starts from the same parameters."""
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


def outside_of(m):
    return [p for n, p in m.named_parameters() if n.startswith("cls_head.")]


def gather(m, outside, what="p"):
    flat = (m._flat if what == "p" else m._flat_grad).detach().cpu()
    rest = [(p.detach() if what == "p" else p.grad).reshape(-1).cpu() for p in outside]
    return torch.cat([flat] + rest)


def layout(m, ids_by_name):
    """The model's real layout for the restatement: [(off, n)] of the flat tensors, then the outside parameters behind them, and
    one id per element from the test's own table."""
    flat_names = [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
    tensors = list(zip(m._offs, m._sizes))
    ids = torch.full((m._flat.numel(),), 2, dtype=torch.uint8)
    for n, off, size in zip(flat_names, m._offs, m._sizes):
        ids[off:off + size] = ids_by_name[n]
    end, rest = m._flat.numel(), []
    for n, p in m.named_parameters():
        if n.startswith("cls_head."):
            tensors.append((end, p.numel()))
            rest.append(torch.full((p.numel(),), ids_by_name[n], dtype=torch.uint8))
            end += p.numel()
    return flat_names, tensors, torch.cat([ids] + rest)


def frozen_names(m, freeze=()):
    return tuple(n for n, p in m.named_parameters() if not p.requires_grad) + tuple(freeze)


@pytest.mark.parametrize("layer_decay", [None, 0.75])
@pytest.mark.parametrize("kind", ["HSIMAE", "DualViT"])
def test_fused_lamb_three_scheduled_steps_match_the_restatement_in_fp64(kind, layer_decay):
    """3 steps of FusedLAMB with CosineLRScheduler writing lr between them, every step fed the gradients of one real backward; the
    fp64 restatement carries its own trajectory over the model's real layout beside it.  The clip bites (max_grad_norm is half
    these gradients' norm).  Worst |p - p64| against the summed bound; the first step's ratios against delta_r."""
    from hsimae_amd import FusedLAMB, CosineLRScheduler
    m = tiny(kind)
    backward(m)
    outside = outside_of(m)
    names = [n for n, _ in m.named_parameters()]
    clip = 0.5 * math.sqrt(float((gather(m, outside, "g").nan_to_num().double() ** 2).sum()))
    opt = FusedLAMB(m, layer_decay=layer_decay, max_grad_norm=clip, skip_nonfinite=True, trust_clip=10.0, **OPT_KW)
    sched = CosineLRScheduler(opt, t_initial=10, lr_min=2e-5, warmup_t=2, warmup_lr_init=2e-4)
    by_name, unit, _ = G.layer_table(names, DEPTH, S_DEPTH, layer_decay, 1.0, OPT_KW["weight_decay"], frozen=frozen_names(m))
    flat_names, tensors, ids = layout(m, by_name)
    ng = len(unit)
    assert ng == opt._ngroups and opt.trust_ratio_names == flat_names
    g = gather(m, outside, "g")
    live = G.live_mask(ids, ng)
    assert bool(torch.isfinite(g[live]).all()) and float(g.abs().max()) > 0
    p0 = gather(m, outside).double()
    p64, m64, v64 = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    total = torch.zeros_like(p0)
    lrs = []
    for t in (1, 2, 3):
        base = opt.param_groups[0]["lr"]
        lrs.append(base)
        table = [(R.f32(base * scale), R.f32(wd)) for scale, wd in unit]
        opt.step()
        coef = float(opt.clip_coef)                            # the fp32 coefficient the step read
        assert 0.49 < coef < 0.51
        ref = L.lamb_ref(p64, g, m64, v64, tensors, ids, table, coef, 1, t, *OPT_KW["betas"], EPS, 10.0, False)
        total += ref["p"].bound()
        if t == 1:                                             # both sides still stand on the same state
            got_r = torch.cat([opt.trust_ratios.cpu(), opt.trust_ratios_outside.cpu()])
            assert got_r.numel() == len(tensors) == len(flat_names) + len(outside)
            rr = ref["r"].ratio(got_r)
            adapted = ref["r"].ref[ref["r"].ref != 1.0]
            print(f"[lamb model {kind} ld {layer_decay}] ratios {float(adapted.min()):.4g} .. {float(adapted.max()):.4g} over "
                  f"{adapted.numel()} adapted tensors, worst err / bound {rr:.3f}")
            assert rr <= 1.0 and adapted.numel() > 20
        p64, m64, v64 = ref["p"].ref, ref["m"].ref, ref["v"].ref
        sched.step(t)
    assert len(set(lrs)) == 3, lrs
    torch.cuda.synchronize()
    assert int(opt.table_error) == 0 and int(opt.skipped_steps) == 0
    got = gather(m, outside).double()
    err = (got - p64).abs()
    assert torch.equal(got[~live], p0[~live]), "a frozen element moved"
    assert bool((err[live] > 0).any()) and float((got - p0).abs().max()) > 1e-5
    ratio = float((err[live] / total[live].clamp_min(1e-300)).max())
    print(f"[lamb model {kind} ld {layer_decay}] worst |p - p64| / summed bound {ratio:.3f}")
    assert ratio <= 1.0
    # a NaN gradient with skip_nonfinite: no parameter, moment or ratio bit changes, and the count advances
    before = bits(gather(m, outside)).clone()
    state = [bits(t).clone() for t in (opt.exp_avg, opt.exp_avg_sq, *opt._out_m, *opt._out_v, opt.trust_ratios, opt.trust_ratios_outside)]
    m.blocks[0].mlp.w1.weight.grad.view(-1)[5] = NAN
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(gather(m, outside)), before), "a skipped step moved a parameter"
    for t, im in zip((opt.exp_avg, opt.exp_avg_sq, *opt._out_m, *opt._out_v, opt.trust_ratios, opt.trust_ratios_outside), state):
        assert torch.equal(bits(t), im)
    assert int(opt.skipped_steps) == 1


FROZEN = ("patch_embed", "blocks_1.0.", "blocks_2.0.")


def test_frozen_prefixes_stay_bit_unchanged_and_report_ratio_one():
    from hsimae_amd import FusedLAMB
    m = tiny("HSIMAE")
    opt = FusedLAMB(m, freeze=FROZEN, always_adapt=True, **OPT_KW)
    before = None
    for step in (1, 2):
        opt.zero_grad()
        backward(m, step)
        if before is None:
            before = {n: bits(p.detach()).clone() for n, p in m.named_parameters()}
        opt.step()
    torch.cuda.synchronize()
    flat_names = [n for n, _ in m.named_parameters()]
    assert opt.trust_ratio_names == flat_names and opt.trust_ratios.numel() == len(flat_names) == len(m._offs)
    assert opt.trust_ratios_outside.numel() == 0
    ratios = opt.trust_ratios.cpu()
    moved = 0
    for k, (n, off, size) in enumerate(zip(flat_names, m._offs, m._sizes)):
        p = dict(m.named_parameters())[n]
        if n.startswith(FROZEN) or not p.requires_grad or n == "mask_token":
            assert torch.equal(bits(p.detach()), before[n]), f"{n} moved"
            assert not bool(opt.exp_avg[off:off + size].any()) and not bool(opt.exp_avg_sq[off:off + size].any()), f"{n}: moments"
            assert float(ratios[k]) == 1.0, n
        else:
            moved += int(not torch.equal(bits(p.detach()), before[n]) and float(ratios[k]) != 1.0)
    assert moved > 40 and int(opt.table_error) == 0


# ------------------------------------------------------------------------------------------------ no ATen op, no host wait
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
def test_step_issues_no_torch_op_and_no_host_wait(kind, monkeypatch):
    from torch.utils._python_dispatch import TorchDispatchMode
    from hsimae_amd import FusedLAMB, optim

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    m = tiny(kind)
    opt = FusedLAMB(m, layer_decay=0.75, freeze=("patch_embed",), max_grad_norm=1.0, skip_nonfinite=True, **OPT_KW)
    spy = Spy(optim._lib.load())
    monkeypatch.setattr(optim._lib, "load", lambda: spy)
    for k in range(2):
        opt.zero_grad()
        backward(m, k)
        if k == 0:
            opt.step()
            continue
        before = m._flat.clone()
        torch.cuda.synchronize()
        spy.calls.clear()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with Count() as c:
                opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert c.ops == [], c.ops[:8]
        assert spy.calls == ["hsimae_grad_norm"] + ["hsimae_lamb_step"] * (1 if kind == "HSIMAE" else 3), spy.calls
        assert not torch.equal(before, m._flat) and float(opt.grad_norm) > 0 and m._packed_version == -1


# ------------------------------------------------------------------------------------------------ state_dict
def test_state_dict_resumes_bit_for_bit_and_refuses_the_other_optimizers_checkpoint(monkeypatch):
    """2 steps, save, load into a fresh optimizer, 2 more steps: bit-identical to 4 uninterrupted steps in deterministic mode."""
    from hsimae_amd import FusedLAMB, FusedAdamW, CosineLRScheduler
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
    oa = FusedLAMB(ma, **kw)
    sa = schedule(oa)
    steps(ma, oa, sa, (0, 1, 2, 3))
    ob = FusedLAMB(mb, **kw)
    sb = schedule(ob)
    steps(mb, ob, sb, (0, 1))
    blob = io.BytesIO()
    torch.save({"opt": ob.state_dict(), "sched": sb.state_dict()}, blob)
    blob.seek(0)
    sd = torch.load(blob, map_location="cpu")
    assert sd["opt"]["optimizer"] == "lamb" and not any("ratio" in k for k in sd["opt"])
    fresh = FusedLAMB(mb, **kw)
    fs = schedule(fresh)
    fresh.load_state_dict(sd["opt"])
    fs.load_state_dict(sd["sched"])
    assert fresh.step_count == 2 and fresh.param_groups[0]["lr"] == ob.param_groups[0]["lr"]
    steps(mb, fresh, fs, (2, 3))
    torch.cuda.synchronize()
    assert torch.equal(bits(ma._flat), bits(mb._flat))
    assert torch.equal(bits(oa.exp_avg), bits(fresh.exp_avg)) and torch.equal(bits(oa.exp_avg_sq), bits(fresh.exp_avg_sq))
    for a, b in zip(outside_of(ma), outside_of(mb)):
        assert torch.equal(bits(a.detach()), bits(b.detach()))
    assert torch.equal(bits(oa.trust_ratios), bits(fresh.trust_ratios))
    adam = FusedAdamW(mb, **kw)
    adam._bind()
    assert "optimizer" not in adam.state_dict()
    with pytest.raises(ValueError, match="adamw"):
        FusedLAMB(mb, **kw).load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="lamb"):
        FusedAdamW(mb, **kw).load_state_dict(fresh.state_dict())


# ------------------------------------------------------------------------------------------------ the pretraining loop
def cubes():
    """Two random scenes cut into 9 x 9 x 32 cubes at stride 3, as tests/test_gpu_train.py cuts them."""
    from oracle import loader_oracle as LO
    rng = np.random.default_rng(5)
    scenes = [rng.random((16, 17, 32)).astype(np.float32), rng.random((13, 15, 32)).astype(np.float32)]
    cut = []
    for num, sc in enumerate(scenes):
        cut += LO.split_info(sc.shape, (9, 9, 32), (3, 3, 1), num, 1, 0)
    return [scenes, np.array(cut, dtype=np.int16)]


LOOP_KW = dict(img_size=9, bands=32, mask_ratio=0.5, lr=5e-3, wd=5e-2, bs=8, depth=3, dim=32, s_depth=2, dec_dim=32, dec_depth=2)


def test_mask_pretraining_with_lamb_writes_the_files_logs_the_ratios_and_resumes(tmp_path):
    import hsimae_amd
    import hsimae_amd.pretrain as P
    from hsimae_amd.pretrain import seed_everything

    def run(*a, **k):
        seed_everything(0)
        lines = []
        out = hsimae_amd.mask_pretraining(*a, optimizer="lamb", log=lambda *s: lines.append(" ".join(map(str, s))), **LOOP_KW, **k)
        return out, lines
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    (model, losses), lines = run(cubes(), d1, "m.pkl", epochs=2)
    assert len(losses) == 2 and all(np.isfinite(losses))
    sd = torch.load(os.path.join(d1, "m.pkl"))
    ref = model.state_dict()
    assert list(sd) == list(ref) and all(v.dtype == torch.float32 and v.shape == ref[k].shape for k, v in sd.items())
    log = np.load(os.path.join(d1, "train_log.npy"), allow_pickle=True)
    assert np.allclose(np.array(list(log[0]), dtype=np.float64), losses)
    logged = [re.search(r"largest gradient norm (\S+), (\d+) steps skipped so far, trust ratio (\S+) \.\. (\S+)$", ln) for ln in lines]
    logged = [h for h in logged if h]
    assert len(logged) == 2, lines
    for h in logged:
        lo, hi = float(h.group(3)), float(h.group(4))
        assert 0 < lo < hi and math.isfinite(hi) and int(h.group(2)) == 0
    # interrupted after epoch 1 of 2, then resumed: the uninterrupted losses (atomics reorder the last bits of the gradients)
    os.makedirs(d2)
    ck = os.path.join(d2, "resume.pt")
    real_save, real_final = P.save_resume, P.save_final

    def stop_after_one(*a, **k):
        real_save(*a, **k)
        raise KeyboardInterrupt
    try:
        P.save_final = lambda *a, **k: None
        P.save_resume = stop_after_one
        with pytest.raises(KeyboardInterrupt):
            run(cubes(), d2, "m.pkl", epochs=2, resume_path=ck)
    finally:
        P.save_resume, P.save_final = real_save, real_final
    assert torch.load(ck, map_location="cpu", weights_only=False)["optimizer"]["optimizer"] == "lamb"
    (_, l2), lines2 = run(cubes(), d2, "m.pkl", epochs=2, resume_path=ck)
    assert len(l2) == 2 and any("resumed at epoch 1" in ln for ln in lines2)
    assert np.allclose(l2, losses, rtol=2e-3), (l2, losses)
    with pytest.raises(ValueError, match="optimizer"):
        hsimae_amd.mask_pretraining(cubes(), d2, "x.pkl", epochs=1, optimizer="lars", **LOOP_KW)


# ------------------------------------------------------------------------------------------------ FusedAdamW is untouched
def test_fused_adamw_steps_are_what_they_were_bit_for_bit(monkeypatch):
    """One default step and one clipped layer_decay step on two identically seeded models in deterministic mode: bit-identical.
    This shows only that importing and building the new unit perturbs nothing."""
    from hsimae_amd import FusedAdamW
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    for kw in (dict(), dict(layer_decay=0.75, max_grad_norm=1.0, skip_nonfinite=True)):
        ma, mb = tiny("HSIMAE"), tiny("HSIMAE")
        ma.deterministic = mb.deterministic = True
        oa, ob = FusedAdamW(ma, **OPT_KW, **kw), FusedAdamW(mb, **OPT_KW, **kw)
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad()
            backward(m, 7)
            o.step()
        torch.cuda.synchronize()
        assert torch.equal(bits(ma._flat_grad), bits(mb._flat_grad))
        assert torch.equal(bits(ma._flat), bits(mb._flat))
        assert torch.equal(bits(oa.exp_avg), bits(ob.exp_avg)) and torch.equal(bits(oa.exp_avg_sq), bits(ob.exp_avg_sq))
        assert bool(oa.exp_avg.any())
