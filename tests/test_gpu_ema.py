"""The moving average of the weights (hsimae_ema_update / hsimae_ema_swap, csrc/ema.hip) on the GPU against the fp64 restatement
and the derived bound of tests/ema_ref.py: through the C ABI at every size, alignment, control-block mode, decay and step, the
refusals and the exchange; the Python layer (FusedAdamW / FusedLAMB ema_decay, swap_ema, ema_state_dict, the state_dict) on
HSIMAE and DualViT; and the loops (fine-tuning with keep_best, pretraining with its resume)."""
import contextlib
import ctypes as C
import io
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
import ema_ref as E  # noqa: E402
import test_gpu_groups as TG  # noqa: E402  (tiny models, one real backward)
import test_gpu_clip as TC  # noqa: E402  (the toy set of the loop tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
GUARD = 64                                                       # floats (and bytes, around the control block)
OK, EDIMS, EALIGN, ENULL = 0, -1, -3, -4
CANARY = np.array([0x7FA5A5A5], dtype=np.uint32).view(np.float32)[0]       # a NaN with a payload: a read of it poisons the result
DECAYS = [0.0, 0.9, 0.9999]
STEPS = [1, 2, 10, 1000]
ALIGN = [(oe, op) for oe in range(4) for op in range(4)]
bits = TG.bits


@pytest.fixture(autouse=True)
def rng_state_left_as_found():
    """These tests seed the global generators (model initialisation, the loops' splits); tests that run after this file and draw
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


# ------------------------------------------------------------------------------------------------ device state between canaries
class Buf:
    """One fp32 array in device memory, `off` floats behind a 256-byte boundary, NaN canaries on both sides."""

    def __init__(self, values, off=0):
        values = np.asarray(values, dtype=np.float32)
        self.n, self.lo = values.size, GUARD + off
        full = np.full(self.n + 2 * GUARD + 4, CANARY, dtype=np.float32)
        full[self.lo:self.lo + self.n] = values
        self.image = full.view(np.uint32).copy()
        self.t = torch.from_numpy(full).to(DEV)
        assert self.t.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lo

    def words(self):
        return self.t.cpu().numpy().view(np.uint32)

    def body(self):
        return self.words()[self.lo:self.lo + self.n].view(np.float32).copy()

    def frame_intact(self):
        w = self.words()
        return np.array_equal(w[:self.lo], self.image[:self.lo]) and np.array_equal(w[self.lo + self.n:], self.image[self.lo + self.n:])

    def unchanged(self):
        return np.array_equal(self.words(), self.image)


def ctl_block(apply_, skipped):
    """(device buffer, pointer): a control block as hsimae_grad_norm would have left it, between 0xA5 bytes."""
    _lib, _ = libs()
    c = _lib.ClipCtl(sumsq=1.0, norm=1.0, coef=1.0, finite=apply_, apply=apply_, skipped=skipped, inv_bc1=1.0, inv_sqrt_bc2=1.0, norm_max=1.0)
    host = torch.full((C.sizeof(c) + 2 * GUARD,), 0xA5, dtype=torch.uint8)
    host[GUARD:GUARD + C.sizeof(c)] = torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8)
    buf = host.to(DEV)
    return buf, buf.data_ptr() + GUARD


def mode_ctl(mode, step):
    """-> (buffer, pointer, apply, skipped before this step's own decision is counted out of t)."""
    if mode == "null":
        return None, None, True, 0
    if mode == "skip":                                             # this step is the skipped one: counted already, nothing may move
        buf, ptr = ctl_block(0, 1)
        return buf, ptr, False, 1
    skipped = min(1, step - 1)                                     # an earlier step was skipped (where there was one)
    buf, ptr = ctl_block(1, skipped)
    return buf, ptr, True, skipped


def check_update(ema0, p, oe, op, mode, warmup, decay, step, tag):
    """Two launches on fresh arrays: the result against the restatement, equal elements and everything else against their bits."""
    _, lib = libs()
    runs = []
    for _ in range(2):
        e, q = Buf(ema0, oe), Buf(p, op)
        buf, ptr, apply_, skipped = mode_ctl(mode, step)
        img = None if buf is None else buf.clone()
        assert lib.hsimae_ema_update(e.ptr, q.ptr, e.n, decay, int(warmup), step, ptr, stream()) == OK, tag
        torch.cuda.synchronize()
        assert e.frame_intact() and q.unchanged(), f"{tag}: a canary or params was written"
        assert buf is None or torch.equal(buf, img), f"{tag}: the control block was written"
        runs.append(e)
    got = runs[0].body()
    assert np.array_equal(runs[0].words(), runs[1].words()), f"{tag}: two runs differ"
    if not apply_:
        assert runs[0].unchanged(), f"{tag}: a skipped step wrote"
        return 0.0
    assert E.kept(ema0, p, got), f"{tag}: an element equal to its average changed"
    avg = E.Average(ema0, skipped=skipped).step(p, decay, warmup, step)
    r = avg.ratio(got)
    assert r <= 1.0, f"{tag}: err / bound {r}"
    if e.n > 4 and decay < 1.0:
        assert not np.array_equal(E.f32bits(got), E.f32bits(ema0)), f"{tag}: nothing moved"
    return r


# ------------------------------------------------------------------------------------------------ 1. the C ABI against the bound
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("mode", ["null", "apply", "skip"])
def test_update_every_small_size_alignment_decay_and_step(mode, warmup):
    """n in {0, 1, 3, 4, 5, 7, 8, 255, 256, 257} x the 16 pairs of base offsets (0 .. 3 floats each: the 16-byte body, the mixed
    case, the scalar path); the decays and steps rotate so that every (decay, step) pair meets every size."""
    worst, k = 0.0, 0
    for n in E.SMALL_N:
        ema0, p = E.inputs(n, 100 + n)
        for oe, op in ALIGN:
            decay, step = DECAYS[k % 3], STEPS[(k // 3 + k // 48) % 4]
            k += 1
            worst = max(worst, check_update(ema0, p, oe, op, mode, warmup, decay, step, f"n {n} off {oe}/{op} d {decay} step {step}"))
    print(f"[ema abi] {mode} warm-up {warmup}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("warmup", [False, True])
def test_update_every_decay_at_every_step(warmup):
    ema0, p = E.inputs(257, 7)
    worst = 0.0
    for decay in DECAYS:
        for step in STEPS:
            for mode in ("null", "apply"):
                for off in ((0, 0), (1, 2)):
                    worst = max(worst, check_update(ema0, p, *off, mode, warmup, decay, step, f"d {decay} step {step} {mode} off {off}"))
    print(f"[ema abi] decays x steps, warm-up {warmup}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("off", [(0, 0), (0, 1), (3, 3)])
def test_update_where_the_stride_loop_runs_twice(off):
    """More float4s than the capped grid has threads: part of the grid takes a second pass (and every thread a fourth on the
    scalar path), then a tail of 3."""
    _lib, _ = libs()
    assert _lib.EMA_MAX_GRID == E.GRID and E.N_TWICE // 4 > E.GRID * 256 and E.N_TWICE % 4 == 3
    ema0, p = E.inputs(E.N_TWICE, 9)
    for mode in ("null", "apply"):
        r = check_update(ema0, p, *off, mode, True, 0.9999, 10, f"n {E.N_TWICE} off {off} {mode}")
        print(f"[ema abi] n {E.N_TWICE} off {off} {mode}: err / bound {r:.3f}")


def test_three_skipped_steps_of_ten_warm_up_as_seven():
    _, lib = libs()
    ema0, p = E.inputs(261, 21, equal_every=0)
    e, q = Buf(ema0), Buf(p)
    buf, ptr = ctl_block(1, 3)
    assert lib.hsimae_ema_update(e.ptr, q.ptr, e.n, 0.9999, 1, 10, ptr, stream()) == OK
    torch.cuda.synchronize()
    got = e.body()
    seven = E.Average(ema0, skipped=3).step(p, 0.9999, True, 10)
    ten = E.Average(ema0, skipped=0).step(p, 0.9999, True, 10)
    assert E.decay_at(0.9999, True, 7) == 8 / 17 and E.decay_at(0.9999, True, 10) == 11 / 20
    print(f"[ema abi] skipped 3 of 10: err / bound {seven.ratio(got):.3f} against t = 7, {ten.ratio(got):.3g} against t = 10")
    assert seven.ratio(got) <= 1.0 and ten.ratio(got) > 100.0


@pytest.mark.parametrize("off", [(0, 0), (1, 1), (0, 2)])
def test_elements_equal_to_their_average_keep_their_bits(off):
    n = 4 * 64 + 3
    ema0, p = E.inputs(n, 31, equal_every=0)
    special = np.array([0x80000000, 0x00001C2F, 0x7FC01234, 0xFF800001, 0x7F800000, 0x00000000], dtype=np.uint32).view(np.float32)
    at = [0, 1, 2, 3, 130, 131, n - 3, n - 2, n - 1, 64, 65, 66]            # in the body and in the tail of 3
    for j, i in enumerate(at):
        ema0[i] = p[i] = special[j % len(special)]
    _, lib = libs()
    e, q = Buf(ema0, off[0]), Buf(p, off[1])
    assert lib.hsimae_ema_update(e.ptr, q.ptr, n, 0.9, 0, 1, None, stream()) == OK
    torch.cuda.synchronize()
    got = e.body()
    assert e.frame_intact() and q.unchanged()
    assert E.kept(ema0, p, got)
    assert np.array_equal(E.f32bits(got)[at], E.f32bits(ema0)[at])
    rest = np.ones(n, dtype=bool)
    rest[at] = False
    assert E.Average(ema0[rest]).step(p[rest], 0.9, False, 1).ratio(got[rest]) <= 1.0


def test_update_refusals_return_their_code_and_write_nothing():
    _, lib = libs()
    n = 64
    ema0, p = E.inputs(n, 41)
    e, q = Buf(ema0), Buf(p)
    buf, ptr = ctl_block(1, 0)
    img = buf.clone()

    def up(ema=e.ptr, params=q.ptr, cnt=n, decay=0.9, warmup=1, step=1, ctl=None):
        return lib.hsimae_ema_update(ema, params, cnt, decay, warmup, step, ctl, stream())
    assert up(cnt=-1) == EDIMS
    assert up(decay=NAN) == EDIMS and up(decay=1.0) == EDIMS and up(decay=-1e-9) == EDIMS and up(decay=INF) == EDIMS and up(decay=2.0) == EDIMS
    assert up(step=0) == EDIMS and up(step=-3) == EDIMS and up(step=0, ctl=ptr) == EDIMS
    assert up(ema=None) == ENULL and up(params=None) == ENULL
    assert up(ema=e.ptr + 1) == EALIGN and up(ema=e.ptr + 2) == EALIGN and up(params=q.ptr + 3) == EALIGN
    assert up(ctl=ptr + 4) == EALIGN
    assert up(cnt=0) == OK and up(cnt=0, ema=None, params=None) == OK
    torch.cuda.synchronize()
    assert e.unchanged() and q.unchanged() and torch.equal(buf, img)


# ------------------------------------------------------------------------------------------------ 2. the exchange
def swap_inputs(n, seed):
    a, b = E.inputs(n, seed, equal_every=0)
    if n > 2:
        a[1] = np.array([0x7FC01234], dtype=np.uint32).view(np.float32)[0]
        b[n - 1] = np.array([0xFF800055], dtype=np.uint32).view(np.float32)[0]
        a[2] = np.float32(-0.0)
    return a, b


def test_swap_exchanges_bit_for_bit_and_twice_is_the_identity():
    _, lib = libs()
    for n in E.SMALL_N:
        a0, b0 = swap_inputs(n, 200 + n)
        for oa, ob in ALIGN:
            a, b = Buf(a0, oa), Buf(b0, ob)
            assert lib.hsimae_ema_swap(a.ptr, b.ptr, n, stream()) == OK
            torch.cuda.synchronize()
            assert a.frame_intact() and b.frame_intact(), (n, oa, ob)
            assert E.swapped(a0, b0, a.body(), b.body()), (n, oa, ob)
            assert lib.hsimae_ema_swap(a.ptr, b.ptr, n, stream()) == OK
            torch.cuda.synchronize()
            assert a.unchanged() and b.unchanged(), (n, oa, ob)


@pytest.mark.parametrize("off", [(0, 0), (2, 0)])
def test_swap_where_the_stride_loop_runs_twice(off):
    _, lib = libs()
    a0, b0 = swap_inputs(E.N_TWICE, 5)
    a, b = Buf(a0, off[0]), Buf(b0, off[1])
    assert lib.hsimae_ema_swap(a.ptr, b.ptr, a.n, stream()) == OK
    torch.cuda.synchronize()
    assert a.frame_intact() and b.frame_intact() and E.swapped(a0, b0, a.body(), b.body())


def test_swap_refuses_an_overlap_and_bad_arguments_and_writes_nothing():
    _, lib = libs()
    n = 40
    a0, b0 = swap_inputs(2 * n, 6)
    a, b = Buf(a0), Buf(b0)

    def sw(x=a.ptr, y=b.ptr, cnt=n):
        return lib.hsimae_ema_swap(x, y, cnt, stream())
    assert sw(y=a.ptr) == EDIMS and sw(y=a.ptr + 4) == EDIMS and sw(y=a.ptr + 4 * (n - 1)) == EDIMS
    assert sw(x=a.ptr + 4 * (n - 1), y=a.ptr) == EDIMS and sw(cnt=-1) == EDIMS
    assert sw(x=None) == ENULL and sw(y=None) == ENULL
    assert sw(x=a.ptr + 2) == EALIGN and sw(y=b.ptr + 1) == EALIGN
    assert sw(cnt=0) == OK and sw(cnt=0, x=None, y=None) == OK
    torch.cuda.synchronize()
    assert a.unchanged() and b.unchanged()
    assert sw(y=a.ptr + 4 * n) == OK                                 # two halves of one array touch, they do not overlap
    torch.cuda.synchronize()
    assert a.frame_intact() and b.unchanged() and E.swapped(a0[:n], a0[n:], a.body()[:n], a.body()[n:])


# ------------------------------------------------------------------------------------------------ 3. the optimizer
KINDS = ["HSIMAE", "DualViT"]
CONFIGS = {"plain": ("FusedAdamW", {}),
           "clip": ("FusedAdamW", dict(layer_decay=0.75, max_grad_norm=1.0, skip_nonfinite=True)),
           "lamb": ("FusedLAMB", dict(skip_nonfinite=True))}
EMA = {"plain": dict(ema_decay=0.9, ema_warmup=False), "clip": dict(ema_decay=0.9999, ema_warmup=True),
       "lamb": dict(ema_decay=0.9, ema_warmup=True)}


def make(config, m, **kw):
    import hsimae_amd
    name, extra = CONFIGS[config]
    return getattr(hsimae_amd, name)(m, **TG.OPT_KW, **extra, **kw)


def schedule(opt):
    from hsimae_amd import CosineLRScheduler
    return CosineLRScheduler(opt, t_initial=8, lr_min=2e-5, warmup_t=2, warmup_lr_init=2e-4)


def head(m):
    return [p for n, p in m.named_parameters() if n.startswith("cls_head.")]


def weights(m):
    return torch.cat([m._flat] + [p.detach().reshape(-1) for p in head(m)]).cpu().numpy()


def averages(opt, m):
    """The average of every element of weights(m): the flat one, then the head's in the model's order."""
    rest = []
    for p in head(m):
        k = [i for i, q in enumerate(opt._ema_params) if q is p]
        assert len(k) == 1, "a live parameter outside the flat buffer has no average"
        rest.append(opt._ema_out[k[0]])
    return torch.cat([opt.ema] + rest).cpu().numpy()


def steps(m, opt, sched, which, seed0=50):
    for t in which:
        opt.zero_grad()
        TG.backward(m, seed0 + t)
        opt.step()
        sched.step(t)


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_three_scheduled_steps_stay_inside_the_summed_bound(kind, config):
    """The average against the fp64 recursion fed the parameter values cloned after each step (the step's own error is not its
    business), for plain AdamW, layer_decay + clip, and LAMB; the head's average exists in both modes."""
    m = TG.tiny(kind)
    opt = make(config, m, **EMA[config])
    sched = schedule(opt)
    avg = None
    for t in range(3):
        opt.zero_grad()
        TG.backward(m, 50 + t)
        if avg is None:
            avg = E.Average(weights(m))                            # the weights before this optimizer's first step
        opt.step()
        sched.step(t)
        avg.step(weights(m), EMA[config]["ema_decay"], EMA[config]["ema_warmup"], t + 1)
    torch.cuda.synchronize()
    got = averages(opt, m)
    r = avg.ratio(got)
    print(f"[ema opt] {kind} {config}: worst err / summed bound {r:.3f} over {got.size} elements")
    assert r <= 1.0
    assert got.size == m._flat.numel() + sum(p.numel() for p in head(m))
    moved = E.f32bits(got) != E.f32bits(weights(m))
    assert moved.mean() > 0.5                                       # it is an average, not a copy of the weights
    if kind == "DualViT":
        assert len(opt._ema_out) == 2 and bool(moved[m._flat.numel():].any())
        sd = opt.ema_state_dict()
        assert not torch.equal(sd["cls_head.weight"], m.cls_head.weight.detach())


@pytest.mark.parametrize("config", ["clip", "lamb"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_gradient_leaves_the_average_alone_and_the_count_unadvanced(kind, config):
    m = TG.tiny(kind)
    ema_kw = dict(ema_decay=0.9999, ema_warmup=True)                # in warm-up the step size shows t
    opt = make(config, m, **ema_kw)
    avg = wrong = None
    for t in range(3):
        opt.zero_grad()
        TG.backward(m, 60 + t)
        if avg is None:
            avg, wrong = E.Average(weights(m)), E.Average(weights(m))
        if t == 1:
            m.blocks[0].mlp.w1.weight.grad.view(-1)[5] = NAN
            before_w, before_e = weights(m), averages(opt, m)
        opt.step()
        if t == 1:
            torch.cuda.synchronize()
            assert int(opt.skipped_steps) == 1
            assert np.array_equal(E.f32bits(weights(m)), E.f32bits(before_w))
            assert np.array_equal(E.f32bits(averages(opt, m)), E.f32bits(before_e)), "a skipped step moved the average"
        avg.step(weights(m), 0.9999, True, t + 1, apply_=t != 1)
        wrong.step(weights(m), 0.9999, True, t + 1)                 # as if the skipped step had counted
    got = averages(opt, m)
    print(f"[ema opt] {kind} {config} NaN at step 2: err / bound {avg.ratio(got):.3f}, with t advanced {wrong.ratio(got):.3g}")
    assert avg.skipped == 1 and avg.ratio(got) <= 1.0 and wrong.ratio(got) > 1.0


@pytest.mark.parametrize("config", ["plain", "clip"])
def test_frozen_prefixes_stay_bit_equal_to_their_average(config):
    m = TG.tiny("HSIMAE")
    opt = make(config, m, freeze=TG.FROZEN, ema_decay=0.9, ema_warmup=False)
    steps(m, opt, schedule(opt), range(3))
    torch.cuda.synchronize()
    names = [n for n, _ in m.named_parameters()]
    frozen = moved = 0
    for n, off, size in zip(names, m._offs, m._sizes):
        same = torch.equal(bits(opt.ema[off:off + size]), bits(m._flat[off:off + size]))
        if n.startswith(TG.FROZEN) or n == "mask_token":
            assert same, f"{n}: frozen, and its average left it"
            frozen += 1
        else:
            moved += int(not same)
    assert frozen > 5 and moved > 40


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_the_average_never_feeds_back_into_the_weights(kind, config, monkeypatch):
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    ma, mb = TG.tiny(kind), TG.tiny(kind)
    ma.deterministic = mb.deterministic = True
    oa, ob = make(config, ma), make(config, mb, **EMA[config])
    steps(ma, oa, schedule(oa), range(3))
    steps(mb, ob, schedule(ob), range(3))
    torch.cuda.synchronize()
    assert np.array_equal(E.f32bits(weights(ma)), E.f32bits(weights(mb)))
    assert torch.equal(bits(oa.exp_avg), bits(ob.exp_avg)) and torch.equal(bits(oa.exp_avg_sq), bits(ob.exp_avg_sq))
    assert oa.ema is None and "ema" not in oa.state_dict() and ob.ema is not None


@pytest.mark.parametrize("kind,config", [("HSIMAE", "plain"), ("HSIMAE", "clip"), ("HSIMAE", "lamb"), ("DualViT", "clip"), ("DualViT", "lamb")])
def test_step_with_the_average_issues_no_torch_op_and_no_host_wait(kind, config):
    """(DualViT's plain mode steps its head with torch.optim.AdamW, which is made of torch ops: the average adds none to them,
    see the count below.)"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    m = TG.tiny(kind)
    opt = make(config, m, **EMA[config])
    for k in range(2):
        opt.zero_grad()
        TG.backward(m, k)
        if k == 0:
            opt.step()
            continue
        before = opt.ema.clone()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with Count() as c:
                opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert c.ops == [], c.ops[:8]
        assert not torch.equal(before, opt.ema)


def test_the_average_adds_no_torch_op_to_the_plain_dualvit_step():
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.ops.append(str(func))
            return func(*args, **(kwargs or {}))

    counts = []
    for kw in ({}, EMA["plain"]):
        m = TG.tiny("DualViT")
        opt = make("plain", m, **kw)
        for k in range(2):
            opt.zero_grad()
            TG.backward(m, k)
            if k == 0:
                opt.step()
                continue
            with Count() as c:
                opt.step()
            counts.append(list(c.ops))
    assert counts[0] == counts[1] and len(counts[0]) > 0


def eval_forward(m, kind, x, noise, grid):
    m.eval()
    with torch.no_grad():
        out = (m(x),) if kind == "DualViT" else m(x, 0.5, noise=noise, grid=grid)[:2]
    m.train()
    return [o.detach().clone() for o in out]


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_inside_swap_ema_is_the_forward_of_a_model_loaded_from_the_average(kind, config, monkeypatch):
    """A forward right before the swap leaves the packed bf16 images (and DualViT's packed head) of the RAW weights behind: the
    forward inside must not use them.  On leaving, weights and forward are what they were, bit for bit."""
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    m = TG.tiny(kind)
    m.deterministic = True
    opt = make(config, m, **EMA[config])
    steps(m, opt, schedule(opt), range(3))
    g = torch.Generator().manual_seed(3)
    x = torch.rand(16, 1, 32, 9, 9, generator=g).to(DEV)
    T, L = m.input_size[0], m.input_size[1] ** 2
    noise = (torch.rand(16, T, generator=g), torch.rand(16, L, generator=g))
    grid = m.grid_candidates(T, L, 0.5)[0]
    if kind == "DualViT" and config != "plain":
        # The clipped and LAMB steps write cls_head through its data pointer, which DualViT._packed_head's key (Parameter._version)
        # does not see: without this line "before" would be the forward of a head packed steps ago.  Not this feature's business.
        m._head_pack = None
    w_before = bits(torch.from_numpy(weights(m))).clone()
    before = eval_forward(m, kind, x, noise, grid)
    with opt.swap_ema():
        inside = eval_forward(m, kind, x, noise, grid)
        assert np.array_equal(E.f32bits(weights(m)), E.f32bits(averages_from_state(opt.ema_state_dict(), m)))
        with pytest.raises(RuntimeError, match="swap_ema"):
            opt.step()
        with pytest.raises(RuntimeError, match="swap_ema"):
            with opt.swap_ema():
                pass
    after = eval_forward(m, kind, x, noise, grid)
    assert torch.equal(bits(torch.from_numpy(weights(m))), w_before)
    assert same_bits(before, after)
    fresh = TG.tiny(kind)
    fresh.deterministic = True
    sd = opt.ema_state_dict()
    ref = m.state_dict()
    assert list(sd) == list(ref) and all(v.dtype == ref[k].dtype and v.shape == ref[k].shape for k, v in sd.items())
    fresh.load_state_dict(sd)
    want = eval_forward(fresh, kind, x, noise, grid)
    assert same_bits(inside, want)
    assert not same_bits(inside, before)


def averages_from_state(sd, m):
    """A state_dict as weights(m) lays the model out."""
    names = [n for n, _ in m.named_parameters() if not n.startswith("cls_head.")]
    flat = torch.zeros_like(m._flat)
    for n, off, size in zip(names, m._offs, m._sizes):
        flat[off:off + size] = sd[n].reshape(-1)
    return torch.cat([flat] + [sd[n].reshape(-1) for n, _ in m.named_parameters() if n.startswith("cls_head.")]).cpu().numpy()


def test_ema_state_dict_loads_into_the_evaluation_model_key_filtered():
    from hsimae_amd import HSIViT
    m = TG.tiny("DualViT")
    opt = make("plain", m, **EMA["plain"])
    steps(m, opt, schedule(opt), range(2))
    sd = opt.ema_state_dict()
    kw = {k: v for k, v in TG.MODEL_KW.items() if k in ("img_size", "patch_size", "in_chans", "bands", "b_patch_size", "embed_dim", "depth",
                                                           "s_depth", "num_heads")}
    with contextlib.redirect_stdout(io.StringIO()):
        ev = HSIViT(num_class=4, **kw).to(DEV)
    own = ev.state_dict()
    own.update({k: v for k, v in sd.items() if k in own})           # as test_model does
    ev.load_state_dict(own)
    ev.eval()
    x = torch.rand(8, 1, 32, 9, 9, generator=torch.Generator().manual_seed(1)).to(DEV)
    with opt.swap_ema():
        m.eval()
        with torch.no_grad():
            want = m(x).clone()
        m.train()
    assert torch.equal(bits(ev(x)), bits(want))


def test_ema_decay_is_validated_and_an_optimizer_without_it_has_no_average():
    from hsimae_amd import FusedAdamW, FusedLAMB
    m = TG.tiny("HSIMAE")
    for bad in (1.0, -0.1, NAN, 2, "0.9", True):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(m, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        FusedLAMB(m, ema_decay=1.5)
    assert FusedAdamW(m, ema_decay=0).ema_decay == 0.0
    opt = FusedAdamW(m)
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.ema_state_dict()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with opt.swap_ema():
            pass


# ------------------------------------------------------------------------------------------------ 4. state_dict
@pytest.mark.parametrize("kind,config", [("HSIMAE", "plain"), ("DualViT", "clip"), ("HSIMAE", "lamb")])
def test_state_dict_resumes_the_average_bit_for_bit(kind, config, monkeypatch):
    """2 steps, save, load into a fresh optimizer, 2 more: the weights and the averages of 4 uninterrupted steps, bit for bit, in
    deterministic mode.  A checkpoint without an average starts one from the loaded weights; an optimizer without ema_decay
    ignores the keys."""
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    ma, mb = TG.tiny(kind), TG.tiny(kind)
    ma.deterministic = mb.deterministic = True
    oa = make(config, ma, **EMA[config])
    sa = schedule(oa)
    steps(ma, oa, sa, (0, 1, 2, 3))
    ob = make(config, mb, **EMA[config])
    sb = schedule(ob)
    steps(mb, ob, sb, (0, 1))
    blob = io.BytesIO()
    torch.save({"opt": ob.state_dict(), "sched": sb.state_dict()}, blob)
    blob.seek(0)
    sd = torch.load(blob, map_location="cpu", weights_only=False)
    assert sd["opt"]["ema_decay"] == EMA[config]["ema_decay"] and sd["opt"]["ema"].numel() == mb._flat.numel()
    assert len(sd["opt"]["outside_ema"]) == (2 if kind == "DualViT" else 0)
    fresh = make(config, mb, **EMA[config])
    fs = schedule(fresh)
    fresh.load_state_dict(sd["opt"])
    fs.load_state_dict(sd["sched"])
    steps(mb, fresh, fs, (2, 3))
    torch.cuda.synchronize()
    assert np.array_equal(E.f32bits(weights(ma)), E.f32bits(weights(mb)))
    assert np.array_equal(E.f32bits(averages(oa, ma)), E.f32bits(averages(fresh, mb)))
    # a checkpoint written without the feature: the average starts from the weights as loaded
    plain_sd = {k: v for k, v in sd["opt"].items() if k not in ("ema", "outside_ema", "ema_decay")}
    late = make(config, mb, **EMA[config])
    late.load_state_dict(plain_sd)
    late._bind()
    assert np.array_equal(E.f32bits(averages(late, mb)), E.f32bits(weights(mb)))
    # ... and an optimizer without the feature ignores the keys
    none = make(config, mb)
    blob.seek(0)
    none.load_state_dict(torch.load(blob, map_location="cpu", weights_only=False)["opt"])
    assert none.ema is None and "ema" not in none.state_dict()


# ------------------------------------------------------------------------------------------------ 5. the loops
def spy_on_validated_weights(monkeypatch):
    """Every swap_ema() of the loop records the weights the model holds inside it: what that epoch validates."""
    from hsimae_amd import FusedAdamW
    real, seen = FusedAdamW.swap_ema, []

    @contextlib.contextmanager
    def spy(self):
        with real(self) as o:
            seen.append({k: v.detach().clone().cpu() for k, v in self.model.state_dict().items()})
            yield o
    monkeypatch.setattr(FusedAdamW, "swap_ema", spy)
    return seen


@pytest.mark.parametrize("source", ["cubes", "scene"])
def test_finetuning_loop_writes_the_average_and_keeps_its_best_epoch(source, tmp_path, monkeypatch):
    import test_gpu_scene_data as TS
    from hsimae_amd import dual_branch_finetuning, dual_branch_finetuning_scene, test_model_scene
    from hsimae_amd.finetune_train import best_epoch
    seen = spy_on_validated_weights(monkeypatch)
    lines = []
    kw = dict(TC.LOOP_KW, epochs=3, ema_decay=0.9, keep_best=True, log=lambda *a: lines.append(" ".join(map(str, a))))
    scene, labeled, gt = TS.toy_scene()
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        if source == "cubes":
            out = dual_branch_finetuning(*TC.toy_set(), str(tmp_path), "ft.pkl", **kw)
        else:
            out = dual_branch_finetuning_scene(scene, list(labeled), gt, str(tmp_path), "ft.pkl", **kw)
    assert len(out) == 3 and len(out[0]) == 4 and len(out[1]) == 3 and len(out[2]) == 3
    raw, ema, best = (torch.load(os.path.join(str(tmp_path), f), map_location="cpu") for f in ("ft.pkl", "ft_ema.pkl", "ft_best.pkl"))
    for other in (ema, best):
        assert list(other) == list(raw) and all(v.dtype == raw[k].dtype and v.shape == raw[k].shape for k, v in other.items())
        assert all(bool(torch.isfinite(v).all()) for v in other.values())
    assert any(not torch.equal(ema[k], raw[k]) for k in raw) and not torch.equal(ema["cls_head.weight"], raw["cls_head.weight"])
    val = [re.search(r"epoch (\d+): validated on the EMA weights.* val_aa (\S+)$", ln) for ln in lines]
    val = [(int(h.group(1)), float(h.group(2))) for h in val if h]
    assert [e for e, _ in val] == [0, 1, 2], lines
    assert abs(val[-1][1] - sum(out[0][:3]) / 3) < 1e-6             # the returned scores are the last epoch's, as before
    logged = [re.search(r"best epoch (\d+): val_aa (\S+) on the EMA weights", ln) for ln in lines]
    logged = [h for h in logged if h]
    assert len(logged) == 1, lines
    at = int(logged[0].group(1))
    assert at == best_epoch([s for _, s in val])
    assert len(seen) == 3
    for k in raw:
        assert torch.equal(bits(best[k]), bits(seen[at][k])), f"{k}: _best is not what epoch {at} validated"
        assert torch.equal(bits(ema[k]), bits(seen[2][k])), f"{k}: _ema is not the average after the last epoch"
    gt_map = np.zeros(18 * 18, dtype=np.int64)
    gt_map[labeled] = gt
    gt_map = gt_map.reshape(18, 18)
    with contextlib.redirect_stdout(io.StringIO()):
        res = test_model_scene(scene, gt_map, gt_map, str(tmp_path), "ft_ema.pkl", depth=4, dim=64, s_depth=2, batch_size=256)
    assert 0.0 <= res[0] <= 1.0 and res[4].shape == (18, 18)


def test_keep_best_without_the_average_snapshots_the_raw_weights(tmp_path):
    from hsimae_amd import dual_branch_finetuning
    from hsimae_amd.finetune_train import best_epoch
    lines = []
    kw = dict(TC.LOOP_KW, keep_best=True, log=lambda *a: lines.append(" ".join(map(str, a))))
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        dual_branch_finetuning(*TC.toy_set(), str(tmp_path), "ft.pkl", **kw)
    assert not os.path.exists(os.path.join(str(tmp_path), "ft_ema.pkl"))
    raw, best = (torch.load(os.path.join(str(tmp_path), f), map_location="cpu") for f in ("ft.pkl", "ft_best.pkl"))
    val = [float(h.group(1)) for h in (re.search(r"validated on the raw weights.* val_aa (\S+)$", ln) for ln in lines) if h]
    at = int(next(h for h in (re.search(r"best epoch (\d+)", ln) for ln in lines) if h).group(1))
    assert len(val) == 2 and at == best_epoch(val) and list(best) == list(raw)
    if at == 1:                                                      # the last epoch: the snapshot is the file itself
        assert all(torch.equal(bits(best[k]), bits(raw[k])) for k in raw)
    else:
        assert any(not torch.equal(best[k], raw[k]) for k in raw)


def test_resumed_pretraining_writes_the_same_average_as_an_uninterrupted_run(tmp_path, monkeypatch):
    import hsimae_amd
    import hsimae_amd.pretrain as P
    import test_gpu_lamb as TL
    from hsimae_amd.pretrain import seed_everything
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")

    def run(*a, **k):
        seed_everything(0)
        return hsimae_amd.mask_pretraining(*a, ema_decay=0.9, log=lambda *_: None, **TL.LOOP_KW, **k)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    run(TL.cubes(), d1, "m.pkl", epochs=2)
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
            run(TL.cubes(), d2, "m.pkl", epochs=2, resume_path=ck)
    finally:
        P.save_resume, P.save_final = real_save, real_final
    saved = torch.load(ck, map_location="cpu", weights_only=False)["optimizer"]
    assert saved["ema_decay"] == 0.9 and saved["ema"] is not None
    assert not os.path.exists(os.path.join(d2, "m_ema.pkl"))
    run(TL.cubes(), d2, "m.pkl", epochs=2, resume_path=ck)
    a, b = (torch.load(os.path.join(d, "m_ema.pkl"), map_location="cpu") for d in (d1, d2))
    raw = torch.load(os.path.join(d1, "m.pkl"), map_location="cpu")
    assert list(a) == list(b) == list(raw)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert any(not torch.equal(a[k], raw[k]) for k in raw)
