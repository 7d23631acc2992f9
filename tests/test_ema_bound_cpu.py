"""tests/ema_ref.py kept honest without a GPU: the restatement against an independently written loop and the closed form, an fp32
emulation of the sequence include/hsimae_hip.h states inside the derived bound, seven planted faults outside it, and the rule by
which the fine-tuning loop keeps its best epoch."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ema_ref as E  # noqa: E402

N = 257
NAN = float("nan")


def fma32(a, s, e):
    """fl32(a s + e) with ONE rounding, for fp32 arrays: the product of two fp32 values is exact in fp64; the fp64 sum is made
    round-to-odd from its exact residual (TwoSum), after which the rounding to fp32 is the correct one."""
    a, s, e = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, s, e))
    prod = a * s
    sm = prod + e
    bb = sm - prod
    res = (prod - (sm - bb)) + (e - bb)
    even = (sm.view(np.int64) & 1) == 0
    fix = (res != 0) & even & np.isfinite(sm)
    sm = np.where(fix, np.nextafter(sm, np.where(res > 0, np.inf, -np.inf)), sm)
    return sm.astype(np.float32)


def emulate(ema, p, decay, warmup, step, skipped=0, apply_=True, fault=None):
    """One hsimae_ema_update in fp32 numpy, as the header states it; `fault` plants one of the mistakes the bound must catch."""
    ema, p = np.asarray(ema, dtype=np.float32), np.asarray(p, dtype=np.float32)
    if not apply_ and fault != "update_on_skip":
        return ema.copy()
    t = step - (0 if fault == "skipped_ignored" else skipped)
    if fault == "t_off_by_one":
        t += 1
    d = decay
    if warmup:
        d = (max if fault == "max_for_min" else min)(decay, (1.0 + t) / (10.0 + t))
    a = np.float32(d if fault == "decay_for_one_minus" else 1.0 - d)
    with np.errstate(all="ignore"):
        r = fma32(a, p - ema, ema)
    if fault == "equal_by_arithmetic":
        return r
    out = np.where(E.f32bits(p) == E.f32bits(ema), ema, r)
    if fault == "equal_perturbed":
        same = np.flatnonzero((E.f32bits(p) == E.f32bits(ema)) & np.isfinite(ema) & (ema != 0))
        out[same[0]] = np.nextafter(out[same[0]], np.float32(np.inf))
    return out


def accepted(avg, before, p, after):
    return avg.ratio(after) <= 1.0 and E.kept(before, p, after)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_restatement_equals_an_independent_loop_and_the_closed_form(decay, warmup):
    rng = np.random.default_rng(3)
    ema0, _ = E.inputs(N, 1)
    ps = [(ema0 + 0.01 * rng.standard_normal(N)).astype(np.float32) for _ in range(20)]
    avg = E.Average(ema0)
    mine = ema0.astype(np.float64)
    for k, p in enumerate(ps):
        avg.step(p, decay, warmup, k + 1)
        d = decay
        if warmup and (1 + (k + 1)) / (10 + (k + 1)) < decay:
            d = (1 + (k + 1)) / (10 + (k + 1))
        mine = d * mine + (1 - d) * p.astype(np.float64)
    assert np.max(np.abs(avg.ref - mine)) <= 1e-12
    const = ps[0].astype(np.float64)
    avg, prod = E.Average(ema0), 1.0
    for k in range(20):
        avg.step(ps[0], decay, warmup, k + 1)
        prod *= E.decay_at(decay, warmup, k + 1)
    assert np.max(np.abs(avg.ref - (const + (ema0.astype(np.float64) - const) * prod))) <= 1e-12


def test_a_skipped_step_moves_neither_the_average_nor_the_count():
    ema0, p = E.inputs(N, 2)
    a, b = E.Average(ema0), E.Average(ema0)
    a.step(p, 0.9999, True, 1).step(p, 0.9999, True, 2, apply_=False).step(p, 0.9999, True, 3)
    b.step(p, 0.9999, True, 1).step(p, 0.9999, True, 2)
    assert a.skipped == 1 and np.array_equal(a.ref, b.ref) and np.array_equal(a.err, b.err)


# ------------------------------------------------------------------------------------------------ the emulation inside the bound
@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_fp32_emulation_of_the_stated_sequence_stays_inside_the_bound(decay, warmup):
    rng = np.random.default_rng(7)
    ema0, p = E.inputs(N, 4)
    ema0[3], p[3] = np.float32(1e-41), np.float32(3e-41)          # denormals: the absolute term of the bound
    avg, cur, worst, skipped = E.Average(ema0), ema0.copy(), 0.0, 0
    for step in range(1, 21):
        apply_ = step not in (4, 9)
        before = cur.copy()
        cur = emulate(cur, p, decay, warmup, step, skipped, apply_)
        skipped += 0 if apply_ else 1
        avg.step(p, decay, warmup, step, apply_)
        assert E.kept(before, p, cur)
        worst = max(worst, avg.ratio(cur))
        p = (p * (1 + 0.02 * rng.standard_normal(N))).astype(np.float32)
        p[::5] = cur[::5]                                          # some elements always sit on their average
    print(f"[ema bound] decay {decay} warm-up {warmup}: worst err / bound over 20 steps {worst:.3f}")
    assert worst <= 1.0
    assert avg.skipped == 2


# ------------------------------------------------------------------------------------------------ planted faults
FAULTS = {  # name -> (decay, warmup, step, skipped, apply)
    "decay_for_one_minus": (0.9, False, 1, 0, True),
    "t_off_by_one": (0.9999, True, 2, 0, True),
    "max_for_min": (0.9, True, 2, 0, True),
    "skipped_ignored": (0.9999, True, 10, 3, True),
    "update_on_skip": (0.9, False, 2, 1, False),
    "equal_perturbed": (0.9, False, 1, 0, True),
    "equal_by_arithmetic": (0.9, False, 1, 0, True),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_planted_fault_leaves_the_bound(fault):
    decay, warmup, step, skipped, apply_ = FAULTS[fault]
    ema0, p = E.inputs(N, 11)
    ema0[5] = p[5] = np.float32(-0.0)                              # arithmetic turns it into +0.0
    good = emulate(ema0, p, decay, warmup, step, skipped, apply_)
    bad = emulate(ema0, p, decay, warmup, step, skipped, apply_, fault=fault)

    def verdict(after):
        avg = E.Average(ema0, skipped=skipped - (0 if apply_ else 1))
        avg.step(p, decay, warmup, step, apply_)
        return accepted(avg, ema0, p, after)
    assert verdict(good)
    assert not verdict(bad), fault


def test_a_swap_that_copies_one_way_is_seen():
    a0, b0 = E.inputs(N, 12, equal_every=0)
    a0[7] = np.array([0x7FC01234], dtype=np.uint32).view(np.float32)[0]      # a NaN with a payload
    assert E.swapped(a0, b0, b0.copy(), a0.copy())
    assert not E.swapped(a0, b0, b0.copy(), b0.copy()) and not E.swapped(a0, b0, a0.copy(), a0.copy())
    quiet = a0.copy()
    quiet[7] = np.float32(NAN)                                       # the payload lost on the way
    assert not E.swapped(a0, b0, b0.copy(), quiet)


# ------------------------------------------------------------------------------------------------ the best epoch
def test_best_epoch_is_early_stoppings_rule_with_delta_zero():
    from hsimae_amd.finetune_train import best_epoch, val_score
    assert best_epoch([]) is None
    assert best_epoch([0.5]) == 0
    assert best_epoch([0.5, 0.7, 0.6]) == 1
    assert best_epoch([0.7, 0.7, 0.6]) == 1                          # a tie: the later epoch replaces the snapshot
    assert best_epoch([0.7, 0.6, 0.7, 0.7]) == 3
    assert best_epoch([0.9, 0.8, 0.7]) == 0
    assert best_epoch([0.1, 0.2, 0.3]) == 2
    assert best_epoch([0.4, NAN, 0.3]) == 0                          # a NaN never replaces a number
    assert best_epoch([NAN, 0.1]) == 1 and best_epoch([NAN, 0.1, NAN]) == 1
    assert best_epoch([0.0, -0.0]) == 1
    assert val_score(0.9, 0.6, 0.3) == pytest.approx(0.6) and math.isclose(val_score(1.0, 1.0, 1.0), 1.0)
