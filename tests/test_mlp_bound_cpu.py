"""The bounds of tests/mlp_ref.py, without a GPU: an fp32 emulation of the fused MLP-half kernels' order (mlp_ref.emulate) must
sit inside every bound at all three widths and at each `hidden` edge, and every planted fault must land outside the bound of the
output it corrupts.  One more test restates common.h's silu_nr in float32."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as R  # noqa: E402

WIDTHS = [128, 256, 64]
M = 2 * 48 + 17                                            # two whole panels and a ragged one at every width; all five row factors


def hiddens(d):
    hp = R.SHAPES[d][0]
    return [hp, hp - 31, R.MODEL_HIDDEN[d]]


def ratios(p, inp, out, res2=True, rowscale=True):
    i2 = dict(inp) if rowscale else {**inp, "rs_mlp": None, "rs_attn": None}
    r = R.bwd_ratios(p, i2, out)
    r["x2"] = R.fwd_ratio(p, out["x2"], inp["x1"], inp["res2"] if res2 else None, inp["rs"] if rowscale else None)
    return r


@pytest.mark.parametrize("d", WIDTHS)
def test_the_emulation_is_inside_every_bound(d):
    for i, h in enumerate(hiddens(d)):
        p = R.Mlp(d, h, seed=3 + i)
        for m, res2, rowscale, newton in ((M, True, True, True), (1, False, False, True), (p.R + 1, True, False, False)):
            inp = R.make_inputs(p, m, seed=11 * i + m)
            r = ratios(p, inp, R.emulate(p, inp, res2, rowscale, newton), res2, rowscale)
            print(f"RATIO d={d} hidden={h} M={m} " + " ".join(f"{k} {v:.3f}" for k, v in sorted(r.items())))
            assert len(r) == 10 and all(v <= 1.0 for v in r.values()), r


def test_expected_names_the_seven_instantiations():
    got = set()
    for d in WIDTHS:
        for h in hiddens(d):
            for pr in (0, 200):
                e = R.expected(d, h, pr, True)
                assert e[:3] == (d,) + R.SHAPES[d] and e[3] == (d == 256 and pr > 0)
                got |= {R.fwd_name(e), R.bwd_name(e)}
        assert R.expected(d, h, 200, False)[3] is False        # no planar operands to store: the early form
        assert R.expected(d, R.SHAPES[d][0] - 32, 0) is None and R.expected(d, R.SHAPES[d][0] + 1, 0) is None
    assert R.expected(96, 344) is None
    assert got == R.INSTANTIATIONS and len(got) == 7


# fault -> (width, hidden, the outputs whose bound it must exceed)
PLANTED = {
    "half_chunk_dropped": (128, 344, ("x2", "dx1")),
    "bias_not_zeroed": (128, 321, ("g",)),
    "rs_on_residual": (64, 172, ("x2",)),
    "res2_before_scale": (256, 684, ("x2",)),
    "dyb_unscaled": (128, 344, ("dh1", "dh3", "dx1")),
    "dh_swapped": (256, 684, ("dx1",)),
    "no_derivative_term": (64, 172, ("dh1",)),
    "ln_bwd_no_mean": (128, 344, ("dx1",)),
    "n2b_over_pad_rows": (64, 161, ("g_n2b",)),
    "dx1_scaled_dy": (256, 673, ("dx1",)),
}


def test_every_fault_of_the_emulation_is_planted():
    assert set(PLANTED) == set(R.FAULTS)


@pytest.mark.parametrize("fault", sorted(PLANTED))
def test_a_planted_fault_exceeds_the_bound(fault):
    d, h, hit = PLANTED[fault]
    p = R.Mlp(d, h, seed=5)
    inp = R.make_inputs(p, M, seed=7)
    good = ratios(p, inp, R.emulate(p, inp))
    assert all(v <= 1.0 for v in good.values()), good
    bad = ratios(p, inp, R.emulate(p, inp, fault=fault))
    print(f"FAULT {fault}: " + " ".join(f"{k} {bad[k]:.3g}" for k in hit))
    for k in hit:
        assert bad[k] > 1.0, (fault, k, bad[k])


@pytest.mark.parametrize("d", WIDTHS)
def test_extreme_gate_preactivations(d):
    """Rows of W1 scaled until h1 passes -95 and +95: the fixed formula stays finite and inside the forward bound; the formula
    without the fmin gives NaN."""
    p = R.Mlp(d, R.MODEL_HIDDEN[d], seed=9, w1_scale=(slice(3, 40, 4), 60.0))
    inp = R.make_inputs(p, 50, seed=2)
    h1 = R.fwd_ref(p, inp["x1"], inp["res2"], inp["rs"])[2]
    assert float(h1.min()) < -95 and float(h1.max()) > 95
    x2 = R.emulate(p, inp)["x2"]
    assert bool(torch.isfinite(x2).all()) and R.fwd_ratio(p, x2, inp["x1"], inp["res2"], inp["rs"]) <= 1.0
    assert not bool(torch.isfinite(R.emulate(p, inp, fixed=False)["x2"]).all())


def test_flip_marks_the_values_near_a_rounding_midpoint():
    ulp = 2.0 ** -7                                          # of [1, 2)
    v = torch.tensor([1.0, 1 + ulp / 2 - 1e-6, 1 + ulp / 2 + 1e-6, 1 + ulp / 4, 1 + 1e-7, 2 - ulp / 2 + 1e-7, -(1 + 1.5 * ulp)], dtype=torch.float64)
    assert R.flip(v, torch.full_like(v, 1e-5)).tolist() == [0.0, ulp, ulp, 0.0, 0.0, ulp, ulp]
    # the midpoint under the binade's lower edge (1 - 2^-10) is seen from 1 + 1e-7 once e reaches it
    assert float(R.flip(v[4:5], torch.tensor([2e-3], dtype=torch.float64))) == ulp
    # e at or above half an ulp: e + ulp
    assert float(R.flip(v[:1], torch.tensor([ulp], dtype=torch.float64))) == 2 * ulp
    assert float(R.flip(torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))) == 0.0


# ------------------------------------------------------------------------------------------------ silu_nr in float32
def silu_nr32(a, fixed):
    """common.h silu_nr, instruction by instruction, in float32 (numpy): v_mul, v_exp, v_add, v_rcp, v_fma, [v_min,] v_fma, v_mul."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        a = f(a)
        d = f(1) + np.exp2(f(a * f(-R.LOG2E)), dtype=np.float32)
        r = f(1) / d
        res = f(np.float64(-d) * np.float64(r) + 1.0)       # fma: the product of two floats is exact in float64
        if fixed:
            res = np.fmin(res, f(1))                        # v_min_f32 / fminf: a NaN operand gives the other one
        r = f(np.float64(res) * np.float64(r) + np.float64(r))
        return f(a * r)


def test_silu_nr_is_finite_for_every_finite_argument():
    for a in (-1e4, -100.0, -89.0, -88.0, -20.0, 0.0, 20.0, 100.0):
        ref = a / (1.0 + math.exp(-a)) if a > -700 else 0.0
        got = float(silu_nr32(a, True))
        assert math.isfinite(got) and abs(got - ref) <= R.EPS_FN * abs(ref) + 2.0 ** -100, (a, got, ref)
    assert float(silu_nr32(-3e38, True)) == 0.0              # r = 0, not e^-88: no finite argument is too large
    # the formula before the fix: fma(-inf, 0, 1) is NaN from the first argument whose exponential overflows
    assert math.isnan(float(silu_nr32(-89.0, False))) and math.isnan(float(silu_nr32(-100.0, False)))
    assert math.isfinite(float(silu_nr32(-88.0, False))) and math.isfinite(float(silu_nr32(-80.0, False)))
