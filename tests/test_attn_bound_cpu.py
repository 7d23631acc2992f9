"""The attention error bound of tests/attn_ref.py on the CPU: it accepts what the kernels compute (an fp32 emulation with their
bf16 roundings) and rejects each planted fault a subtly wrong kernel could make — a key from the neighbouring sample, a class
boundary one token off, the ragged last key tile dropped, two heads swapped, lse in natural units, the DropPath factor
missing, delta from the wrong row, the LayerNorm-1 backward without its mean term."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

CASES = [(32, 2, 27, 1, 9), (32, 2, 27, 2, 9), (64, 4, 20, 0, 1), (16, 2, 40, 1, 7)]     # d, heads, Ts, mode, len_l (hd 16 / 16 / 16 / 8)
N = 3


def inputs(d, Ts, seed, spread=1.5):
    g = torch.Generator().manual_seed(seed)
    qkv = R.bf(torch.randn(N * Ts, 3 * d, generator=g) * spread)
    dout = R.bf(torch.randn(N * Ts, d, generator=g))
    return qkv, dout


def fwd_ratios(qkv, d, heads, Ts, mode, len_l, o, lse):
    ref = R.attn_fwd64(qkv, d, heads, Ts, mode, len_l)
    return R.ratio(o, ref["o"], ref["bo"]), R.ratio(lse, ref["lse"], ref["blse"])


def bwd_worst(qkv, dout, lse, d, heads, Ts, mode, len_l, got, pdp=True, o=None):
    ref = R.attn_bwd64(qkv, dout, lse, d, heads, Ts, mode, len_l, pdp=pdp, o=o)
    return max(R.ratio(g, ref[n], ref["b" + n]) for g, n in zip(got, ("dq", "dk", "dv")))


@pytest.mark.parametrize("case", CASES)
def test_bound_accepts_the_kernels_arithmetic(case):
    d, heads, Ts, mode, len_l = case
    for seed, spread in ((1, 1.5), (2, 6.0)):            # spread 6: scores over about +-80 in log2 units
        qkv, dout = inputs(d, Ts, seed, spread)
        o, lse = R.emu_fwd(qkv, d, heads, Ts, mode, len_l)
        ro, rl = fwd_ratios(qkv, d, heads, Ts, mode, len_l, o, lse)
        assert ro <= 1 and rl <= 1, (ro, rl)
        assert ro > 0.05, f"bound on o is loose: worst err / bound {ro:.3g}"
        for pdp in (True, False):
            got = R.emu_bwd(qkv, dout, lse, d, heads, Ts, mode, len_l, pdp=pdp, o=o)
            r = bwd_worst(qkv, dout, lse, d, heads, Ts, mode, len_l, got, pdp, o)
            assert 0.05 < r <= 1, (pdp, r)


def test_neighbouring_sample_key_is_rejected():
    d, heads, Ts, mode, len_l = CASES[0]
    qkv, _ = inputs(d, Ts, 3)
    bad = qkv.clone()
    bad[Ts - 1, d:2 * d] = qkv[Ts, d:2 * d]                  # the last key of sample 0 read from sample 1's first row
    o, lse = R.emu_fwd(bad, d, heads, Ts, mode, len_l)
    ro, rl = fwd_ratios(qkv, d, heads, Ts, mode, len_l, o, lse)
    assert ro > 1 and rl > 1


@pytest.mark.parametrize("mode", [1, 2])
def test_class_boundary_one_token_off_is_rejected(mode):
    d, heads, Ts, len_l = 32, 2, 27, 9
    qkv, _ = inputs(d, Ts, 4)
    cls = R.classes(Ts, mode, len_l)
    if mode == 1:
        cls[len_l] = 0                                        # the first token of class 1 counted in class 0
    else:
        cls[len_l - 1], cls[len_l] = cls[len_l], cls[len_l - 1]
    o, lse = R.emu_fwd(qkv, d, heads, Ts, mode, len_l, cls=cls)
    ro, rl = fwd_ratios(qkv, d, heads, Ts, mode, len_l, o, lse)
    assert ro > 1 and rl > 1


def test_dropped_last_key_tile_is_rejected():
    d, heads, Ts, mode, len_l = 32, 2, 20, 0, 1              # keys 16 .. 19: a ragged second tile
    qkv, _ = inputs(d, Ts, 5)
    o, lse = R.emu_fwd(qkv, d, heads, Ts, mode, len_l, drop_tile=True)
    ro, rl = fwd_ratios(qkv, d, heads, Ts, mode, len_l, o, lse)
    assert ro > 1 and rl > 1


def test_swapped_heads_are_rejected():
    d, heads, Ts, mode, len_l = CASES[2]
    hd = d // heads
    qkv, dout = inputs(d, Ts, 6)
    o, lse = R.emu_fwd(qkv, d, heads, Ts, mode, len_l)
    o2 = o.clone()
    o2[:, :hd], o2[:, hd:2 * hd] = o[:, hd:2 * hd], o[:, :hd]
    assert fwd_ratios(qkv, d, heads, Ts, mode, len_l, o2, lse)[0] > 1
    dq, dk, dv = R.emu_bwd(qkv, dout, lse, d, heads, Ts, mode, len_l)
    dv2 = dv.clone()
    dv2[:, :hd], dv2[:, hd:2 * hd] = dv[:, hd:2 * hd], dv[:, :hd]
    assert bwd_worst(qkv, dout, lse, d, heads, Ts, mode, len_l, (dq, dk, dv2)) > 1


def test_natural_log_lse_is_rejected():
    d, heads, Ts, mode, len_l = CASES[0]
    qkv, _ = inputs(d, Ts, 7)
    o, lse = R.emu_fwd(qkv, d, heads, Ts, mode, len_l)
    assert fwd_ratios(qkv, d, heads, Ts, mode, len_l, o, lse * math.log(2.0))[1] > 1


@pytest.mark.parametrize("pdp", [True, False])
def test_delta_from_the_wrong_row_is_rejected(pdp):
    d, heads, Ts, mode, len_l = CASES[1]
    qkv, dout = inputs(d, Ts, 8)
    o, lse = R.emu_fwd(qkv, d, heads, Ts, mode, len_l)
    got = R.emu_bwd(qkv, dout, lse, d, heads, Ts, mode, len_l, pdp=pdp, o=o, delta_shift=1)
    assert bwd_worst(qkv, dout, lse, d, heads, Ts, mode, len_l, got, pdp, o) > 1


def test_missing_droppath_factor_is_rejected():
    g = torch.Generator().manual_seed(9)
    M, d = 54, 64
    x = torch.randn(M, d, generator=g)
    o = R.bf(torch.randn(M, d, generator=g))
    Wp = torch.randn(d, d, generator=g) * 0.1
    pb = torch.randn(d, generator=g) * 0.1
    rs = torch.tensor([0.0, 1.25]).repeat_interleave(27)
    y = o @ R.bf(Wp).t() + pb
    x1_ok, x1_bad = x + rs[:, None] * y, x + y
    ref, bnd = R.x1_64(x, o, Wp, pb, rs)
    assert R.ratio(x1_ok, ref, bnd) <= 1
    assert R.ratio(x1_bad, ref, bnd) > 1


def test_ln1_backward_without_mean_term_is_rejected():
    g = torch.Generator().manual_seed(10)
    M, d = 40, 64
    dqkv = R.bf(torch.randn(M, 3 * d, generator=g) * 0.1)
    W = torch.randn(3 * d, d, generator=g) * 0.1
    x = torch.randn(M, d, generator=g) * 2 + 0.5
    gamma = 1 + 0.2 * torch.randn(d, generator=g)
    dres = torch.randn(M, d, generator=g)
    du = dqkv @ R.bf(W)
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (x - mean) * rstd
    t = du * gamma
    a, b = t.mean(1, keepdim=True), (t * xh).mean(1, keepdim=True)
    ok, bad = dres + rstd * (t - a - xh * b), dres + rstd * (t - xh * b)
    dx, bdx, dg, bg, db, bb = R.ln1_bwd64(dqkv, W, x, gamma, dres)
    assert R.ratio(ok, dx, bdx) <= 1
    assert R.ratio(bad, dx, bdx) > 1
    assert R.ratio((du * xh).sum(0), dg, bg) <= 1 and R.ratio(du.sum(0), db, bb) <= 1
