"""The element-wise bound of tests/gemm_ref.py can tell a wrong GEMM from a right one (pure torch on the CPU).

It must accept an fp32-accumulated product of the bf16 operands at shapes of the GPU matrix, and reject each of the
structural mistakes a tiled kernel makes: a 32-deep k-slice left out, an 8-column octet read one column off, the last row
panel's rows taken from the previous panel, a bias added twice, and a wrong LayerNorm statistic.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as R  # noqa: E402


def operands(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = R.bf(torch.randn(M, K, generator=g) * 0.7 + 0.05)          # not symmetric: a mean offset
    W = R.bf(torch.randn(N, K, generator=g) * 0.1)
    bias = torch.randn(N, generator=g) * 0.3
    return A, W, bias


def fp32_gemm(A, W, bias=None):
    """A correct kernel: fp32 accumulation in 32-deep steps, then the bias."""
    y = torch.zeros(A.shape[0], W.shape[0])
    for k in range(0, A.shape[1], 32):
        y = y + A[:, k:k + 32] @ W[:, k:k + 32].t()
    return y if bias is None else y + bias


def bound_of(A, W, bias):
    y64, ab = R.prod64(A, W)
    y64 = y64 + bias.double()
    return y64, R.acc_bound(A.shape[1], ab) + R.C2 * R.U * (y64.abs() + bias.double().abs())


SHAPES = [(300, 144, 288), (129, 512, 1536), (1000, 16, 3072), (65, 80, 96), (257, 384, 1056)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bound_accepts_fp32_accumulated_product(M, N, K):
    A, W, bias = operands(M, N, K)
    y64, bnd = bound_of(A, W, bias)
    r = R.ratio(fp32_gemm(A, W, bias), y64, bnd)
    assert r <= 1.0, r
    # and a result rounded to bf16 under the bf16 output term
    r = R.ratio(R.bf(fp32_gemm(A, W, bias)), y64, bnd * (1 + R.UB) + R.UB * y64.abs())
    assert r <= 1.0, r


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bound_rejects_structural_mistakes(M, N, K):
    A, W, bias = operands(M, N, K, seed=1)
    y64, bnd = bound_of(A, W, bias)
    good = fp32_gemm(A, W, bias)
    # one 32-deep k-slice left out (the last, partial-chunk one: where a k loop bound goes wrong)
    ks = (K // 32 - 1) * 32
    assert R.ratio(good - A[:, ks:ks + 32] @ W[:, ks:ks + 32].t(), y64, bnd) > 1
    # one 8-column octet read one column off
    if N >= 16:
        bad = good.clone()
        bad[:, 8:16] = fp32_gemm(A, W[9:17], bias[9:17]) if N > 16 else fp32_gemm(A, torch.cat([W[9:16], W[:1]]),
                                                                                       torch.cat([bias[9:16], bias[:1]]))
        assert R.ratio(bad, y64, bnd) > 1
    # the last row panel's rows (64-row panels) taken from the previous panel
    if M > 64:
        last = (M - 1) // 64 * 64
        bad = good.clone()
        bad[last:] = good[last - 64:last - 64 + (M - last)]
        assert R.ratio(bad, y64, bnd) > 1
    # bias added twice
    assert R.ratio(good + bias, y64, bnd) > 1


@pytest.mark.parametrize("K,width", [(128, 0), (96, 72), (160, 144)])
def test_bound_rejects_wrong_layernorm_statistics(K, width):
    """The LayerNorm-prologue output (u_out, bf16) against ln64 under ln_out_bound: the biased variance and the epsilon
    are pinned (a row of small variance makes a missing epsilon visible; at these widths the unbiased variance moves
    the larger |x-hat| by more than a bf16 rounding)."""
    g = torch.Generator().manual_seed(2)
    M = 200
    x = torch.randn(M, K, generator=g) * 2 + 0.3
    x[3] = 0.3                                                 # zero variance
    x[4] = 0.5 + 1e-3 * torch.randn(K, generator=g)            # variance far below epsilon
    x[5] = 1000 + torch.randn(K, generator=g)                  # large mean
    w = width or K
    if width:
        x[:, width:] = 0
    gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    y64, xh, rstd, kappa = R.ln64(x, gamma, beta, width)
    bnd = R.ln_out_bound(y64, xh, kappa, gamma, beta, width)
    good = R.bf(torch.nn.functional.layer_norm(x[:, :w], (w,), gamma[:w], beta[:w], 1e-5))
    good = torch.cat([good, torch.zeros(M, K - w)], 1)
    assert R.ratio(good, y64, bnd) <= 1
    unb, _, _, _ = R.ln64(x, gamma, beta, width, unbiased=True)
    assert R.ratio(R.bf(unb.float()), y64, bnd) > 1
    noeps, _, _, _ = R.ln64(x, gamma, beta, width, eps=0.0)
    assert R.ratio(R.bf(noeps.float()), y64, bnd) > 1
    # statistics over the padded storage width instead of the LayerNorm's width
    if width:
        wide, _, _, _ = R.ln64(x, gamma, beta, None)
        wide[:, width:] = 0
        assert R.ratio(R.bf(wide.float()), y64, bnd) > 1


def test_layernorm_backward_bound_accepts_fp32_and_rejects_a_wrong_mean():
    g = torch.Generator().manual_seed(3)
    M, N, K = 300, 256, 384
    A, W, _ = operands(M, N, K, seed=3)
    x = torch.randn(M, N, generator=g) * 2 + 0.5
    x[7] = 100 + torch.randn(N, generator=g)
    gamma = 1 + 0.1 * torch.randn(N, generator=g)
    du64, ab = R.prod64(A, W)
    dx64, dg64, db64, xhat, rstd, kappa = R.ln_bwd64(du64, x, gamma, N)
    bnd = R.ln_bwd_bound(R.acc_bound(K, ab), du64, xhat, rstd, kappa, gamma)
    du = fp32_gemm(A, W)
    xv = x - x.mean(1, keepdim=True)
    rs = torch.rsqrt(xv.pow(2).mean(1, keepdim=True) + 1e-5)
    xh = xv * rs
    t = du * gamma
    dx = rs * (t - t.mean(1, keepdim=True) - xh * (t * xh).mean(1, keepdim=True))
    assert R.ratio(dx, dx64, bnd) <= 1
    bad = rs * (t - xh * (t * xh).mean(1, keepdim=True))      # the mean of t left out
    assert R.ratio(bad, dx64, bnd) > 1
