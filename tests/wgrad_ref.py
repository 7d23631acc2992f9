"""fp64 reference, element-wise error bound and launch rule of hsimae_wgrad (tests/test_gpu_wgrad.py, tests/test_wgrad_bound_cpu.py).

A plain module, not a conftest: the GPU tests and the CPU test of the bound import the same functions.

hsimae_wgrad accumulates  dW[N][K] += dOb^T A  and  db[N] += colsum(dOb)  over the M token rows, where dOb is the bf16 operand
the matrix core multiplies: a bf16 dO as it is, an fp32 dO times its optional row factor (the product formed in fp32) and then
rounded to bf16.  `ref64` evaluates exactly that in float64.

The bound is derived, not measured.  Products of two bf16 values are exact in fp32, and one 32-row MFMA step adds one rounding
to the running sum (the premise gemm_ref.py states for the same instruction).  A launch cuts the rows into P slices; the
longest slice takes S steps; the P partial sums meet in the element (float atomics, or the slab reduce kernel), and 2 more
roundings are allowed for the commit onto the value the element held:

    |dW - dW64| <= (S + P + 2) * 2^-24 * (|dOb|^T |A| + |dW0|)

db has the same form with colsum|dOb| on the LDS-DMA kernels (their column sums are one more MFMA against ones).  The
register-staged kernel sums the bias row after row in fp32 and commits it from two half-workgroups per slice, so db gets the
any-order bound (M + 2 P + 2) * 2^-24 * (colsum|dOb| + |db0|) there.  Deterministic commits (det_base / det_acc) round each
addend to a multiple of 2^-44: P * 2^-45 more per element (on the register-staged bias the two extra addends per slice
disappear in the slack of the any-order term, thousands of times larger at any magnitude a gradient has).

`expected` restates the rule by which plan_wgrad (csrc/plan.h) picks one of hs_wgrad's five launch paths, and
tests/test_launch_plan_cpu.py holds it against that function.  The rule has one more branch: operands of 4 GB or more
((M + 32) * ld * 2 >= 2^32) fall back to the register-staged kernel whatever their type.  No GPU test that runs in seconds
reaches it, so it has no case here and `expected` does not model it.
"""
import torch

from gemm_ref import U, UB, bf, ratio  # noqa: F401  (re-exported: the tests use R.U, R.bf, R.ratio)

PATHS = ("reg", "dma6", "dma3", "big", "big_slab")
DET_ULP = 2.0 ** -44      # one unit of the fixed-point accumulators (common.h HS_DET_SCALE)


def rup(x, m):
    return (x + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


def tiles(tasks, T):
    """Number of T x T dW tiles of a launch; a task is (N, K) or (N, K, dO_f32)."""
    return sum(cdiv(t[0], T) * cdiv(t[1], T) for t in tasks)


def plan_msplit(ntiles, M):
    """The row split hsimae_backward passes (csrc/plan.h wgrad_msplit, one launch at a time)."""
    chunks = (M + 63) // 64
    ms = max(1, 512 // max(1, ntiles))
    if ms >= 8:
        ms &= ~7
    return max(1, min(ms, chunks))


def grid128(t128, msplit):
    """Workgroups of a launch on 128 x 128 tiles (decode_wg: whole groups of 8 slices, else 8 contiguous parts of the tile list)."""
    return 8 * t128 * (msplit // 8) if msplit % 8 == 0 else 8 * cdiv(t128, 8) * msplit


def expected(tasks, M, msplit, slab, aligned=True):
    """(path, P, S) of the launch hs_wgrad makes: the kernel, the number of row slices whose partial sums meet in one element
    and the number of 32-row MFMA steps of the longest slice."""
    if any(len(t) > 2 and t[2] for t in tasks) or not aligned:
        cpw = cdiv(cdiv(M, 64), msplit)                  # 64-row chunks = 2 steps each
        return "reg", msplit, 2 * cpw
    nch = cdiv(M, 32)
    if all(t[0] >= 256 and t[1] >= 256 for t in tasks):
        t256 = tiles(tasks, 256)
        P = max(1, min(256 // t256, nch))
        path = "big_slab" if slab and t256 * P <= 256 and P >= 8 else "big"
        return path, P, cdiv(nch, P)
    path = "dma3" if grid128(tiles(tasks, 128), msplit) > 256 else "dma6"
    return path, msplit, cdiv(nch, msplit)


def operand(dO, rowscale=None):
    """The dO operand as the kernel multiplies it, in fp32: a bf16 tensor as it is; fp32 values times the row factor (fp32
    product, as load_rows forms it) rounded to bf16 (cvt8)."""
    if dO.dtype == torch.bfloat16:
        assert rowscale is None
        return dO.float()
    d = dO.float()
    if rowscale is not None:
        d = d * rowscale.float()[:, None]
    return bf(d)


def ref64(dO, A, N, K, dW0, db0, rowscale=None):
    """(dW64, db64, absW, absb): dW0 + dOb^T A, db0 + colsum(dOb), |dOb|^T |A| and colsum|dOb| in float64, from the first N
    columns of dO [M, >= N] and the first K of A [M, >= K]."""
    d = operand(dO[:, :N], rowscale).double()
    a = A[:, :K].double()
    dW64 = d.t() @ a
    db64 = d.sum(0)
    if dW0 is not None:
        dW64 = dW64 + dW0.double()
    if db0 is not None:
        db64 = db64 + db0.double()
    return dW64, db64, d.abs().t() @ a.abs(), d.abs().sum(0)


def bound_dW(path, P, S, absW, dW0, det=False):
    b = (S + P + 2) * U * (absW + (dW0.double().abs() if dW0 is not None else 0.0))
    return b + P * DET_ULP / 2 if det else b


def bound_db(path, P, S, M, absb, db0, det=False):
    n = M + 2 * P + 2 if path == "reg" else S + P + 2
    b = n * U * (absb + (db0.double().abs() if db0 is not None else 0.0))
    return b + P * DET_ULP / 2 if det else b
