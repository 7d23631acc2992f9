"""The element-wise bound of tests/wgrad_ref.py can tell a wrong weight gradient from a right one (pure torch on the CPU).

It must accept an fp32 emulation of the kernels' order at the shapes of the GPU matrix (tests/test_gpu_wgrad.py): 32-row MFMA
steps with one rounding each, P row slices, the slices' partial sums added one after another onto the initial value.  And it
must reject each structural mistake a split-M tiled kernel makes: the ragged last row lost, a 32-row step lost, a slice
committed twice, an 8-column piece of A read one column off, a pad column of dO leaking into the last valid column, a bias
short of one row, an edge tile's bias taken from the tile before it, a row factor applied on the wrong side of the bf16
rounding.  The last part pins `expected`, the restatement of hs_wgrad's launch rule, on a table that names every path.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as R  # noqa: E402

BLOCK128 = [(128, 128)] * 4 + [(344, 128)] * 2 + [(128, 344)]          # q, k, v, proj, w1, w3, w2 at d = 128, h = 344
BLOCK256 = [(256, 256)] * 4 + [(680, 256)] * 2 + [(256, 680)]          # ... at d = 256, h = 680

# (id, M, N, K, the launch's tasks, msplit, slab, f32 dO, aligned, rowscale): the GPU matrix's shapes, one task of each block batch
SHAPES = [
    ("reg-45", 45, 72, 64, [(72, 64, 1)], 3, False, True, True, False),
    ("reg-333", 333, 136, 72, [(136, 72, 1)], 2, False, True, True, False),
    ("reg-1", 1, 128, 128, [(128, 128, 1)], 1, False, True, True, False),
    ("reg-rowscale", 333, 136, 72, [(136, 72, 1)], 2, False, True, True, True),
    ("reg-unaligned", 333, 136, 72, [(136, 72)], 2, False, False, False, False),
    ("dma6-45", 45, 72, 64, [(72, 64)], 3, False, False, True, False),
    ("dma6-610", 610, 344, 136, [(344, 136)], 1, False, False, True, False),
    ("dma6-1000", 1000, 128, 128, [(128, 128)], 8, False, False, True, False),
    ("dma6-block-w1", 333, 344, 128, BLOCK128, 3, False, False, True, False),
    ("dma3-block-w2", 2733, 128, 344, BLOCK128, 17, False, False, True, False),
    ("dma3-block-w1", 2733, 344, 128, BLOCK128, 24, False, False, True, False),
    ("big-200", 200, 256, 256, [(256, 256)], 8, True, False, True, False),
    ("big-333", 333, 344, 264, [(344, 264)], 8, False, False, True, False),
    ("big-1500", 1500, 256, 696, [(256, 696)], 8, False, False, True, False),
    ("big-block-w2", 3685, 256, 680, BLOCK256, 8, False, False, True, False),
    ("slab-256", 256, 256, 256, [(256, 256)], 8, True, False, True, False),
    ("slab-357", 357, 256, 256, [(256, 256)], 8, True, False, True, False),
    ("slab-325", 325, 344, 264, [(344, 264)], 8, True, False, True, False),
    ("slab-block-w1", 3685, 680, 256, BLOCK256, 8, True, False, True, False),
]
RS = [0.0, 1.0, 1.0 / 0.9, 1.0 / 0.7, 1.3]                 # DropPath factors: 0, 1 and non-powers of two


def operands(M, N, K, f32, rowscale, seed=0):
    g = torch.Generator().manual_seed(seed)
    dO = torch.randn(M, N, generator=g) * 0.5 + 0.05       # a mean offset: dropped terms and sign errors do not cancel
    A = R.bf(torch.randn(M, K, generator=g) * 0.5 + 0.05)
    dW0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    rs = torch.tensor(RS)[torch.arange(M) % len(RS)] if rowscale else None
    if not f32:
        dO = dO.to(torch.bfloat16)
    return dO, A, dW0, db0, rs


def emulate(d, a, dW0, db0, path, P, S, dup_slice=None):
    """The kernels' order in fp32: per slice a running sum with one rounding per 32-row step, then the slices onto dW0 / db0
    one after another.  Bias: the same against ones; on `reg` row after row in two halves of each 64-row chunk."""
    M = d.shape[0]
    dW, db = dW0.clone(), db0.clone()
    order = list(range(P)) + ([dup_slice] if dup_slice is not None else [])
    for p in order:
        r0, r1 = min(M, p * S * 32), min(M, (p + 1) * S * 32)
        accW = torch.zeros_like(dW0)
        accb = [torch.zeros_like(db0), torch.zeros_like(db0)]
        for s in range(r0, r1, 32):
            ds, as_ = d[s:min(s + 32, r1)].double(), a[s:min(s + 32, r1)].double()
            accW = (accW.double() + ds.t() @ as_).float()              # exact products, one rounding of the running sum
            if path == "reg":
                h = (s // 32) % 2
                for row in d[s:min(s + 32, r1)]:
                    accb[h] = accb[h] + row
            else:
                accb[0] = (accb[0].double() + ds.sum(0)).float()
        dW = dW + accW
        db = db + accb[0]
        if path == "reg":
            db = db + accb[1]
    return dW, db


def setup(shape):
    sid, M, N, K, tasks, msplit, slab, f32, aligned, rowscale = shape
    path, P, S = R.expected(tasks, M, msplit, slab, aligned)
    dO, A, dW0, db0, rs = operands(M, N, K, f32, rowscale)
    d = R.operand(dO, rs)
    dW64, db64, absW, absb = R.ref64(dO, A, N, K, dW0, db0, rs)
    bW, bb = R.bound_dW(path, P, S, absW, dW0), R.bound_db(path, P, S, M, absb, db0)
    return dict(M=M, N=N, K=K, path=path, P=P, S=S, dO=dO, A=A, d=d, dW0=dW0, db0=db0, rs=rs, dW64=dW64, db64=db64, bW=bW, bb=bb)


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_bound_accepts_the_kernels_order(shape):
    c = setup(shape)
    assert c["path"] == shape[0].split("-")[0].replace("slab", "big_slab")
    dW, db = emulate(c["d"], c["A"], c["dW0"], c["db0"], c["path"], c["P"], c["S"])
    rW, rb = R.ratio(dW, c["dW64"], c["bW"]), R.ratio(db, c["db64"], c["bb"])
    print(f"RATIO emulation {shape[0]:<16s} dW={rW:.4f} db={rb:.4f}")
    assert rW <= 1 and rb <= 1, (rW, rb)
    # deterministic commits: every addend rounded to a multiple of 2^-44, summed exactly
    P, S, M = c["P"], c["S"], c["M"]
    q = torch.zeros_like(c["dW64"])
    for p in range(P):
        part, _ = emulate(c["d"][p * S * 32:(p + 1) * S * 32], c["A"][p * S * 32:(p + 1) * S * 32], torch.zeros_like(c["dW0"]),
                          torch.zeros_like(c["db0"]), c["path"], 1, S)
        q += torch.round(part.double() * 2.0 ** 44)
    det = c["dW0"].double() + q * R.DET_ULP
    absW = R.ref64(c["dO"], c["A"], c["N"], c["K"], None, None, c["rs"])[2]
    assert R.ratio(det, c["dW64"], R.bound_dW(c["path"], P, S, absW, c["dW0"], det=True)) <= 1


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_bound_rejects_structural_mistakes(shape):
    c = setup(shape)
    M, N, K, path, P, S = c["M"], c["N"], c["K"], c["path"], c["P"], c["S"]
    d, a = c["d"], c["A"]
    T = 256 if path.startswith("big") else 128

    def run(dd=d, aa=a, **kw):
        dW, db = emulate(dd, aa, c["dW0"], c["db0"], path, P, S, **kw)
        return R.ratio(dW, c["dW64"], c["bW"]), R.ratio(db, c["db64"], c["bb"])

    # the last row (the ragged chunk) left out
    d2 = d.clone()
    d2[M - 1] = 0
    rW, rb = run(d2)
    assert rW > 1 and rb > 1, ("last row", rW, rb)
    # one 32-row step left out in the middle of a slice
    if M > 32:
        s = min(S, R.cdiv(M, 32)) // 2 * 32
        d2 = d.clone()
        d2[s:s + 32] = 0
        assert run(d2)[0] > 1, "step"
    # one slice committed twice
    assert run(dup_slice=0)[0] > 1, "slice twice"
    # one 8-column piece of A read one column off
    a2 = a.clone()
    a2[:, 8:16] = a[:, 9:17]
    assert run(aa=a2)[0] > 1, "A one column off"
    # one pad column of dO (value 1.0) added into column N - 1
    d2 = d.clone()
    d2[:, N - 1] += 1.0
    rW, rb = run(d2)
    assert rW > 1 and rb > 1, ("pad column", rW, rb)
    # the bias summed over M - 1 rows
    good_W, good_b = emulate(d, a, c["dW0"], c["db0"], path, P, S)
    d2 = d.clone()
    d2[M - 1] = 0
    short_b = emulate(d2, a, c["dW0"], c["db0"], path, P, S)[1]
    assert R.ratio(short_b, c["db64"], c["bb"]) > 1, "bias over M - 1 rows"
    # the bias of an edge tile taken from the previous tile
    if N > T:
        e = (N - 1) // T * T
        bad = good_b.clone()
        bad[e:] = good_b[e - T:e - T + (N - e)]
        assert R.ratio(bad, c["db64"], c["bb"]) > 1, "edge tile's bias"
    # the row factor applied after the bf16 rounding instead of before
    if c["rs"] is not None:
        d2 = R.bf(R.bf(c["dO"]) * c["rs"][:, None])
        assert not torch.equal(d2, d)
        rW, rb = run(d2)
        print(f"RATIO rowscale-after-rounding dW={rW:.3g} db={rb:.3g}")
        assert rW > 1 and rb > 1, ("rowscale after the rounding", rW, rb)


def test_row_factor_zero_and_one_are_exact():
    dO, A, dW0, db0, rs = operands(40, 16, 16, True, True)
    d = R.operand(dO, rs)
    assert torch.equal(d[0], torch.zeros(16)) and torch.equal(d[1], R.bf(dO[1]))


DISPATCH = [
    # tasks, M, msplit, slab, aligned -> (path, P, S)
    ([(72, 64, 1)], 45, 3, False, True, ("reg", 3, 2)),
    ([(136, 72, 1)], 333, 2, False, True, ("reg", 2, 6)),
    ([(128, 128, 1)], 1, 1, False, True, ("reg", 1, 2)),
    ([(136, 72)], 333, 2, False, False, ("reg", 2, 6)),                   # a pointer with addr & 15
    ([(72, 64, 1), (136, 72)], 333, 2, False, True, ("reg", 2, 6)),       # one fp32 task takes the whole launch
    ([(256, 256, 1)], 1500, 3, True, True, ("reg", 3, 16)),               # fp32 beats the 256-tiles
    ([(72, 64)], 45, 3, False, True, ("dma6", 3, 1)),                     # grid = 8 * ceil(1 / 8) * 3 = 24
    ([(344, 136)], 610, 1, False, True, ("dma6", 1, 20)),                 # grid = 8 * ceil(6 / 8) * 1 = 8
    ([(128, 128)], 1000, 8, False, True, ("dma6", 8, 4)),                 # msplit % 8 == 0: grid = 8 * 1 * 1 = 8
    ([(128, 128)], 1000, 256, False, True, ("dma6", 256, 1)),             # grid = 8 * 1 * 32 = 256: not above 256
    ([(128, 128)], 1000, 264, False, True, ("dma3", 264, 1)),             # grid = 8 * 1 * 33 = 264
    (BLOCK128, 333, 3, False, True, ("dma6", 3, 4)),                      # grid = 8 * 2 * 3 = 48
    (BLOCK128, 2733, 17, False, True, ("dma3", 17, 6)),                   # grid = 8 * 2 * 17 = 272, contiguous parts
    (BLOCK128, 2733, 24, False, True, ("dma3", 24, 4)),                   # grid = 8 * 13 * 3 = 312, XCD groups
    (BLOCK128, 2733, 16, False, True, ("dma6", 16, 6)),                   # grid = 8 * 13 * 2 = 208
    (BLOCK128, 2733, 32, False, True, ("dma3", 32, 3)),                   # the planner's own split: grid = 416
    (BLOCK128, 333, 24, False, True, ("dma3", 24, 1)),                    # more slices than chunks: grid = 312
    (BLOCK256, 1800, 8, False, True, ("big", 19, 3)),
    (BLOCK256, 640, 8, True, True, ("big_slab", 19, 2)),                  # 20 chunks: 10 slices of 2, 9 empty
    ([(256, 256), (128, 256)], 1000, 8, True, True, ("dma6", 8, 4)),      # one narrow task keeps the launch on 128-tiles
    ([(256, 256)], 200, 8, True, True, ("big", 7, 1)),                    # slab given, P = 7 < 8
    ([(256, 256)], 256, 8, False, True, ("big", 8, 1)),                   # no slab given
    ([(256, 256)], 256, 8, True, True, ("big_slab", 8, 1)),
    ([(256, 256)], 357, 8, True, True, ("big_slab", 12, 1)),
    ([(344, 264)], 333, 8, False, True, ("big", 11, 1)),
    ([(344, 264)], 325, 8, True, True, ("big_slab", 11, 1)),
    ([(256, 696)], 1500, 8, False, True, ("big", 47, 1)),
    (BLOCK256, 3685, 8, False, True, ("big", 19, 7)),
    (BLOCK256, 3685, 8, True, True, ("big_slab", 19, 7)),
    ([(5120, 3840)], 3685, 8, True, True, ("big", 1, 116)),               # 300 tiles: t256 * P > 256, slab ignored
]


def test_dispatch_rule():
    for tasks, M, msplit, slab, aligned, want in DISPATCH:
        assert R.expected(tasks, M, msplit, slab, aligned) == want, (tasks, M, msplit, slab, aligned)
    assert {row[5][0] for row in DISPATCH} == set(R.PATHS)
    assert R.tiles(BLOCK128, 128) == 13 and R.tiles(BLOCK256, 256) == 13 and R.tiles(BLOCK256, 128) == 52
    assert R.grid128(13, 17) == 272 and R.grid128(13, 24) == 312
    assert R.plan_msplit(13, 2733) == 32 and R.plan_msplit(13, 333) == 6 and R.plan_msplit(52, 3685) == 8
