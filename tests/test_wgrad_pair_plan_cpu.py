"""The weight gradients of two consecutive encoder blocks go out as ONE launch on the fused d = 128 path (csrc/plan.h
BlockPlan::wgrad_pair, csrc/api.hip WgPair): 14 tasks, 26 tiles of 128 x 128, or 15 tasks and 27 tiles when decoder_embed's
weight gradient rides with the first pair of fusion blocks.  What such a launch looks like is decided by two pure functions of
plan.h, wgrad_msplit (the row split api.hip passes) and plan_wgrad (path and grid), and this test asks the stand-alone sanitizer
build of plan.h (csrc/plan_sched_main.cpp) for their answers, without a GPU:

  * the grid fits one resident wave of workgroups (three per CU: 768), at the flagship M = 110,592 and at M = 162, with one
    launch resident (`concurrent` 1) and with two (the forked axis stacks);
  * the row split is a whole number of groups of 8 slices wherever the one-block launch's was (wgrad.hip places slice ms on XCD
    ms % 8), and the paired launch has as many workgroups as the one-block launch with half the row slices;
  * a launch takes at most 16 tasks: 14 and 15 are accepted, 17 refused;
  * plan_block answers wgrad_pair exactly where the schedule bit is set AND the block runs the fused MLP half with the d = 128
    attention backward kernel: never at d = 256 (256-tiles, slab) or on the layer-at-a-time schedule."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_ref as WR  # noqa: E402
from test_launch_plan_cpu import ask_wgrad, one  # noqa: E402
from test_sched_plan_cpu import GOLDEN, NAMES, Probe, ask_block, golden_rows  # noqa: E402

OK, EDIMS = 0, -1
BLOCK = [(128, 128)] * 4 + [(344, 128)] * 2 + [(128, 344)]         # q, k, v, proj, w1, w3, w2 of a d = 128 block: 13 tiles
DEC_EMBED = (64, 128)                                              # decoder_embed: 1 tile
PAIR = 1 << len(NAMES)                                             # SC_WGRAD_PAIR, the bit after the 15 the older tests sweep
WAVE = 768                                                         # 256 CUs x 3 workgroups of wgrad_dma_kernel<3, false>
MS = (110592, 162)


def planar(tasks, M):
    """The tasks as block_bwd passes them: dh1 | dh3 and g as 64-column planes of M + 48 rows (M a multiple of 32)."""
    if M % 32:
        return tasks
    return [(N, K, 0, 384 if N == 344 else 0, 384 if K == 344 else 0, 0, M + 48 if N == 344 else 0, M + 48 if K == 344 else 0) for N, K in tasks]


@pytest.mark.parametrize("extra", [0, 1], ids=["26-tiles", "27-tiles"])
def test_paired_launch_fits_one_wave(extra):
    tasks = BLOCK + BLOCK + [DEC_EMBED] * extra
    tiles = WR.tiles(tasks, 128)
    assert tiles == 26 + extra and len(tasks) <= 16 and WR.tiles(BLOCK, 128) == 13
    pr = Probe()
    qs = {(M, conc): (pr.ask("S %d %d %d" % (tiles, M, conc), 1), pr.ask("S 13 %d %d" % (M, conc), 1)) for M in MS for conc in (1, 2)}
    pr.run()
    split = {k: (int(pr.answers[a][0]), int(pr.answers[b][0])) for k, (a, b) in qs.items()}
    pr = Probe()
    ws = {k: (ask_wgrad(pr, planar(tasks, k[0]), [k[0]], [ms2]), ask_wgrad(pr, planar(BLOCK, k[0]), [k[0]], [ms1])) for k, (ms2, ms1) in split.items()}
    pr.run()
    for (M, conc), (ms2, ms1) in split.items():
        code2, path2, s2, grid2, red2 = one(pr.answers[ws[M, conc][0]])
        code1, path1, s1, grid1, red1 = one(pr.answers[ws[M, conc][1]])
        assert (code2, code1) == (OK, OK) and (s2, s1) == (ms2, ms1) and red2 == red1 == 0
        assert WR.PATHS[path2] in ("dma3", "dma6") and WR.PATHS[path1] in ("dma3", "dma6")           # 128-tiles, LDS-DMA
        assert 0 < grid2 <= WAVE and grid2 == WR.grid128(tiles, ms2), (M, conc, grid2)
        assert 1 <= ms2 <= (M + 63) // 64
        if ms1 % 8 == 0:
            # whole XCD groups where the one-block launch had them; half its slices, so (to the 27th tile) its workgroup count
            assert ms2 % 8 == 0 and ms2 >= 8 and 2 * ms2 == ms1, (M, conc, ms2, ms1)
            assert grid2 == grid1 + 8 * extra * (ms2 // 8)
        if M == 110592:
            assert ms1 % 8 == 0 and (ms2, ms1) == ((16, 32) if conc == 1 else (8, 16))
        else:
            assert ms2 == ms1 == 3                        # 3 chunks of 64 rows: one slice each


def test_a_launch_takes_16_tasks():
    pr = Probe()
    q16 = ask_wgrad(pr, BLOCK + BLOCK + [DEC_EMBED] * 2, [110592], [16])
    q17 = ask_wgrad(pr, BLOCK + BLOCK + [DEC_EMBED] * 2, [110592], [16], ntasks=17)
    pr.run()
    assert one(pr.answers[q16])[0] == OK and one(pr.answers[q16])[3] == 8 * 28 * 2
    assert one(pr.answers[q17])[0] == EDIMS


def test_plan_block_pairs_only_the_fused_128_path():
    """Every stack the library runs, the default word and each of the 15 older switches flipped alone, with and without the bit."""
    pr = Probe()
    qs = {(k, sw, p): ask_block(pr, *q[:7], sc0=q[7] | p, count=1) for k, sw, q, _ in golden_rows() for p in (0, PAIR)}
    pr.run()
    assert len(qs) == 2 * len(GOLDEN) * (1 + len(NAMES))
    for (k, sw, p), i in qs.items():
        w = int(pr.answers[i][0])
        mlp_fused, attn_bwd, pair = w >> 3 & 1, w >> 5 & 3, w >> 15 & 1
        want = bool(p) and mlp_fused == 1 and attn_bwd in (1, 2) and GOLDEN[k][0][0] == 128     # BLK128 / BLK128_RECOMPUTE
        assert bool(pair) == want, (k, sw, p, w)
    # the default word pairs Base (bf16 and fp8: both run the fused bf16 kernels) and nothing else
    for k in GOLDEN:
        w = int(pr.answers[qs[k, None, PAIR]][0])
        assert (w >> 15 & 1) == (k in ("base", "base_fp8")), k
