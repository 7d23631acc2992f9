"""Which gemm_kernel instantiation a GEMM call launches and which path a weight-gradient launch takes are decided in csrc/plan.h:
plan_gemm() with the list HS_GEMM_INSTANCES, and plan_wgrad().  gemm.hip and wgrad.hip launch what they answer.

The GPU tests restate both rules in Python (gemm_ref.expected / TABLE, wgrad_ref.expected / grid128) to know which kernel a case
reaches.  This test holds the restatements against the library's own functions: it runs csrc/plan_sched_main.cpp, the stand-alone
program around plan.h built with -fsanitize=address,undefined (hsimae_amd.build.build_sched_probe), and compares what it prints.
No GPU and no libhsimae_hip.so; a sanitizer report fails it.  A rule that moves in plan.h without its restatement, an instantiation
the rule can answer but the list lacks, or a row of the table nothing launches any more fails here."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G  # noqa: E402
import wgrad_ref as WR  # noqa: E402
from test_sched_plan_cpu import Probe  # noqa: E402
from test_wgrad_bound_cpu import BLOCK128, BLOCK256, DISPATCH  # noqa: E402

OK, EDIMS, EUNSUP = 0, -1, -2

# ------------------------------------------------------------------------------------------------ GEMM
AKINDS = (G.AB, G.AF, G.LN)
EPIS = (G.EB, G.EF, G.ER, G.EP, G.ES, G.ESB, G.ELB)
NS = range(16, 1536 + 1, 16)
KS = range(32, 3072 + 1, 32)
TILINGS = [(bm, kc) for bm in (0, 64, 128) for kc in (0, 128, 256)]
# the (A kind, epilogue) pairs that have a kernel: LayerNorm prologue -> bf16 / gate pair / fp32; bf16 A -> every plain epilogue and
# the LayerNorm backward; fp32 A -> the gate backward, bf16, fp32
PAIRS = {(G.LN, G.EB), (G.LN, G.ES), (G.LN, G.EF), (G.AB, G.ER), (G.AB, G.EP), (G.AB, G.EF), (G.AB, G.EB), (G.AB, G.ELB),
         (G.AF, G.ESB), (G.AF, G.EB), (G.AF, G.EF)}


def refuses(ak, epi, prec, N, K):
    """The refusals the shape alone decides (all HSIMAE_EUNSUPPORTED)."""
    return ((ak, epi) not in PAIRS                              # no kernel for the pair
            or (ak == G.LN and K > 512)                         # the LayerNorm prologue stages the whole row as one chunk
            or (prec == G.FP8 and epi == G.EP)                  # the MX form has no position-embedding epilogue
            or (epi == G.ELB and N not in (128, 256, 512))      # LayerNorm backward over rows of one, two or four 128-column chunks
            or (prec == G.FP8 and epi == G.ELB and N == 128))   # ... the one-chunk form is bf16 only


@functools.lru_cache(maxsize=None)
def gemm_results():
    pr = Probe()
    qs = [((ak, epi, prec, bm, kc), pr.ask("G %d %d %d %d %d %d %d %d %d" % (ak, epi, prec, bm, kc, NS[0], NS[-1], KS[0], KS[-1]),
                                            len(NS) * len(KS) * 5))
          for ak in AKINDS for epi in EPIS for prec in (G.BF16, G.FP8) for bm, kc in TILINGS]
    pr.run()
    return [(q, pr.answers[i].reshape(len(NS), len(KS), 5)) for q, i in qs]


def test_instance_list_is_the_table():
    pr = Probe()
    i = pr.ask("I", 1 + 6 * len(G.TABLE))                        # (another length fails the probe's own size check)
    pr.run()
    a = pr.answers[i]
    assert a[0] == len(G.TABLE) == 90
    got = [tuple(int(v) for v in row) for row in a[1:].reshape(-1, 6)]
    assert len(set(got)) == len(got), "an instantiation listed twice"
    assert set(got) == G.TABLE, (sorted(set(got) - G.TABLE), sorted(G.TABLE - set(got)))


def test_plan_gemm_is_the_restated_rule_over_the_whole_domain():
    """3 x 7 (A kind, epilogue) pairs x 2 precisions x 96 N x 96 K x 9 tile overrides."""
    res = gemm_results()
    assert len(res) == 3 * 7 * 2 * 9
    reached, fails = set(), []
    for (ak, epi, prec, bm, kc), got in res:
        want = np.array([[(EUNSUP, 0, 0, 0, 0) if refuses(ak, epi, prec, N, K) else (OK,) + G.expected(ak, epi, prec, N, K, bm, kc)[2:]
                          for K in KS] for N in NS], dtype=np.int32)
        bad = np.argwhere((got != want).any(-1))
        if bad.size:
            n, k = bad[0]
            fails.append("a%d e%d prec%d bm%d kc%d N=%d K=%d: plan_gemm (code, kc, bm, f8, nch) = %s, expected %s (%d points)"
                         % (ak, epi, prec, bm, kc, NS[n], KS[k], got[n, k].tolist(), want[n, k].tolist(), len(bad)))
        ok = got[..., 0] == OK
        if ok.any():
            assert G.expected(ak, epi, prec, 128, 128, bm, kc)[:2] == (ak, epi)        # expected() names the pair it was asked for
            reached |= {(ak, epi) + tuple(int(v) for v in row) for row in np.unique(got[ok][:, 1:], axis=0)}
    assert not fails, "\n".join(fails[:20])
    assert reached <= G.TABLE, "plan_gemm answers an instantiation outside TABLE: " + ", ".join(G.inst_name(t) for t in sorted(reached - G.TABLE))
    assert reached == G.TABLE, "rows of TABLE no point of the sweep launches: " + ", ".join(G.inst_name(t) for t in sorted(G.TABLE - reached))


# ------------------------------------------------------------------------------------------------ weight gradients
SINGLES = [(72, 64), (136, 72), (344, 136), (256, 256), (344, 264), (256, 696)]
TASKSETS = [[t] for t in SINGLES] + [BLOCK128, BLOCK256]
MS = [1, 45, 200, 256, 333, 640, 2733, 3685]
SPLITS = [1, 2, 3, 8, 17, 24, 32]


def ask_wgrad(pr, tasks, Ms, splits, ntasks=None):
    """tasks: (N, K[, f32[, ldo, lda, rowscale, dO_plane_rows, A_plane_rows]]); answer [M][msplit][slab][4 bytes off][code, path, msplit, grid, reduce grid]."""
    full = [tuple(t) + (0,) * (8 - len(t)) for t in tasks]
    line = "W %d %d %s %d %s %d %s" % (len(tasks) if ntasks is None else ntasks, len(tasks), " ".join("%d %d %d %d %d %d %d %d" % t for t in full),
                                      len(Ms), " ".join(map(str, Ms)), len(splits), " ".join(map(str, splits)))
    assert len(line) < 1000
    return pr.ask(line, len(Ms) * len(splits) * 2 * 2 * 5)


def one(a, slab=False, aligned=True):
    """The answer of a one-M, one-msplit query."""
    return [int(v) for v in a.reshape(2, 2, 5)[int(slab), int(not aligned)]]


def test_plan_wgrad_on_the_dispatch_table():
    pr = Probe()
    rows = [(row, ask_wgrad(pr, row[0], [row[1]], [row[2]])) for row in DISPATCH]
    pr.run()
    for (tasks, M, msplit, slab, aligned, want), i in rows:
        code, path, split, grid, red = one(pr.answers[i], slab, aligned)
        assert WR.expected(tasks, M, msplit, slab, aligned) == want
        assert (code, WR.PATHS[path], split) == (OK,) + want[:2], (tasks, M, msplit, slab, aligned)


def test_plan_wgrad_is_the_restated_rule_over_the_sweep():
    pr = Probe()
    qs = []
    for ts in TASKSETS:
        for f32 in (0, 1):                                      # no fp32 dO, or the first task's
            tasks = [(N, K, int(bool(f32 and j == 0))) for j, (N, K) in enumerate(ts)]
            qs.append((tasks, ask_wgrad(pr, tasks, MS, SPLITS)))
    pr.run()
    seen, fails = set(), []
    for tasks, i in qs:
        a = pr.answers[i].reshape(len(MS), len(SPLITS), 2, 2, 5)
        t128, t256 = WR.tiles(tasks, 128), WR.tiles(tasks, 256)
        for mi, M in enumerate(MS):
            for si, msplit in enumerate(SPLITS):
                for slab in (0, 1):
                    for off in (0, 1):
                        code, path, split, grid, red = (int(v) for v in a[mi, si, slab, off])
                        wpath, P, _ = WR.expected(tasks, M, msplit, bool(slab), not off)
                        wgrid = 8 * WR.cdiv(t256 * P, 8) if wpath.startswith("big") else WR.grid128(t128, msplit)
                        wred = t256 * 128 if wpath == "big_slab" else 0
                        if (code, WR.PATHS[path], split, grid, red) != (OK, wpath, P, wgrid, wred):
                            fails.append("%s M=%d msplit=%d slab=%d off=%d: plan_wgrad %s, expected %s"
                                         % (tasks, M, msplit, slab, off, (code, WR.PATHS[path], split, grid, red), (OK, wpath, P, wgrid, wred)))
                        seen.add(wpath)
    assert not fails, "\n".join(fails[:20])
    assert seen == set(WR.PATHS)


def test_plan_wgrad_refusals():
    """The codes hs_wgrad returned before plan_wgrad existed, and which of two refusals wins."""
    pr = Probe()
    T = (128, 128, 0)
    planar_dO = (128, 128, 0, 128, 0, 0, 64 + 48, 0)            # dO as 64-column planes of M + 48 rows at M = 64
    planar_A = (128, 128, 0, 0, 128, 0, 0, 64 + 48)
    cases = [
        ("no tasks", OK, ask_wgrad(pr, [], [64], [8]), {}),
        ("no rows", OK, ask_wgrad(pr, [T], [0], [8]), {}),
        ("ntasks > 16", EDIMS, ask_wgrad(pr, [T] * 16, [64], [8], ntasks=17), {}),
        ("msplit < 1", EDIMS, ask_wgrad(pr, [T], [64], [0]), {}),
        ("ldo % 8", EDIMS, ask_wgrad(pr, [(128, 128, 0, 132, 0)], [64], [8]), {}),
        ("lda % 8", EDIMS, ask_wgrad(pr, [(128, 128, 0, 0, 132)], [64], [8]), {}),
        ("bf16 dO with a row factor", EUNSUP, ask_wgrad(pr, [(128, 128, 0, 0, 0, 1)], [64], [8]), {}),
        ("fp32 dO with a row factor", OK, ask_wgrad(pr, [(128, 128, 1, 0, 0, 1)], [64], [8]), {}),
        ("ldo % 8 before the row factor", EDIMS, ask_wgrad(pr, [(128, 128, 0, 132, 0, 1)], [64], [8]), {}),
        ("task 0's row factor before task 1's ldo", EUNSUP, ask_wgrad(pr, [(128, 128, 0, 0, 0, 1), (128, 128, 0, 132, 0)], [64], [8]), {}),
        ("planar dO", OK, ask_wgrad(pr, [planar_dO], [64], [8]), {}),
        ("planar A", OK, ask_wgrad(pr, [planar_A], [64], [8]), {}),
        ("planar dO, M % 32", EDIMS, ask_wgrad(pr, [planar_dO], [45], [8]), {}),
        ("planar A, M % 32", EDIMS, ask_wgrad(pr, [planar_A], [45], [8]), {}),
        ("planar dO, plane_rows < M", EDIMS, ask_wgrad(pr, [planar_dO], [128], [8]), {}),
        ("planar A, plane_rows < M", EDIMS, ask_wgrad(pr, [planar_A], [128], [8]), {}),
        ("planar dO, ldo % 64", EDIMS, ask_wgrad(pr, [(128, 128, 0, 136, 0, 0, 112, 0)], [64], [8]), {}),
        ("planar dO in fp32", EDIMS, ask_wgrad(pr, [(128, 128, 1, 128, 0, 0, 112, 0)], [64], [8]), {}),
        ("planar A under an fp32 dO", EUNSUP, ask_wgrad(pr, [(128, 128, 1, 0, 128, 0, 0, 112)], [64], [8]), {}),
        ("planar dO next to an fp32 task", EUNSUP, ask_wgrad(pr, [planar_dO, (128, 128, 1)], [64], [8]), {}),
        ("planar dO, operands 4 bytes off", EUNSUP, ask_wgrad(pr, [planar_dO], [64], [8]), dict(aligned=False)),
        ("planar A, operands 4 bytes off", EUNSUP, ask_wgrad(pr, [planar_A], [64], [8]), dict(aligned=False)),
        ("planes past 32-bit byte offsets", EDIMS, ask_wgrad(pr, [(128, 128, 0, 128, 0, 0, 1 << 23, 0)], [64], [8]), {}),
    ]
    pr.run()
    for what, want, i, kw in cases:
        code, path, split, grid, red = one(pr.answers[i], **kw)
        assert code == want, (what, code, want)
        if what.startswith("no "):
            assert grid == 0 and red == 0, what                  # HSIMAE_OK and nothing to launch
        elif want == OK:
            assert grid > 0, what
