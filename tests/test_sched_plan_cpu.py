"""Which generation of kernels runs a transformer block is decided in one place: csrc/plan.h plan_block() / plan_dec(), from the
block's shape and the pass's schedule word (SC_*, 15 switches).  block_fwd and block_bwd (csrc/api.hip) switch on the result, so
the forward and the backward of a pass cannot disagree about what is in the workspace.

This test runs csrc/plan_sched_main.cpp, a stand-alone program around the planner built with -fsanitize=address,undefined
(hsimae_amd.build.build_sched_probe), and checks what it prints: no GPU and no libhsimae_hip.so; a sanitizer report fails it.

  * invariants, over all 2^15 schedule words and every shape below: the backward never reads q|k|v the forward did not write (the
    round-4 defect), and every fused kernel is chosen only where its shape predicate and its switches allow it;
  * a golden table of what the library ran BEFORE the planner existed, read off the old block_fwd / block_bwd expression by
    expression: the default word and each switch flipped alone, for every stack the library runs."""
import functools
import os
import subprocess

import numpy as np

# (attn_fwd, save_qkv, mlp_fused, gemm_fp8, attn_bwd, ln1_bwd, ln2_bwd, plane_rows, wgrad_slab) of the default word, then of each
# switch whose flip changes the row (every switch not listed leaves it as the default's).  Stack: (d, heads, hidden, Ts, nsamples,
# model precision is fp8, encoder stack); M = nsamples * Ts rows, a multiple of 32, so the planar layout is live where it can be.
GOLDEN = {
    "base": ((128, 8, 344, 14, 32, 0, 1), ('BLK128', 0, 1, 0, 'BLK128_RECOMPUTE', 'IN_KERNEL', 'IN_KERNEL', 496, 1), {
        "FUSED_MLP": ('BLK128', 1, 0, 0, 'LAYERED', 'GEMM_EPILOGUE', 'SEPARATE', 0, 1),
        "ATTN_BLOCK": ('LAYERED', 1, 1, 0, 'BLK128', 'IN_KERNEL', 'IN_KERNEL', 496, 1),
        "ATTN_BLOCK_BWD": ('BLK128', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 496, 1),
        "PROJ_BWD": ('BLK128', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 496, 1),
        "LNBWD": ('BLK128', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 496, 1),
        "RECOMPUTE": ('BLK128', 1, 1, 0, 'BLK128', 'IN_KERNEL', 'IN_KERNEL', 496, 1),
        "WGRAD_SLAB": ('BLK128', 0, 1, 0, 'BLK128_RECOMPUTE', 'IN_KERNEL', 'IN_KERNEL', 496, 0),
        "PLANAR": ('BLK128', 0, 1, 0, 'BLK128_RECOMPUTE', 'IN_KERNEL', 'IN_KERNEL', 0, 1),
    }),
    "large": ((256, 16, 684, 21, 32, 0, 1), ('BLK256', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 720, 1), {
        "FUSED_MLP": ('BLK256', 1, 0, 0, 'BLK256', 'IN_KERNEL', 'GEMM_EPILOGUE', 0, 1),
        "ATTN_BLOCK256": ('LAYERED', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 720, 1),
        "PROJ_BWD": ('BLK256', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 720, 1),
        "LNBWD": ('BLK256', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 720, 1),
        "WGRAD_SLAB": ('BLK256', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 720, 0),
        "PLANAR": ('BLK256', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 0, 1),
        "ATTN_BLOCK256_BWD": ('BLK256', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 720, 1),
    }),
    "large_fp8": ((256, 16, 684, 21, 32, 1, 1), ('BLK256', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 720, 1), {
        "FP8_UNFUSED": ('LAYERED', 1, 0, 1, 'LAYERED', 'GEMM_EPILOGUE', 'GEMM_EPILOGUE', 0, 1),
        "FUSED_MLP": ('BLK256', 1, 0, 0, 'BLK256', 'IN_KERNEL', 'GEMM_EPILOGUE', 0, 1),
        "ATTN_BLOCK256": ('LAYERED', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 720, 1),
        "PROJ_BWD": ('BLK256', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 720, 1),
        "LNBWD": ('BLK256', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 720, 1),
        "WGRAD_SLAB": ('BLK256', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 720, 0),
        "PLANAR": ('BLK256', 1, 1, 0, 'BLK256', 'IN_KERNEL', 'IN_KERNEL', 0, 1),
        "ATTN_BLOCK256_BWD": ('BLK256', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 720, 1),
    }),
    "huge_bf16": ((512, 32, "@H512@", 21, 32, 0, 1), ('LAYERED', 1, 0, 0, 'LAYERED', 'SEPARATE', 'SEPARATE', 0, 1), {
        "WGRAD_SLAB": ('LAYERED', 1, 0, 0, 'LAYERED', 'SEPARATE', 'SEPARATE', 0, 0),
    }),
    "huge_fp8": ((512, 32, "@H512@", 21, 32, 1, 1), ('LAYERED', 1, 0, 1, 'LAYERED', 'GEMM_EPILOGUE', 'GEMM_EPILOGUE', 0, 1), {
        "LNBWD": ('LAYERED', 1, 0, 1, 'LAYERED', 'SEPARATE', 'SEPARATE', 0, 1),
        "LNBWD_512": ('LAYERED', 1, 0, 1, 'LAYERED', 'SEPARATE', 'SEPARATE', 0, 1),
        "WGRAD_SLAB": ('LAYERED', 1, 0, 1, 'LAYERED', 'GEMM_EPILOGUE', 'GEMM_EPILOGUE', 0, 0),
    }),
    "base_fp8": ((128, 8, 344, 14, 32, 1, 1), ('BLK128', 0, 1, 0, 'BLK128_RECOMPUTE', 'IN_KERNEL', 'IN_KERNEL', 496, 1), {
        "FP8_UNFUSED": ('LAYERED', 1, 0, 1, 'LAYERED', 'SEPARATE', 'SEPARATE', 0, 1),
        "FUSED_MLP": ('BLK128', 1, 0, 0, 'LAYERED', 'GEMM_EPILOGUE', 'SEPARATE', 0, 1),
        "ATTN_BLOCK": ('LAYERED', 1, 1, 0, 'BLK128', 'IN_KERNEL', 'IN_KERNEL', 496, 1),
        "ATTN_BLOCK_BWD": ('BLK128', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 496, 1),
        "PROJ_BWD": ('BLK128', 1, 1, 0, 'LAYERED', 'GEMM_EPILOGUE', 'IN_KERNEL', 496, 1),
        "LNBWD": ('BLK128', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 496, 1),
        "RECOMPUTE": ('BLK128', 1, 1, 0, 'BLK128', 'IN_KERNEL', 'IN_KERNEL', 496, 1),
        "WGRAD_SLAB": ('BLK128', 0, 1, 0, 'BLK128_RECOMPUTE', 'IN_KERNEL', 'IN_KERNEL', 496, 0),
        "PLANAR": ('BLK128', 0, 1, 0, 'BLK128_RECOMPUTE', 'IN_KERNEL', 'IN_KERNEL', 0, 1),
    }),
    "decoder_layered": ((64, 8, 172, 54, 32, 0, 0), ('LAYERED', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 1776, 1), {
        "FUSED_MLP": ('LAYERED', 1, 0, 0, 'LAYERED', 'SEPARATE', 'SEPARATE', 0, 1),
        "WGRAD_SLAB": ('LAYERED', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 1776, 0),
        "PLANAR": ('LAYERED', 1, 1, 0, 'LAYERED', 'SEPARATE', 'IN_KERNEL', 0, 1),
    }),
}

NAMES = ["FUSED_DEC", "DEC_SPLIT", "FP8_UNFUSED", "FUSED_MLP", "ATTN_BLOCK", "ATTN_BLOCK256", "ATTN_BLOCK_BWD", "PROJ_BWD", "LNBWD",
         "LNBWD_512", "RECOMPUTE", "WGRAD_SLAB", "DEC_SLAB", "PLANAR", "ATTN_BLOCK256_BWD"]                 # bit i of the schedule word
SC = {n: 1 << i for i, n in enumerate(NAMES)}
NW = 1 << len(NAMES)
DEFAULT = (NW - 1) & ~SC["FP8_UNFUSED"]                   # what an empty environment gives
FWD = ["LAYERED", "BLK128", "BLK256"]
BWD = ["LAYERED", "BLK128", "BLK128_RECOMPUTE", "BLK256"]
LN = ["SEPARATE", "GEMM_EPILOGUE", "IN_KERNEL"]
ARENA_PAD = 64                                            # rows the arena reserves per plane beyond M (plan.h kPlanePadRows)
MLP_SHAPES = ((128, 352), (256, 704), (64, 192))          # (d, rup(hidden, 32)) of the fused MLP half


def rup(x, m):
    return (x + m - 1) // m * m


class Probe:
    """One run of the sanitizer-built program: queries in on stdin, int32 answers back on stdout, in order."""

    def __init__(self):
        from hsimae_amd import build as B
        self.queries, self.counts = [], []
        self.exe = B.build_sched_probe()

    def ask(self, line, count):
        self.queries.append(line)
        self.counts.append(count)
        return len(self.counts) - 1

    def run(self):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        r = subprocess.run([self.exe], input=("\n".join(self.queries) + "\n").encode(), capture_output=True, timeout=600, env=env)
        err = r.stderr.decode(errors="replace")
        assert "Sanitizer" not in err and "runtime error" not in err and r.returncode == 0, (r.returncode, err[-3000:])
        out = np.frombuffer(r.stdout, dtype=np.int32)
        assert out.size == sum(self.counts), (out.size, sum(self.counts))
        self.answers = np.split(out, np.cumsum(self.counts)[:-1])


def ask_block(pr, d, heads, hidden, Ts, ns, M, fp8, sc0=0, count=NW):
    return pr.ask("B %d %d %d %d %d %d %d %d %d" % (d, heads, hidden, Ts, ns, M, fp8, sc0, count), 3 * count)


def fields(a):
    a = a.reshape(-1, 3)
    w = a[:, 0]
    bits = [("attn_fwd", 0, 3), ("save_qkv", 2, 1), ("mlp_fused", 3, 1), ("gemm_fp8", 4, 1), ("attn_bwd", 5, 3), ("proj_bwd_fused", 7, 1),
            ("ln1_bwd", 8, 3), ("ln2_bwd", 10, 3), ("planar", 12, 1), ("wgrad_slab", 13, 1), ("shape_ok", 14, 1)]
    p = {n: (w >> sh) & m for n, sh, m in bits}
    p.update(plane_rows=a[:, 1], dp=a[:, 2] >> 16, hp=a[:, 2] & 0xffff)
    return p


def h512():
    from hsimae_amd.model import swiglu_hidden
    return swiglu_hidden(512, 4.0)


def invariant_shapes():
    widths = [(128, 8, 344), (256, 16, 684), (512, 32, h512()), (144, 9, 384), (72, 9, 192), (64, 4, 172)]
    shapes = []
    for (d, heads, hidden) in widths:
        for Ts in (1, 14, 32, 33):
            ns_list = [32, 33]                                # M = ns * Ts: a multiple of 32 and (Ts = 1, 14, 33) not
            if d == 256:                                      # one sample count on each side of the kernels' 32-bit offset bound
                edge = ((1 << 31) - 1) // (Ts * 768)
                ns_list += [edge, edge + 1]
            shapes += [(d, heads, hidden, Ts, ns) for ns in ns_list]
    return shapes + [(64, 8, 172, 108, 32), (64, 8, 172, 108, 33), (64, 8, 172, 54, 32), (64, 8, 172, 54, 33)]      # the decoder layer at a time


DEC_SHAPES = [(64, 8, 172, 108), (64, 8, 172, 54), (64, 8, 172, 9), (64, 8, 172, 117), (64, 8, 160, 54), (64, 8, 170, 54),
              (64, 4, 172, 54), (72, 9, 192, 54), (32, 4, 88, 36), (128, 8, 344, 54)]
FP8_CASES = [(prec, D, sc) for prec in (0, 1) for D in (64, 128, 256, 504, 512) for sc in (0, SC["FP8_UNFUSED"], DEFAULT, NW - 1)]


def golden_rows():
    for name, (stack, dflt, flips) in GOLDEN.items():
        d, heads, hidden, Ts, ns, model_fp8, enc = stack
        hidden = h512() if hidden == "@H512@" else hidden
        for sw in [None] + NAMES:
            sc = DEFAULT ^ (SC[sw] if sw else 0)
            # BlkP::prec before the planner: the model's precision with D >= 512 || SC_FP8_UNFUSED, encoder stacks only
            fp8 = int(bool(enc and model_fp8 and (d >= 512 or sc & SC["FP8_UNFUSED"])))
            yield name, sw, (d, heads, hidden, Ts, ns, ns * Ts, fp8, sc, 1), list(flips.get(sw, dflt))


@functools.lru_cache(maxsize=None)
def results():
    pr = Probe()
    pad = pr.ask("P", 1)
    inv = [(sh, fp8, ask_block(pr, *sh, sh[4] * sh[3], fp8)) for sh in invariant_shapes() for fp8 in (0, 1)]
    dec = [(sh, pr.ask("D %d %d %d %d 0 %d" % (*sh, NW), NW)) for sh in DEC_SHAPES]
    f8 = [(c, pr.ask("F %d %d %d" % c, 1)) for c in FP8_CASES]
    gold = [(name, sw, want, ask_block(pr, *q)) for name, sw, q, want in golden_rows()]
    pr.run()
    A = pr.answers
    return {"pad": int(A[pad][0]), "inv": [(sh, fp8, fields(A[i])) for sh, fp8, i in inv], "dec": [(sh, A[i]) for sh, i in dec],
            "f8": [(c, int(A[i][0])) for c, i in f8], "gold": [(name, sw, want, fields(A[i])) for name, sw, want, i in gold]}


def test_forward_and_backward_agree_for_every_schedule_word():
    """!save_qkv => BLK128_RECOMPUTE, BLK128_RECOMPUTE => BLK128 forward, and every fused kernel only inside its shape and
    switches: all 2^15 words x every width / Ts / row count / precision the library runs or a predicate flips at."""
    res = results()
    PAD = res["pad"]
    words = np.arange(NW, dtype=np.int64)
    on = lambda name: (words & SC[name]) != 0
    fails = []
    assert len(res["inv"]) >= 100
    for (d, heads, hidden, Ts, ns), fp8, p in res["inv"]:
        M = ns * Ts
        sh = "d=%d heads=%d hidden=%d Ts=%d nsamples=%d fp8=%d" % (d, heads, hidden, Ts, ns, fp8)

        def need(cond, what):                             # cond: bool vector over the words
            cond = np.broadcast_to(cond, (NW,))
            if not cond.all():
                fails.append("%s: %s, e.g. word 0x%x (%d words)" % (sh, what, int(words[~cond][0]), int((~cond).sum())))

        assert p["attn_fwd"].size == NW
        dp, hp = rup(d, 32), rup(hidden, 32)
        need((p["dp"] == dp) & (p["hp"] == hp) & (p["shape_ok"] == 1), "shape fields")
        all_fp8 = on("FP8_UNFUSED") if fp8 else np.zeros(NW, bool)
        # the shape predicates, from the kernels' documented limits
        s128 = d == 128 and heads == 8 and Ts <= 32
        s256 = d == 256 and heads == 16 and 1 <= Ts <= 32 and ns * Ts * 768 < 2**31
        smlp = (d, hp) in MLP_SHAPES
        fwd, bwd = p["attn_fwd"], p["attn_bwd"]
        b128 = (bwd == 1) | (bwd == 2)
        need((p["save_qkv"] == 1) | (bwd == 2), "q|k|v not saved but the backward does not recompute them")
        need((p["save_qkv"] == 0) == (bwd == 2), "the backward recomputes q|k|v that the forward saved")
        need((bwd != 2) | (fwd == 1), "BLK128_RECOMPUTE without the BLK128 forward")
        need(~b128 | (s128 and dp == d), "blk128_bwd outside its shape")
        need(~b128 | ((p["mlp_fused"] == 1) & (p["proj_bwd_fused"] == 1) & on("PROJ_BWD") & on("LNBWD") & on("ATTN_BLOCK_BWD") &
                      (p["ln1_bwd"] == 2) & (p["ln2_bwd"] == 2)), "blk128_bwd without what it builds on")
        need(~b128 | ~all_fp8, "blk128_bwd under the all-fp8 schedule")
        need((bwd != 2) | (on("RECOMPUTE") & on("ATTN_BLOCK")), "recompute without its switches")
        need((bwd != 3) | ((s256 and dp == d and not fp8) & on("ATTN_BLOCK256_BWD") & on("PROJ_BWD") & on("LNBWD")), "blk256_bwd outside its shape / switches")
        need((fwd != 1) | (s128 & on("ATTN_BLOCK") & ~all_fp8), "blk128_fwd outside its shape / switches")
        need((fwd != 2) | ((s256 and dp == d and not fp8) & on("ATTN_BLOCK256")), "blk256_fwd outside its shape / switches")
        need((p["mlp_fused"] == 0) | (smlp & on("FUSED_MLP") & ~all_fp8), "fused MLP outside its shape / switches")
        need(p["gemm_fp8"] == fp8, "gemm_fp8")
        need(p["proj_bwd_fused"] == (bwd != 0), "proj_bwd_fused")
        # the byte bound of the expression block_bwd had: planes of M + ARENA_PAD rows addressed with 32-bit byte offsets
        byte_bound = (M + ARENA_PAD) * 2 * (rup(hp, 64) + 256) * 2 < 2**32
        need((p["planar"] == 1) == ((p["mlp_fused"] == 1) & on("PLANAR") & (M % 32 == 0 and byte_bound)), "planar exactly under its conditions")
        need(p["plane_rows"] == np.where(p["planar"] == 1, M + PAD, 0), "plane_rows")
        need(p["wgrad_slab"] == on("WGRAD_SLAB"), "wgrad_slab")
        wide_ok = d in (128, 256) or (d == 512 and fp8)
        for ln in ("ln1_bwd", "ln2_bwd"):
            epi = p[ln] == 1
            need(~epi | (on("LNBWD") & (wide_ok and dp == d)), ln + " GEMM_EPILOGUE at an unsupported width")
            if d == 512:
                need(~epi | on("LNBWD_512"), ln + " GEMM_EPILOGUE at d = 512 without SC_LNBWD_512")
        need((p["ln1_bwd"] == 2) == (bwd != 0), "ln1_bwd IN_KERNEL exactly inside a fused attention backward")
        need((p["ln2_bwd"] == 2) == (p["mlp_fused"] == 1), "ln2_bwd IN_KERNEL exactly inside the fused MLP backward")
        need((p["ln2_bwd"] != 1) | (d != 128), "ln2_bwd GEMM_EPILOGUE at d = 128")
    assert not fails, "\n".join(fails[:20])


def test_decoder_plan_and_fp8_rule():
    res = results()
    words = np.arange(NW)
    for (Dd, heads, hidden, TL), got in res["dec"]:
        shape_ok = Dd == 64 and heads == 8 and rup(hidden, 32) == 192 and hidden % 4 == 0 and 16 <= TL <= 112
        mlp_ok = (Dd, rup(hidden, 32)) in MLP_SHAPES
        want = ((words & SC["FUSED_DEC"]) != 0) * int(shape_ok) | ((words & SC["DEC_SPLIT"]) != 0) * int(mlp_ok) << 1 | ((words & SC["DEC_SLAB"]) != 0) << 2
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "Dd=%d heads=%d hidden=%d TL=%d word 0x%x: %d, expected %d" % (Dd, heads, hidden, TL, bad[0], got[bad[0]], want[bad[0]])
    for (prec, D, sc), got in res["f8"]:
        assert got == int(prec == 1 and (D >= 512 or bool(sc & SC["FP8_UNFUSED"]))), (prec, D, sc)


def test_plan_reproduces_what_the_library_ran_before_it():
    """The default word and each of the 15 switches flipped alone, for Base, Large, Large fp8, Huge bf16, Huge fp8, Base fp8 and
    the layer-at-a-time decoder: 7 x 16 rows."""
    res = results()
    assert len(res["gold"]) == len(GOLDEN) * 16
    fails = []
    for name, sw, want, p in res["gold"]:
        got = [FWD[p["attn_fwd"][0]], int(p["save_qkv"][0]), int(p["mlp_fused"][0]), int(p["gemm_fp8"][0]), BWD[p["attn_bwd"][0]],
               LN[p["ln1_bwd"][0]], LN[p["ln2_bwd"][0]], int(p["plane_rows"][0]), int(p["wgrad_slab"][0])]
        if got != want:
            fails.append("%s, %s: %s, the library ran %s" % (name, sw or "default word", got, want))
    assert not fails, "\n".join(fails)
