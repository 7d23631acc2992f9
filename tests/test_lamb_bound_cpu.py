"""The LAMB step without a GPU: the fp64 restatement (tests/lamb_ref.py) against torch.optim.AdamW in fp64 when every ratio is 1 and
against a second, independently written per-tensor loop; the bound against an fp32 emulation and against planted faults; the C
ABI's declaration, export and refusals; and the tensor-table builder on the manifest's real layouts."""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lamb_ref as L  # noqa: E402

HP = L.HP


@pytest.fixture(autouse=True)
def rng_state_left_as_found():
    """Tests that run after this file and draw from the global generators without seeding find them as they would have without it."""
    import random
    saved = random.getstate(), np.random.get_state(), torch.get_rng_state()
    yield
    random.setstate(saved[0])
    np.random.set_state(saved[1])
    torch.set_rng_state(saved[2])


# ------------------------------------------------------------------------------------------------ 1. ratios = 1 is AdamW
def test_with_every_ratio_one_the_restatement_is_torch_adamw_in_fp64():
    """Three steps with changing gradients and rates, one torch group per table entry.  Every value the restatement rounds to
    fp32 is exact there (b1 = 1/2, b2 = 3/4, eps = 2^-20, torch's step count held at 1: both bias corrections are exactly 2, the
    table rounded before torch sees it), so 1e-12 of each array's magnitude can be asked."""
    b1, b2, eps = 0.5, 0.75, 2.0 ** -20
    sizes = [1, 7, 4097, 300001, 64, 5]
    inp = L.inputs(sizes, 3, {4: "frozen"})
    ids, tensors = inp["ids"], inp["tensors"]
    live = [k for k in (0, 1, 3, 4)]
    idx = {k: torch.nonzero(ids == k).reshape(-1) for k in live}
    assert all(i.numel() for i in idx.values())
    params = {k: torch.nn.Parameter(inp["p"][i].double()) for k, i in idx.items()}
    opt = torch.optim.AdamW([dict(params=[params[k]], lr=1.0, weight_decay=0.0) for k in idx], lr=1.0, betas=(b1, b2), eps=eps)
    for k, i in idx.items():
        opt.state[params[k]] = dict(step=torch.tensor(0.0), exp_avg=inp["m"][i].double().clone(), exp_avg_sq=inp["v"][i].double().clone())
    state = {k: inp[k].double() for k in "pmv"}
    worst = 0.0
    for step, base in enumerate((1e-3, 3.3e-4, 2.5e-3)):
        g = (inp["g"].double() * (1.0 + 0.37 * step) - 0.004 * step).float()
        table = [(L.f32(lr * base / 1e-3), L.f32(wd) if wd == wd else wd) for lr, wd in L.TABLE]
        for grp, k in zip(opt.param_groups, idx):
            grp["lr"], grp["weight_decay"] = table[k]
            params[k].grad = g[idx[k]].double()
            opt.state[params[k]]["step"] = torch.tensor(0.0)
        opt.step()
        ref = L.lamb_ref(state["p"], g, state["m"], state["v"], tensors, ids, table, 1.0, 1, 1, b1, b2, eps, None, False, ratios=1.0)
        for k, i in idx.items():
            st = opt.state[params[k]]
            for name, got in (("p", params[k].detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
                want = ref[name].ref[i]
                err = float((got - want).abs().max()) / float(want.abs().max())
                worst = max(worst, err)
                assert err <= 1e-12, (step, k, name, err)
        dead = ids == 2
        for name in "pmv":
            assert torch.equal(ref[name].ref[dead], state[name][dead]) and not bool(ref[name].bound()[dead].any())
        state = {name: ref[name].ref for name in "pmv"}
    print(f"[lamb == adamw at r = 1] worst relative difference {worst:.3g}")


def test_bias_corrections_at_step_three_are_torchs():
    """One step with torch's step count at 3 (b1 = 1/2, b2 = 3/4, eps = 2^-20: exact in fp32).  The restatement rounds its two
    bias-correction factors to fp32 as the control block holds them (8/7 and 1/sqrt(37/64) are not exact there), torch keeps them
    in fp64: each factor differs by at most 2^-24 relative, which reaches p as that fraction of the Adam part of the update,
    lr |ua| = |p' - p (1 - lr wd)|.  Asked: 3 * 2^-24 of that per element (two factors, first order, and slack for the second),
    plus 1e-12 of |p|; the moments do not see the factors and agree to 1e-12."""
    b1, b2, eps = 0.5, 0.75, 2.0 ** -20
    inp = L.inputs([1, 7, 4097, 64, 5], 5)
    ids, tensors = inp["ids"], inp["tensors"]
    idx = {k: torch.nonzero(ids == k).reshape(-1) for k in (0, 1, 3, 4)}
    assert all(i.numel() for i in idx.values())
    table = [(L.f32(lr), L.f32(wd) if wd == wd else wd) for lr, wd in L.TABLE]
    params = {k: torch.nn.Parameter(inp["p"][i].double()) for k, i in idx.items()}
    opt = torch.optim.AdamW([dict(params=[params[k]], lr=table[k][0], weight_decay=table[k][1]) for k in idx], betas=(b1, b2), eps=eps)
    for k, i in idx.items():
        opt.state[params[k]] = dict(step=torch.tensor(2.0), exp_avg=inp["m"][i].double().clone(), exp_avg_sq=inp["v"][i].double().clone())
        params[k].grad = inp["g"][i].double()
    opt.step()
    ref = L.lamb_ref(inp["p"], inp["g"], inp["m"], inp["v"], tensors, ids, table, 1.0, 1, 3, b1, b2, eps, None, False, ratios=1.0)
    seen = 0.0
    for k, i in idx.items():
        st = opt.state[params[k]]
        assert int(st["step"]) == 3
        p0 = inp["p"][i].double()
        adam_part = (ref["p"].ref[i] - p0 * (1 - table[k][0] * table[k][1])).abs()
        err = (params[k].detach() - ref["p"].ref[i]).abs()
        assert bool((err <= 3 * L.U * adam_part + 1e-12 * p0.abs()).all()), (k, float(err.max()))
        seen = max(seen, float((err / adam_part.clamp_min(1e-300)).max()))
        for name, got in (("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
            assert float((got - ref[name].ref[i]).abs().max()) <= 1e-12 * float(ref[name].ref[i].abs().max()), (k, name)
    assert seen > 1e-9, "the factors were compared with themselves"      # the fp32 rounding of 8/7 is visible: this is t = 3, not 1
    # and with t = 2 handed to the restatement the same step lies far outside
    wrong = L.lamb_ref(inp["p"], inp["g"], inp["m"], inp["v"], tensors, ids, table, 1.0, 1, 2, b1, b2, eps, None, False, ratios=1.0)
    i = idx[0]
    assert float(((params[0].detach() - wrong["p"].ref[i]).abs() / (ref["p"].ref[i] - inp["p"][i].double()).abs().clamp_min(1e-300)).max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. an independent loop
def second_opinion(inp, table, coef, t, hp, trust_clip, always_adapt):
    """LAMB written once more, from the paper's formulas with torch ops on fp64 tensors, one parameter tensor at a time."""
    f = L.f32
    beta1, beta2, eps = f(hp["b1"]), f(hp["b2"]), f(hp["eps"])
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    c1, c2 = f(1.0 / bc1), f(1.0 / math.sqrt(bc2))
    out = {k: inp[k].double().clone() for k in "pmv"}
    ratios = []
    for off, n in inp["tensors"]:
        gid = int(inp["ids"][off])
        if gid == 2 or gid >= len(table):
            ratios.append(1.0)
            continue
        lr, wd = f(table[gid][0]), f(table[gid][1])
        w = inp["p"][off:off + n].double()
        grad = inp["g"][off:off + n].double().mul(f(coef))
        exp_avg = torch.lerp(inp["m"][off:off + n].double(), grad, 1.0 - beta1)
        exp_avg_sq = inp["v"][off:off + n].double().mul(beta2).addcmul(grad, grad, value=1.0 - beta2)
        update = (exp_avg * c1).div(exp_avg_sq.sqrt().mul(c2).add(eps))
        if wd != 0.0:
            update = update.add(w, alpha=wd)
        w_norm, u_norm = torch.linalg.vector_norm(w), torch.linalg.vector_norm(update)
        trust = 1.0
        if (wd != 0.0 or always_adapt) and float(w_norm) > 0 and float(u_norm) > 0:
            trust = float(w_norm / u_norm)
        if trust_clip is not None:
            trust = min(trust, f(trust_clip))
        ratios.append(trust)
        out["p"][off:off + n] = w.add(update, alpha=-lr * trust)
        out["m"][off:off + n], out["v"][off:off + n] = exp_avg, exp_avg_sq
    return out, torch.tensor(ratios, dtype=torch.float64)


@pytest.mark.parametrize("always_adapt", [False, True])
@pytest.mark.parametrize("trust_clip", [None, 1.0])
def test_restatement_equals_an_independent_per_tensor_loop(trust_clip, always_adapt):
    inp = L.case_inputs("A")
    for coef, t in ((1.0, 1), (0.3, 2), (0.3, 1000)):
        ref = L.lamb_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["tensors"], inp["ids"], L.TABLE, coef, 1, t, HP["b1"], HP["b2"],
                         HP["eps"], trust_clip, always_adapt)
        other, ratios = second_opinion(inp, L.TABLE, coef, t, HP, trust_clip, always_adapt)
        for k in "pmv":
            err = float((other[k] - ref[k].ref).abs().max())
            assert err <= 1e-12 * float(ref[k].ref.abs().max()), (k, coef, t, err)
        assert float(((ratios - ref["r"].ref).abs() / ref["r"].ref).max()) <= 1e-12
        adapted = ref["r"].ref[ref["r"].ref != 1.0]
        if trust_clip is None:
            assert float(adapted.min()) < 0.5 and float(adapted.max()) > 2.0      # both sides of 1


# ------------------------------------------------------------------------------------------------ 3, 4. emulation and faults
FAULT_SIZES = [5, 64, 6000, 7, 255, 4097, 3, 1000, 9000, 64, 300, 12]
FAULT_PLANTS = {4: "zero_w", 6: "frozen", 9: "zero_u"}
FAULTS = ["ratio_inverted", "norm_after_update", "boundary_shifted", "decay_left_out_of_u", "no_decay_tensor_adapted",
          "trust_clip_ignored", "zero_norm_ratio_zero", "coef_not_applied", "last_chunk_dropped", "one_global_ratio"]


def fault_inputs():
    return L.inputs(FAULT_SIZES, 17, FAULT_PLANTS)


def emulate(inp, table, coef, t, hp, trust_clip, always_adapt, fault=None):
    """The three kernels as they compute: fp32 element by element, the two sums of a tensor in fp64 from the fp32 values chunk by
    chunk, the ratio rounded once to fp32, u formed a second time for the step."""
    f = np.float32
    b1, b2, eps, coef = f(hp["b1"]), f(hp["b2"]), f(hp["eps"]), f(1.0 if fault == "coef_not_applied" else coef)
    i1, i2 = (f(a) for a in L.R.bias_corrections(t, hp["b1"], hp["b2"]))
    out = {k: inp[k].clone() for k in "pmv"}
    tensors = list(inp["tensors"])
    if fault == "boundary_shifted":                            # tensor 1 gives its last element to tensor 2
        (o1, n1), (o2, n2) = tensors[1], tensors[2]
        tensors[1], tensors[2] = (o1, n1 - 1), (o2 - 1, n2 + 1)
    ratios, work = [], []
    for off, n in tensors:
        gid = int(inp["ids"][off + (1 if fault == "boundary_shifted" and (off, n) == tensors[2] else 0)])
        if gid == 2 or gid >= len(table):
            ratios.append(f(1))
            work.append(None)
            continue
        lr, wd = f(table[gid][0]), f(table[gid][1])
        p, g, m, v = (inp[k][off:off + n].numpy() for k in "pgmv")
        gc = g * coef
        mn = m + (gc - m) * (f(1) - b1)
        vn = v * b2 + gc * gc * (f(1) - b2)
        u = (mn * i1) / (np.sqrt(vn) * i2 + eps)
        if wd != 0 and fault != "decay_left_out_of_u":
            u = u + wd * p
        assert u.dtype == np.float32 and mn.dtype == np.float32
        chunks = [(c, min(c + L.CHUNK, n)) for c in range(0, n, L.CHUNK)]
        if fault == "last_chunk_dropped" and len(chunks) > 1:
            chunks = chunks[:-1]
        w = (p - lr * u).astype(np.float32) if fault == "norm_after_update" else p
        sp = math.fsum(float((w[a:b].astype(np.float64) ** 2).sum()) for a, b in chunks)
        su = math.fsum(float((u[a:b].astype(np.float64) ** 2).sum()) for a, b in chunks)
        work.append((off, n, lr, wd, p, mn, vn, u, sp, su))
        r = f(1)
        adapt = wd != 0 or always_adapt or fault == "no_decay_tensor_adapted"
        if adapt and sp > 0 and su > 0:
            r = f(math.sqrt(su / sp)) if fault == "ratio_inverted" else f(math.sqrt(sp / su))
        elif adapt and fault == "zero_norm_ratio_zero":
            r = f(0)
        if trust_clip is not None and fault != "trust_clip_ignored":
            r = min(r, f(trust_clip))
        ratios.append(r)
    if fault == "one_global_ratio":
        sp, su = sum(w[8] for w in work if w), sum(w[9] for w in work if w)
        ratios = [f(math.sqrt(sp / su)) if w else f(1) for w in work]
    for r, w in zip(ratios, work):
        if w is None:
            continue
        off, n, lr, wd, p, mn, vn, u = w[:8]
        out["p"][off:off + n] = torch.from_numpy((p - (lr * r) * u).astype(np.float32))
        out["m"][off:off + n], out["v"][off:off + n] = torch.from_numpy(mn), torch.from_numpy(vn)
    return out, torch.tensor([float(r) for r in ratios], dtype=torch.float64)


def judge(got, ratios, inp, table, coef, t, hp, trust_clip, always_adapt):
    ref = L.lamb_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["tensors"], inp["ids"], table, coef, 1, t, hp["b1"], hp["b2"],
                     hp["eps"], trust_clip, always_adapt)
    return {k: ref[k].ratio(got[k]) for k in "pmv"} | {"r": ref["r"].ratio(ratios)}


@pytest.mark.parametrize("always_adapt", [False, True])
@pytest.mark.parametrize("trust_clip", [None, 1.0])
@pytest.mark.parametrize("name", ["A", "C", "faults"])
def test_fp32_emulation_stays_within_the_bound(name, trust_clip, always_adapt):
    inp = fault_inputs() if name == "faults" else L.case_inputs(name)
    for coef, t in ((1.0, 1), (0.3, 2), (0.3, 1000)):
        got, ratios = emulate(inp, L.TABLE, coef, t, HP, trust_clip, always_adapt)
        w = judge(got, ratios, inp, L.TABLE, coef, t, HP, trust_clip, always_adapt)
        print(f"{name} clip {trust_clip} adapt {always_adapt} coef {coef} t {t}: worst err / bound " +
              ", ".join(f"{k} {x:.3f}" for k, x in w.items()))
        assert all(x <= 1.0 for x in w.values()), w


@pytest.mark.parametrize("fault", FAULTS)
def test_bound_rejects_planted_faults(fault):
    """The weights' scale varies by 100 x between tensors, so the ratios fall on both sides of 1 and of trust_clip = 1."""
    inp = fault_inputs()
    trust_clip = 1.0 if fault == "trust_clip_ignored" else None
    coef = 0.3
    clean, ratios = emulate(inp, L.TABLE, coef, L.T_STEP, HP, trust_clip, False)
    w0 = judge(clean, ratios, inp, L.TABLE, coef, L.T_STEP, HP, trust_clip, False)
    assert all(x <= 1.0 for x in w0.values()), w0              # the harness itself is clean on this very input
    free = emulate(inp, L.TABLE, coef, L.T_STEP, HP, None, False)[1]
    assert float(free.min()) < 0.5 and float(free.max()) > 2.0 and int((free != 1.0).sum()) >= 4
    got, ratios = emulate(inp, L.TABLE, coef, L.T_STEP, HP, trust_clip, False, fault)
    w = judge(got, ratios, inp, L.TABLE, coef, L.T_STEP, HP, trust_clip, False)
    print(f"{fault}: worst err / bound " + ", ".join(f"{k} {x:.3g}" for k, x in w.items()))
    assert max(w.values()) > 1.0, w
    assert max(w["p"], w["m"], w["v"]) > 1.0, w                # not only the reported ratio: the step itself leaves the bound


# ------------------------------------------------------------------------------------------------ 5. the C ABI
def test_library_declares_exports_and_refuses_before_any_launch():
    from hsimae_amd import _lib, FusedLAMB  # noqa: F401
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert "hsimae_lamb_step" in _lib.SYMBOLS and re.search(r"\bhsimae_lamb_step\s*\(", hdr)
    assert lib.hsimae_lamb_step is not None and lib.hsimae_version() == _lib.ABI_VERSION == 108
    assert int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1)) == 108
    assert int(re.search(r"#define HSIMAE_LAMB_CHUNK (\d+)", hdr).group(1)) == _lib.LAMB_CHUNK == L.CHUNK == 4096
    decl = re.search(r"typedef struct \{([^}]*)\} hsimae_lamb_tensor;\s*/\* device table, (\d+) bytes \*/", hdr)
    assert decl and int(decl.group(2)) == C.sizeof(_lib.LambTensor) == 24
    fields = re.findall(r"(int64_t|int32_t) (\w+);", decl.group(1))
    assert [n for _, n in fields] == [n for n, _ in _lib.LambTensor._fields_]
    assert [C.sizeof(t) for _, t in _lib.LambTensor._fields_] == [8 if t == "int64_t" else 4 for t, _ in fields]
    assert (_lib.LambTensor.off.offset, _lib.LambTensor.n.offset, _lib.LambTensor.chunk0.offset) == (0, 8, 16)

    tab = (_lib.AdamWGroup * 3)(_lib.AdamWGroup(1e-3, 0.05), _lib.AdamWGroup(1e-3, 0.0), _lib.AdamWGroup(-1.0, float("nan")))

    def st(p=1 << 20, g=1 << 21, m=1 << 22, v=1 << 23, group=None, gu=0, n=17, tensors=1 << 24, nt=1, nch=1, table=tab, ng=3,
           partials=1 << 25, ratios=1 << 26, bad=1 << 27, ctl=1 << 28):
        return lib.hsimae_lamb_step(p, g, m, v, group, gu, n, tensors, nt, nch, table, ng, 0.9, 0.999, 1e-6, 0.0, 0, partials, ratios,
                                    bad, ctl, None)
    for k in ("p", "g", "m", "v", "tensors", "table", "partials", "ratios", "bad", "ctl"):
        assert st(**{k: None}) == -4, k
    assert st(n=-1) == -1 and st(nt=0) == -1 and st(nch=0) == -1 and st(ng=0) == -1 and st(ng=65) == -1
    assert st(gu=-1) == -1 and st(gu=3) == -1 and st(gu=64) == -1
    nan = float("nan")
    for bad_tab in ((-1e-3, 0.0), (1e-3, -0.1), (nan, 0.0), (1e-3, nan)):
        t2 = (_lib.AdamWGroup * 3)(_lib.AdamWGroup(*bad_tab), _lib.AdamWGroup(1e-3, 0.0), _lib.AdamWGroup(1e-3, 0.0))
        assert st(table=t2) == -1, bad_tab
    assert st(partials=(1 << 25) + 4) == -3 and st(p=(1 << 20) + 2) == -3 and st(ctl=(1 << 28) + 4) == -3
    assert st(n=0) == 0                                        # nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------ 6. the tensor table
def manifest():
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("key", ["C2_base96", "C1_base48", "HSIMAE_base32", "DualViT_base32"])
def test_tensor_table_tiles_the_manifests_layouts(key):
    """The flat buffer of each layout (Base at 96 bands; the 144 / 72 defaults at 48 and 32 bands), packed in registration order."""
    from hsimae_amd.optim import lamb_tensor_table
    rows_m = [r for r in manifest()[key] if not r[0].startswith("cls_head.")]
    sizes = [int(np.prod(r[1])) for r in rows_m]
    offs = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    assert min(sizes) >= 1 and max(sizes) > L.CHUNK
    rows, nchunks = lamb_tensor_table(offs, sizes)
    want, want_chunks = L.chunk_table(list(zip(offs, sizes)))
    assert nchunks == want_chunks and rows.dtype.itemsize == 24 and len(rows) == len(sizes)
    assert [(int(r["off"]), int(r["n"]), int(r["chunk0"])) for r in rows] == want and not rows["reserved"].any()
    # walk the chunks as the kernels do: each covers [off + 4096 c, off + min(n, 4096 (c + 1))) of the last tensor whose chunk0 <= chunk
    chunk0 = rows["chunk0"]
    covered = np.zeros(sum(sizes), dtype=np.int32)
    for chunk in range(nchunks):
        T = int(np.searchsorted(chunk0, chunk, side="right")) - 1
        c = chunk - int(chunk0[T])
        lo = offs[T] + L.CHUNK * c
        hi = offs[T] + min(sizes[T], L.CHUNK * (c + 1))
        assert 0 <= c < -(-sizes[T] // L.CHUNK) and offs[T] <= lo < hi <= offs[T] + sizes[T] and hi - lo <= L.CHUNK
        covered[lo:hi] += 1
    assert bool((covered == 1).all())                          # every element exactly once, no chunk across a boundary
    assert chunk0[0] == 0 and bool((np.diff(chunk0) == -(-np.asarray(sizes[:-1]) // L.CHUNK)).all())
