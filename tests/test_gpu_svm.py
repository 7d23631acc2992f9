"""csrc/svm.hip on the GPU: hsimae_svm_gram inside the bound of the fp64 restatement, hsimae_svm_solve BIT-EQUAL to the restated
SMO run on the device's own kernel matrix, hsimae_svm_pack bit-equal to libsvm's compact form, hsimae_svm_predict inside its
bound and under the label rule; RBFSVM end to end against recorded sklearn results (tests/golden/svm_cases.npz; no sklearn
needed here).  Every call uses guarded buffers and runs twice bit for bit."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
FILL = -7
F32 = np.float32
GOLD = os.path.join(ROOT, "tests", "golden", "svm_cases.npz")


def guarded(n, dtype, fill=FILL):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def intact(whole, fill=FILL):
    w = whole.cpu()
    return bool((w[:GUARD] == fill).all() and (w[-GUARD:] == fill).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ Gram
def run_gram(x, D, gammas, ldk=None):
    """x device fp32 [M, ldx] -> (K whole, K [n_gamma, M, ldk], sumsq whole, sumsq [M])."""
    from hsimae_amd import _lib
    M, ldx = x.shape
    ldk = ldk or M + 3
    kw, k = guarded(len(gammas) * M * ldk, torch.float32)
    sw, s = guarded(M, torch.float32)
    p = _lib.SvmGramParams(x=x.data_ptr(), ldx=ldx, M=M, D=D, n_gamma=len(gammas), gamma=(C.c_float * 16)(*gammas), K=k.data_ptr(),
                           ldk=ldk, sumsq=s.data_ptr())
    _lib.check(_lib.load().hsimae_svm_gram(C.byref(p), stream()), "hsimae_svm_gram")
    return kw, k.view(len(gammas), M, ldk), sw, s


@pytest.mark.parametrize("D", [4, 36, 132])
def test_gram_lies_inside_the_bound_and_is_symmetric_with_a_unit_diagonal(D):
    for M, gammas in itertools.product((1, 2, 63, 64, 65, 257), ([1.0 / D], [0.01, 1.0 / D, 2.0])):
        x = R.gram_case(M, D, D + 4)
        xd = torch.from_numpy(x).cuda()
        kw, k, sw, s = run_gram(xd, D, gammas)
        K = k.cpu().numpy()
        ref, bound = R.gram_ref(x, D, gammas)
        got = K[:, :, :M]
        worst = float(np.max(np.abs(got - ref) / np.where(bound > 0, bound, 1.0) * (np.abs(got - ref) > 0)))
        print(f"M {M} D {D} gammas {len(gammas)}: err / bound {worst:.3f}")
        assert worst <= 1.0 and np.all(np.abs(got - ref) <= bound)
        assert intact(kw) and intact(sw) and np.all(K[:, :, M:] == FILL)
        for g in range(len(gammas)):
            assert same_bits(got[g], np.ascontiguousarray(got[g].T)) and np.all(np.diagonal(got[g]) == 1.0)
        if M >= 3:
            assert np.all(got[:, 0, 2] == 1.0) and np.all(got[:, 2, 0] == 1.0)              # duplicate rows: exactly 1
        n64 = (x[:, :D].astype(np.float64) ** 2).sum(1)
        assert np.all(np.abs(s.cpu().numpy() - n64) <= R.GD(D) * n64)                       # sumsq: the chain's bound
        kw2, _, sw2, _ = run_gram(xd, D, gammas)
        assert torch.equal(kw2.view(torch.int32), kw.view(torch.int32)) and torch.equal(sw2.view(torch.int32), sw.view(torch.int32))


def test_gram_keeps_a_nan_row_in_its_row_and_column():
    M, D, row = 130, 36, 70
    x = R.gram_case(M, D, D, nan_row=row)
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), D, [0.05])
    K = k.cpu().numpy()[0, :, :M]
    nan = np.isnan(K)
    want = np.zeros((M, M), bool)
    want[row, :] = want[:, row] = True
    want[row, row] = False
    assert np.array_equal(nan, want) and K[row, row] == 1.0


# ------------------------------------------------------------------ solver
def make_table(rows):
    """[(k_index, C, a0, na, b0, nb, out_offset)] -> int64 [n, 8] (C's bits in column 1)."""
    t = np.zeros((len(rows), 8), np.int64)
    for r, (k, c, a0, na, b0, nb, off) in enumerate(rows):
        t[r] = [k, np.float64(c).view(np.int64), a0, na, b0, nb, off, 0]
    return t


def run_solve(K, rows, alpha_len, eps=1e-3, max_iter=10 ** 6, resume=None):
    """K device [n_k, M, ldk]; rows as make_table -> (alpha, grad, state) numpy; resume = (alpha, grad, state) to go on from."""
    from hsimae_amd import _lib
    n_k, M, ldk = K.shape
    table = torch.from_numpy(make_table(rows)).cuda()
    aw, a = guarded(alpha_len, torch.float64)
    gw, g = guarded(alpha_len, torch.float64)
    sw, s = guarded(8 * len(rows), torch.float64)
    if resume is not None:
        a.copy_(torch.from_numpy(resume[0]))
        g.copy_(torch.from_numpy(resume[1]))
        s.copy_(torch.from_numpy(resume[2]).reshape(-1))
    p = _lib.SvmSolveParams(K=K.data_ptr(), ldk=ldk, M=M, n_k=n_k, table=table.data_ptr(), n_problems=len(rows),
                            resume=int(resume is not None), max_iter=max_iter, eps=eps, alpha=a.data_ptr(), grad=g.data_ptr(),
                            alpha_len=alpha_len, state=s.data_ptr())
    _lib.check(_lib.load().hsimae_svm_solve(C.byref(p), stream()), "hsimae_svm_solve")
    torch.cuda.synchronize()
    assert intact(aw) and intact(gw) and intact(sw)
    return a.cpu().numpy(), g.cpu().numpy(), s.cpu().numpy().reshape(len(rows), 8)


def assert_solution(sol, alpha, grad, state, what):
    want = np.array([sol["iterations"], sol["converged"], sol["gap"], sol["n_sv"], sol["n_bounded"], sol["rho"], 0, 0], np.float64)
    assert same_bits(alpha, sol["alpha"]), (what, "alpha", float(np.abs(alpha - sol["alpha"]).max()))
    assert same_bits(grad, sol["G"]), (what, "G", float(np.abs(grad - sol["G"]).max()))
    assert same_bits(state, want), (what, state, want)


PAIRS = [(1, 1), (1, 2), (31, 33), (40, 40), (257, 300), (2049, 2047)]
CS = [2.0 ** -3, 8.0, 2.0 ** 9]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "x".join(map(str, p)))
def test_solver_is_bit_equal_to_the_restatement_on_the_devices_own_kernel_matrix(pair):
    na, nb = pair
    n, D = na + nb, 8
    x = R.pair_case(na, nb, D, spread=1.5)
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), D, [1.0 / D], ldk=n)
    K = k.cpu().numpy()[0]
    rows = [(0, c, 0, na, na, nb, i * n) for i, c in enumerate(CS)]
    alpha, grad, state = run_solve(k, rows, 3 * n)
    for i, c in enumerate(CS):
        sol = R.smo(K, na, nb, c)
        print(f"{pair} C {c}: {sol['iterations']} iterations, gap {sol['gap']:.3g}, sv {sol['n_sv']}, bounded {sol['n_bounded']}")
        assert_solution(sol, alpha[i * n:(i + 1) * n], grad[i * n:(i + 1) * n], state[i], (pair, c))
        assert sol["converged"] == 1
        gap, nC = R.certificate(K, na, nb, c, alpha[i * n:(i + 1) * n], state[i, 5])
        assert 0 <= gap <= nC * 1e-3, (gap, nC)
    again = run_solve(k, rows, 3 * n)
    assert all(same_bits(u, v) for u, v in zip(again, (alpha, grad, state)))
    if n >= 64:
        assert state[0, 4] >= 0.5 * state[0, 3] and state[2, 4] <= 0.05 * state[2, 3]         # C = 1/8: most at the bound; C = 512: hardly any


def test_solver_identical_points_with_opposite_labels_take_the_tau_branch():
    x = np.zeros((2, 4), F32)
    x[:] = [0.5, -1.0, 2.0, 0.25]
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), 4, [0.5], ldk=4)
    K = k.cpu().numpy()[0]
    assert K[0, 1] == 1.0
    alpha, grad, state = run_solve(k, [(0, 8.0, 0, 1, 1, 1, 0)], 2)
    assert_solution(R.smo(K[:2, :2], 1, 1, 8.0), alpha, grad, state[0], "identical")
    assert np.all(alpha == 8.0)


def test_solver_stops_unconverged_at_max_iter_and_resumes_bit_for_bit():
    na, nb, D = 40, 40, 8
    n = na + nb
    x = R.pair_case(na, nb, D)
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), D, [1.0 / D], ldk=n)
    K = k.cpu().numpy()[0]
    row = [(0, 8.0, 0, na, na, nb, 0)]
    five = run_solve(k, row, n, max_iter=5)
    sol = R.smo(K, na, nb, 8.0, max_iter=5)
    assert sol["converged"] == 0 and sol["iterations"] == 5
    assert_solution(sol, five[0], five[1], five[2][0], "max_iter 5")
    step = run_solve(k, row, n, max_iter=1)
    for _ in range(4):
        step = run_solve(k, row, n, max_iter=1, resume=step)
    assert all(same_bits(u, v) for u, v in zip(step, five))
    whole = run_solve(k, row, n)
    rest = run_solve(k, row, n, resume=five)
    assert all(same_bits(u, v) for u, v in zip(rest, whole)) and whole[2][0, 1] == 1
    done = run_solve(k, row, n, max_iter=7, resume=whole)                                   # converged: nothing moves
    assert all(same_bits(u, v) for u, v in zip(done, whole))


def test_solver_one_launch_of_189_problems_equals_189_launches():
    n_class, per, D = 7, 12, 8
    bank, _, _, _ = R.clusters(n_class, D=D, per_class=per, Q=1)
    M = n_class * per
    gammas = [0.02, 1.0 / D, 1.0]
    _, k, _, _ = run_gram(torch.from_numpy(bank).cuda(), D, gammas, ldk=M)
    rows, off = [], 0
    for g, c in itertools.product(range(3), CS):
        for a, b in R.pairs(n_class):
            rows.append((g, c, a * per, per, b * per, per, off))
            off += 2 * per
    assert len(rows) == 189
    alpha, grad, state = run_solve(k, rows, off)
    assert np.all(state[:, 1] == 1)
    Kh = k.cpu().numpy()
    for r in (0, 57, 188):                                                                  # three of them against the restatement
        g, c, a0, na, b0, nb, o = rows[r]
        idx = np.r_[a0:a0 + na, b0:b0 + nb]
        assert_solution(R.smo(Kh[g][np.ix_(idx, idx)], na, nb, c), alpha[o:o + 24], grad[o:o + 24], state[r], r)
    for r, row in enumerate(rows):
        one = run_solve(k, [row[:6] + (0,)], 2 * per)
        o = row[6]
        assert same_bits(one[0], alpha[o:o + 24]) and same_bits(one[1], grad[o:o + 24]) and same_bits(one[2][0], state[r]), r


def test_solver_refuses_a_bad_table_row_and_reports_an_empty_class():
    x = R.pair_case(5, 5, 4)
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), 4, [0.25], ldk=12)
    rows = [(1, 8.0, 0, 5, 5, 5, 0), (0, 8.0, 0, 5, 6, 5, 0), (0, 8.0, 0, 5, 5, 5, 11), (0, -1.0, 0, 5, 5, 5, 0), (0, 8.0, 0, 0, 5, 5, 10),
            (0, 8.0, -1, 5, 5, 5, 0)]
    alpha, grad, state = run_solve(k, rows, 20)
    assert list(state[:, 1]) == [-1, -1, -1, -1, -2, -1]
    assert np.all(alpha[:10] == FILL) and np.all(alpha[10:15] == 0) and np.all(grad[10:15] == -1) and np.all(alpha[15:] == FILL)


def test_solver_reports_a_nan_in_the_bank_as_a_state_of_its_own():
    from hsimae_amd import RBFSVM
    x = R.pair_case(5, 5, 4)
    x[3] = np.nan
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), 4, [0.25], ldk=12)
    alpha, grad, state = run_solve(k, [(0, 8.0, 0, 5, 5, 5, 0)], 10)
    sol = R.smo(k.cpu().numpy()[0][:10, :10], 5, 5, 8.0)
    assert sol["converged"] == -3 and state[0, 1] == -3 and state[0, 0] == sol["iterations"] and np.isnan(grad).any()
    bank, by, _, _ = R.clusters(3, D=8, per_class=6, Q=1)
    bank[4] = np.nan
    with pytest.raises(RuntimeError, match="converge"):
        RBFSVM(num_class=4, gamma=0.125).fit(torch.from_numpy(bank).cuda(), by).check()


def test_solver_at_the_cap_of_8192_variables_uses_the_whole_lds_budget():
    na = nb = 4096                                           # n = M = 8192: 128 KiB of alpha and G + the scratch
    x = R.pair_case(na, nb, 8, spread=1.5)
    _, k, _, _ = run_gram(torch.from_numpy(x).cuda(), 8, [0.125], ldk=8192)
    row = [(0, 8.0, 0, na, na, nb, 0)]
    alpha, grad, state = run_solve(k, row, 8192, max_iter=40)
    K = k.cpu().numpy()[0]
    assert_solution(R.smo(K, na, nb, 8.0, max_iter=40), alpha, grad, state[0], "cap")
    assert state[0, 0] == 40 and state[0, 1] == 0
    again = run_solve(k, row, 8192, max_iter=40)
    assert all(same_bits(u, v) for u, v in zip(again, (alpha, grad, state)))


# ------------------------------------------------------------------ pack and predict
def device_fit(bank, counts, Cc, gamma, D):
    """Gram, solve and pack through the C ABI for a class-sorted bank -> dict of numpy results and device tensors."""
    from hsimae_amd import _lib
    n = len(counts)
    M = int(sum(counts))
    starts = np.cumsum(counts) - counts
    xd = torch.from_numpy(bank).cuda()
    _, k, _, sumsq = run_gram(xd, D, [gamma], ldk=(M + 3) // 4 * 4)
    rows, off = [], 0
    for a, b in R.pairs(n):
        rows.append((0, Cc, int(starts[a]), int(counts[a]), int(starts[b]), int(counts[b]), off))
        off += int(counts[a] + counts[b])
    alpha, grad, state = run_solve(k, rows, off)
    P = len(rows)
    table = torch.from_numpy(make_table(rows)).cuda()
    ad, sd = torch.from_numpy(alpha).cuda(), torch.from_numpy(state).cuda()
    bufs = {"sv_index": guarded(M, torch.int32), "sv_start": guarded(n + 1, torch.int32), "coef": guarded((n - 1) * M, torch.float32),
            "rho": guarded(P, torch.float32), "sv": guarded(M * D, torch.float32), "sv_sumsq": guarded(M, torch.float32)}
    p = _lib.SvmPackParams(table=table.data_ptr(), first_problem=0, n_class=n, alpha=ad.data_ptr(), alpha_len=off, state=sd.data_ptr(),
                           x=xd.data_ptr(), ldx=bank.shape[1], M=M, D=D, sumsq=sumsq.data_ptr(), sv_index=bufs["sv_index"][1].data_ptr(),
                           sv_start=bufs["sv_start"][1].data_ptr(), coef=bufs["coef"][1].data_ptr(), ldc=M, rho=bufs["rho"][1].data_ptr(),
                           sv=bufs["sv"][1].data_ptr(), ldsv=D, sv_sumsq=bufs["sv_sumsq"][1].data_ptr())
    _lib.check(_lib.load().hsimae_svm_pack(C.byref(p), stream()), "hsimae_svm_pack")
    torch.cuda.synchronize()
    assert all(intact(w) for w, _ in bufs.values())
    out = {key: v[1].cpu().numpy() for key, v in bufs.items()}
    out.update(dev={key: v[1] for key, v in bufs.items()}, whole={key: v[0] for key, v in bufs.items()}, K=k.cpu().numpy()[0][:, :M],
               alpha=alpha, state=state, rows=rows, starts=starts, sumsq=sumsq.cpu().numpy(), M=M, n=n, D=D, gamma=gamma)
    return out


def check_pack(fit, counts, Cc):
    sols = R.fit_ref(fit["K"], fit["starts"], counts, Cc)
    ref = R.pack_ref(sols, fit["starts"], counts)
    S, M, n = int(ref["sv_start"][-1]), fit["M"], fit["n"]
    assert np.array_equal(fit["sv_start"], ref["sv_start"]) and np.array_equal(fit["sv_index"][:S], ref["sv_index"])
    assert np.all(fit["sv_index"][S:] == FILL)
    coef = fit["coef"].reshape(n - 1, M)
    assert same_bits(np.ascontiguousarray(coef[:, :S]), ref["coef"]) and np.all(coef[:, S:] == FILL)
    assert same_bits(fit["rho"], ref["rho"])
    assert same_bits(fit["sv_sumsq"][:S], fit["sumsq"][ref["sv_index"]])
    return ref, sols


def test_pack_is_bit_equal_to_libsvms_compact_form():
    D = 8
    for counts, Cc in (([20] * 7, 8.0), ([1, 30, 7, 12], 8.0), ([25, 25, 25], 2.0 ** 9), ([300, 1, 280], 0.125)):
        n = len(counts)
        rng = np.random.RandomState(n + counts[0])
        centres = 1.2 * rng.standard_normal((n, D))
        bank = (centres[np.repeat(np.arange(n), counts)] + rng.standard_normal((sum(counts), D))).astype(F32)
        fit = device_fit(bank, np.array(counts), Cc, 1.0 / D, D)
        ref, sols = check_pack(fit, counts, Cc)
        S = int(ref["sv_start"][-1])
        assert same_bits(fit["sv"].reshape(-1, D)[:S], bank[ref["sv_index"]])
        if Cc == 2.0 ** 9:
            assert all(s["n_bounded"] == 0 for s in sols)                                   # a pair with no bounded SV
        again = device_fit(bank, np.array(counts), Cc, 1.0 / D, D)                          # twice, bit for bit, guards included
        for key, whole in fit["whole"].items():
            assert torch.equal(again["whole"][key].view(torch.int32), whole.view(torch.int32)), key
        print(f"counts {counts} C {Cc}: S = {S}")


def run_predict(fit, q, first=1, H=None, W=None, p0=0, pixels=None, conf=True, margin=True, probs=True, decision=True, outside=True,
                S_model=None):
    from hsimae_amd import _lib
    Q, n, M, D = q.shape[0], fit["n"], fit["M"], fit["D"]
    H, W = (1, Q) if H is None else (H, W)
    P, nc = n * (n - 1) // 2, first + n
    out = {"label": guarded(H * W, torch.int64), "conf": guarded(H * W, torch.float32) if conf else None,
           "margin": guarded(H * W, torch.float32) if margin else None, "probs": guarded(Q * (nc + 2), torch.float32) if probs else None,
           "decision": guarded(Q * (P + 1), torch.float32) if decision else None, "outside": guarded(2048, torch.int32) if outside else None}
    ptr = {key: (None if v is None else v[1].data_ptr()) for key, v in out.items()}
    d = fit["dev"]
    p = _lib.SvmPredictParams(q=q.data_ptr(), ldq=q.shape[1], Q=Q, D=D, sv=d["sv"].data_ptr(), ldsv=D, sv_sumsq=d["sv_sumsq"].data_ptr(),
                              sv_start=d["sv_start"].data_ptr(), S_max=M, coef=d["coef"].data_ptr(), ldc=M, rho=d["rho"].data_ptr(),
                              n_class=n, first=first, gamma=fit["gamma"], H=H, W=W, p0=p0, pixels=_lib.ptr(pixels), label_map=ptr["label"],
                              conf_map=ptr["conf"], margin_map=ptr["margin"], probs=ptr["probs"], ldp=nc + 2, decision=ptr["decision"],
                              ldd=P + 1, outside=ptr["outside"])
    _lib.check(_lib.load().hsimae_svm_predict(C.byref(p), stream()), "hsimae_svm_predict")
    torch.cuda.synchronize()
    assert all(v is None or intact(v[0]) for v in out.values())
    return out


def model_of(n, S, D, seed=0):
    """R.model_case with its arrays also on the device."""
    host = R.model_case(n, S, D, seed)
    host["dev"] = {key: torch.from_numpy(host[key]).cuda() for key in ("sv_start", "sv", "coef", "rho", "sv_sumsq")}
    return host


def check_predict(fit, q_host, out, first, row_of=None):
    Q, n, D = q_host.shape[0], fit["n"], fit["D"]
    P, nc = n * (n - 1) // 2, first + n
    S = int(fit["sv_start"][-1])
    dec = out["decision"][1].view(Q, P + 1).cpu().numpy()
    ref, bound = R.predict_ref(q_host, fit["sv"].reshape(-1, D)[:S], fit["sv_sumsq"][:S], fit["sv_start"],
                               fit["coef"].reshape(n - 1, -1)[:, :S], fit["rho"], fit["gamma"], D)
    err = np.abs(dec[:, :P] - ref)
    worst = float((err / bound).max())
    assert worst <= 1.0 and np.all(dec[:, P] == FILL), worst
    # the label rule from the restatement; the shares exactly from the device's own decision values
    decided, best = R.decided_rows(ref, bound, n)
    label, votes = R.votes_of(dec[:, :P], n, first)
    probs, conf, margin = R.shares_of(votes, label, first, nc)
    row_of = np.arange(Q) if row_of is None else row_of
    lm = out["label"][1].cpu().numpy()[row_of]
    assert np.array_equal(lm, label) and np.array_equal(lm[decided], first + best[decided])
    assert same_bits(out["conf"][1].cpu().numpy()[row_of], conf) and same_bits(out["margin"][1].cpu().numpy()[row_of], margin)
    pr = out["probs"][1].view(Q, nc + 2).cpu().numpy()
    assert same_bits(np.ascontiguousarray(pr[:, :nc]), probs) and np.all(pr[:, nc:] == FILL)
    return worst, 1.0 - float(decided.mean())


PAST_THE_GRID = 2048 * 64 + 1
# the whole product Q x S x C below the grid cap; past the cap two cases (the host restatement of 131,073 rows against 634 support
# rows and 190 pairs is what limits it); and 32 classes, the cap: 496 pairs, 141 KiB of LDS
PREDICT_CASES = list(itertools.product((1, 63, 65, 1000), (2, 64, 65, 634), (2, 7, 16, 20))) + [(PAST_THE_GRID, 64, 7), (PAST_THE_GRID, 2, 2),
                                                                                                  (65, 634, 32)]


@pytest.mark.parametrize("case", PREDICT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_predict_lies_inside_the_bound_and_follows_the_label_rule(case):
    Q, S, n = case
    D = 4 if Q == PAST_THE_GRID else 36
    fit = model_of(n, S, D)
    q = (0.6 * np.random.RandomState(Q + S).standard_normal((Q, D + 4))).astype(F32)
    q[:, D:] = np.nan
    qd = torch.from_numpy(q).cuda()
    out = run_predict(fit, qd)
    worst, open_share = check_predict(fit, q, out, 1)
    print(f"{case}: err / bound {worst:.3f}, share left open {open_share:.4f}")
    assert int(out["outside"][1].sum()) == 0
    again = run_predict(fit, qd)
    for key, v in out.items():
        assert torch.equal(again[key][0].view(torch.int32), v[0].view(torch.int32)), key


def test_predict_planted_vote_ties_go_to_the_lower_class():
    # three classes, no support rows: d_p = -rho_p.  rho = (-1, 1, -1): (0,1) -> 0, (0,2) -> 2, (1,2) -> 1: one vote each
    fit = model_of(3, 2, 4)
    fit["dev"]["sv_start"] = torch.zeros(4, dtype=torch.int32, device="cuda")
    fit["dev"]["rho"] = torch.tensor([-1.0, 1.0, -1.0], device="cuda")
    out = run_predict(fit, torch.ones(5, 4, device="cuda"), first=1)
    assert (out["label"][1] == 1).all() and (out["conf"][1] == np.float32(1) / np.float32(3)).all() and (out["margin"][1] == 0).all()
    fit["dev"]["rho"] = torch.tensor([1.0, 1.0, 0.0], device="cuda")                        # d = 0 votes for b: 0, 2 votes for 1 and 2
    out = run_predict(fit, torch.ones(5, 4, device="cuda"), first=0)
    assert (out["label"][1] == 2).all() and (out["probs"][1].view(5, 5)[:, :3].cpu() == torch.tensor([0.0, 1 / 3, 2 / 3])).all()


def test_predict_optional_outputs_pixel_forms_and_pixels_outside():
    Q, S, n, D = 130, 65, 7, 8
    fit = model_of(n, S, D, seed=3)
    q = (0.6 * np.random.RandomState(1).standard_normal((Q, D))).astype(F32)
    qd = torch.from_numpy(q).cuda()
    full = run_predict(fit, qd, H=10, W=15, p0=7)                                           # the range form: pixels 7 .. 136
    check_predict(fit, q, full, 1, row_of=np.arange(7, 137))
    assert (full["label"][1][:7] == FILL).all() and (full["label"][1][137:] == FILL).all()
    for flags in itertools.product((False, True), repeat=5):
        out = run_predict(fit, qd, H=10, W=15, p0=7, **dict(zip(("conf", "margin", "probs", "decision", "outside"), flags)))
        for key in ("label", "conf", "margin", "probs", "decision", "outside"):
            if out[key] is not None:
                assert torch.equal(out[key][0].view(torch.int32), full[key][0].view(torch.int32)), (key, flags)
    pix = np.random.RandomState(2).permutation(150)[:Q].astype(np.int64)
    pix[[3, 64, 129]] = [-1, 150, 1 << 40]                                                   # outside: counted, nothing written
    out = run_predict(fit, qd, H=10, W=15, pixels=torch.from_numpy(pix).cuda())
    inside = (pix >= 0) & (pix < 150)
    lm = out["label"][1].cpu().numpy()
    assert np.array_equal(lm[pix[inside]], full["label"][1].cpu().numpy()[7:137][inside])
    untouched = np.ones(150, bool)
    untouched[pix[inside]] = False
    assert np.all(lm[untouched] == FILL) and np.all(out["conf"][1].cpu().numpy()[untouched] == FILL)
    assert list(out["outside"][1][:4].cpu()) == [1, 1, 1, 0] and int(out["outside"][1].sum()) == 3
    assert torch.equal(out["decision"][1], full["decision"][1])


def test_refusals_write_nothing():
    from hsimae_amd import _lib
    for what, got, want in R.refusals(_lib.load(), _lib):
        assert got == want, (what, got, want)


# ------------------------------------------------------------------ RBFSVM against the reference record
@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("name,n", [("c7", 7), ("c16", 16)])
def test_rbfsvm_agrees_with_the_recorded_sklearn_results(gold, name, n):
    from hsimae_amd import RBFSVM
    bank, by, qs, _ = R.clusters(n, D=32, Q=200)
    svm = RBFSVM(num_class=n + 1, C=8.0, gamma=1.0 / 32).fit(torch.from_numpy(bank).cuda(), torch.from_numpy(by))
    svm.check()
    qd = torch.from_numpy(qs).cuda()
    dec = svm.decision_function(qd).cpu().numpy().astype(np.float64)
    m = svm.model
    S = int(m["sv_start"][-1])
    _, bound = R.predict_ref(qs, m["sv"].cpu().numpy()[:S], m["sv_sumsq"].cpu().numpy()[:S], m["sv_start"].cpu().numpy(),
                             m["coef"].cpu().numpy()[:, :S], m["rho"].cpu().numpy(), 1.0 / 32, 32)
    d10, dd_max = gold[f"{name}_t10_decision"], float(gold[f"{name}_dd_max"])
    tau = 4 * dd_max + bound
    worst = float((np.abs(dec - d10) / tau).max())
    decided, best = R.decided_rows(d10, tau, n)
    labels, conf, margin, probs = svm.predict(qd, return_probs=True)
    lab = labels.cpu().numpy()
    print(f"{name}: |d - d_sklearn| / tau {worst:.3f} (dd_max {dd_max:.3g}), share left open {1 - decided.mean():.4f}, "
          f"support rows {S} (sklearn at 1e-3: {gold[f'{name}_t3_support'].size})")
    assert worst <= 1.0
    assert np.array_equal(lab[decided], 1 + best[decided]) and np.array_equal(lab[decided], gold[f"{name}_t10_labels"][decided])
    assert 1 - decided.mean() <= 0.02
    assert float(probs[:, 0].max()) == 0 and torch.equal(probs.argmax(1), labels) and torch.equal(probs.max(1).values, conf)
    assert int(svm.n_support.sum()) == S and bool((svm.dual_gap < 1e-3).all()) and int(svm.iterations.min()) > 0
    again = RBFSVM(num_class=n + 1, C=8.0, gamma=1.0 / 32).fit(torch.from_numpy(bank).cuda(), torch.from_numpy(by))
    assert torch.equal(again.decision_function(qd).view(torch.int32), svm.decision_function(qd).view(torch.int32))
    # rows in another order: fit sorts them by class (stable), the model is the same
    perm = np.random.RandomState(1).permutation(by.size)
    shuffled = RBFSVM(num_class=n + 1, C=8.0, gamma=1.0 / 32).fit(torch.from_numpy(bank[perm]).cuda(), torch.from_numpy(by[perm]))
    shuffled.check()
    assert torch.equal(shuffled.bank.labels.cpu(), torch.from_numpy(np.sort(by)))
    assert torch.equal(shuffled.bank.x.cpu(), torch.from_numpy(bank[perm][np.argsort(by[perm], kind="stable")]))
    assert np.array_equal(shuffled.predict(qd)[0].cpu().numpy()[decided], lab[decided])


def test_rbfsvm_gamma_scale_and_check():
    from hsimae_amd import RBFSVM
    bank, by, qs, qy = R.clusters(7, D=32, Q=200)
    svm = RBFSVM(num_class=8).fit(torch.from_numpy(bank).cuda(), by)
    assert abs(svm.gamma_ - 1.0 / (32 * bank.astype(np.float64).var())) <= 1e-12 * svm.gamma_
    svm.check()
    acc = float((svm.predict(torch.from_numpy(qs).cuda())[0].cpu().numpy() == qy).mean())
    print(f"gamma scale {svm.gamma_:.5f}, accuracy {acc:.3f}")
    assert acc >= 0.9
    with pytest.raises(RuntimeError, match="converge"):
        RBFSVM(num_class=8, gamma=1.0 / 32, C=8.0, max_iter=3).fit(torch.from_numpy(bank).cuda(), by).check()
    with pytest.raises(RuntimeError, match="outside"):
        RBFSVM(num_class=7, gamma=1.0 / 32).fit(torch.from_numpy(bank).cuda(), by).check()      # label 7 is past num_class
    with pytest.raises(RuntimeError, match="no row"):
        RBFSVM(num_class=9, gamma=1.0 / 32).fit(torch.from_numpy(bank).cuda(), by).check()      # class 8 is empty
    with torch.cuda.device(0):
        x, y = torch.from_numpy(bank).cuda(), torch.from_numpy(by).cuda()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            quiet = RBFSVM(num_class=8, gamma=1.0 / 32, C=8.0).fit(x, y)                         # a float gamma waits for nothing
            out = quiet.predict(x)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert float((out[0] == y).float().mean()) >= 0.95


def test_grid_search_returns_the_recorded_sklearn_winner(gold):
    from hsimae_amd import RBFSVM
    bank, by, _, _ = R.clusters(7, D=32, Q=200)
    Cs, gammas = list(gold["grid_cs"]), list(gold["grid_gammas"])
    np.random.seed(123)
    svm = RBFSVM(num_class=8)
    c, g, table, (tr, va) = svm.grid_search(torch.from_numpy(bank).cuda(), by, Cs, gammas, keep_models=True)
    assert np.array_equal(tr, gold["grid_tr"]) and np.array_equal(va, gold["grid_va"])
    print("device\n", table, "\nsklearn\n", gold["grid_table"])
    assert (c, g) == (float(gold["grid_winner"][0]), float(gold["grid_winner"][1]))
    # a grid point agrees wherever none of its validation rows is undecided (tau = 4 dd_max + the prediction bound)
    agree = 0
    for m, (ci, gi) in enumerate(itertools.product(range(len(Cs)), range(len(gammas)))):
        mc, mg, mod = svm.last_search[m]
        assert (mc, mg) == (Cs[ci], gammas[gi])
        S = int(mod["sv_start"][-1])
        _, bound = R.predict_ref(bank[va], mod["sv"].cpu().numpy()[:S], mod["sv_sumsq"].cpu().numpy()[:S], mod["sv_start"].cpu().numpy(),
                                 mod["coef"].cpu().numpy()[:, :S], mod["rho"].cpu().numpy(), mg, 32)
        decided, _ = R.decided_rows(gold["grid_t10_decision"][m], 4 * float(gold["grid_dd_max"][m]) + bound, 7)
        if decided.all():
            agree += 1
            assert abs(table[ci, gi] - gold["grid_table"][ci, gi]) <= 1e-12, (ci, gi)
    assert agree >= 5


# ------------------------------------------------------------------ svm_scene, svm_eval_scene
def test_svm_scene_is_fit_and_predict_into_on_scene_features():
    from test_gpu_knn import scene_23x19, tiny_hsivit
    from hsimae_amd import RBFSVM
    from hsimae_amd.finetune import SceneClassification
    m = tiny_hsivit(seed=2)
    scene = scene_23x19(seed=6)
    rng = np.random.default_rng(3)
    bank_pix = rng.choice(437, 60, replace=False)
    bank_y = rng.integers(1, 7, 60)
    bank_y[:6] = np.arange(1, 7)
    sub = rng.permutation(437)[:300]
    res = m.svm_scene(scene, bank_pix, bank_y, pixels=sub, C=8.0, gamma=0.5, batch_size=256, return_probs=True)
    assert isinstance(res, SceneClassification) and not res.labels.is_cuda and tuple(res.labels.shape) == (23, 19)
    fb, fq = m.scene_features(scene, bank_pix, 256), m.scene_features(scene, sub, 256)
    svm = RBFSVM(num_class=7, C=8.0, gamma=0.5).fit(fb, torch.from_numpy(bank_y))
    lw, lm = guarded(437, torch.int64)
    cw, cm = guarded(437, torch.float32)
    mw, mm = guarded(437, torch.float32)
    pw, pm = guarded(300 * 7, torch.float32)
    svm.predict_into(fq, 23, 19, torch.from_numpy(sub).cuda(), lm, cm, mm, pm.view(300, 7))
    torch.cuda.synchronize()
    assert intact(lw) and intact(cw) and intact(mw) and intact(pw)
    asked = np.zeros(437, bool)
    asked[sub] = True
    for got, want in ((res.labels, lm), (res.confidence, cm), (res.margin, mm)):
        got, want = got.reshape(-1), want.cpu()
        assert torch.equal(got[asked], want[asked]) and (got[~asked] == 0).all() and (want[~asked] == FILL).all()
    assert torch.equal(res.probs, pm.view(300, 7).cpu()) and res.labels.reshape(-1)[asked].min() >= 1
    assert torch.equal(m.last_svm.model["coef"], svm.model["coef"]) and torch.equal(m.last_svm.model["sv_start"], svm.model["sv_start"])
    dev = m.svm_scene(torch.from_numpy(scene).cuda(), bank_pix, bank_y, C=8.0, gamma=0.5, batch_size=256, on_device=True)
    assert dev.probs is None and all(t.is_cuda for t in dev[:3]) and int(dev.labels.min()) >= 1 and float(dev.confidence.min()) > 0
    m.svm_scene(scene, bank_pix, bank_y, pixels=sub[:10], bank_flips="flips", gamma=0.5, batch_size=256)
    assert tuple(m.last_svm.bank.x.shape) == (240, 128)
    with pytest.raises(ValueError):
        m.svm_scene(scene, bank_pix, bank_y[:-1])
    with pytest.raises(ValueError):
        m.svm_scene(scene, bank_pix, bank_y, features="pixels")


def test_svm_scene_on_spectra_waits_for_nothing_with_a_float_gamma():
    from test_gpu_knn import tiny_hsivit
    m = tiny_hsivit(num_class=6, seed=2)                     # classes 1 .. 5, the planted scene's; never run: 12 bands are not its 32
    scene, gt = spectral_scene(bands=12)
    rng = np.random.RandomState(4)
    bank_pix = np.sort(rng.permutation(gt.size)[:150])
    bank_y = gt.reshape(-1)[bank_pix]
    sub = rng.permutation(gt.size)[:700]
    want = m.svm_scene(scene, bank_pix, bank_y, pixels=sub, features="spectra", C=8.0, gamma=0.05, return_probs=True)
    ds, y_dev = torch.from_numpy(scene).cuda(), torch.from_numpy(bank_y).cuda()   # the test's own uploads, before the region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = m.svm_scene(ds, bank_pix, bank_y, pixels=sub, features="spectra", C=8.0, gamma=0.05, return_probs=True, on_device=True)
        whole = m.svm_scene(ds, torch.from_numpy(bank_pix), y_dev, features="spectra", C=8.0, gamma=0.05,
                            on_device=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in res)
    for got, ref in zip(res, want):
        assert torch.equal(got.cpu(), ref)
    asked = np.zeros(gt.size, bool)
    asked[sub] = True
    assert torch.equal(whole.labels.reshape(-1).cpu()[asked], want.labels.reshape(-1)[asked]) and int(whole.labels.min()) >= 1
    assert float((whole.labels.cpu().numpy() == gt).mean()) >= 0.9


def spectral_scene(seed=0, bands=10):
    """smooth_ref's planted 48 x 40 layout (five classes) as a spectral scene: a signature per class plus noise."""
    import smooth_ref
    truth = smooth_ref.planted_scene()["truth"].reshape(48, 40)
    rng = np.random.RandomState(50 + seed)
    sig = rng.standard_normal((6, bands))
    return (sig[truth] + 0.6 * rng.standard_normal((48, 40, bands))), truth


def test_svm_eval_scene_scores_its_own_map_without_a_checkpoint(tmp_path):
    from test_gpu_knn import quiet
    from hsimae_amd import EdgeFilter, Superpixels, label_to_colormap, svm_eval_scene
    from hsimae_amd.finetune_train import scores
    import prob_ref
    scene, gt = spectral_scene()                              # 10 bands: no multiple of 8, the encoder could not take it
    rng = np.random.RandomState(4)
    flat = gt.reshape(-1)
    train_index = np.sort(rng.permutation(flat.size)[:150])
    train_labels = flat[train_index]
    test_gt = gt.copy()
    test_gt.reshape(-1)[train_index] = 0
    out = quiet(svm_eval_scene, scene, train_index, train_labels, test_gt, gt, search=False, C=8.0, gamma=0.05, save_dir=str(tmp_path),
                save_images=True)
    oa, aa, kappa, ca, pred = out
    assert pred.shape == gt.shape and pred.dtype == np.int64 and pred.min() >= 1 and pred.max() <= 5
    want = scores(test_gt.reshape(-1), np.where(gt == 0, 0, pred).reshape(-1))
    assert abs(oa - want[0]) <= 1e-12 and abs(aa - want[1]) <= 1e-12 and abs(kappa - want[2]) <= 1e-12
    assert np.allclose(ca, want[3], rtol=0, atol=1e-12) and oa >= 0.9
    tag = str(np.around(oa * 100, 2))
    assert sorted(os.listdir(os.path.join(tmp_path, "svm_rbf"))) == sorted([f"svm_rbf_all_oa_{tag}.png", f"svm_rbf_oa_{tag}.png"])
    whole = prob_ref.decode_png(open(os.path.join(tmp_path, "svm_rbf", f"svm_rbf_all_oa_{tag}.png"), "rb").read())
    assert np.array_equal(whole, label_to_colormap(pred))
    for smooth in (True, Superpixels()):
        sm = quiet(svm_eval_scene, scene, train_index, train_labels, test_gt, gt, search=False, C=8.0, gamma=0.05, smooth=smooth)
        assert sm[4].shape == gt.shape and sm[0] >= oa - 0.02, (smooth, sm[0], oa)
    np.random.seed(7)
    best = quiet(svm_eval_scene, scene, train_index, train_labels, test_gt, gt, search=True)
    print(f"planted spectral scene: OA {oa:.4f} at C = 8, gamma = 0.05; {best[0]:.4f} after the reference's grid search")
    assert best[0] >= 0.9
