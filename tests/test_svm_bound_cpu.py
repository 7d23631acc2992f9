"""CPU checks behind tests/test_gpu_svm.py: the restatement of csrc/svm.hip (tests/svm_ref.py) against recorded sklearn results
(tests/golden/svm_cases.npz), its fp32 emulations against its bounds at the GPU test's shapes, planted faults, the label rule on
the recorded values alone, and the bindings and host rules of hsimae_amd/svm.py.  No GPU, no sklearn."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svm_ref as R  # noqa: E402

F32 = np.float32
D, GAMMA, CC = 32, 1.0 / 32, 8.0
CASES = [("c7", 7), ("c16", 16)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "svm_cases.npz"))


_FITS = {}


def fitted(n):
    """The restatement fitted in fp64 on the cluster case of n classes (computed once, shared, never changed)."""
    if n not in _FITS:
        bank, by, qs, qy = R.clusters(n, D=D, Q=200)
        x = bank.astype(np.float64)
        K = np.exp(-GAMMA * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        counts = [20] * n
        starts = [20 * c for c in range(n)]
        sols = R.fit_ref(K, starts, counts, CC)
        pk = R.pack_ref(sols, starts, counts)
        sv = bank[pk["sv_index"]]
        ss = np.diagonal(R.chain_dot(sv, sv)).copy()
        dec, bound = R.predict_ref(qs, sv, ss, pk["sv_start"], pk["coef"], pk["rho"], GAMMA, D)
        _FITS[n] = dict(bank=bank, by=by, qs=qs, K=K, counts=counts, starts=starts, sols=sols, pk=pk, sv=sv, ss=ss, dec=dec, bound=bound)
    return _FITS[n]


# ------------------------------------------------------------------ the restatement against sklearn
@pytest.mark.parametrize("name,n", CASES)
def test_restatement_reaches_sklearns_decision_values_and_its_certificate_holds(gold, name, n):
    """Two eps-stopped solvers on different paths (libsvm shrinks and caches, the restatement does neither) are each up to
    dd_max from the optimum; doubled for safety: 4 dd_max.  Measured: |d - d_sklearn(1e-10)| / dd_max = 0.96 (c7), 1.00 (c16)."""
    f = fitted(n)
    dd_max = float(gold[f"{name}_dd_max"])
    ratio = float(np.abs(f["dec"] - gold[f"{name}_t10_decision"]).max()) / dd_max
    print(f"{name}: |d - d_sklearn(1e-10)| / dd_max = {ratio:.3f}, dd_max {dd_max:.3g}")
    assert ratio <= 4.0
    assert np.array_equal(f["pk"]["sv_index"], np.sort(gold[f"{name}_t3_support"]))
    for s, (a, b) in zip(f["sols"], R.pairs(n)):
        rows = np.r_[20 * a:20 * a + 20, 20 * b:20 * b + 20]
        gap, nC = R.certificate(f["K"][np.ix_(rows, rows)], 20, 20, CC, s["alpha"], s["rho"])
        assert s["converged"] == 1 and 0 <= gap <= nC * 1e-3, (a, b, gap)


@pytest.mark.parametrize("name,n", CASES)
def test_label_rule_leaves_few_rows_open_on_the_recorded_values_alone(gold, name, n):
    bank, _, qs, _ = R.clusters(n, D=D, Q=200)
    sup = gold[f"{name}_t10_support"]
    sv = bank[sup]
    start = np.searchsorted(sup, 20 * np.arange(n + 1)).astype(np.int32)
    _, bound = R.predict_ref(qs, sv, np.diagonal(R.chain_dot(sv, sv)), start, gold[f"{name}_t10_dual_coef"].astype(F32),
                             -gold[f"{name}_t10_intercept"].astype(F32), GAMMA, D)
    tau = 4 * float(gold[f"{name}_dd_max"]) + bound
    decided, best = R.decided_rows(gold[f"{name}_t10_decision"], tau, n)
    print(f"{name}: tau up to {tau.max():.3g}, share left open {1 - decided.mean():.4f}")
    assert 1 - decided.mean() <= 0.02
    assert np.array_equal(1 + best[decided], gold[f"{name}_t10_labels"][decided])


# ------------------------------------------------------------------ the emulations inside their bounds
@pytest.mark.parametrize("Dd", [4, 36, 132])
def test_gram_emulation_stays_inside_its_bound_at_every_gpu_shape(Dd):
    for M, gammas in itertools.product((1, 2, 63, 64, 65, 257), ([1.0 / Dd], [0.01, 1.0 / Dd, 2.0])):
        x = R.gram_case(M, Dd, Dd + 4)
        K, n = R.gram_emulate(x, Dd, gammas)
        ref, bound = R.gram_ref(x, Dd, gammas)
        assert np.all(np.abs(K - ref) <= bound), (M, Dd)
        for g in range(len(gammas)):
            assert np.array_equal(K[g], K[g].T) and np.all(np.diagonal(K[g]) == 1)
        if M >= 3:
            assert np.all(K[:, 0, 2] == 1)


@pytest.mark.parametrize("case", [(1, 2, 2), (1, 634, 20), (63, 64, 7), (65, 65, 16), (1000, 634, 20), (65, 634, 2), (1000, 2, 16), (63, 65, 20),
                                  (65, 634, 32), (2048 * 64 + 1, 64, 7)], ids=lambda c: "x".join(map(str, c)))
def test_predict_emulation_stays_inside_its_bound_at_the_gpu_tests_extreme_shapes(case):
    """The corners of the GPU test's Q x S x C product (the emulation is per row and per pair: a size in between adds nothing),
    the 32-class cap and the case past the grid cap, with the GPU test's own D (36; 4 past the cap)."""
    Q, S, n = case
    Dd = 4 if Q > 1000 else 36
    m = R.model_case(n, S, Dd)
    q = (0.6 * np.random.RandomState(Q + S).standard_normal((Q, Dd))).astype(F32)
    dec = R.predict_emulate(q, m["sv"], m["sv_sumsq"], m["sv_start"], m["coef"], m["rho"], m["gamma"], Dd)
    ref, bound = R.predict_ref(q, m["sv"], m["sv_sumsq"], m["sv_start"], m["coef"], m["rho"], m["gamma"], Dd)
    worst = float((np.abs(dec - ref) / bound).max())
    print(f"{case}: err / bound {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ planted faults
def test_planted_faults_are_rejected(gold):
    f = fitted(7)
    rows = np.r_[0:20, 20:40]
    K = f["K"][np.ix_(rows, rows)]
    good = R.smo(K, 20, 20, CC)
    rejected = []
    # 1. j by the first-order rule: another trajectory
    bad = R.smo(K, 20, 20, CC, fault="first_order")
    assert bad["converged"] == 1 and not np.array_equal(bad["alpha"], good["alpha"])
    rejected.append("first_order")
    # 2. ties to the higher index: at the start every -y G of the positive class is 1
    bad = R.smo(K, 20, 20, CC, max_iter=1, fault="tie_higher_index")
    one = R.smo(K, 20, 20, CC, max_iter=1)
    assert np.flatnonzero(one["alpha"])[0] == 0 and np.flatnonzero(bad["alpha"])[0] == 19
    rejected.append("tie_higher_index")
    # 3. the update without clipping leaves the box
    small = R.smo(K, 20, 20, 2.0 ** -3)
    bad = R.smo(K, 20, 20, 2.0 ** -3, max_iter=small["iterations"], fault="unclipped")
    assert small["alpha"].max() <= 2.0 ** -3 < bad["alpha"].max()
    rejected.append("unclipped")
    # 4. rho from the bounded variables only
    bad = R.smo(K, 20, 20, CC, fault="rho_bounded_only")
    assert np.array_equal(bad["alpha"], good["alpha"]) and bad["rho"] != good["rho"]
    gap_bad, nC = R.certificate(K, 20, 20, CC, bad["alpha"], bad["rho"])
    gap_good, _ = R.certificate(K, 20, 20, CC, good["alpha"], good["rho"])
    assert gap_bad > gap_good
    rejected.append("rho_bounded_only")
    # 5, 6. an asymmetric K, a diagonal that is not 1
    x = R.gram_case(65, 36, 36)
    Ka, _ = R.gram_emulate(x, 36, [1 / 36], fault="asymmetric")
    assert not np.array_equal(Ka[0], Ka[0].T)
    Kd, _ = R.gram_emulate(x, 36, [1 / 36], fault="diag_computed")
    assert not np.all(np.diagonal(Kd[0]) == 1)
    rejected += ["asymmetric", "diag_computed"]
    # 7. a vote tie to the higher class
    dec = np.array([[1.0, -1.0, 1.0]])                                  # one vote each for 0, 2, 1
    assert R.votes_of(dec, 3, 1)[0][0] == 1 and R.votes_of(dec, 3, 1, fault="tie_higher_class")[0][0] == 3
    rejected.append("tie_higher_class")
    # 8. the decision sign flipped for the b side: labels leave sklearn's on decided rows
    tau = 4 * float(gold["c7_dd_max"]) + f["bound"]
    decided, _ = R.decided_rows(gold["c7_t10_decision"], tau, 7)
    lab = R.votes_of(f["dec"], 7, 1)[0]
    bad_lab = R.votes_of(f["dec"], 7, 1, fault="b_sign_flipped")[0]
    assert np.array_equal(lab[decided], gold["c7_t10_labels"][decided]) and not np.array_equal(bad_lab[decided], gold["c7_t10_labels"][decided])
    rejected.append("b_sign_flipped")
    # 9. pack takes the coefficient of the wrong opposing class: the decision values leave the bound
    bad_pk = R.pack_ref(f["sols"], f["starts"], f["counts"], fault="wrong_opponent")
    assert not np.array_equal(bad_pk["coef"], f["pk"]["coef"])
    bad_dec, _ = R.predict_ref(f["qs"], f["sv"], f["ss"], bad_pk["sv_start"], bad_pk["coef"], bad_pk["rho"], GAMMA, D)
    assert np.abs(bad_dec - gold["c7_t10_decision"]).max() > tau.max()
    rejected.append("wrong_opponent")
    assert len(rejected) >= 8


def test_resume_of_the_restatement_is_bit_exact():
    x = R.pair_case(31, 33).astype(np.float64)
    K = np.exp(-((x[:, None] - x[None]) ** 2).sum(-1) / 8).astype(F32)
    whole = R.smo(K, 31, 33, CC, max_iter=7)
    step = R.smo(K, 31, 33, CC, max_iter=1)
    for _ in range(6):
        step = R.smo(K, 31, 33, CC, max_iter=1, alpha=step["alpha"], G=step["G"])
    assert step["alpha"].tobytes() == whole["alpha"].tobytes() and step["G"].tobytes() == whole["G"].tobytes()


# ------------------------------------------------------------------ bindings and host rules
def test_reference_grid_equals_the_two_lists_written_out():
    from hsimae_amd import reference_grid
    cs, gs = reference_grid()
    assert cs == [0.125, 0.5, 2.0, 8.0, 32.0, 128.0, 512.0] and gs == [0.03125, 0.125, 0.5, 2.0, 8.0]
    cs, gs = reference_grid(8.0, 0.125)
    mult = [2.0 ** e for e in (-1.75, -1.5, -1.25, -1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75)]
    assert cs == [8.0 * m for m in mult] and gs == [0.125 * m for m in mult] and len(cs) == 15


def test_pick_winner_takes_only_a_strict_improvement_in_product_order():
    from hsimae_amd.svm import pick_winner
    Cs, gs = [1.0, 2.0], [0.1, 0.2, 0.3]
    assert pick_winner(Cs, gs, [[1.0, 2.5, 2.5], [2.5, 2.0, 2.5]]) == (1.0, 0.2, 2.5)          # the first of the equals
    assert pick_winner(Cs, gs, [[1.0, 2.5, 2.5], [2.5, 2.6, 2.5]]) == (2.0, 0.2, 2.6)
    assert pick_winner(Cs, gs, [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]) == (0, 0, 0)                # nothing beats the start value 0
    assert pick_winner(Cs, gs, [[0.0, -1.0, 0.0], [0.0, 1e-9, 0.0]]) == (2.0, 0.2, 1e-9)


def test_struct_mirrors_match_the_header_and_the_abi_is_still_108():
    from hsimae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    for name, struct in (("hsimae_svm_gram_params", _lib.SvmGramParams), ("hsimae_svm_problem", _lib.SvmProblem),
                         ("hsimae_svm_solve_params", _lib.SvmSolveParams), ("hsimae_svm_pack_params", _lib.SvmPackParams),
                         ("hsimae_svm_predict_params", _lib.SvmPredictParams)):
        want = R.header_fields(hdr, name)
        got = [(f[0], f[1]) for f in struct._fields_]
        assert [w[0] for w in want] == [g[0] for g in got], name
        for (fn, wt), (_, gt) in zip(want, got):
            assert ctypes.sizeof(wt) == ctypes.sizeof(gt) and (wt is gt or issubclass(gt, ctypes.Array) == issubclass(wt, ctypes.Array)), (name, fn)
    assert ctypes.sizeof(_lib.SvmProblem) == 64
    assert "#define HSIMAE_VERSION 108" in hdr and _lib.ABI_VERSION == 108 and _lib.load().hsimae_version() == 108
    for sym in ("hsimae_svm_gram", "hsimae_svm_solve", "hsimae_svm_pack", "hsimae_svm_predict"):
        assert sym in _lib.SYMBOLS


def test_refusals_through_the_library():
    from hsimae_amd import _lib
    for what, got, want in R.refusals(_lib.load(), _lib):
        assert got == want, (what, got, want)


def test_host_side_refusals_of_rbfsvm():
    from hsimae_amd import RBFSVM
    for kw in (dict(num_class=2), dict(num_class=35), dict(num_class=8, C=0.0), dict(num_class=8, gamma=-1.0), dict(num_class=8, eps=0.0),
               dict(num_class=8, first=-1)):
        with pytest.raises(ValueError):
            RBFSVM(**kw)
    with pytest.raises(RuntimeError, match="fit"):
        RBFSVM(num_class=8).n_support
