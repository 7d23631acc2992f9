"""csrc/knn.hip without a GPU: the fp64 restatement (tests/knn_ref.py) against DINO's arithmetic composed from torch in fp64, the
kernels' sequences in exactly rounded fp32 inside their bounds, the bounds and checks against planted faults, the share of rows
the label rules leave open, and the three new entry points under ABI 108 (struct mirrors, refusal codes)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import knn_ref as R  # noqa: E402

VOTE_CPU = [s for s in R.VOTE_SHAPES if s[0] <= 512]


def test_restatement_equals_dinos_arithmetic_in_torch_fp64():
    """F.normalize, @, topk, exp(s / T) WITHOUT the shift, a one-hot index_add and the normalisation."""
    bank, by, qs, _ = R.clusters()
    k, T, Cc, first = 20, 0.07, 8, 1
    qn = torch.nn.functional.normalize(torch.from_numpy(qs).double(), dim=1)
    bn = torch.nn.functional.normalize(torch.from_numpy(bank).double(), dim=1)
    out, _, n, _ = R.normalize_ref(qs, qs.shape[1])
    assert np.allclose(out, qn.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(n, torch.from_numpy(qs).double().norm(dim=1).numpy(), rtol=1e-14, atol=0)
    sim, idx = (qn @ bn.T).topk(k, dim=1)
    s64, _ = R.dots(qn.numpy(), bn.numpy(), qs.shape[1])
    assert np.array_equal(R.order_of(s64)[:, :k], idx.numpy())
    w = torch.exp(sim / T)
    votes = torch.zeros(qs.shape[0], Cc, dtype=torch.float64)
    votes.scatter_add_(1, torch.from_numpy(by)[idx], w)
    want = (votes / votes.sum(1, keepdim=True)).numpy()
    ref = R.vote_ref(idx.numpy(), sim.numpy(), by, Cc, first, 1.0 / T)
    assert np.allclose(ref["p"], want, rtol=0, atol=1e-12) and np.all(ref["p"][:, 0] == 0)
    assert np.array_equal(ref["label"], np.argmax(want, 1)) and not ref["bad"].any()
    top2 = np.sort(want, 1)[:, -2:]
    assert np.allclose(ref["conf"], top2[:, 1], rtol=0, atol=1e-12) and np.allclose(ref["margin"], top2[:, 1] - top2[:, 0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("D", [1, 4, 63, 64, 65, 1536])
def test_normalize_sequence_lies_inside_its_bound(D):
    for N in (1, 5, 257):
        x = R.normalize_case(N, D, D + 3)
        out, bound, n, nb = R.normalize_ref(x, D)
        got, gn = R.emulate_normalize(x, D)
        assert R.ratio(got, out, bound) <= 1.0 and R.ratio(gn, n, nb) <= 1.0, (N, D)
        if N >= 5:
            assert np.all(got[0] == 0) and n[1] < 1e-12 and np.isfinite(got[2]).all() and abs(abs(got[3, D // 2]) - 1) <= 2 * R.U


@pytest.mark.parametrize("case", [(1, 20, 4, 1), (63, 64, 8, 2), (65, 65, 36, 20), (130, 257, 512, 64), (5, 1000, 1536, 20)],
                         ids=lambda c: "x".join(map(str, c)))
def test_topk_sequence_passes_every_check(case):
    Q, M, D, k = case
    q, b = R.topk_case(Q, M, D, D + 4, D + 8)
    idx, sim = R.emulate_topk(q, b, D, k)
    w = R.check_topk(idx, sim, q, b, D, k)
    assert w["ok"] and w["b_worst"] <= 1.0, w
    if D <= 36:
        q, b = R.topk_case(Q, M, D, D + 4, D, exact=True)
        w = R.check_topk(*R.emulate_topk(q, b, D, k), q, b, D, k, exact=True)
        assert w["ok"] and w["b_worst"] == 0.0, w


@pytest.mark.parametrize("shape", VOTE_CPU, ids=lambda s: "x".join(map(str, s)))
def test_vote_sequence_lies_inside_its_bound(shape):
    Q, Cc, _ = shape
    for first in (0, 1):
        for k in R.KS:
            for T in R.TEMPS:
                idx, sim, labels = R.vote_case(Q, Cc, first, k, T)
                ref = R.vote_ref(idx, sim, labels, Cc, first, R.inv_t32(T))
                w = R.vote_worst(R.emulate_vote(idx, sim, labels, Cc, first, R.inv_t32(T)), ref, first)
                assert w["all"] <= 1.0, (shape, first, k, T, w)


def test_planted_ties_go_to_the_lower_class():
    for idx, sim, labels, Cc, first, want in R.tie_cases():
        ref = R.vote_ref(idx, sim, labels, Cc, first, R.inv_t32(0.07))
        p, label, conf, margin = R.emulate_vote(idx, sim, labels, Cc, first, R.inv_t32(0.07))
        assert ref["label"][0] == want == label[0] and conf[0] == 0.5 and margin[0] == 0 and ref["margin"][0] == 0


VOTE_FAULTS = ["no_shift", "T_not_invT", "tie_higher_class", "class0_nonzero"]
TOPK_FAULTS = ["tie_higher_index", "drop_kth", "unsorted", "transposed_idx"]


@pytest.mark.parametrize("fault", VOTE_FAULTS)
def test_vote_bound_rejects_planted_faults(fault):
    Q, Cc, first, k, T = 65, 33, 1, 20, 0.01
    if fault == "tie_higher_class":
        for idx, sim, labels, Cc2, f2, want in R.tie_cases():
            ref = R.vote_ref(idx, sim, labels, Cc2, f2, R.inv_t32(T))
            ref["decided"][:] = True                          # an exact tie: the lower class, whatever the gap
            assert R.vote_worst(R.emulate_vote(idx, sim, labels, Cc2, f2, R.inv_t32(T)), ref, f2)["all"] <= 1.0
            assert R.vote_worst(R.emulate_vote(idx, sim, labels, Cc2, f2, R.inv_t32(T), fault), ref, f2)["wrong"] == 1
        return
    idx, sim, labels = R.vote_case(Q, Cc, first, k, T)
    ref = R.vote_ref(idx, sim, labels, Cc, first, R.inv_t32(T))
    assert R.vote_worst(R.emulate_vote(idx, sim, labels, Cc, first, R.inv_t32(T)), ref, first)["all"] <= 1.0
    w = R.vote_worst(R.emulate_vote(idx, sim, labels, Cc, first, R.inv_t32(T), fault, T=T), ref, first)
    print(f"{fault}: worst err / bound = {w['all']:.3g}")
    assert w["all"] > 10.0, w


@pytest.mark.parametrize("fault", TOPK_FAULTS)
def test_topk_checks_reject_planted_faults(fault):
    Q, M, D, k = 65, 257, 8, 20
    exact = fault == "tie_higher_index"
    q, b = R.topk_case(Q, M, D, D, D, exact=exact)
    assert R.check_topk(*R.emulate_topk(q, b, D, k), q, b, D, k, exact=exact)["ok"]
    w = R.check_topk(*R.emulate_topk(q, b, D, k, fault), q, b, D, k, exact=exact)
    print(fault, w)
    assert not w["ok"]
    broken = {"tie_higher_index": ("a_sorted", "d_idx"), "drop_kth": ("c_left_out",), "unsorted": ("a_sorted",),
              "transposed_idx": ("b_sim",)}[fault]
    assert all(w[key] > 0 for key in broken), w


def test_normalize_bound_rejects_a_wrong_eps_rule():
    x = R.normalize_case(5, 64, 64)
    out, bound, _, _ = R.normalize_ref(x, 64)
    assert R.ratio(R.emulate_normalize(x, 64)[0], out, bound) <= 1.0
    assert R.ratio(R.emulate_normalize(x, 64, "eps_added")[0], out, bound) > 10.0


def test_vote_label_rule_leaves_out_at_most_a_hundredth_of_a_case():
    worst, total = 0.0, 0
    for Q, Cc, _ in R.VOTE_SHAPES:
        for first in (0, 1):
            for k in R.KS:
                for T in R.TEMPS:
                    idx, sim, labels = R.vote_case(Q, Cc, first, k, T)
                    ref = R.vote_ref(idx, sim, labels, Cc, first, R.inv_t32(T))
                    share = float((~ref["decided"]).sum()) / Q
                    worst, total = max(worst, share), total + Q
                    assert share <= 0.01, ((Q, Cc), first, k, T, share)
    print(f"{total} rows, worst share left open {worst:.5f}")


def test_predict_rule_leaves_out_at_most_a_fiftieth_of_the_cloud():
    bank, by, qs, qy = R.clusters()
    qn, bn = R.emulate_normalize(qs, 32)[0], R.emulate_normalize(bank, 32)[0]
    ref = R.predict_ref(qn, bn, by, 20, 8, 1, R.inv_t32(0.07))
    share = float((~ref["decided"]).sum()) / qs.shape[0]
    acc = float((ref["label"] == qy).mean())
    print(f"share left open {share:.4f}, k-NN accuracy of the restatement on the clusters {acc:.3f}")
    assert share <= 0.02 and acc > 0.9


def test_library_exports_the_knn_entry_points_under_abi_108():
    import hsimae_amd
    from hsimae_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    for name, struct in (("hsimae_row_normalize", _lib.RowNormalizeParams), ("hsimae_knn_topk", _lib.KnnTopkParams),
                         ("hsimae_knn_vote", _lib.KnnVoteParams)):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
        assert R.header_fields(hdr, name + "_params") == [(n, t) for n, t in struct._fields_], name
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    for cls in (hsimae_amd.DualViT, hsimae_amd.HSIViT):
        assert callable(cls.scene_features) and callable(cls.knn_scene)
    assert callable(hsimae_amd.knn_eval_scene) and hsimae_amd.KNNClassifier(k=20).temperature == 0.07
    from hsimae_amd import build
    assert "knn" in build.UNITS


def test_classifier_refuses_what_it_cannot_serve():
    from hsimae_amd import KNNClassifier
    for kw in (dict(k=0), dict(k=65), dict(temperature=0), dict(temperature=-1), dict(first=-1)):
        with pytest.raises(ValueError):
            KNNClassifier(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KNNClassifier().fit(torch.zeros(30, 8), torch.ones(30, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="fit"):
        KNNClassifier().predict(torch.zeros(3, 8))
