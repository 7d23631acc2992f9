"""tests/kmeans_ref.py without a GPU: the fp64 restatement of csrc/kmeans.hip against plain numpy and sklearn, the emulated fp32
sequences inside their bounds at the GPU test's shapes, planted faults rejected by the checks, the Hungarian matching and the
partition scores of hsimae_amd/cluster.py, the ABI, and KMeans' argument refusals."""
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as R  # noqa: E402

SMALL = [c for c in R.CASES if c[0] < 10000]


def test_restatement_equals_plain_numpy_fp64():
    rng = np.random.RandomState(0)
    x, c = rng.standard_normal((300, 12)), rng.standard_normal((9, 12))
    s64, _ = R.scores_ref(x, c, 0.5 * (c * c).sum(1), 12)
    d2 = ((x[:, None, :] - c[None]) ** 2).sum(2)
    lab, best, second = R.assign_ref(s64)
    assert np.array_equal(lab, np.argmin(d2, axis=1))                                    # argmax score = argmin distance
    assert np.allclose(best - second, 0.5 * (np.sort(d2, 1)[:, 1] - np.sort(d2, 1)[:, 0]), rtol=0, atol=1e-12)
    lab[:3] = 8                                                                          # cluster 7 may or may not be empty: make one
    lab = np.where(lab == 7, 6, lab)
    u = R.update_ref(x, lab + 1, c, 9, 12, 1, False)
    sums, counts = np.zeros((9, 12)), np.bincount(lab, minlength=9)
    np.add.at(sums, lab, x)
    assert np.array_equal(u["counts"], counts) and counts[7] == 0 and u["empty"] == 1 and u["bad"] == 0
    m = counts > 0
    assert np.allclose(u["c"][m], sums[m] / counts[m, None], rtol=1e-15, atol=0) and np.array_equal(u["c"][~m], c[~m])
    assert abs(u["inertia"] - d2[np.arange(300), lab].sum()) <= 1e-12 * u["inertia"]
    un = R.update_ref(x, lab + 1, c, 9, 12, 1, True)
    assert np.allclose(np.linalg.norm(un["c"][m], axis=1), 1, rtol=0, atol=1e-15)
    assert R.update_ref(x, np.r_[0, 10, lab[2:] + 1], c, 9, 12, 1, False)["bad"] == 2


def test_fit_restatement_recovers_the_planted_clusters_in_two_changing_rounds():
    bank, by, qs, qy = R.clusters()
    seeds = R.class_seeds(bank, by, 7)
    f = R.fit_ref(qs, seeds, "euclidean", 20)
    assert np.array_equal(f["labels"], qy) and f["n_iter"] == 2 and abs(f["inertia"] - 31697.0988) < 1e-3
    c32 = f["c"].astype(np.float32)
    _, beta = R.scores_ref(qs, c32, R.bias_ref(c32, 32)[0].astype(np.float32), 32)
    print(f"smallest best-to-second gap at any round {f['min_gap']:.3f}, {f['min_gap'] / (2 * beta.max()):.0f} x twice the largest bound")
    assert abs(f["min_gap"] - 0.189) < 1e-3 and f["min_gap"] > 100 * 2 * beta.max()   # every label is decided far outside the bounds
    g = R.fit_ref(qs, seeds, "cosine", 20)
    assert np.array_equal(g["labels"], qy) and g["n_iter"] == 2
    for metric in ("euclidean", "cosine"):                                               # rounds past the fixed point change nothing
        a, b = R.fit_ref(qs, seeds, metric, 5), R.fit_ref(qs, seeds, metric, 20)
        assert np.array_equal(a["c"], b["c"]) and a["inertia"] == b["inertia"]


def test_fit_restatement_equals_sklearns_lloyd():
    sk = pytest.importorskip("sklearn.cluster")
    metrics = pytest.importorskip("sklearn.metrics")
    bank, by, qs, qy = R.clusters()
    seeds = R.class_seeds(bank, by, 7)
    f = R.fit_ref(qs, seeds, "euclidean", 20)
    km = sk.KMeans(n_clusters=7, init=seeds.astype(np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=20).fit(qs.astype(np.float64))
    assert np.array_equal(km.labels_ + 1, f["labels"]) and abs(km.inertia_ - f["inertia"]) <= 1e-9 * f["inertia"]
    assert metrics.adjusted_rand_score(qy, f["labels"]) == 1.0


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_emulated_sequences_lie_inside_their_bounds(case):
    N, K, D = case
    for exact, with_bias in ((False, True), (True, True), (False, False)):
        x, c, b = R.assign_case(N, K, D, D + 4, D + 8, exact=exact, bias=with_bias, spherical=not with_bias)
        s64, beta = R.scores_ref(x, c, b, D)
        lab, score, margin = R.emulate_assign(x, c, b, D, 1)
        w = R.check_assign(lab, score, margin, s64, beta, 1, exact=exact)
        assert w["ok"] and w["b_worst"] <= 1.0 and w["c_worst"] <= 1.0, (case, exact, with_bias, w)
    for normalize in (False, True):
        x, c, b = R.assign_case(N, K, D, D + 4, D + 8, seed=1, bias=not normalize, spherical=normalize)
        lab = R.emulate_assign(x, c, b, D, 1)[0]
        ref = R.update_ref(x, lab, c, K, D, 1, normalize)
        c32, b32, sums = R.emulate_update(x, lab, c, b, K, D, 1, normalize)
        assert np.array_equal(sums.view(np.int64), ref["sums"].view(np.int64))
        assert R.ratio(c32, ref["c"], ref["c_bound"]) <= 1.0
        if not normalize:
            b64, bb = R.bias_ref(c32, D)
            assert R.ratio(b32[ref["member"]], b64[ref["member"]], bb[ref["member"]]) <= 1.0


ASSIGN_FAULTS = ["bias_sign", "bias_no_half", "tie_higher"]


@pytest.mark.parametrize("fault", ASSIGN_FAULTS)
def test_assign_checks_reject_planted_faults(fault):
    N, K, D = 65, 65, 36
    exact = fault == "tie_higher"                             # only planted ties can see the tie rule: check (d)
    x, c, b = R.assign_case(N, K, D, D, D, exact=exact)
    s64, beta = R.scores_ref(x, c, b, D)
    good = R.check_assign(*R.emulate_assign(x, c, b, D, 1), s64, beta, 1, exact=exact)
    bad = R.check_assign(*R.emulate_assign(x, c, b, D, 1, fault=fault), s64, beta, 1, exact=exact)
    assert good["ok"] and not bad["ok"], (fault, bad)
    if fault == "tie_higher":
        assert bad["d_label"] > 0 and bad["a_better_left"] == 0      # the bounds alone cannot see it


@pytest.mark.parametrize("fault", ["empty_zeroed", "no_renorm", "descending"])
def test_update_checks_reject_planted_faults(fault):
    N, K, D = 130, 9, 36
    normalize = fault == "no_renorm"
    x, c, b = R.assign_case(N, K, D, D, D, seed=2, bias=not normalize, spherical=normalize)
    lab = R.emulate_assign(x, c, b, D, 1)[0]
    if fault == "descending":                                 # (a few fp32 values of one magnitude add exactly in fp64, in any order)
        x = R.wide_rows(x)
    lab = np.where(lab == lab[0], 1 + lab[0] % K, lab)                                   # cluster lab[0] - 1 is empty
    ref = R.update_ref(x, lab, c, K, D, 1, normalize)
    assert ref["empty"] >= 1
    m = ref["member"]

    def verdict(c32, b32, sums):
        return {"sums": np.array_equal(sums.view(np.int64), ref["sums"].view(np.int64)),
                "c": R.ratio(c32, ref["c"], ref["c_bound"]) <= 1.0,
                "kept": np.array_equal(c32[~m].view(np.int32), c[~m, :D].view(np.int32)) and
                (b32 is None or np.array_equal(b32[~m].view(np.int32), b[~m].view(np.int32)))}

    good = verdict(*R.emulate_update(x, lab, c, b, K, D, 1, normalize))
    bad = verdict(*R.emulate_update(x, lab, c, b, K, D, 1, normalize, fault=fault))
    assert all(good.values()), good
    if fault == "descending":                                 # the centroids stay inside their bound: only the exact-bits check
        assert not bad["sums"] and bad["c"] and bad["kept"]    # of the fp64 sums (the ascending chain) sees the order
    elif fault == "empty_zeroed":
        assert not bad["kept"] and not bad["c"]
    else:
        assert not bad["c"]


def test_hungarian_against_brute_force_and_scipy():
    from hsimae_amd.cluster import cluster_mapping, hungarian_max
    rng = np.random.RandomState(3)
    for n in range(1, 7):
        for _ in range(15):
            t = rng.randint(0, 12, (n, n)).astype(np.float64)
            r, c = hungarian_max(t)
            best = max(sum(t[i, p[i]] for i in range(n)) for p in itertools.permutations(range(n)))
            assert sorted(r) == list(range(n)) and sorted(c) == list(range(n)) and t[r, c].sum() == best
    t = np.array([[5, 0, 4], [0, 0, 9]], np.float64)                                    # 2 classes, 3 clusters
    assert list(cluster_mapping(t)) == [0, 0, 1]              # cluster 1 (matched to nothing) takes its majority class, ties low
    opt = pytest.importorskip("scipy.optimize")
    for shape in ((40, 17), (17, 40), (5, 9), (1, 3), (23, 23)):
        t = rng.randint(0, 100, shape).astype(np.float64)
        r, c = hungarian_max(t)
        r2, c2 = opt.linear_sum_assignment(t, maximize=True)
        assert len(r) == min(shape) and len(set(r)) == len(r) and len(set(c)) == len(c) and t[r, c].sum() == t[r2, c2].sum()


def test_partition_scores_against_hand_computed_tables_and_sklearn():
    from hsimae_amd.cluster import ari, nmi, purity
    same = np.diag([3.0, 5.0, 2.0])[:, [2, 0, 1]]                                       # a relabelling of the classes
    assert purity(same) == 1.0 and abs(nmi(same) - 1) <= 1e-15 and ari(same) == 1.0
    t = np.array([[2, 0], [1, 1]], np.float64)                # classes (0, 0, 1, 1) against clusters (0, 0, 0, 1)
    assert purity(t) == 0.75
    assert abs(ari(t) - 0.0) <= 1e-15                         # pairs: 1 together in both, expected 2 * 3 / 6 = 1 -> (1 - 1) / (2.5 - 1)
    h_a, h_b = np.log(2), -(0.75 * np.log(0.75) + 0.25 * np.log(0.25))
    mi = 0.5 * np.log(0.5 / (0.5 * 0.75)) + 0.25 * np.log(0.25 / (0.5 * 0.75)) + 0.25 * np.log(0.25 / (0.5 * 0.25))
    assert abs(nmi(t) - mi / ((h_a + h_b) / 2)) <= 1e-15
    indep = np.ones((3, 4)) * 5
    assert nmi(indep) == 0.0 and abs(ari(indep)) < 0.05 and nmi(np.array([[7.0]])) == 1.0 and ari(np.array([[7.0]])) == 1.0
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(5)
    a = rng.randint(0, 5, 500)
    b = (a + (rng.rand(500) < 0.3) * rng.randint(0, 7, 500)) % 7
    t = np.zeros((5, 7))
    np.add.at(t, (a, b), 1)
    assert abs(nmi(t) - metrics.normalized_mutual_info_score(a, b)) <= 1e-12
    assert abs(ari(t) - metrics.adjusted_rand_score(a, b)) <= 1e-12


def test_library_exports_the_kmeans_entry_points_under_abi_108():
    import hsimae_amd
    from hsimae_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    for name, struct in (("hsimae_kmeans_assign", _lib.KmeansAssignParams), ("hsimae_kmeans_update", _lib.KmeansUpdateParams)):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
        assert R.header_fields(hdr, name + "_params") == [(n, t) for n, t in struct._fields_], name
    assert _lib.KMEANS_GRID == R.GRID == int(re.search(r"#define HSIMAE_KMEANS_GRID (\d+)", hdr).group(1))
    assert _lib.KMEANS_STATE == int(re.search(r"#define HSIMAE_KMEANS_STATE (\d+)", hdr).group(1))
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    for cls in (hsimae_amd.DualViT, hsimae_amd.HSIViT):
        assert callable(cls.cluster_scene)
    assert callable(hsimae_amd.cluster_eval_scene) and hsimae_amd.SceneClustering._fields[0] == "labels"
    assert "kmeans" in build.UNITS and os.path.exists(os.path.join(build.CSRC, "dot_tile.h"))
    knn, km = (open(os.path.join(build.CSRC, f)).read() for f in ("knn.hip", "kmeans.hip"))
    for src in (knn, km):                                     # the tile is defined once, in the header both units include
        assert '#include "dot_tile.h"' in src and "mfma_f32_32x32x2f32" not in src and "atomic" not in src.split("#include")[-1]


def test_kmeans_refuses_what_it_cannot_serve():
    from hsimae_amd import KMeans
    for kw in (dict(n_clusters=0), dict(n_clusters=1025), dict(n_clusters=3, metric="manhattan"), dict(n_clusters=3, max_iter=0),
               dict(n_clusters=3, n_init=0), dict(n_clusters=3, first=-1), dict(n_clusters=3, init="k-means++")):
        with pytest.raises(ValueError):
            KMeans(**kw)
    with pytest.raises(TypeError):
        KMeans(3, init=np.zeros((3, 8), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KMeans(3).fit(torch.zeros(30, 8))
    with pytest.raises(RuntimeError, match="fit"):
        KMeans(3).predict(torch.zeros(3, 8))
    km = KMeans(4, metric="euclidean", max_iter=7, n_init=2)
    assert (km.n_clusters, km.metric, km.max_iter, km.n_init, km.first) == (4, "euclidean", 7, 2, 1)
