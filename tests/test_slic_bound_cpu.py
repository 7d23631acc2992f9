"""tests/slic_ref.py without a GPU: the fp64 restatement of csrc/slic.hip against an independently written per-pixel loop, the
emulated fp32 sequence inside its bounds and the share of pixels left open at the GPU test's cases, the planted scene, planted
faults rejected by the checks, the ABI, and the argument refusals of the Python layer."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slic_ref as R  # noqa: E402
import smooth_ref  # noqa: E402

FILL = -7


def pixel_loop(guide, scale, centres, w, S):
    """One assign and one update written pixel by pixel in Python floats (fp64), sharing nothing with slic_ref
    -> (label [H, W], dist [H, W], new centres [K, G + 2] as fp64 means, counts)."""
    H, W, G = guide.shape
    ny, nx = -(-H // S), -(-W // S)
    label, dist = np.zeros((H, W), np.int64), np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            hi, hj = y * ny // H, x * nx // W
            best, bd = hi * nx + hj, float("nan")
            for ci in range(hi - 1, hi + 2):
                for cj in range(hj - 1, hj + 2):
                    if not (0 <= ci < ny and 0 <= cj < nx):
                        continue
                    c = centres[ci * nx + cj]
                    d = sum((float(scale[g]) * float(guide[y, x, g]) - float(c[g])) ** 2 for g in range(G))
                    d += w * ((y - float(c[G])) ** 2 + (x - float(c[G + 1])) ** 2)
                    if d == d and (bd != bd or d < bd):
                        best, bd = ci * nx + cj, d
            label[y, x], dist[y, x] = best, bd
    K = ny * nx
    new, cnt = np.zeros((K, G + 2)), np.zeros(K, np.int64)
    for k in range(K):
        tot = [0.0] * (G + 2)
        for y in range(H):
            rowsum = [0.0] * (G + 2)
            for x in range(W):
                if label[y, x] == k:
                    cnt[k] += 1
                    vals = [float(np.float32(scale[g]) * np.float32(guide[y, x, g])) for g in range(G)] + [float(y), float(x)]
                    rowsum = [a + b for a, b in zip(rowsum, vals)]
            tot = [a + b for a, b in zip(tot, rowsum)]
        new[k] = [t / max(cnt[k], 1) for t in tot]
    return label, dist, new, cnt


@pytest.mark.parametrize("c", [(9, 17, 8, 1, ""), (23, 19, 3, 3, "const"), (17, 33, 4, 4, "nan")], ids=R.case_id)
def test_restatement_equals_a_per_pixel_double_loop(c):
    case = R.make_case(*c)
    H, W, S, G, _ = c
    guide, scale, w = case["guide"], case["scale"], case["w"]
    centres = R.update_ref(guide, scale, R.emulate_assign(guide, scale, case["start"], w, S)[0], case["start"])[0]    # off the grid
    ref = R.assign_ref(guide, scale, centres, w, S)
    label, dist, new, cnt = pixel_loop(guide, scale, centres, w, S)
    settled = ~ref["open"]
    assert settled.mean() > 0.98 and np.array_equal(ref["label"][settled], label[settled])
    same = ref["label"] == label
    assert np.allclose(ref["dist"][same], dist[same], rtol=1e-12, atol=0, equal_nan=True)
    got, bound, counts = R.update_ref(guide, scale, label, centres)
    assert np.array_equal(counts, cnt)
    has = cnt > 0
    err = np.abs(got[has, :G + 2].astype(np.float64) - new[has])
    ok = np.isnan(new[has]) & np.isnan(got[has, :G + 2]) | (err <= bound[has, :G + 2])
    assert ok.all()
    assert np.array_equal(got[~has].view(np.int32), centres[~has].view(np.int32))


def test_grid_start_and_candidates_are_the_definition():
    H, W, S = 9, 17, 8
    assert R.grid(H, W, S) == (2, 3)
    hi, hj = R.homes(H, W, S)
    assert hi.tolist() == [y * 2 // 9 for y in range(9)] and hj.tolist() == [x * 3 // 17 for x in range(17)]
    case = R.make_case(H, W, S, 1, "")
    c = R.init_centres(case["guide"], case["scale"], S)
    assert c[:, 1].tolist() == [2, 2, 2, 6, 6, 6] and c[:, 2].tolist() == [2, 8, 14, 2, 8, 14] and not c[:, 3:].any()
    assert c[4, 0] == np.float32(case["scale"][0] * case["guide"][6, 8, 0])
    cand = R.candidates(H, W, S)
    assert cand[0, 0].tolist() == [-1, -1, -1, -1, 0, 1, -1, 3, 4] and cand[8, 16].tolist() == [1, 2, -1, 4, 5, -1, -1, -1, -1]
    assert R.weight(0.1, 8) == float(np.float32(0.01 / 64)) and R.weight(2.0, 8) == 0.0625


def run_case(c, fault=None):
    """The emulated device through the GPU test's sequence of checks -> (assign from the start, update, assign from the new centres)."""
    case = R.make_case(*c)
    S = c[2]
    guide, scale, w, start = case["guide"], case["scale"], case["w"], case["start"]
    afault = fault if fault in R.ASSIGN_FAULTS else None
    lab, dist, cnt = R.emulate_assign(guide, scale, start, w, S, afault)
    if fault == "count_off":
        cnt = cnt.copy()
        cnt[cnt.argmax()] -= 1
    a = R.check_assign(guide, scale, start, w, S, lab, dist, cnt, exact=case["exact"])
    new = R.update_ref(guide, scale, lab, start, fault)[0]
    u = R.check_update(guide, scale, lab, start, new)
    lab2, dist2, cnt2 = R.emulate_assign(guide, scale, new, w, S, afault)
    b = R.check_assign(guide, scale, new, w, S, lab2, dist2, cnt2)
    return case, a, u, b


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_emulated_fp32_sequence_stays_inside_the_bounds_and_few_labels_stay_open(c):
    case, a, u, b = run_case(c)
    print(f"{R.case_id(c)}: start: dist err / bound {a['dist']:.3f}, open {a['open']:.5f}; update err / bound {u['ratio']:.3f}, "
          f"{u['empty']} empty; next: dist {b['dist']:.3f}, open {b['open']:.5f}")
    assert a["wrong"] == 0 and a["counts"] and a["first"] and a["dist"] <= 1.0
    assert u["kept"] and u["bits"] and u["ratio"] <= 1.0
    assert b["wrong"] == 0 and b["counts"] and b["dist"] <= 1.0
    if case["exact"]:
        return            # every tie of exact inputs is open by construction; there the labels must equal the first argmin instead
    assert a["open"] <= 0.02 and b["open"] <= 0.02
    if c[4] == "empty":
        assert u["empty"] >= 1


def test_exact_cases_do_hold_ties_and_the_empty_start_has_an_empty_centre():
    ties = 0
    for c in R.CASES:
        if c[4] == "dyadic" and R.grid(*c[:3]) != (1, 1):
            case = R.make_case(*c)
            ref = R.assign_ref(case["guide"], case["scale"], case["start"], case["w"], c[2])
            key = np.sort(np.where(np.isnan(ref["d"]), np.inf, ref["d"]), axis=2)
            ties += int(np.sum(key[..., 0] == key[..., 1]))
    assert ties > 0


VOTE_FAULT_CASE = (23, 19, 3, 18, 1, "subset", 0, 1)


@pytest.mark.parametrize("fault", ["tie_upward", "border_cell_dropped", "spatial_unweighted", "empty_overwritten", "count_off"])
def test_a_planted_fault_in_the_segmentation_is_caught(fault):
    c = {"tie_upward": (17, 33, 4, 4, "dyadic"), "border_cell_dropped": (17, 33, 4, 4, ""), "spatial_unweighted": (23, 19, 3, 3, ""),
         "empty_overwritten": (23, 19, 3, 3, "empty"), "count_off": (9, 17, 8, 1, "")}[fault]
    assert c in R.CASES
    _, a, u, b = run_case(c)
    assert a["all"] <= 1.0 and u["all"] <= 1.0 and b["all"] <= 1.0
    _, a, u, b = run_case(c, fault)
    assert max(a["all"], u["all"], b["all"]) > 1.0, fault


@pytest.mark.parametrize("fault", ["mean_over_unclassified", "fill_ignored"])
def test_a_planted_fault_in_the_vote_is_caught(fault):
    c = VOTE_FAULT_CASE
    assert c in R.VOTE_CASES
    H, W, S, C, first, form, mode, fill = c
    case = R.make_vote_case(*c)
    ref = R.vote_ref(case["probs"], case["n"], C, first, case["row_of"], case["label"], S, mode, fill)
    good = R.emulate_vote(case["probs"], case["n"], C, first, case["row_of"], case["label"], S, mode, fill, FILL)
    assert R.check_vote(ref, first, C, *good, FILL)["all"] <= 1.0
    bad = R.emulate_vote(case["probs"], case["n"], C, first, case["row_of"], case["label"], S, mode, fill, FILL, fault)
    assert R.check_vote(ref, first, C, *bad, FILL)["all"] > 1.0, fault


@pytest.mark.parametrize("c", R.VOTE_CASES, ids=R.vote_id)
def test_vote_cases_hold_what_they_promise(c):
    H, W, S, C, first, form, mode, fill = c
    case = R.make_vote_case(*c)
    lab = case["label"].astype(np.int64)
    ny, nx = R.grid(H, W, S)
    hi, hj = R.homes(H, W, S)
    assert np.abs(lab // nx - hi[:, None]).max() <= 1 and np.abs(lab % nx - hj[None, :]).max() <= 1     # the locality the kernel rests on
    ref = R.vote_ref(case["probs"], case["n"], C, first, case["row_of"], case["label"], S, mode, fill)
    if form == "subset":
        assert ref["cnt"][case["dead"]] == 0 and (lab == case["dead"]).any() and not ref["written"][ref["seg"] == case["dead"]].any()
        if fill and H * W > 100:                                                                        # fill does reach pixels without a row
            assert ref["written"].sum() > (np.asarray(case["row_of"]) >= 0).sum()
    if form == "ties":
        v = ref["vec"][ref["live"]]
        top = np.sort(v[:, first:], axis=1)
        assert np.sum(top[:, -1] == top[:, -2]) > 0                                                     # exact ties do occur
    got = R.emulate_vote(case["probs"], case["n"], C, first, case["row_of"], case["label"], S, mode, fill, FILL)
    assert R.check_vote(ref, first, C, *got, FILL)["all"] <= 1.0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_planted_scene_is_segmented_purely_and_repaired_by_both_votes(seed):
    s = smooth_ref.planted_scene(seed)
    H, W, C = s["H"], s["W"], s["C"]
    raw = 1 + np.argmax(s["probs"][:, 1:], axis=1)
    assert abs(R.oa(raw, s["truth"]) - 0.75) < 1e-12
    seg, centres, cnt = R.fit_ref(s["guide"], s["scale"], 8, 0.1, 10)
    assert cnt.size == 30 and cnt.min() > 0 and R.purity(seg, s["truth"]) == 1.0
    for mode in (0, 1):
        ref = R.vote_ref(s["probs"], H * W, C, 1, None, seg, 8, mode, 0)
        assert R.oa(ref["label"][seg.reshape(-1)], s["truth"]) == 1.0
    rigid = R.fit_ref(s["guide"], s["scale"], 8, 10.0, 10)[0]
    ref = R.vote_ref(s["probs"], H * W, C, 1, None, rigid, 8, 0, 0)
    assert R.oa(ref["label"][rigid.reshape(-1)], s["truth"]) < 0.95
    print(f"planted scene seed {seed}: OA raw {R.oa(raw, s['truth']):.4f}, superpixels 1.0 (purity 1.0, 30 segments), near-rigid grid "
          f"(compactness 10) {R.oa(ref['label'][rigid.reshape(-1)], s['truth']):.4f}")


def test_abi_struct_mirror_refusals_and_exports():
    import hsimae_amd
    from hsimae_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert R.header_fields(hdr, "hsimae_slic_params") == [(n, t) for n, t in _lib.SlicParams._fields_]
    assert R.header_fields(hdr, "hsimae_segment_vote_params") == [(n, t) for n, t in _lib.SegmentVoteParams._fields_]
    assert "hsimae_slic" in _lib.SYMBOLS and "hsimae_segment_vote" in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 108 and lib.hsimae_version() == 108
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    assert "slic" in build.UNITS and build.UNITS.index("slic") < build.UNITS.index("api")
    src = open(os.path.join(build.CSRC, "slic.hip")).read()
    body = src.split("#include")[-1]
    assert '#include "row_wave.h"' in src and "atomic" not in body and "arg_better(" in body and "write_maps(" in body
    assert body.count("slic_nearest(") == 2                    # one definition, one call: the round and the final assign share it
    for name in ("Superpixels", "SceneSegments", "scene_segments", "segment_classification"):
        assert callable(getattr(hsimae_amd, name))
    for fn in (hsimae_amd.test_model_scene, hsimae_amd.knn_eval_scene, hsimae_amd.linear_probe_scene):
        assert inspect.signature(fn).parameters["smooth"].default is None


def test_superpixels_refuse_what_they_cannot_serve():
    from hsimae_amd import EdgeFilter, SceneSegments, Superpixels, segment_classification
    from hsimae_amd.finetune import SceneClassification
    from hsimae_amd.segment import spatial_step_of
    for kw in (dict(size=1), dict(size=33), dict(size=8.0), dict(size=True), dict(compactness=0.0), dict(compactness=-1.0),
               dict(compactness=float("nan")), dict(compactness=float("inf")), dict(compactness=1e30), dict(compactness="0.1"),
               dict(max_iter=-1), dict(max_iter=2.5), dict(max_iter=True)):
        with pytest.raises(ValueError):
            Superpixels(**kw)
    sp = Superpixels()
    assert (sp.size, sp.compactness, sp.max_iter) == (8, 0.1, 10) and sp.w == R.weight(0.1, 8)
    assert spatial_step_of(None) is None and spatial_step_of(sp) is sp and isinstance(spatial_step_of(True), EdgeFilter)
    f = EdgeFilter(radius=2)
    assert spatial_step_of(f) is f
    for bad in (3, "yes", 1.0):
        with pytest.raises(TypeError):
            spatial_step_of(bad)
    segs = SceneSegments(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(1, 3), torch.full((1,), 6, dtype=torch.int32), (1, 1), 8)
    assert segs.check() is segs
    with pytest.raises(ValueError, match="counts"):
        segs._replace(counts=torch.full((1,), 5, dtype=torch.int32)).check()
    with pytest.raises(ValueError, match="home cell"):
        SceneSegments(torch.full((9, 3), 2, dtype=torch.int32), torch.zeros(3, 3), torch.tensor([0, 0, 27], dtype=torch.int32), (3, 1), 3).check()
    res = SceneClassification(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3), torch.zeros(2, 3), None)
    with pytest.raises(ValueError, match="return_probs=True"):
        segment_classification(res, segs)
    with pytest.raises(TypeError):
        segment_classification(res, torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        segment_classification(res._replace(probs=torch.zeros(6, 4)), segs)
    with pytest.raises(ValueError, match="mode"):
        segment_classification(res._replace(probs=torch.zeros(6, 4)), segs, mode="median")
