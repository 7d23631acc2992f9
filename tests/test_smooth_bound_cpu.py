"""tests/smooth_ref.py without a GPU: the fp64 restatement of csrc/smooth.hip against an independently written per-pixel loop and
against a box mean, the emulated fp32 sequence inside its bounds at the GPU test's shapes, planted faults rejected by the checks,
the share of pixels the label rule leaves open, the planted scene, the ABI, and EdgeFilter's argument refusals."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_ref as R  # noqa: E402


def pixel_loop(probs, C, first, H, W, row_of, guide, scale, radius, a_s, a_r):
    """The filter written pixel by pixel and tap by tap in Python floats (fp64), sharing nothing with filter_ref -> [H W, C]."""
    out = np.zeros((H * W, C))
    n = probs.shape[0]

    def row(y, x):
        if not (0 <= y < H and 0 <= x < W):
            return -1
        k = y * W + x if row_of is None else int(row_of[y * W + x])
        return k if 0 <= k < n else -1

    for y in range(H):
        for x in range(W):
            if row(y, x) < 0:
                continue
            acc, wsum = [0.0] * C, 0.0
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    k = row(y + dy, x + dx)
                    if k < 0:
                        continue
                    e = a_s * (dy * dy + dx * dx)
                    if a_r != 0:
                        e += a_r * sum(((float(guide[y + dy, x + dx, g]) - float(guide[y, x, g])) * float(scale[g])) ** 2
                                       for g in range(guide.shape[2]))
                    w = 2.0 ** -e
                    wsum += w
                    for c in range(first, C):
                        acc[c] += w * float(probs[k, c])
            out[y * W + x] = [a / wsum for a in acc]
    return out


@pytest.mark.parametrize("c", [R.CASES[i] for i in (0, 3, 5, 6, 8, 18)], ids=R.case_id)
def test_restatement_equals_a_per_pixel_double_loop(c):
    H, W, radius, C, first, G, form = c
    case = R.make_case(*c)
    ref = R.case_ref(c, case)
    want = pixel_loop(case["probs"], C, first, H, W, case["row_of"], case["guide"], case["scale"], radius, case["a_s"], case["a_r"])
    assert np.abs(ref["out"] - want).max() <= 1e-12
    assert ref["has"].sum() > 0 and not ref["out"][~ref["has"]].any() and np.all(ref["out"][:, :first] == 0)
    assert np.allclose(ref["out"][ref["has"]].sum(1), 1.0, atol=1e-6)          # a weighted mean of probability rows


def test_without_range_term_and_a_wide_gaussian_it_is_the_box_mean_over_the_taps_in_the_scene():
    H, W, C, first, r = 9, 13, 5, 1, 2
    rng = np.random.RandomState(3)
    probs = rng.rand(H * W, C).astype(np.float32)
    ref = R.filter_ref(probs, C, first, H, W, None, None, None, r, R.coef(1e9), 0.0)
    P = probs.astype(np.float64).reshape(H, W, C)
    for y in range(H):
        for x in range(W):
            box = P[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1, first:].reshape(-1, C - first)
            assert np.abs(ref["out"][y * W + x, first:] - box.mean(0)).max() <= 1e-12
            assert ref["taps"][y * W + x] == box.shape[0]


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_emulated_fp32_sequence_stays_inside_the_bounds_and_few_labels_stay_open(c):
    H, W, radius, C, first, G, form = c
    case = R.make_case(*c)
    ref = R.case_ref(c, case)
    got = R.emulate(case["probs"], C, first, H, W, case["row_of"], case["guide"], case["scale"], radius, case["a_s"], case["a_r"])
    w = R.worst(got, ref, first)
    print(f"{R.case_id(c)}: err / bound: out {w['out']:.3f}, conf {w['conf']:.3f}, margin {w['margin']:.3f}; labels wrong "
          f"{w['wrong']}, share left open {w['open']:.5f}")
    assert w["zeros"] and w["wrong"] == 0
    assert w["out"] <= 1.0 and w["conf"] <= 1.0 and w["margin"] <= 1.0
    assert w["open"] <= 0.02
    assert np.all(ref["taps"][ref["has"]] >= 1) and ref["taps"].max() <= (2 * radius + 1) ** 2


FAULT_CASES = {"reflect": (17, 33, 3, 18, 1, 4, "subset"), "divide_by_count": (15, 17, 3, 16, 1, 1, "subset"),
               "unsquared": (15, 17, 3, 16, 1, 1, "subset"), "rowless_counted": (17, 33, 3, 18, 1, 4, "subset"),
               "scale_ignored": (16, 16, 3, 17, 1, 3, "padded"), "swap_dydx": (17, 33, 3, 18, 1, 4, "subset"),
               "runner_up_with_winner": (15, 17, 3, 16, 1, 1, "subset")}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_a_planted_fault_leaves_the_bounds(fault):
    c = FAULT_CASES[fault]
    assert c in R.CASES and (fault != "swap_dydx" or c[0] != c[1])                 # (a square scene would hide the swap)
    H, W, radius, C, first, G, form = c
    case = R.make_case(*c)
    ref = R.case_ref(c, case)
    a = (case["probs"], C, first, H, W, case["row_of"], case["guide"], case["scale"], radius, case["a_s"], case["a_r"])
    assert R.worst(R.emulate(*a), ref, first)["all"] <= 1.0
    assert R.worst(R.emulate(*a, fault=fault), ref, first)["all"] > 1.0, fault


def test_the_planted_scene_is_repaired_by_the_guided_filter_only():
    s = R.planted_scene()
    H, W, C, first = s["H"], s["W"], s["C"], s["first"]
    raw = first + np.argmax(s["probs"][:, first:], axis=1)
    assert R.oa(raw, s["truth"]) < 0.8
    guided = R.filter_ref(s["probs"], C, first, H, W, None, s["guide"], s["scale"], 3, R.coef(3.0), R.coef(0.1))
    assert R.oa(guided["label"], s["truth"]) == 1.0
    assert guided["decided"].all() and guided["gap"].min() > 0.05 > 1e3 * guided["bound"].max()
    plain = R.filter_ref(s["probs"], C, first, H, W, None, None, None, 3, R.coef(3.0), 0.0)
    assert R.oa(plain["label"], s["truth"]) < 1.0
    print(f"planted scene: OA raw {R.oa(raw, s['truth']):.4f}, guided {R.oa(guided['label'], s['truth']):.4f} (smallest top-two gap "
          f"{guided['gap'].min():.4f}, largest bound {guided['bound'].max():.2e}), unguided {R.oa(plain['label'], s['truth']):.4f}")
    got = R.emulate(s["probs"], C, first, H, W, None, s["guide"], s["scale"], 3, R.coef(3.0), R.coef(0.1))
    assert R.oa(got[1], s["truth"]) == 1.0


def test_the_lane_to_pixel_map_keeps_every_tap_read_free_of_bank_conflicts():
    """csrc/smooth.hip, "LDS banks", restated: plane row stride SP and tile-row pairing k per radius, the lane -> pixel map, and
    ds_read_b32's banking (two groups of 32 lanes, bank = word address mod 32): at every radius the 32 lanes of a group read 32
    different banks of a class-major plane, every pixel of the tile has one lane, and a pixel-major slab would be a 16-way conflict."""
    for r in range(1, 9):
        S = 16 + 2 * r
        SP = 34 if S == 32 else S
        ks = next(k for k in (3, 2, 1) if (SP << k) % 32 == 16)
        pix = []
        for tid in range(256):
            x, q = tid & 15, tid >> 4
            t = q >> 1
            y = ((t >> ks) << (ks + 1)) | ((q & 1) << ks) | (t & ((1 << ks) - 1))
            pix.append((y, x))
        assert sorted(pix) == [(y, x) for y in range(16) for x in range(16)]
        for g in range(8):
            lanes = pix[32 * g:32 * g + 32]
            for dy, dx in ((-r, -r), (0, 0), (r, r), (-r, r)):
                assert len({((y + r + dy) * SP + x + r + dx) % 32 for y, x in lanes}) == 32, (r, g)
            assert len({(((y + r) * SP + x + r) * 16) % 32 for y, x in lanes}) == 2                # [pixel][16 classes]
        assert SP * S * (1 + 4 + 16) * 4 <= 91392                                                  # what the launcher opts in to


def test_abi_struct_mirror_refusals_and_exports():
    import hsimae_amd
    from hsimae_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert R.header_fields(hdr, "hsimae_prob_filter_params") == [(n, t) for n, t in _lib.ProbFilterParams._fields_]
    assert "hsimae_prob_filter" in _lib.SYMBOLS and _lib.ABI_VERSION == 108 and lib.hsimae_version() == 108
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    assert "smooth" in build.UNITS and build.UNITS.index("smooth") < build.UNITS.index("api")
    src = open(os.path.join(build.CSRC, "smooth.hip")).read()
    body = src.split("#include")[-1]
    assert '#include "row_wave.h"' in src and "atomic" not in body and "arg_better(" in body and "write_maps(" in body
    for name in ("EdgeFilter", "scene_guide", "as_guide", "smooth_classification"):
        assert callable(getattr(hsimae_amd, name))
    import inspect
    for fn in (hsimae_amd.test_model_scene, hsimae_amd.knn_eval_scene, hsimae_amd.linear_probe_scene):
        assert inspect.signature(fn).parameters["smooth"].default is None
    assert "smooth" not in inspect.signature(hsimae_amd.cluster_eval_scene).parameters


def test_edge_filter_refuses_what_it_cannot_serve():
    from hsimae_amd import EdgeFilter, scene_guide, smooth_classification
    from hsimae_amd.finetune import SceneClassification
    from hsimae_amd.smooth import edge_filter_of
    for kw in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(sigma_s=0.0), dict(sigma_s=-1.0),
               dict(sigma_s=float("nan")), dict(sigma_s=float("inf")), dict(sigma_s=None), dict(sigma_r=0.0), dict(sigma_r=-0.2),
               dict(sigma_r=float("nan")), dict(sigma_r=1e-30), dict(sigma_s="3")):
        with pytest.raises(ValueError):
            EdgeFilter(**kw)
    f = EdgeFilter()
    assert (f.radius, f.sigma_s, f.sigma_r) == (3, 3.0, 0.2)                       # Kang et al.'s EPF-B settings
    assert f.a_s == R.coef(3.0) and f.a_r == R.coef(0.2) and EdgeFilter(sigma_r=None).a_r == 0.0
    assert f.a_s == float(np.float32(math.log2(math.e) / 18.0))
    assert edge_filter_of(None) is None and edge_filter_of(f) is f and edge_filter_of(True).radius == 3
    with pytest.raises(TypeError):
        edge_filter_of(3)
    with pytest.raises(ValueError, match="GPU"):
        f.apply(torch.zeros(6, 4), 2, 3, None)
    res = SceneClassification(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3), torch.zeros(2, 3), None)
    with pytest.raises(ValueError, match="return_probs=True"):
        smooth_classification(res, None)
    with pytest.raises(TypeError):
        smooth_classification(res, None, filt="bilateral")
    with pytest.raises(ValueError, match="explicit guide"):
        scene_guide(np.zeros((4, 4, 129), np.float32))
    for ch in (0, 5, 1.0, True):
        with pytest.raises(ValueError):
            scene_guide(np.zeros((4, 4, 8), np.float32), channels=ch)
