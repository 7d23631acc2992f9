"""csrc/prob.hip without a GPU: the fp64 restatement (tests/prob_ref.py) against torch's fp64 softmax averaged over the views,
the kernel's sequence in exactly rounded fp32 inside the bound, the bound against planted faults, the share of rows the label
rule leaves open, the new entry point under ABI 108, classify_scene's `views`, the colour maps and the PNG writer."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prob_ref as R  # noqa: E402

CPU_CASES = [c for c in R.cases() if c[0] <= 512]             # the 8193-row shape: only in the open-share test (no emulation)


def case_id(c):
    return "x".join(map(str, c[:3])) + f"-first{c[3]}-v{c[4]}"


@pytest.mark.parametrize("case", CPU_CASES, ids=case_id)
def test_restatement_equals_torch_fp64_and_the_fp32_sequence_lies_inside_the_bound(case):
    N, Cc, ld, first, V = case
    z = R.make_case(*case)
    ref = R.prob_ref(z, Cc, first)
    zt = torch.from_numpy(z[:, :, first:Cc].copy())
    want = torch.softmax(zt, dim=2, dtype=torch.float64).mean(0).numpy()
    finite = ~np.isnan(want).any(1)
    assert finite.sum() >= N - 1                                # only the planted NaN row
    assert np.allclose(ref["mean"][finite][:, first:], want[finite], rtol=0, atol=1e-12)
    assert np.isnan(ref["mean"][~finite][:, first:]).all() and np.all(ref["mean"][:, :first] == 0)
    assert np.allclose(ref["mean"][finite].sum(1), 1.0, rtol=0, atol=1e-12)
    if V == 1:
        assert np.array_equal(ref["label"], first + torch.argmax(zt[0], 1).numpy())
    else:
        assert np.array_equal(ref["label"][finite], first + np.argmax(want[finite], 1))
    rows = np.arange(N)
    assert np.array_equal(ref["conf"][finite], ref["mean"][rows, ref["label"]][finite])
    if Cc - first > 1:
        top2 = np.sort(want[finite], 1)[:, -2:]
        assert np.allclose(ref["margin"][finite], top2[:, 1] - top2[:, 0], rtol=0, atol=1e-12)
    else:
        assert np.array_equal(ref["margin"], ref["conf"])
    if N >= R.PLANTED:                                          # the tied row: the lowest of the three tied classes
        tied = np.flatnonzero(z[0, 1, :Cc] == np.nanmax(z[0, 1, first:Cc]))
        assert ref["label"][1] == tied[tied >= first].min()
    w = R.worst(R.emulate(z, Cc, first), z, Cc, first, ref)
    print(f"{case_id(case)}: exactly rounded fp32 err / bound: mean {w['mean']:.3f}, conf {w['conf']:.3f}, margin {w['margin']:.3f}; "
          f"open {w['open']:.5f}")
    assert w["wrong"] == 0 and w["zeros"] and w["all"] <= 1.0


@pytest.mark.parametrize("fault", R.FAULTS)
def test_bound_rejects_planted_faults(fault):
    N, Cc, ld, first, V = 65, 33, 48, 1, 3
    z = R.make_case(N, Cc, ld, first, V)
    z[:, 5, 0] = 100.0                                         # class 0, below `first`, is the overall maximum of a row
    if fault == "pad_column":
        z[:, :, Cc:] = 4.0                                      # a finite pad: the fault must show without the NaN canary too
    ref = R.prob_ref(z, Cc, first)
    clean = R.worst(R.emulate(z, Cc, first), z, Cc, first, ref)
    assert clean["all"] <= 1.0                                  # the harness itself is clean
    w = R.worst(R.emulate(z, Cc, first, fault), z, Cc, first, ref)
    print(f"{fault}: worst err / bound = {w['all']:.3g} (wrong labels {w['wrong']})")
    assert w["all"] > 10.0, w


def test_label_rule_leaves_out_at_most_a_thousandth_of_the_rows():
    worst, total = 0.0, 0
    for case in R.cases():
        N, Cc, ld, first, V = case
        ref = R.prob_ref(R.make_case(*case), Cc, first)
        free = np.ones(N, bool)
        free[:R.PLANTED if N >= R.PLANTED else 0] = False
        share = float((~ref["decided"] & free).sum()) / max(1, int(free.sum()))
        worst, total = max(worst, share), total + int(free.sum())
        assert share <= 1e-3, (case, share)
        if V == 1:
            assert ref["decided"].all()
    print(f"{total} non-planted rows, worst share left open {worst:.5f}")


def test_library_exports_class_prob_under_abi_108():
    import hsimae_amd
    from hsimae_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert "hsimae_class_prob" in _lib.SYMBOLS and lib.hsimae_class_prob is not None
    assert re.search(r"\bhsimae_class_prob\s*\(", hdr)
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    body = re.search(r"typedef struct \{([^}]*)\} hsimae_class_prob_params;", hdr).group(1)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl)            # a pointer is declared alone: `type* name`
        for name in m.group(3).split(","):
            fields.append((name.strip(), C.c_void_p if m.group(2) else ctype[m.group(1)]))
    assert fields == [(n, t) for n, t in _lib.ClassProbParams._fields_]
    assert callable(hsimae_amd.DualViT.classify_scene) and callable(hsimae_amd.HSIViT.classify_scene)
    for rc in R.refusals(lib, _lib):
        assert rc[1] == rc[2], rc


def test_views_are_validated():
    from hsimae_amd.finetune import scene_views
    assert scene_views((0,)) == (0,) and scene_views("flips") == (0, 1, 2, 3) and scene_views([3, 0]) == (3, 0)
    assert scene_views(np.array([1, 2])) == (1, 2)
    for bad in ("all", "", (), (0, 0), (4,), (-1,), (0, 1.5), (True,), 2, None, ("0",)):
        with pytest.raises(ValueError):
            scene_views(bad)


def test_label_to_colormap_equals_the_reference_fixture():
    from hsimae_amd import label_to_colormap
    fx = np.load(os.path.join(ROOT, "tests", "golden", "colormap.npz"))
    assert fx["label"].shape == (1, 20) and fx["colors"].shape == (1, 20, 3) and fx["colors"].dtype == np.uint8
    got = label_to_colormap(fx["label"])
    assert got.dtype == np.uint8 and np.array_equal(got, fx["colors"])
    lab = np.random.RandomState(0).randint(0, 20, (7, 5))
    assert np.array_equal(label_to_colormap(torch.from_numpy(lab)), fx["colors"][0][lab])
    assert np.array_equal(label_to_colormap(lab.astype(np.int32)), fx["colors"][0][lab])
    with pytest.raises(ValueError, match="20"):
        label_to_colormap(np.array([[0, 20]]))
    with pytest.raises(ValueError):
        label_to_colormap(np.array([[0, -1]]))
    with pytest.raises(ValueError):
        label_to_colormap(np.zeros((2, 2), np.float32))
    pal = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    assert np.array_equal(label_to_colormap(np.array([[1, 0]]), pal), pal[[1, 0]][None])
    with pytest.raises(ValueError):
        label_to_colormap(np.array([[2]]), pal)


def test_png_round_trip(tmp_path):
    from hsimae_amd import label_to_colormap, save_label_png
    lab = np.random.RandomState(1).randint(0, 20, (23, 19))
    path = tmp_path / "map.png"
    save_label_png(path, lab)
    assert np.array_equal(R.decode_png(path.read_bytes()), label_to_colormap(lab))
    save_label_png(str(path), torch.from_numpy(lab[:1, :1]))                     # a single pixel, a tensor, a str path
    assert np.array_equal(R.decode_png(path.read_bytes()), label_to_colormap(lab[:1, :1]))
