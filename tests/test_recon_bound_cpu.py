"""csrc/recon.hip without a GPU: the restatement (tests/recon_ref.py) against an independent np.add.at / arccos formulation in
fp64, the kernels' own sequence inside the derived bounds, the bounds and the bit-equality against planted faults, the window
grid, and the two new entry points under ABI 108 (struct mirrors, refusal codes)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recon_ref as R  # noqa: E402
from knn_ref import header_fields  # noqa: E402

SHAPES = [(9, 9, 8, 9), (5, 3, 8, 9), (13, 10, 16, 9), (20, 23, 24, 4)]


def replay(H, W, C, stride, seed=0, chunk=None, fault=None, passes=1):
    scene, rows, cols, pred, mask = R.make_windows(H, W, C, stride, seed)
    acc, cnt = np.zeros((H, W, C), np.float32), np.zeros((H, W, C), np.int32)
    n = pred.shape[0]
    chunk = chunk or n
    for _ in range(passes):
        for w0 in range(0, n, chunk):
            R.accumulate(pred[w0:w0 + chunk], mask[w0:w0 + chunk], rows, cols, w0, H, W, acc, cnt, fault)
    return scene, rows, cols, pred, mask, acc, cnt


@pytest.mark.parametrize("shape", SHAPES)
def test_accumulate_equals_add_at_in_fp64(shape):
    """One np.add.at over the list of (voxel, value) pairs of every un-reflected, masked position, in fp64: the fp32 replay is
    within the rounding of its own additions, the counts are equal, and no planted NaN surfaces."""
    H, W, C, stride = shape
    scene, rows, cols, pred, mask, acc, cnt = replay(*shape, chunk=3)
    w, b, i, j = np.nonzero(mask)
    r = rows[w // len(cols)].astype(np.int64) - 4 + i
    c = cols[w % len(cols)].astype(np.int64) - 4 + j
    ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    flat = ((r * W + c) * C + b)[ok]
    s64, k64 = np.zeros(H * W * C), np.zeros(H * W * C, np.int64)
    np.add.at(s64, flat, pred[w, b, i, j][ok].astype(np.float64))
    np.add.at(k64, flat, 1)
    assert np.isfinite(acc).all() and np.array_equal(cnt.reshape(-1), k64)
    assert np.all(np.abs(acc.reshape(-1) - s64) <= k64 * 2.0 ** -24 * np.abs(s64) * 1.01)
    assert (cnt.max() > 1) == (len(rows) * len(cols) > 1)
    # the chunking does not matter, and a second pass doubles the counts
    assert np.array_equal(acc, replay(*shape)[5])
    assert np.array_equal(replay(*shape, passes=2)[6], 2 * cnt)


def test_finish_equals_arccos_formulation_where_it_is_well_conditioned():
    scene, acc, cnt, special = R.make_sums(11, 7, 24, 3)
    ref = R.finish(scene, acc, cnt)
    x = scene.astype(np.float32).astype(np.float64)
    on = cnt > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(on, (acc / cnt.astype(np.float32)).astype(np.float64), x)
    assert np.array_equal(ref["recon"].astype(np.float64), r) and np.array_equal(ref["cover"], on.sum(axis=2))
    ordinary = np.ones(11 * 7, bool)
    ordinary[list(special.values())] = False
    for px in np.flatnonzero(ordinary):
        s = on.reshape(-1, 24)[px]
        rv, xv = r.reshape(-1, 24)[px][s], x.reshape(-1, 24)[px][s]
        if not s.any():
            continue
        want_rmse = np.sqrt(np.mean((rv - xv) ** 2))
        want_sam = np.arccos(rv @ xv / (np.linalg.norm(rv) * np.linalg.norm(xv)))
        assert abs(ref["rmse"].reshape(-1)[px] - want_rmse) <= 1e-12
        assert abs(ref["sam"].reshape(-1)[px] - want_sam) <= 1e-12 / max(np.sin(want_sam), 1e-3), (px, want_sam)
    flat = {k: v.reshape(-1) for k, v in ref.items() if k in ("rmse", "sam", "cover")}
    assert flat["cover"][special["empty"]] == 0 and flat["rmse"][special["empty"]] == 0 and flat["sam"][special["empty"]] == 0
    assert flat["sam"][special["both_zero"]] == 0 and flat["rmse"][special["both_zero"]] == 0
    assert flat["sam"][special["one_zero"]] == np.pi / 2
    assert flat["sam"][special["same"]] == 0 and flat["rmse"][special["same"]] == 0 and flat["cover"][special["same"]] == 23
    assert 0 < flat["sam"][special["near"]] < 1e-6
    have = ref["cover"] > 0
    assert ref["stats"][1] == on.sum() and ref["stats"][3] == have.sum()


def ratios(got, ref):
    out = {}
    for k in ("rmse", "sam"):
        out[k] = float(np.max(np.abs(got[k].astype(np.float64) - ref[k]) / ref["b_" + k]))
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = np.abs(got["stats"] - ref["stats"]) / ref["b_stats"]
    out["stats"] = float(np.max(np.where(ref["b_stats"] > 0, rs, np.where(got["stats"] == ref["stats"], 0.0, np.inf))))
    return out


@pytest.mark.parametrize("shape", [(11, 7, 24, 3), (12, 12, 200, 5), (70, 61, 8, 7)])
def test_emulated_kernel_sequence_stays_inside_the_bound(shape):
    H, W, C, seed = shape
    scene, acc, cnt, _ = R.make_sums(H, W, C, seed)
    ref, emu = R.finish(scene, acc, cnt), R.finish_emulated(scene, acc, cnt)
    assert np.array_equal(emu["recon"], ref["recon"]) and np.array_equal(emu["cover"], ref["cover"])
    worst = ratios(emu, ref)
    print(shape, {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) < 1.0


@pytest.mark.parametrize("fault", ["reflected", "multiply", "descending", "no_increment"])
def test_bit_equality_rejects_planted_accumulate_faults(fault):
    good = replay(20, 23, 24, 4, chunk=7)
    bad = replay(20, 23, 24, 4, chunk=7, fault=fault)
    same = np.array_equal(good[5], bad[5], equal_nan=True) and np.array_equal(good[6], bad[6])
    assert not same
    if fault in ("reflected", "multiply"):                 # the planted NaN surfaces
        assert np.isnan(bad[5]).any() and not np.isnan(good[5]).any()
    if fault == "reflected":                               # and on a scene smaller than the pad the counts are wrong too
        assert not np.array_equal(replay(5, 3, 8, 9)[6], replay(5, 3, 8, 9, fault=fault)[6])


@pytest.mark.parametrize("fault,key", [("acos", "sam"), ("all_bands", "sam"), ("div_C", "rmse"), ("no_fill", "recon")])
def test_bound_rejects_planted_finish_faults(fault, key):
    scene, acc, cnt, _ = R.make_sums(11, 7, 24, 3)
    ref, bad = R.finish(scene, acc, cnt), R.finish(scene, acc, cnt, fault)
    if key == "recon":
        assert not np.array_equal(ref["recon"], bad["recon"])
    else:
        assert ratios(bad, ref)[key] > 10.0


def test_window_grid_covers_every_pixel_and_meets_the_unlabeled_tiles():
    from hsimae_amd import window_centres
    from hsimae_amd.scene_data import tile_origins
    for L in range(1, 31):
        for s in range(1, 10):
            c = window_centres(L, s)
            assert np.array_equal(c, R.centres(L, s)) and c.dtype == np.int32
            assert np.all(np.diff(c) > 0) and c[0] >= 0 and c[-1] <= L - 1
            covered = np.zeros(L, bool)
            for v in c:
                covered[max(0, v - 4):min(L, v + 5)] = True
            assert covered.all(), (L, s)
        if L >= 9:
            whole = L // 9
            assert np.array_equal(window_centres(L, 9)[:whole], tile_origins(L)[:whole] + 4)
    for bad in (0, 10):
        with pytest.raises(ValueError):
            window_centres(12, bad)


def refusals(lib, _lib):
    E_DIMS, E_ALIGN, E_NULL = -1, -3, -4
    out = []

    def run(fn, struct, ok, table):
        out.append((fn + " params NULL", getattr(lib, fn)(None, None), E_NULL))
        for kw, want in table:
            a = dict(ok)
            a.update(kw)
            out.append((fn + " " + str(kw), getattr(lib, fn)(ctypes.byref(struct(**a)), None), want))

    run("hsimae_recon_accumulate", _lib.ReconAccumulateParams,
        dict(pred_img=1 << 20, mask_img=1 << 21, n=3, w0=1, rows=1 << 22, nrows=2, cols=1 << 23, ncols=2, H=13, W=10, C=8,
             sum=1 << 24, cnt=1 << 25),
        [(dict(n=-1), E_DIMS), (dict(w0=-1), E_DIMS), (dict(H=0), E_DIMS), (dict(W=0), E_DIMS), (dict(C=0), E_DIMS),
         (dict(nrows=0), E_DIMS), (dict(ncols=0), E_DIMS), (dict(nrows=14), E_DIMS), (dict(ncols=11), E_DIMS),
         (dict(w0=2), E_DIMS), (dict(n=4), E_DIMS),
         (dict(pred_img=None), E_NULL), (dict(mask_img=None), E_NULL), (dict(rows=None), E_NULL), (dict(cols=None), E_NULL),
         (dict(sum=None), E_NULL), (dict(cnt=None), E_NULL),
         (dict(pred_img=(1 << 20) + 2), E_ALIGN), (dict(mask_img=(1 << 21) + 1), E_ALIGN), (dict(rows=(1 << 22) + 2), E_ALIGN),
         (dict(cols=(1 << 23) + 1), E_ALIGN), (dict(sum=(1 << 24) + 2), E_ALIGN), (dict(cnt=(1 << 25) + 3), E_ALIGN),
         (dict(n=0), 0), (dict(n=0, pred_img=None, mask_img=None, rows=None, cols=None, sum=None, cnt=None), 0)])
    run("hsimae_recon_finish", _lib.ReconFinishParams,
        dict(scene=1 << 20, scene_f64=1, H=13, W=10, C=8, sum=1 << 21, cnt=1 << 22, recon=1 << 23, cover=1 << 24, rmse=1 << 25,
             sam=1 << 26, partials=1 << 27, stats=1 << 28),
        [(dict(H=0), E_DIMS), (dict(W=-1), E_DIMS), (dict(C=0), E_DIMS),
         (dict(scene=None), E_NULL), (dict(sum=None), E_NULL), (dict(cnt=None), E_NULL), (dict(partials=None), E_NULL),
         (dict(stats=None), E_NULL),
         (dict(scene=(1 << 20) + 4), E_ALIGN), (dict(scene=(1 << 20) + 2, scene_f64=0), E_ALIGN), (dict(sum=(1 << 21) + 2), E_ALIGN),
         (dict(cnt=(1 << 22) + 1), E_ALIGN), (dict(recon=(1 << 23) + 2), E_ALIGN), (dict(cover=(1 << 24) + 2), E_ALIGN),
         (dict(rmse=(1 << 25) + 1), E_ALIGN), (dict(sam=(1 << 26) + 3), E_ALIGN), (dict(partials=(1 << 27) + 4), E_ALIGN),
         (dict(stats=(1 << 28) + 4), E_ALIGN)])
    return out


def test_library_exports_the_recon_entry_points_under_abi_108():
    import hsimae_amd
    from hsimae_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    declared = set(re.findall(r"\b(hsimae_[a-z0-9_]+)\s*\(", hdr)) - {"hsimae_bucket_cb"}
    assert declared == set(_lib.SYMBOLS.keys())
    for name, struct in (("hsimae_recon_accumulate", _lib.ReconAccumulateParams), ("hsimae_recon_finish", _lib.ReconFinishParams)):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
        assert header_fields(hdr, name + "_params") == [(n, t) for n, t in struct._fields_], name
    assert int(re.search(r"#define HSIMAE_RECON_GRID (\d+)", hdr).group(1)) == _lib.RECON_GRID == R.GRID
    for what, got, want in refusals(lib, _lib):
        assert got == want, (what, got, want)
    assert "recon" in build.UNITS
    assert callable(hsimae_amd.reconstruct_scene) and callable(hsimae_amd.recon_eval_scene)
    assert hsimae_amd.SceneReconstruction._fields == ("recon", "count", "cover", "rmse", "sam", "loss", "mse", "psnr", "mean_sam",
                                                      "coverage")


def test_reconstruct_scene_refuses_what_it_cannot_serve():
    import torch
    import hsimae_amd
    from hsimae_amd import reconstruct_scene
    m = hsimae_amd.HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=16, b_patch_size=8, embed_dim=64, depth=2, num_heads=4,
                          s_depth=1, decoder_embed_dim=48, decoder_depth=1, decoder_num_heads=6)
    scene = np.zeros((12, 12, 16), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reconstruct_scene(m, scene)
    for kw in (dict(passes=0), dict(stride=0), dict(stride=10), dict(mask_ratio=1.0), dict(batch_size=0)):
        with pytest.raises(ValueError):
            reconstruct_scene(m, scene, **kw)
    for bad in (np.zeros((12, 12), np.float32), np.zeros((12, 12, 8), np.float32), np.zeros((12, 12, 16), np.int32)):
        with pytest.raises(ValueError):
            reconstruct_scene(m, bad)
    assert m.want_recons is True
    v = hsimae_amd.HSIViT(img_size=9, patch_size=3, in_chans=1, bands=16, b_patch_size=8, num_class=5, embed_dim=64, depth=2,
                          num_heads=4, s_depth=1)
    with pytest.raises(ValueError, match="decoder"):
        reconstruct_scene(v, torch.zeros(12, 12, 16))
