"""Group-wise PCA on the GPU (hsimae_gwpca_fit / hsimae_gwpca_apply, hsimae_amd.GWPCA): the reference's record and the fp64
restatement within the derived per-component bound (tests/gwpca_ref.py), a Pavia-sized scene, the whitening invariants,
bit-reproducibility, canaries, the fp32 output and input paths, edge shapes, degenerate input, every refusal code, and
predict_scene fed by fit_transform.  Every test runs under its own time limit; nothing here provokes a fault."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gwpca_ref as R  # noqa: E402
from test_gwpca_cpu import FX, TAGS, check_whitened, scene  # noqa: E402

pytestmark = pytest.mark.gpu
TIME_LIMIT = 300          # seconds per test: a GPU step that does not return ends the process instead of hanging the run


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def fit_transform(raw, nc=32, group=4, whiten=True, dtype=torch.float64):
    from hsimae_amd import GWPCA
    pca = GWPCA(nc=nc, group=group, whiten=whiten)
    return pca, pca.fit_transform(raw, dtype=dtype)


def compare(tag, pca, out, ref, extra=None, mask=None):
    """Per-component comparison against the restatement (bound) and optionally a record (bound + `extra`); prints the worst
    err / bound.  -> worst ratio against the restatement."""
    got = out.cpu().numpy()
    err = R.component_err(got, ref["out"])
    ratio = err / ref["bound"]
    if mask is not None:
        ratio = ratio[mask]
    print(f"{tag}: worst err / bound vs restatement {ratio.max():.3f} (err up to {err.max():.2e})")
    assert np.all(ratio <= 1.0), ratio.max()
    assert pca.min_.item() == ref["min"] and pca.max_.item() == ref["max"]                      # bit-exact
    merr = np.abs(pca.mean_.cpu().numpy() - ref["mean"]).max()
    lerr = np.abs(pca.explained_variance_.cpu().numpy() - ref["lam"]) / ref["lam_bound"]
    print(f"{tag}: mean err / bound {merr / ref['mean_bound']:.3f}, eigenvalue err / bound {lerr.max():.3f}")
    assert merr <= ref["mean_bound"] and np.all(lerr <= 1.0)
    return float(ratio.max())


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_scenes_match_the_reference_record_and_the_restatement(tag):
    raw, nc, group, whiten = scene(tag)
    ref = R.gwpca_ref(raw.astype(np.float64), nc, group, whiten)
    pca, out = fit_transform(raw, nc, group, whiten)
    assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == raw.shape[:2] + (nc,)
    compare(tag, pca, out, ref)
    err = R.component_err(out.cpu().numpy(), FX[tag + "_out"])
    lim = ref["bound"] + FX[tag + "_dist"]
    print(f"{tag}: worst err / (bound + recorded distance) vs the reference record {np.max(err / lim):.3f}")
    assert np.all(err <= lim)
    if whiten:
        check_whitened(out.cpu().numpy(), ref["bound"], group)
    comps = pca.components_
    for g, (cd, cr) in enumerate(zip(comps, ref["comps"])):                                     # signed unit eigenvectors
        assert tuple(cd.shape) == cr.shape
        assert np.abs(np.abs((cd.cpu().numpy() * cr).sum(1)) - 1).max() < 1e-9 and ((cd.cpu().numpy() * cr).sum(1) > 0).all()
    assert pca.group_offsets_ == [a for a, _ in R.groups(raw.shape[2], group)] + [raw.shape[2]]


def test_pavia_sized_scene_against_the_restatement():
    from hsimae_amd import apply_gwpca
    raw = R.graded(610, 340, 103, seed=11)
    ref = R.gwpca_ref(raw)
    assert ref["gap_rel"].min() >= 0.2 and ref["lam_rel"].min() >= 1e-4
    pca, out = fit_transform(raw)
    compare("pavia", pca, out, ref)
    check_whitened(out.cpu().numpy(), ref["bound"], 4)
    _, again = fit_transform(raw)
    assert torch.equal(out, again)                                                              # two runs are bit-identical
    host = apply_gwpca(raw)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and np.array_equal(host, out.cpu().numpy())


@pytest.mark.parametrize("tag", ["A", "B", "F", "G"])
def test_two_runs_are_bit_identical_and_fp32_paths_are_exact_roundings(tag):
    raw, nc, group, whiten = scene(tag)
    pca, out = fit_transform(raw, nc, group, whiten)
    pca2, out2 = fit_transform(raw, nc, group, whiten)
    assert torch.equal(out, out2) and torch.equal(pca.mean_, pca2.mean_) and torch.equal(pca.explained_variance_, pca2.explained_variance_)
    out32 = pca.transform(raw, dtype=torch.float32)
    assert out32.dtype == torch.float32 and torch.equal(out32, out.to(torch.float32))          # round to nearest even, bit for bit
    raw32 = raw.astype(np.float32)
    _, a = fit_transform(raw32, nc, group, whiten)
    _, b = fit_transform(raw32.astype(np.float64), nc, group, whiten)
    assert torch.equal(a, b)                                                                    # an fp32 scene = the fp64 path on its widening


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("nc,group", [(32, 4), (12, 4), (6, 2)])
def test_output_sits_inside_nan_canaries(dtype, nc, group):
    """Through ctypes, into the middle of a NaN-filled buffer; (12, 4) and (6, 2) have 3 components per group: the scalar stores."""
    from hsimae_amd import GWPCA, _lib
    raw = torch.from_numpy(FX["B_raw"]).cuda()
    H, W, Cb = raw.shape
    pca = GWPCA(nc=nc, group=group).fit(raw)
    want = pca.transform(raw, dtype=dtype)
    pad = 64
    buf = torch.full((pad + H * W * nc + pad,), float("nan"), dtype=dtype, device="cuda")
    p = pca._params(raw, pca._model)
    _lib.check(_lib.load().hsimae_gwpca_apply(C.byref(p), buf.data_ptr() + pad * buf.element_size(), int(dtype == torch.float64),
                                              torch.cuda.current_stream().cuda_stream), "hsimae_gwpca_apply")
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all()
    assert torch.equal(buf[pad:-pad].view(H, W, nc), want) and not torch.isnan(want).any()


@pytest.mark.parametrize("shape,group,nc", [((1, 131, 64), 4, 32), ((131, 1, 64), 4, 32), ((37, 41, 103), 4, 32), ((30, 40, 128), 1, 8),
                                             ((30, 44, 256), 2, 16)])
def test_edge_shapes(shape, group, nc):
    """1 x n and n x 1 scenes, pixel counts that are no multiple of any tile, a group of exactly 128 bands (one and two of them)."""
    raw = R.graded(*shape, seed=21, group=group, k=max(14, nc // group + 6))
    ref = R.gwpca_ref(raw, nc, group)
    assert ref["gap_rel"].min() >= 0.2 and ref["lam_rel"].min() >= 1e-4
    pca, out = fit_transform(raw, nc, group)
    compare(str(shape), pca, out, ref)
    check_whitened(out.cpu().numpy(), ref["bound"], group)


def test_rank_deficient_scene_clips_trailing_eigenvalues():
    """n < w: 5 x 6 pixels, 204 bands (groups of 51).  At most n - 1 = 29 eigenvalues are non-zero; the rest are rounding noise of
    either sign and must come out clipped at 0.  Only the components the fixture condition covers are compared."""
    raw = R.graded(5, 6, 204, seed=3, ratio=0.4)
    ref = R.gwpca_ref(raw)
    ok = (ref["gap_rel"] >= 0.2) & (ref["lam_rel"] >= 1e-4)
    assert ok.sum() >= 24
    pca, out = fit_transform(raw)
    compare("rank-deficient", pca, out, ref, mask=ok)
    lam = pca.explained_variance_.cpu().numpy()
    assert (lam >= 0).all()
    for a, e in R.groups(204):
        assert np.all(lam[a + 29:e] <= ref["lam_bound"][a])


def test_apply_on_a_second_scene_with_the_first_scenes_fit():
    from hsimae_amd import GWPCA
    raw, raw2 = FX["A_raw"], R.graded(7, 9, 64, seed=99)
    pca = GWPCA().fit(raw)
    got = pca.transform(raw2).cpu().numpy()
    ref = R.gwpca_ref(raw)
    x2 = (raw2.reshape(-1, 64) - ref["min"]) / (ref["max"] - ref["min"])
    want = np.concatenate([(x2[:, a:e] - ref["mean"][a:e]) @ ref["comps"][g].T / R.whiten_scale(ref["lam"][a:a + 8], True)
                           for g, (a, e) in enumerate(R.groups(64))], 1).reshape(7, 9, 32)
    # the second scene's values scale every term of the bound by at most the ratio of the largest centred magnitudes
    x1 = (raw.reshape(-1, 64) - ref["min"]) / (ref["max"] - ref["min"])
    scale = max(1.0, np.abs(x2 - ref["mean"]).max() / np.abs(x1 - ref["mean"]).max())
    err = R.component_err(got, want)
    print(f"second scene: worst err / bound {np.max(err / (scale * ref['bound'])):.3f}")
    assert np.all(err <= scale * ref["bound"])
    with pytest.raises(ValueError, match="103 bands"):
        pca.transform(FX["B_raw"])


DEGENERATE = """
import sys, numpy as np, torch
sys.path.insert(0, %r)
from hsimae_amd import GWPCA
raw = np.load(%r)["A_raw"].copy()
if %r == "constant":
    raw[:] = 1234.5
else:
    raw[3, 4, 17] = np.nan
pca = GWPCA()
out = pca.fit_transform(raw)
torch.cuda.synchronize()
assert torch.isnan(out).all(), int(torch.isnan(out).sum())
print("all-nan", tuple(out.shape))
"""


@pytest.mark.parametrize("kind", ["constant", "nan"])
def test_constant_and_nan_scenes_return_all_nan(kind):
    """max == min and a NaN cannot be seen without a host wait: the output is NaN as in the reference, and the eigen-solver's
    sweep cap makes the call return.  Legal input, run in a child process under a time limit."""
    code = DEGENERATE % (ROOT, os.path.join(ROOT, "tests", "golden", "gwpca.npz"), kind)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0 and "all-nan (13, 13, 32)" in r.stdout, r.stderr[-2000:]


def test_every_refusal_code_of_the_three_entry_points():
    from hsimae_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    H, W, Cb, nc = 10, 9, 103, 32
    raw = torch.from_numpy(FX["B_raw"]).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    mm, mean, lam, proj, goff = torch.zeros(2, **f64), torch.zeros(Cb, **f64), torch.zeros(Cb, **f64), torch.zeros(Cb, 8, **f64), \
        torch.zeros(5, dtype=torch.int32, device="cuda")
    out = torch.zeros(H, W, nc, **f64)

    def params(**kw):
        a = dict(scene=raw.data_ptr(), scene_f64=1, H=H, W=W, C=Cb, nc=nc, group=4, whiten=1, minmax=mm.data_ptr(), mean=mean.data_ptr(),
                 lambda_=lam.data_ptr(), proj=proj.data_ptr(), group_off=goff.data_ptr())
        a.update(kw)
        return _lib.GwpcaParams(**a)
    nbytes = lib.hsimae_gwpca_workspace_bytes(C.byref(params()))
    assert nbytes > 0
    ws = torch.zeros(nbytes // 8, **f64)

    def all_three(p):
        return (lib.hsimae_gwpca_workspace_bytes(C.byref(p)), lib.hsimae_gwpca_fit(C.byref(p), ws.data_ptr(), st),
                lib.hsimae_gwpca_apply(C.byref(p), out.data_ptr(), 1, st))
    EDIMS, EUNSUP, EALIGN, ENULL = -1, -2, -3, -4
    for kw, code in [(dict(H=1, W=1), EDIMS), (dict(H=0), EDIMS), (dict(W=-3), EDIMS), (dict(C=0), EDIMS), (dict(nc=0), EDIMS),
                     (dict(group=3), EUNSUP), (dict(group=0), EUNSUP), (dict(group=8), EUNSUP), (dict(nc=30), EDIMS),
                     (dict(nc=104), EDIMS), (dict(H=2, W=2), EDIMS), (dict(C=516), EUNSUP), (dict(C=129, group=1, nc=8), EUNSUP)]:
        assert all_three(params(**kw)) == (code, code, code), (kw, code)
    assert lib.hsimae_gwpca_workspace_bytes(None) == ENULL
    assert lib.hsimae_gwpca_fit(None, ws.data_ptr(), st) == ENULL and lib.hsimae_gwpca_apply(None, out.data_ptr(), 1, st) == ENULL
    for field in ("scene", "minmax", "mean", "lambda_", "proj", "group_off"):
        p = params(**{field: None})
        assert lib.hsimae_gwpca_fit(C.byref(p), ws.data_ptr(), st) == ENULL and lib.hsimae_gwpca_apply(C.byref(p), out.data_ptr(), 1, st) == ENULL
    assert lib.hsimae_gwpca_fit(C.byref(params()), None, st) == ENULL
    assert lib.hsimae_gwpca_apply(C.byref(params()), None, 1, st) == ENULL
    assert lib.hsimae_gwpca_fit(C.byref(params()), ws.data_ptr() + 8, st) == EALIGN
    assert lib.hsimae_gwpca_apply(C.byref(params()), out.data_ptr() + 8, 1, st) == EALIGN       # misaligned output
    assert lib.hsimae_gwpca_apply(C.byref(params()), out.data_ptr() + 4, 0, st) == EALIGN
    assert lib.hsimae_gwpca_fit(C.byref(params(scene=raw.data_ptr() + 4)), ws.data_ptr(), st) == EALIGN
    assert lib.hsimae_gwpca_fit(C.byref(params(mean=mean.data_ptr() + 4)), ws.data_ptr(), st) == EALIGN
    torch.cuda.synchronize()
    assert not out.any() and not lam.any() and not proj.any()                                   # a refused call launches nothing
    assert all_three(params())[1:] == (0, 0)
    torch.cuda.synchronize()
    assert goff.tolist() == [0, 25, 51, 77, 103]


def test_predict_scene_fed_by_fit_transform():
    """predict_scene(GWPCA().fit_transform(raw)) against predict_scene of the restatement's fp64 scene.  Both scenes are rounded
    to fp32 inside the window kernel; they differ by about 1e-12 against an fp32 ulp of 1e-7, so a few values in ten thousand
    may round the other way and a near-tie pixel may flip.  Gate: ten times the number of labels by which the restatement
    differs from the reference record on the same scene (both computed without the device's PCA); 0 if that is 0."""
    from test_gpu_scene import tiny_hsivit
    m = tiny_hsivit()
    raw = FX["A_raw"]
    rest = R.gwpca_ref(raw)["out"]
    lab_rest = m.predict_scene(rest)
    lab_rec = m.predict_scene(FX["A_out"])
    base_vals = int((rest.astype(np.float32) != FX["A_out"].astype(np.float32)).sum())
    base_labels = int((lab_rest != lab_rec).sum())
    _, dev = fit_transform(raw)
    lab_dev = m.predict_scene(dev)
    vals = int((dev.cpu().numpy().astype(np.float32) != rest.astype(np.float32)).sum())
    labels = int((lab_dev != lab_rest).sum())
    print(f"fp32 values that differ: device vs restatement {vals}, restatement vs record {base_vals} (of {rest.size}); "
          f"labels that differ: {labels}, restatement vs record {base_labels} (of {lab_rest.numel()}); gate {10 * base_labels}")
    assert labels <= 10 * base_labels
    assert len(torch.unique(lab_rest)) > 1
