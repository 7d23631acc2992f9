"""Group-wise PCA without a GPU: the fp64 restatement (tests/gwpca_ref.py) against the reference's record
(tests/golden/gwpca.npz), the group table, the bound against planted faults, the whitening invariants, the Python argument
refusals and the library's new symbols."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gwpca_ref as R  # noqa: E402

FX = np.load(os.path.join(ROOT, "tests", "golden", "gwpca.npz"))
TAGS = ["A", "B", "C", "D", "E", "F", "G", "H"]


def scene(tag):
    raw = FX["B_raw" if tag == "H" else tag + "_raw"]
    nc, group, whiten = (int(v) for v in FX[tag + "_args"])
    return raw, nc, group, bool(whiten)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_agrees_with_the_reference_record(tag):
    raw, nc, group, whiten = scene(tag)
    ref = R.gwpca_ref(raw.astype(np.float64), nc, group, whiten)
    assert ref["gap_rel"].min() >= 0.2 and ref["lam_rel"].min() >= 1e-4            # the fixture condition, every component
    err = R.component_err(ref["out"], FX[tag + "_out"])
    lim = ref["bound"] + FX[tag + "_dist"]
    print(f"{tag}: worst err / (bound + recorded distance) {np.max(err / lim):.3f}; bound {ref['bound'].min():.1e}..{ref['bound'].max():.1e}")
    assert np.all(err <= lim), (err / lim).max()
    # another summation order of the same algorithm stays inside the bound alone
    perm = np.random.RandomState(0).permutation(raw.shape[0] * raw.shape[1])
    err2 = R.component_err(R.gwpca_ref(raw.astype(np.float64), nc, group, whiten, order=perm)["out"], ref["out"])
    assert np.all(err2 <= ref["bound"]), (err2 / ref["bound"]).max()


def test_group_table_equals_the_reference():
    from hsimae_amd.gwpca import group_offsets
    for bands, widths in zip(FX["table_bands"], FX["table_widths"]):
        assert [e - a for a, e in R.groups(int(bands), 4)] == list(widths)
        assert list(np.diff(group_offsets(int(bands), 4))) == list(widths)
    assert [e - a for a, e in R.groups(103, 4)] == [25, 26, 26, 26]
    assert group_offsets(103, 2) == [0, 51, 103] and group_offsets(103, 1) == [0, 103]


def faulty(X, nc, group, whiten, fault):
    """The restatement with one planted fault."""
    H, W, Cb = X.shape
    x, mn, mx = R.normalise(X)
    n, k = x.shape[0], nc // group
    gs = R.groups(Cb, group)
    if fault == "boundary":                                    # first group boundary off by one band
        gs = [(gs[0][0], gs[0][1] + 1), (gs[1][0] + 1, gs[1][1])] + gs[2:]
    mus = [R.centred_cov(x[:, a:e])[0] for a, e in gs]
    outs = []
    for gi, (a, e) in enumerate(gs):
        xg = x[:, a:e]
        if fault == "group_minmax":                            # normalised by the group's own range instead of the scene's
            raw = X.reshape(-1, Cb)[:, a:e].astype(np.float64)
            xg = (raw - raw.min()) / (raw.max() - raw.min())
        mu, Cm = R.centred_cov(xg, drop=slice(16, 20) if fault == "dropped_tile" else None)
        if fault == "divisor_n":
            Cm = Cm * (n - 1) / n
        lam, Vk, _ = R.eig_desc(Cm, k)
        if fault == "wrong_mean" and gi == 1:                  # the mean of another group (truncated / padded to this width)
            mu = np.resize(mus[0], e - a)
        y = (xg - mu) @ Vk.T / R.whiten_scale(lam[:k], whiten and fault != "no_whiten")
        if gi == 0 and fault == "sign":
            y[:, k - 1] = -y[:, k - 1]
        if gi == 0 and fault == "swap":
            y[:, [k - 2, k - 1]] = y[:, [k - 1, k - 2]]
        outs.append(y)
    return np.concatenate(outs, 1).reshape(H, W, nc)


FAULTS = ["dropped_tile", "divisor_n", "boundary", "sign", "swap", "no_whiten", "wrong_mean"]


# A whitened component does not change when its group is rescaled, so normalising by the group's own range is a fault that only
# the unwhitened record (H) can show; every other fault is planted in a whitened scene of either solver branch.
@pytest.mark.parametrize("tag,fault", [(t, f) for t in ("A", "B") for f in FAULTS] + [("H", "group_minmax")])
def test_bound_rejects_planted_faults(tag, fault):
    raw, nc, group, whiten = scene(tag)
    ref = R.gwpca_ref(raw, nc, group, whiten)
    assert np.all(R.component_err(faulty(raw, nc, group, whiten, None), ref["out"]) <= ref["bound"])       # the harness itself is clean
    err = R.component_err(faulty(raw, nc, group, whiten, fault), ref["out"])
    worst = np.max(err / (ref["bound"] + FX[tag + "_dist"]))
    print(f"{tag} {fault}: worst err / (bound + recorded distance) = {worst:.3g}")
    assert worst > 10.0, worst


@pytest.mark.parametrize("tag", ["A", "B", "C", "D", "E", "F", "G"])
def test_whitened_output_is_centred_with_identity_covariance(tag):
    raw, nc, group, whiten = scene(tag)
    ref = R.gwpca_ref(raw.astype(np.float64), nc, group, whiten)
    check_whitened(ref["out"], ref["bound"], group)


def check_whitened(out, bound, group):
    """mean 0 and Y^T Y / (n - 1) = I per group, a check that depends on no eigengap.  With |dy_j| <= b_j and rms(y_l) = 1:
    |mean y_j| <= b_j (+ the sum's own rounding), |(Y^T Y / (n - 1) - I)_jl| <= (b_j + b_l) sqrt(n / (n - 1)) (Cauchy-Schwarz)."""
    y = np.asarray(out, np.float64).reshape(-1, out.shape[-1])
    n, nc = y.shape
    k = nc // group
    for g in range(group):
        yg, b = y[:, g * k:(g + 1) * k], bound[g * k:(g + 1) * k]
        tol_mean = b + 4 * R.U * np.sqrt(n) * np.abs(yg).max(0)
        assert np.all(np.abs(yg.mean(0)) <= tol_mean), (np.abs(yg.mean(0)) / tol_mean).max()
        G = yg.T @ yg / (n - 1)
        tol = 1.1 * (b[:, None] + b[None, :]) * np.abs(yg).max() + 8 * R.U * np.sqrt(n)
        assert np.all(np.abs(G - np.eye(k)) <= tol), (np.abs(G - np.eye(k)) / tol).max()


def test_python_argument_refusals():
    from hsimae_amd import GWPCA, apply_gwpca
    with pytest.raises(ValueError, match="group must be 1, 2 or 4, got 3"):
        GWPCA(nc=30, group=3)
    with pytest.raises(ValueError, match="multiple of group=4, got 30"):
        GWPCA(nc=30, group=4)
    with pytest.raises(TypeError, match="nc must be an int"):
        GWPCA(nc=32.0)
    pca = GWPCA()
    assert (pca.nc, pca.group, pca.whiten) == (32, 4, True)                        # the reference's defaults
    with pytest.raises(RuntimeError, match="not been fitted"):
        pca.mean_
    with pytest.raises(RuntimeError, match="not been fitted"):
        pca.transform(np.zeros((4, 4, 64)))
    with pytest.raises(ValueError, match=r"\[H, W, bands\], got shape \(4, 64\)"):
        pca.fit(np.zeros((4, 64)))
    with pytest.raises(TypeError, match="float32 or float64, got int16"):
        pca.fit(np.zeros((4, 4, 64), np.int16))
    with pytest.raises(TypeError, match="float32 or float64, got torch.float16"):
        pca.fit(torch.zeros(4, 4, 64, dtype=torch.float16))
    with pytest.raises(TypeError, match="numpy array or a torch tensor, got list"):
        pca.fit([[1.0]])
    with pytest.raises(ValueError, match=r"at least 2 pixels, got scene shape \(1, 1, 64\)"):
        pca.fit(np.zeros((1, 1, 64)))
    with pytest.raises(ValueError, match=r"\(4, 4, 24\).*narrowest: 6"):
        pca.fit(np.zeros((4, 4, 24)))                                              # 8 components from groups of 6 bands
    with pytest.raises(ValueError, match=r"\(2, 2, 64\).*at least 8 pixels"):
        pca.fit(np.zeros((2, 2, 64)))
    with pytest.raises(ValueError, match="a group of 150 bands"):
        pca.fit(np.zeros((4, 4, 600)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pca.fit(np.zeros((4, 4, 64)))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            apply_gwpca(torch.zeros(4, 4, 64, dtype=torch.float64))


def test_library_exports_the_gwpca_entry_points_and_answers_abi_108():
    import ctypes as C
    from hsimae_amd import _lib
    lib = _lib.load()
    for name in ("hsimae_gwpca_workspace_bytes", "hsimae_gwpca_fit", "hsimae_gwpca_apply"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    # the argument checks that need no device: the workspace query answers sizes and refusals on the host
    def ws(**kw):
        args = dict(scene=1 << 20, scene_f64=1, H=610, W=340, C=103, nc=32, group=4, whiten=1)
        args.update(kw)
        return lib.hsimae_gwpca_workspace_bytes(C.byref(_lib.GwpcaParams(**args)))
    assert ws() > 0 and ws() % 8 == 0
    assert lib.hsimae_gwpca_workspace_bytes(None) == -4
    assert ws(H=1, W=1) == -1 and ws(H=0) == -1 and ws(nc=0) == -1
    assert ws(group=3) == -2 and ws(group=8) == -2
    assert ws(nc=30) == -1                                    # not a multiple of group
    assert ws(nc=104) == -1                                   # 26 components from the 25-band group
    assert ws(H=2, W=2) == -1                                 # 8 components from 4 pixels
    assert ws(C=516) == -2 and ws(C=512) > 0                  # a 129-band group
    assert ws(C=128, group=1) > 0 and ws(C=129, group=1) == -2
