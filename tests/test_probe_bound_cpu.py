"""tests/probe_ref.py without a GPU: the fp64 restatement of csrc/probe.hip against torch's fp64 autograd and AdamW and against
numpy, the emulated fp32 sequences inside their bounds at the GPU test's shapes, planted faults rejected by the checks, the
planted-cluster facts, the ABI, and LinearProbe's argument refusals."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import probe_ref as R  # noqa: E402


def torch_fit(xs, y, D, C, first, T, hp, schedule):
    """The same iteration in torch fp64: nn.Linear on the standardised rows, F.cross_entropy over the real classes, autograd,
    torch.optim.AdamW with the bias in a no-decay group -> (W [C - first, D], b [C - first], losses)."""
    lin = torch.nn.Linear(D, C - first).double()
    torch.nn.init.zeros_(lin.weight)
    torch.nn.init.zeros_(lin.bias)
    opt = torch.optim.AdamW([{"params": [lin.weight], "weight_decay": R.f32(hp["wd"])}, {"params": [lin.bias], "weight_decay": 0.0}],
                            lr=R.f32(hp["lr"]), betas=(R.f32(hp["b1"]), R.f32(hp["b2"])), eps=R.f32(hp["eps"]))
    x, t = torch.from_numpy(xs[:, :D]), torch.from_numpy(y - first)
    losses = []
    for it in range(T):
        for grp in opt.param_groups:
            grp["lr"] = R.f32(R.lr_at(hp["lr"], it, T, schedule))
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(lin(x), t)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return lin.weight.detach().numpy(), lin.bias.detach().numpy(), np.array(losses)


@pytest.mark.parametrize("T,schedule", [(1, "constant"), (20, "cosine")])
def test_restatement_equals_torch_fp64_autograd_and_adamw(T, schedule):
    for C, first in ((8, 1), (5, 0)):
        # (151 rows: a prime, so no class holds exactly n / (C - first) of them.  Such a class has a zero bias gradient at the uniform
        # start, and AdamW's m / sqrt(v) turns the fp64 rounding noise left in its place into a step of either sign)
        x, y = R.traj_case(n=151, D=12, C=C, first=first, seed=T)
        pr = R.prepare_ref(x, y, 12, C, first)
        f = R.fit_ref(x, y, 12, C, first, T, R.TRAJ_HP, schedule)
        W, b, losses = torch_fit(pr["xs"], y, 12, C, first, T, R.TRAJ_HP, schedule)
        assert np.abs(f["w"][first:, :12] - W).max() <= 1e-12 and np.abs(f["w"][first:, 12] - b).max() <= 1e-12
        assert np.abs(f["losses"] - losses).max() <= 1e-12 and not f["w"][:first].any()
        assert abs(f["losses"][0] - math.log(C - first)) <= 1e-12


def test_prepare_restatement_equals_numpy_population_statistics():
    x, y, *_ = R.step_case(257, 36, 8, 1, ldx=40)
    pr = R.prepare_ref(x, y, 36, 8, 1)
    ok = R.valid_of(y, 1, 8)
    assert pr["bad"] == 1 and pr["nv"] == 256 and not ok[2]
    xv = x[ok, :36].astype(np.float64)
    assert np.allclose(pr["mean"], np.mean(xv, 0), rtol=1e-14, atol=0)
    assert np.allclose(pr["rstd"], 1 / np.sqrt(np.var(xv, 0) + R.f32(1e-6)), rtol=1e-13, atol=0)       # ddof = 0
    assert pr["rstd"][1] == 1 / math.sqrt(R.f32(1e-6)) and not pr["xs"][:, 1].any()                      # the constant column
    assert np.allclose(pr["xs"][ok, :36].std(0)[[0, 2, 35]], 1, rtol=1e-4) and not pr["xs"][2].any() and (pr["xs"][ok, 36] == 1).all()


def test_fold_reproduces_the_standardised_logits():
    x, y = R.traj_case(n=120, D=16, C=6, first=1)
    f = R.fit_ref(x, y, 16, 6, 1, 5, R.TRAJ_HP)
    w64 = np.zeros((R.ROWS, 20))
    w64[:6, :17] = f["w"]
    W, _, b, _ = R.fold_ref(w64, f["mean"], f["rstd"], 16, 6, 1)
    z = R.logits_ref(x, f["mean"], f["rstd"], f["w"], 16, 6, 1)
    folded = x.astype(np.float64) @ W.T + b
    assert np.abs(folded[:, 1:] - z[:, 1:]).max() <= 1e-12 and not W[0].any() and b[0] == 0


def run_emulated(n, D, C, first, fault=None, seed=0):
    x, y, w, m, v = R.step_case(n, D, C, first, ldx=D + 4, seed=seed)
    pre = R.emulate_prepare(x, y, D, C, first)
    pre["state"] = np.array([0, 0, 0, pre["bad"], pre["nv"], 0, 0, 0], np.float64)
    got = R.emulate_step(pre, y, w, m, v, D, C, first, 3, R.HP["lr"], R.HP, fault)
    return R.check_prepare(pre, x, y, D, C, first), R.check_step(got, pre, y, w, m, v, D, C, first, 3, R.HP["lr"], R.HP)


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("D", R.DS)
def test_emulated_sequences_lie_inside_their_bounds(n, D):
    for C, first in R.CLASSES:
        cp, cs = run_emulated(n, D, C, first)
        assert cp["ok"], (C, first, cp)
        assert cs["ok"], (C, first, cs)


@pytest.mark.parametrize("fault,sees", [("seg_swapped", "norm"), ("bias_decayed", "w"), ("n_minus_1", "g"), ("class0_in_softmax", "g")])
def test_step_checks_reject_planted_faults(fault, sees):
    good = run_emulated(600, 36, 8, 1)[1]
    bad = run_emulated(600, 36, 8, 1, fault=fault)[1]
    assert good["ok"] and not bad["ok"] and bad[sees] > 1, (fault, bad)
    if fault == "seg_swapped":                                  # the elements move by ulps of fp32, at the edge of their bounds; the sum
        assert bad["norm"] > 1e3 and bad["g"] <= 1               # of squares, held to fp64's precision, is what sees the order
    if fault == "bias_decayed":
        assert bad["g"] <= 1 and bad["norm"] <= 1 and bad["m"] <= 1


def test_prepare_check_rejects_sample_variance_and_a_counted_bad_row():
    x, y, *_ = R.step_case(65, 32, 8, 1)
    pre = R.emulate_prepare(x, y, 32, 8, 1)
    pre["state"] = np.array([0, 0, 0, pre["bad"], pre["nv"], 0, 0, 0], np.float64)
    assert R.check_prepare(pre, x, y, 32, 8, 1)["ok"]
    sample = dict(pre, rstd=(pre["rstd"].astype(np.float64) * math.sqrt(63 / 64)).astype(np.float32))
    assert R.check_prepare(sample, x, y, 32, 8, 1)["rstd"] > 1
    ycount = y.copy()
    ycount[2] = 3                                               # the statistics of a bank in which the bad row counts
    counted = R.emulate_prepare(x, ycount, 32, 8, 1)
    counted["state"] = pre["state"]
    assert not R.check_prepare(counted, x, y, 32, 8, 1)["ok"]


def test_planted_clusters_with_the_default_recipe():
    bank, by, qs, qy = R.clusters()
    hp = dict(lr=1e-2, wd=1e-4, b1=0.9, b2=0.999, eps=1e-8)
    f = R.fit_ref(bank, by, 32, 8, 1, 100, hp)
    z = R.logits_ref(qs, f["mean"], f["rstd"], f["w"], 32, 8, 1)
    top = np.sort(z[:, 1:], axis=1)
    gap = (top[:, -1] - top[:, -2]).min()
    print(f"loss {f['losses'][0]:.4f} -> {f['losses'][-1]:.4f}, smallest top-1/top-2 gap {gap:.3f}")
    assert np.array_equal(1 + np.argmax(z[:, 1:], axis=1), qy)                                  # 1000 of 1000
    assert abs(f["losses"][0] - math.log(7)) <= 1e-12 and abs(f["losses"][-1] - 0.034) < 1e-3 and abs(gap - 0.72) < 1e-2


def test_trajectory_gate_comes_from_the_emulation():
    x, y = R.traj_case()
    f = R.fit_ref(x, y, 36, 8, 1, R.TRAJ_STEPS, R.TRAJ_HP)
    e = R.emulate_fit(x, y, 36, 8, 1, R.TRAJ_STEPS, R.TRAJ_HP)
    dev = np.abs(e["w"][:8, :37].astype(np.float64) - f["w"]).max()
    print(f"emulation off the restatement by {dev:.3g} after {R.TRAJ_STEPS} steps, |w| up to {np.abs(f['w']).max():.3g}")
    assert 0 < dev < 1e-4 * np.abs(f["w"]).max() and np.abs(e["losses"] - f["losses"]).max() < 1e-5
    assert f["losses"][-1] < f["losses"][0] and not e["w"][8:].any() and not e["w"][:, 37:].any() and not e["w"][0].any()


def test_library_exports_the_probe_entry_points_under_abi_108():
    import hsimae_amd
    from hsimae_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    for name, struct in (("hsimae_probe_prepare", _lib.ProbePrepareParams), ("hsimae_probe_step", _lib.ProbeStepParams),
                         ("hsimae_probe_logits", _lib.ProbeLogitsParams), ("hsimae_probe_fold", _lib.ProbeFoldParams)):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None and re.search(r"\b%s\s*\(" % name, hdr)
        assert R.header_fields(hdr, name + "_params") == [(n, t) for n, t in struct._fields_], name
    assert _lib.PROBE_SEG == R.SEG == int(re.search(r"#define HSIMAE_PROBE_SEG (\d+)", hdr).group(1))
    assert _lib.PROBE_STATE == int(re.search(r"#define HSIMAE_PROBE_STATE (\d+)", hdr).group(1))
    assert _lib.PROBE_ROWS == R.ROWS == int(re.search(r"#define HSIMAE_PROBE_ROWS (\d+)", hdr).group(1))
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    for cls in (hsimae_amd.DualViT, hsimae_amd.HSIViT):
        assert callable(cls.probe_scene)
    assert callable(hsimae_amd.linear_probe_scene) and callable(hsimae_amd.LinearProbe)
    assert "probe" in build.UNITS and build.UNITS.index("probe") < build.UNITS.index("api")
    src = open(os.path.join(build.CSRC, "probe.hip")).read()
    body = src.split("#include")[-1]                            # the tile is the shared one; no atomics, no cooperative launch
    assert '#include "dot_tile.h"' in src and "mfma_f32_32x32x2f32" not in src and "atomic" not in body and "Cooperative" not in body


def test_linear_probe_refuses_what_it_cannot_serve():
    from hsimae_amd import LinearProbe
    for kw in (dict(num_class=1), dict(num_class=65), dict(num_class=8, first=8), dict(num_class=8, first=-1),
               dict(num_class=8, max_iter=0), dict(num_class=8, lr=-1.0), dict(num_class=8, lr=float("nan")),
               dict(num_class=8, weight_decay=-1e-4), dict(num_class=8, betas=(0.9, 1.0)), dict(num_class=8, betas=(0.9,)),
               dict(num_class=8, eps=-1.0), dict(num_class=8, bn_eps=0.0), dict(num_class=8, schedule="step")):
        with pytest.raises(ValueError):
            LinearProbe(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LinearProbe(8).fit(torch.zeros(30, 8), torch.ones(30, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="fit"):
        LinearProbe(8).logits(torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="fit"):
        LinearProbe(8).head()
    p = LinearProbe(20)
    assert (p.num_class, p.first, p.max_iter, p.lr, p.weight_decay, p.betas, p.eps, p.schedule, p.bn_eps) == \
        (20, 1, 100, 1e-2, 1e-4, (0.9, 0.999), 1e-8, "cosine", 1e-6)
    assert p.lr_at(0) == 1e-2 and abs(p.lr_at(50) - 5e-3) < 1e-18 and LinearProbe(8, schedule="constant").lr_at(70) == 1e-2
