"""csrc/cls.hip without a GPU: the fp64 restatement (tests/cls_ref.py) against torch's cross_entropy (value and autograd
gradient, the all-ignored and empty cases settled here), torch's own fp32 result inside the bound, the bound against planted
faults, the restated scores against finetune_train.scores, and the library's new symbols under ABI 108."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cls_ref as R  # noqa: E402

CPU_SHAPES = [s for s in R.SHAPES if s[0] <= 512]            # the 8193-row shape adds nothing on the host but time


def torch_ce(z, y, C, dtype, ignore_index=0):
    zt = torch.tensor(np.ascontiguousarray(z[:, :C]), dtype=dtype, requires_grad=True)
    loss = F.cross_entropy(zt, torch.from_numpy(y), reduction="mean", ignore_index=ignore_index)
    (g,) = torch.autograd.grad(loss, zt)
    return loss.detach().double().item(), g.double().numpy()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_torch_fp64_and_torch_fp32_lies_inside_the_bound(shape, mode):
    N, C, ld = shape
    z, y, nan_row = R.make_case(N, C, ld, mode)
    ref = R.cls_ref(z, y, C, ignore_index=0, first=0)
    rows = np.ones(N, bool)
    if nan_row is not None:
        rows[nan_row] = False                                  # the NaN row: only pred is compared
    loss64, g64 = torch_ce(z, y, C, torch.float64)
    if np.isnan(ref["loss"]):
        assert np.isnan(loss64)
    else:
        assert abs(loss64 - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    assert np.allclose(g64[rows], ref["dlogits"][rows], rtol=0, atol=1e-13)
    # (torch leaves 0 * NaN = NaN in the gradient of an IGNORED row of NaN logits; the kernel and the restatement write zeros)
    assert np.all(g64[~ref["valid"] & rows] == 0) and np.all(ref["dlogits"][~ref["valid"]] == 0)
    zt = torch.from_numpy(np.ascontiguousarray(z[:, :C]))
    assert np.array_equal(torch.argmax(zt, 1).numpy(), ref["pred"])
    assert np.array_equal(1 + torch.argmax(zt[:, 1:], 1).numpy(), R.cls_ref(z, y, C, first=1)["pred"])
    loss32, g32 = torch_ce(z, y, C, torch.float32)
    r_loss = R.ratio(loss32, ref["loss"], ref["loss_bound"])
    r_g = R.ratio(g32[rows], ref["dlogits"][rows], ref["dlogits_bound"][rows])
    print(f"{shape} {mode}: torch fp32 err / bound: loss {r_loss:.3f}, dlogits {r_g:.3f}")
    assert r_loss <= 1.0 and r_g <= 1.0


def test_no_valid_row_is_nan_loss_and_zero_gradient_as_torch():
    z = np.random.RandomState(0).standard_normal((6, 16)).astype(np.float32)
    y = np.zeros(6, np.int64)
    loss, g = torch_ce(z, y, 5, torch.float32)
    ref = R.cls_ref(z, y, 5)
    assert np.isnan(loss) and np.isnan(ref["loss"]) and ref["n_valid"] == 0
    assert np.all(g == 0) and np.all(ref["dlogits"] == 0)
    # N = 0: torch's mean over no rows
    empty = F.cross_entropy(torch.zeros(0, 5), torch.zeros(0, dtype=torch.int64), ignore_index=0)
    assert torch.isnan(empty) and np.isnan(R.cls_ref(np.zeros((0, 8), np.float32), np.zeros(0, np.int64), 5)["loss"])
    # another ignore_index, inside and outside the class range
    for ign in (2, -100):
        y2 = np.array([1, 2, 3, 4, 2, 1], np.int64)
        l64, g64 = torch_ce(z, y2, 5, torch.float64, ignore_index=ign)
        r2 = R.cls_ref(z, y2, 5, ignore_index=ign)
        assert abs(l64 - r2["loss"]) < 1e-12 and np.allclose(g64, r2["dlogits"], atol=1e-13, rtol=0)
    assert R.cls_ref(z, np.array([1, 2, 7, -3, 0, 1]), 5)["bad"] and not ref["bad"]


def faulty(z, y, C, ld, fault, first=0):
    """The restatement with one planted fault -> (loss, dlogits [N, ld], pred)."""
    z64 = z.astype(np.float64)
    N = z.shape[0]
    valid = R.valid_rows(y, C, 0)
    n = int(valid.sum())
    W = C + 1 if fault == "pad_column" and ld > C else C      # a pad column taken for a class
    zz = z64[:, :W]
    rows = np.arange(N)
    with np.errstate(all="ignore"):
        m = np.zeros(N) if fault == "no_max" else np.where(np.isnan(zz), -np.inf, zz).max(1)
        e = np.exp(zz - m[:, None])
        if fault == "no_max":
            e = e.astype(np.float32).astype(np.float64)        # fp32 overflows where fp64 would not yet
        s = e.sum(1)
        p = e / s[:, None]
        yc = np.where(valid, y, 0)
        li = np.log(s) - (zz - m[:, None])[rows, yc]
        oh = np.zeros_like(zz)
        oh[rows, yc - 1 if fault == "onehot_minus_one" else yc] = 1.0
        used = np.ones(N, bool) if fault == "ignored_in_sum" else valid
        div = N if fault == "mean_over_N" else n
        loss = li[used].sum() / div
        dl = np.zeros((N, ld))
        dl[valid, :W] = (p - oh)[valid] / div
        if fault == "ignored_gradient":
            dl[~valid, :W] = (p - oh)[~valid] / div
        f = 0 if fault == "first_ignored" else first
        zc = z64[:, f:C]
        if fault == "last_of_tie":
            pred = f + (zc.shape[1] - 1 - np.argmax(zc[:, ::-1], axis=1))
        else:
            pred = f + np.argmax(zc, axis=1)
    return loss, dl, pred


FAULTS = ["mean_over_N", "ignored_in_sum", "ignored_gradient", "no_max", "pad_column", "onehot_minus_one", "last_of_tie",
          "first_ignored"]


@pytest.mark.parametrize("fault", FAULTS)
def test_bound_rejects_planted_faults(fault):
    N, C, ld = 65, 33, 48
    z, y, nan_row = R.make_case(N, C, ld, "random")
    first = 1 if fault == "first_ignored" else 0
    y[0] = 3                                                   # the +-1e4 row and the tied row count
    y[1] = 5
    if fault == "first_ignored":
        z[5, 0] = 100.0                                        # class 0 is the overall maximum of a row
    if fault == "pad_column":
        z[:, C:] = 4.0                                         # a finite pad: the fault must show without the NaN canary too
    ref = R.cls_ref(z, y, C, first=first, ldd=ld)
    rows = np.arange(N) != nan_row

    def worst(loss, dl, pred):
        return max(R.ratio(loss, ref["loss"], ref["loss_bound"]), R.ratio(dl[rows], ref["dlogits"][rows], ref["dlogits_bound"][rows]),
                   0.0 if np.array_equal(pred, ref["pred"]) else np.inf)

    assert worst(*faulty(z, y, C, ld, None, first)) <= 1.0     # the harness itself is clean
    w = worst(*faulty(z, y, C, ld, fault, first))
    print(f"{fault}: worst err / bound = {w:.3g}")
    assert w > 10.0, w


def score_maps():
    rng = np.random.RandomState(3)
    out = []
    C = 7
    gt = rng.randint(0, C, 500); gt[gt == 4] = 0                # class 4 absent from gt
    pred = rng.randint(0, C, 500); pred[pred == 2] = 3          # class 2 never predicted; predictions of 0 occur
    pred[rng.rand(500) < 0.5] = gt[rng.rand(500) < 0.5][:1]     # some structure
    out.append(("random", C, gt, pred))
    out.append(("single_class_pe_1", 4, np.full(40, 2), np.full(40, 2)))
    out.append(("all_wrong", 3, np.array([1, 1, 2, 2, 0]), np.array([2, 0, 1, 0, 1])))
    gt2 = rng.randint(1, 5, 300)
    out.append(("perfect", 5, gt2, gt2.copy()))
    return out


@pytest.mark.parametrize("case", score_maps(), ids=lambda c: c[0])
def test_restated_scores_equal_the_host_function(case):
    from hsimae_amd.finetune_train import scores
    _, C, gt, pred = case
    cm, _, bad = R.confusion_ref(gt, pred, C)
    assert not bad
    out, bound = R.scores_ref(cm)
    oa, aa, kappa, ca = scores(gt, pred)
    k = C - 1
    assert abs(out[0] - oa) <= 1e-12 and abs(out[1] - aa) <= 1e-12 and abs(out[2] - kappa) <= 1e-12
    assert np.allclose(out[3:3 + k][out[3 + k:] != 0], ca, rtol=0, atol=1e-12)
    assert np.all(bound >= 0) and bound.max() < 1e-9
    if case[0] == "single_class_pe_1":
        assert out[2] == 0.0 and kappa == 0.0


def test_confusion_restatement_masks_and_flags():
    gt = np.array([0, 1, 2, 2, 3, 1])
    pred = np.array([1, 1, 2, 0, 9, -1])
    cm, masked, bad = R.confusion_ref(gt, pred, 4, mask=np.array([0, 1, 1, 1, 1, 0]))
    assert bad and masked.tolist() == [0, 1, 2, 0, 9, 0]
    assert cm.sum() == 4 and cm[1, 1] == 1 and cm[2, 2] == 1 and cm[2, 0] == 1 and cm[1, 0] == 1


NEW = ["hsimae_cls_workspace_bytes", "hsimae_cls_loss", "hsimae_cls_grad_scale", "hsimae_confusion", "hsimae_confusion_map",
       "hsimae_scores"]


def test_library_exports_the_classification_entry_points_under_abi_108():
    import ctypes as C
    import hsimae_amd
    from hsimae_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "hsimae_cls_params" in hdr
    assert lib.hsimae_version() == _lib.ABI_VERSION == 108 == int(re.search(r"#define HSIMAE_VERSION (\d+)", hdr).group(1))
    assert callable(hsimae_amd.ClassLoss) and callable(hsimae_amd.ScoreMeter)
    # the refusals that are decided before anything is launched
    assert lib.hsimae_cls_workspace_bytes(32) > 0 and lib.hsimae_cls_workspace_bytes(0) > 0 and lib.hsimae_cls_workspace_bytes(-1) == -1
    assert lib.hsimae_cls_loss(None, None) == -4
    ok = dict(logits=1 << 20, ld=16, targets=1 << 21, N=4, C=10, ignore_index=0, first=0, loss=1 << 22, workspace=1 << 23)

    def rc(**kw):
        a = dict(ok); a.update(kw)
        return lib.hsimae_cls_loss(C.byref(_lib.ClsParams(**a)), None)
    assert rc(N=-1) == -1 and rc(C=1) == -1 and rc(ld=9) == -1 and rc(first=10) == -1 and rc(first=-1) == -1
    assert rc(dlogits=1 << 24, ldd=9) == -1
    assert rc(C=1025, ld=1040) == -2
    assert rc(loss=None) == -4 and rc(workspace=None) == -4 and rc(logits=None) == -4 and rc(targets=None) == -4
    assert rc(logits=(1 << 20) + 2) == -3 and rc(targets=(1 << 21) + 4) == -3 and rc(workspace=(1 << 23) + 4) == -3
    assert rc(pred=(1 << 24) + 4) == -3 and rc(bad=(1 << 24) + 2) == -3 and rc(loss=(1 << 22) + 1) == -3
    assert lib.hsimae_confusion(8, 16, -1, 4, 24, 32, None) == -1 and lib.hsimae_confusion(8, 16, 5, 1, 24, 32, None) == -1
    assert lib.hsimae_confusion(8, 16, 5, 1025, 24, 32, None) == -2
    assert lib.hsimae_confusion(8, 16, 5, 4, None, 32, None) == -4 and lib.hsimae_confusion(8, 16, 5, 4, 24, None, None) == -4
    assert lib.hsimae_confusion(None, 16, 5, 4, 24, 32, None) == -4 and lib.hsimae_confusion(8, 12, 5, 4, 24, 32, None) == -3
    assert lib.hsimae_confusion(8, 16, 0, 4, 24, 32, None) == 0
    assert lib.hsimae_confusion_map(8, None, 16, None, 5, 4, 24, 32, None) == -4
    assert lib.hsimae_confusion_map(8, 12, 16, 40, 5, 4, 24, 32, None) == -3
    assert lib.hsimae_scores(8, 1, 16, None) == -1 and lib.hsimae_scores(8, 1025, 16, None) == -2
    assert lib.hsimae_scores(None, 4, 16, None) == -4 and lib.hsimae_scores(8, 4, 12, None) == -3
    assert lib.hsimae_cls_grad_scale(4, 8, 12, -1, None) == -1 and lib.hsimae_cls_grad_scale(None, 8, 12, 3, None) == -4
    assert lib.hsimae_cls_grad_scale(4, 8, 12, 0, None) == 0 and lib.hsimae_cls_grad_scale(4, 8, 14, 3, None) == -3


def test_python_refuses_cpu_tensors_and_bad_arguments():
    from hsimae_amd import ClassLoss, ScoreMeter
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ClassLoss()(torch.zeros(4, 5), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="torch tensor"):
        ClassLoss()(np.zeros((4, 5), np.float32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ScoreMeter(5, "cpu")
    with pytest.raises(ValueError, match="between 2 and 1024"):
        ScoreMeter(1, "cuda:0")
