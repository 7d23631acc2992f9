"""csrc/cls.hip on the GPU: hsimae_cls_loss against the fp64 restatement and bound of tests/cls_ref.py on every shape and
target pattern, the confusion counts against np.add.at, hsimae_scores against the restated scores, every documented refusal,
and the Python layer: ClassLoss under DualViT's head, ScoreMeter against finetune_train.scores, the fine-tuning loop."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cls_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I64_CANARY = -(1 << 62) + 12345


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@functools.lru_cache(maxsize=None)
def case(shape, mode, first):
    N, C_, ld = shape
    z, y, nan_row = R.make_case(N, C_, ld, mode)
    return z, y, nan_row, R.cls_ref(z, y, C_, ignore_index=0, first=first, ldd=ld)


def run_cls(z, y, C_, first, ldd, ignore_index=0, want_grad=True):
    """One hsimae_cls_loss call with every output inside a canary frame -> dict of host arrays (frames included)."""
    from hsimae_amd import _lib
    lib = _lib.load()
    N, ld = z.shape
    zt = torch.from_numpy(z).to(DEV)
    z0 = zt.clone()
    yt = torch.from_numpy(y).to(DEV)
    loss = torch.full((3,), float("nan"), device=DEV)
    dl = torch.full((N + 2, ldd), float("nan"), device=DEV)
    nv = torch.full((3,), I64_CANARY, dtype=torch.int64, device=DEV)
    pred = torch.full((N + 2,), I64_CANARY, dtype=torch.int64, device=DEV)
    bad = torch.tensor([7, 0, 7], dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.hsimae_cls_workspace_bytes(N) // 8, dtype=torch.float64, device=DEV)
    p = _lib.ClsParams(logits=zt.data_ptr(), ld=ld, targets=yt.data_ptr(), N=N, C=C_, ignore_index=ignore_index, first=first,
                       loss=loss.data_ptr() + 4, n_valid=nv.data_ptr() + 8, dlogits=dl.data_ptr() + 4 * ldd if want_grad else None,
                       ldd=ldd, pred=pred.data_ptr() + 8, bad=bad.data_ptr() + 4, workspace=ws.data_ptr())
    rc = lib.hsimae_cls_loss(C.byref(p), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    # NaN pads compare unequal to themselves: compare the bit patterns
    assert torch.equal(zt.view(torch.int32), z0.view(torch.int32)), "logits were written"
    return {"loss": loss.cpu().numpy(), "dl": dl.cpu().numpy(), "nv": nv.cpu().numpy(), "pred": pred.cpu().numpy(), "bad": bad.cpu().numpy()}


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cls_loss_within_the_bound_on_every_shape_and_target_pattern(shape, mode):
    N, C_, ld = shape
    first = 1 if (N + C_) % 2 else 0                           # both values of `first` over the shapes
    z, y, nan_row, ref = case(shape, mode, first)
    a = run_cls(z, y, C_, first, ld)
    b = run_cls(z, y, C_, first, ld)
    for k in a:                                                # two runs agree bit for bit (canaries and NaN included)
        assert a[k].tobytes() == b[k].tobytes(), k
    # canaries
    assert np.isnan(a["loss"][[0, 2]]).all() and np.isnan(a["dl"][[0, N + 1]]).all()
    assert (a["nv"][[0, 2]] == I64_CANARY).all() and (a["pred"][[0, N + 1]] == I64_CANARY).all() and a["bad"].tolist() == [7, 0, 7]
    loss, dl, pred = a["loss"][1], a["dl"][1:N + 1], a["pred"][1:N + 1]
    assert a["nv"][1] == ref["n_valid"]
    assert np.array_equal(pred, ref["pred"])
    rows = np.arange(N) != (-1 if nan_row is None else nan_row)          # the NaN row: only pred is checked
    r_loss = R.ratio(loss, ref["loss"], ref["loss_bound"])
    r_dl = R.ratio(dl[rows], ref["dlogits"][rows], ref["dlogits_bound"][rows])
    print(f"[cls {shape} {mode} first={first}] worst err / bound: loss {r_loss:.3f}, dlogits {r_dl:.3f}")
    assert r_loss <= 1.0, (loss, ref["loss"], ref["loss_bound"])
    assert r_dl <= 1.0
    zero_rows = ~ref["valid"]
    assert not dl[zero_rows].any() and not np.signbit(dl[zero_rows]).any()               # exact zeros, the NaN row too when ignored
    assert not dl[:, C_:].any()
    # without a gradient buffer the other outputs are the same bits
    c = run_cls(z, y, C_, first, ld, want_grad=False)
    assert c["loss"].tobytes() == a["loss"].tobytes() and c["pred"].tobytes() == a["pred"].tobytes() and np.isnan(c["dl"]).all()


def test_cls_loss_other_ignore_index_bad_targets_and_empty_batch():
    from hsimae_amd import _lib
    z, y, _ = R.make_case(65, 33, 48, "none_ignored")
    y = y.copy()
    for ign in (5, -100):
        ref = R.cls_ref(z, y, 33, ignore_index=ign, ldd=33)
        a = run_cls(z, y, 33, 0, 33, ignore_index=ign)
        assert a["nv"][1] == ref["n_valid"] and a["bad"].tolist() == [7, 0, 7]
    y[7], y[9] = 33, -1                                        # neither ignore_index nor a class: flagged, treated as ignored
    ref = R.cls_ref(z, y, 33, ignore_index=-100, ldd=33)
    a = run_cls(z, y, 33, 0, 33, ignore_index=-100)
    assert ref["bad"] and a["bad"].tolist() == [7, 1, 7] and a["nv"][1] == ref["n_valid"] == 63
    assert not a["dl"][1:66][[7, 9]].any()
    # N = 0: HSIMAE_OK, the loss torch gives (NaN), n_valid 0
    lib = _lib.load()
    loss = torch.zeros(1, device=DEV)
    nv = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.hsimae_cls_workspace_bytes(0) // 8, dtype=torch.float64, device=DEV)
    p = _lib.ClsParams(logits=None, ld=16, targets=None, N=0, C=10, ignore_index=0, first=0, loss=loss.data_ptr(),
                       n_valid=nv.data_ptr(), workspace=ws.data_ptr())
    assert lib.hsimae_cls_loss(C.byref(p), stream()) == 0
    assert torch.isnan(loss).all() and int(nv) == 0


def test_every_documented_refusal_returns_its_code():
    from hsimae_amd import _lib
    lib = _lib.load()
    t = torch.zeros(4096, dtype=torch.float64, device=DEV)
    a = t.data_ptr()
    ok = dict(logits=a, ld=16, targets=a + 1024, N=4, C=10, ignore_index=0, first=0, loss=a + 2048, workspace=a + 8192)

    def rc(**kw):
        d = dict(ok); d.update(kw)
        return lib.hsimae_cls_loss(C.byref(_lib.ClsParams(**d)), stream())
    assert lib.hsimae_cls_loss(None, stream()) == -4
    assert rc(N=-1) == -1 and rc(C=1) == -1 and rc(ld=9) == -1 and rc(first=10) == -1 and rc(first=-1) == -1
    assert rc(dlogits=a + 4096, ldd=9) == -1
    assert rc(C=1025, ld=1040) == -2
    assert rc(loss=None) == -4 and rc(workspace=None) == -4 and rc(logits=None) == -4 and rc(targets=None) == -4
    assert rc(logits=a + 2) == -3 and rc(targets=a + 1028) == -3 and rc(workspace=a + 8196) == -3 and rc(loss=a + 2049) == -3
    assert rc(pred=a + 4100) == -3 and rc(n_valid=a + 4100) == -3 and rc(bad=a + 4098) == -3 and rc(dlogits=a + 4098, ldd=16) == -3
    assert lib.hsimae_cls_workspace_bytes(-1) == -1
    cf = lib.hsimae_confusion
    assert cf(a, a + 64, -1, 4, a + 512, a + 1024, stream()) == -1 and cf(a, a + 64, 4, 1, a + 512, a + 1024, stream()) == -1
    assert cf(a, a + 64, 4, 1025, a + 512, a + 1024, stream()) == -2
    assert cf(None, a + 64, 4, 4, a + 512, a + 1024, stream()) == -4 and cf(a, None, 4, 4, a + 512, a + 1024, stream()) == -4
    assert cf(a, a + 64, 4, 4, None, a + 1024, stream()) == -4 and cf(a, a + 64, 4, 4, a + 512, None, stream()) == -4
    assert cf(a + 4, a + 64, 4, 4, a + 512, a + 1024, stream()) == -3 and cf(a, a + 64, 4, 4, a + 516, a + 1024, stream()) == -3
    assert cf(a, a + 64, 4, 4, a + 512, a + 1026, stream()) == -3
    assert cf(a, a + 64, 0, 4, a + 512, a + 1024, stream()) == 0
    cmap = lib.hsimae_confusion_map
    assert cmap(a, None, a + 64, None, 4, 4, a + 512, a + 1024, stream()) == -4
    assert cmap(a, a + 4, a + 64, a + 128, 4, 4, a + 512, a + 1024, stream()) == -3
    assert cmap(a, None, a + 64, a + 132, 4, 4, a + 512, a + 1024, stream()) == -3
    assert cmap(a, None, a + 64, a + 128, -1, 4, a + 512, a + 1024, stream()) == -1
    sc = lib.hsimae_scores
    assert sc(a, 1, a + 512, stream()) == -1 and sc(a, 1025, a + 512, stream()) == -2
    assert sc(None, 4, a + 512, stream()) == -4 and sc(a, 4, None, stream()) == -4 and sc(a + 4, 4, a + 512, stream()) == -3
    gs = lib.hsimae_cls_grad_scale
    assert gs(a, a + 64, a + 128, -1, stream()) == -1 and gs(None, a + 64, a + 128, 3, stream()) == -4
    assert gs(a, a + 66, a + 128, 3, stream()) == -3 and gs(a, a + 64, a + 128, 0, stream()) == 0
    torch.cuda.synchronize()
    assert not t.any()                                         # nothing was launched by a refused call


def labels(n, C_, seed, drop=None, never=None):
    rng = np.random.RandomState(seed)
    gt = rng.randint(0, C_, n).astype(np.int64)
    pred = np.where(rng.rand(n) < 0.6, gt, rng.randint(0, C_, n)).astype(np.int64)
    if drop is not None:
        gt[gt == drop] = 0
    if never is not None:
        pred[pred == never] = 0
    return gt, pred


def check_scores(meter, cm_ref):
    from hsimae_amd import _lib
    out_ref, bound = R.scores_ref(cm_ref)
    out = torch.full((len(out_ref) + 2,), float("nan"), dtype=torch.float64, device=DEV)
    assert _lib.load().hsimae_scores(meter.cm.data_ptr(), meter.num_class, out.data_ptr() + 8, stream()) == 0
    got = out.cpu().numpy()
    assert np.isnan(got[[0, -1]]).all()
    r = R.ratio(got[1:-1], out_ref, bound)
    print(f"[scores C={meter.num_class}] worst err / bound {r:.3f}")
    assert r <= 1.0, (got[1:-1], out_ref)


@pytest.mark.parametrize("n,C_", [(1, 2), (777, 7), (5000, 64), (3000, 65), (100000, 17)])
def test_confusion_counts_are_exact_accumulate_and_feed_the_scores(n, C_):
    from hsimae_amd import ScoreMeter
    gt, pred = labels(n, C_, 1, drop=C_ - 1 if C_ > 3 else None, never=2 if C_ > 3 else None)
    gt2, pred2 = labels(n // 2 + 1, C_, 2)
    m = ScoreMeter(C_, DEV)
    m.update(gt, pred)
    ref, _, bad = R.confusion_ref(gt, pred, C_)
    assert not bad and np.array_equal(m.cm.cpu().numpy(), ref)
    m.update(torch.from_numpy(gt2).to(DEV), torch.from_numpy(pred2).to(DEV))
    ref, _, _ = R.confusion_ref(gt2, pred2, C_, cm=ref)
    assert np.array_equal(m.cm.cpu().numpy(), ref)              # counts accumulate over calls
    check_scores(m, ref)
    if ref[1:].sum():
        from hsimae_amd.finetune_train import scores
        oa, aa, kappa, ca = m.compute()
        h = scores(np.concatenate([gt, gt2]), np.concatenate([pred, pred2]))
        assert abs(oa - h[0]) < 1e-12 and abs(aa - h[1]) < 1e-12 and abs(kappa - h[2]) < 1e-12 and np.allclose(ca, h[3], atol=1e-12, rtol=0)
    m.reset()
    assert not m.cm.any()


def test_scores_of_a_single_class_map_and_an_absent_class():
    from hsimae_amd import ScoreMeter
    from hsimae_amd.finetune_train import scores
    m = ScoreMeter(4, DEV)
    gt = np.full(40, 2)
    m.update(gt, gt)                                           # pe = 1: kappa is 0 by definition
    check_scores(m, R.confusion_ref(gt, gt, 4)[0])
    assert m.compute()[:3] == (1.0, 1.0, 0.0) and scores(gt, gt)[:3] == (1.0, 1.0, 0.0)
    m.reset()
    gt, pred = np.array([1, 1, 3, 3, 0, 0]), np.array([1, 0, 3, 1, 2, 2])      # class 2 absent from gt, a prediction of 0
    m.update(gt, pred)
    check_scores(m, R.confusion_ref(gt, pred, 4)[0])
    oa, aa, kappa, ca = m.compute()
    h = scores(gt, pred)
    assert len(ca) == 2 and (oa, aa) == (h[0], h[1]) and abs(kappa - h[2]) < 1e-15


@pytest.mark.parametrize("hw", [(23, 19), (1, 1)])
def test_map_form_equals_the_vector_form_and_masks(hw):
    from hsimae_amd import ScoreMeter
    H, W = hw
    rng = np.random.RandomState(H)
    C_ = 6
    gt_full = rng.randint(0, C_, (H, W)).astype(np.int64)
    test_gt = np.where(rng.rand(H, W) < 0.5, gt_full, 0)
    pred = rng.randint(1, C_, (H, W)).astype(np.int64)
    if H == 1:
        gt_full[:] = test_gt[:] = 3
    a, b = ScoreMeter(C_, DEV), ScoreMeter(C_, DEV)
    masked = a.update_map(test_gt, torch.from_numpy(pred).to(DEV))
    assert masked.shape == (H, W) and masked.is_cuda
    assert np.array_equal(masked.cpu().numpy(), np.where(test_gt != 0, pred, 0))
    b.update(test_gt.reshape(-1), pred.reshape(-1))
    assert torch.equal(a.cm, b.cm) and int(a.cm.sum()) == int((test_gt != 0).sum())
    # masked by another map than the one that is counted (test_model: zeroed where gt is 0, counted against test_gt)
    c = ScoreMeter(C_, DEV)
    gt_mask = np.where(rng.rand(H, W) < 0.7, gt_full, 0)
    masked = c.update_map(test_gt, pred, mask_map=gt_mask)
    cm, mref, _ = R.confusion_ref(test_gt, pred, C_, mask=gt_mask)
    assert np.array_equal(masked.cpu().numpy().reshape(-1), mref) and np.array_equal(c.cm.cpu().numpy(), cm)


def test_out_of_range_labels_set_the_flag():
    from hsimae_amd import ScoreMeter
    m = ScoreMeter(4, DEV)
    m.update(np.array([1, 2, 4, 3]), np.array([1, 2, 1, 3]))   # gt 4 is not a label of 4 classes
    assert int(m.cm.sum()) == 3
    with pytest.raises(RuntimeError, match="outside"):
        m.compute()
    m.reset()
    m.update(np.array([1, 2]), np.array([1, -1]))
    with pytest.raises(RuntimeError, match="outside"):
        m.compute()
    m.reset()
    m.update(np.array([0, 2]), np.array([9, 2]))               # an unlabeled sample's prediction is not looked at
    assert m.compute()[0] == 1.0


def test_score_meter_in_three_uneven_batches_equals_scores_on_the_concatenation():
    from hsimae_amd import ScoreMeter
    from hsimae_amd.finetune_train import scores
    gt, pred = labels(1000, 10, 5, drop=7)
    m = ScoreMeter(10, DEV)
    for a, e in ((0, 1), (1, 334), (334, 1000)):
        m.update(torch.from_numpy(gt[a:e]).to(DEV), torch.from_numpy(pred[a:e]).to(DEV))
    oa, aa, kappa, ca = m.compute()
    h = scores(gt, pred)
    assert abs(oa - h[0]) < 1e-12 and abs(aa - h[1]) < 1e-12 and abs(kappa - h[2]) < 1e-12
    assert ca.shape == h[3].shape and np.allclose(ca, h[3], atol=1e-12, rtol=0)


# ---------------------------------------------------------------------------------------------- the Python layer
def tiny_dualvit():
    from test_gpu_dualvit import quiet
    from hsimae_amd import DualViT
    torch.manual_seed(0)
    m = quiet(DualViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=64, depth=4, s_depth=2,
              num_heads=4, num_class=4, trunc_init=True, drop_path=0.0, decoder_embed_dim=32, decoder_depth=1,
              decoder_num_heads=4, norm_pix_loss=True)
    with torch.no_grad():
        m.cls_head.weight.normal_(0, 0.5)                      # logits that differ between the rows
    return m.to(DEV).train()


@pytest.mark.parametrize("scale", [None, 0.5])
def test_class_loss_under_the_dualvit_head_against_torch_cross_entropy(scale):
    """Yardstick: F.cross_entropy on the same logits, followed by the same hsimae_head_bwd.  The head's gradients are linear in
    dL/dlogits: gw = g^T pooled, gb = column sums of g, so their bound is the dlogits bound pushed through |pooled| and the
    column sum, plus the fp32 accumulation of the N = 16 products (N U relative to sum |g| |pooled|), once for each of the two runs."""
    from hsimae_amd import ClassLoss
    m = tiny_dualvit()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(16, 1, 32, 9, 9, generator=g).to(DEV)
    y = torch.tensor([0, 1, 2, 3, 1, 0, 2, 3, 3, 1, 0, 2, 1, 2, 3, 1], device=DEV)

    def run(criterion):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        logits = m(x)
        assert logits.stride(0) == 16 and logits.shape == (16, 4)          # the padded view, taken as it is
        loss = criterion(logits, y)
        if scale is None:
            loss.backward()
        else:
            loss.backward(torch.tensor(scale, device=DEV))                  # a device scalar arrives
        return loss.detach(), logits.detach(), m.cls_head.weight.grad.clone(), m.cls_head.bias.grad.clone()

    crit = ClassLoss(ignore_index=0)
    loss, logits, gw, gb = run(crit)
    loss_t, logits_t, gw_t, gb_t = run(lambda z, t: F.cross_entropy(z, t, reduction="mean", ignore_index=0))
    assert torch.equal(logits, logits_t)
    assert torch.equal(crit.last_pred, logits.argmax(1)) and int(crit.last_n_valid) == 13
    crit.check()
    z = np.zeros((16, 16), np.float32)
    z[:, :4] = logits.cpu().numpy()
    ref = R.cls_ref(z, y.cpu().numpy(), 4, ldd=4)
    s = 1.0 if scale is None else scale
    r_loss = R.ratio(loss.item(), ref["loss"], ref["loss_bound"])
    assert r_loss <= 1.0 and R.ratio(loss_t.item(), ref["loss"], ref["loss_bound"]) <= 1.0
    # the saved pooled features: recompute them as the head does
    with torch.no_grad():
        m.eval()
        _, pooled = m.head(m.forward_encoder(x))
        m.train()
    P = pooled.double().cpu().numpy()
    G, GB = s * ref["dlogits"], s * (ref["dlogits_bound"] + R.U * np.abs(ref["dlogits"]))
    gw_ref, gb_ref = G.T @ P, G.sum(0)
    acc = 16 * R.U * (np.abs(G).T @ np.abs(P))
    gw_bound, gb_bound = GB.T @ np.abs(P) + acc, GB.sum(0) + 16 * R.U * np.abs(G).sum(0)
    r_w = R.ratio(gw.double().cpu().numpy(), gw_ref, gw_bound)
    r_b = R.ratio(gb.double().cpu().numpy(), gb_ref, gb_bound)
    r_wt = R.ratio(gw_t.double().cpu().numpy(), gw_ref, gw_bound)
    print(f"[ClassLoss scale={scale}] err / bound: loss {r_loss:.3f}, weight.grad {r_w:.3f} (torch's CE: {r_wt:.3f}), bias.grad {r_b:.3f}")
    assert r_w <= 1.0 and r_b <= 1.0 and r_wt <= 1.0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(logits.cpu(), y.cpu())
    bad = ClassLoss(ignore_index=0)
    bad(logits, torch.full_like(y, 4))
    with pytest.raises(RuntimeError, match="neither ignore_index"):
        bad.check()


def test_class_loss_and_score_meter_launch_without_a_host_wait():
    """ClassLoss forward + backward and ScoreMeter.update under torch's sync debug mode "error": any synchronizing call raises."""
    from hsimae_amd import ClassLoss, ScoreMeter
    z = torch.randn(32, 16, device=DEV)[:, :10].requires_grad_(True)
    y = torch.randint(0, 10, (32,), device=DEV)
    half = torch.tensor(0.5, device=DEV)
    crit, meter = ClassLoss(), ScoreMeter(10, DEV)
    crit(z, y).backward()                                      # first use allocates the flag and the workspace
    torch.cuda.synchronize()
    z.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = crit(z, y)
        (2.0 * loss).backward(half)
        meter.update(y, crit.last_pred)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    ref = F.cross_entropy(z.detach().double(), y, ignore_index=0)
    assert abs(loss.item() - ref.item()) < 1e-5 and z.grad.abs().sum() > 0


def test_finetuning_loop_learns_and_scene_scores_agree(tmp_path):
    """dual_branch_finetuning on the toy set of tests/test_gpu_dualvit.py, on ClassLoss / ScoreMeter: train and validation loss
    fall, OA > 0.8; then test_model and test_model_scene on a scene of the same classes return the same five values."""
    import contextlib
    import io
    from hsimae_amd import dual_branch_finetuning, test_model, test_model_scene
    rng = np.random.default_rng(0)
    n_lab, n_unl, bands, classes = 96, 160, 32, 3
    gt = np.tile(np.arange(1, classes + 1), n_lab // classes)
    ramp = np.linspace(0, 1, bands, dtype=np.float32)

    def spectrum(c):
        return 0.25 + 0.2 * c * ramp if c % 2 else 0.75 - 0.2 * c * ramp

    def cube(c):
        return np.clip(spectrum(c)[None, None, :] + 0.05 * rng.standard_normal((9, 9, bands)).astype(np.float32), 0, 1)

    data_list = [cube(int(c)) for c in gt]
    unlabeled = [cube(int(rng.integers(1, classes + 1))) for _ in range(n_unl)]
    with contextlib.redirect_stdout(io.StringIO()):
        val_value, tr_loss, va_loss = dual_branch_finetuning(
            data_list, list(range(n_lab)), unlabeled, gt, str(tmp_path), "ft.pkl", lr=2e-3, wd=5e-3, depth=4, dim=64,
            dec_depth=1, dec_dim=32, s_depth=2, epochs=8, mask_ratio=0.5, lamda=5, batch_size=16, log=lambda *_: None)
    print(f"[finetune loop] train loss {tr_loss[0]:.3f} -> {tr_loss[-1]:.3f}, val loss {va_loss[0]:.3f} -> {va_loss[-1]:.3f}, "
          f"OA/AA/kappa {val_value[0]:.3f}/{val_value[1]:.3f}/{val_value[2]:.3f}")
    assert tr_loss[-1] < tr_loss[0] and va_loss[-1] < va_loss[0]
    assert val_value[0] > 0.8 and len(val_value) == 4 and isinstance(tr_loss[0], float)
    # a 12 x 10 scene of three vertical stripes, partly unlabeled; the cubes are its symmetric-padded windows
    H, W = 12, 10
    full_gt = np.repeat(np.array([1, 2, 3, 1, 2, 3, 1, 2, 3, 1])[None, :], H, 0)
    scene = np.stack([[np.clip(spectrum(int(full_gt[r, c])) + 0.05 * rng.standard_normal(bands).astype(np.float32), 0, 1)
                       for c in range(W)] for r in range(H)]).astype(np.float32)
    gt_map = full_gt.copy(); gt_map[:2] = 0
    test_gt = gt_map.copy(); test_gt[:, :3] = 0
    padded = np.pad(scene, ((4, 4), (4, 4), (0, 0)), mode="symmetric")
    cubes = [padded[r:r + 9, c:c + 9] for r in range(H) for c in range(W)]
    kw = dict(depth=4, dim=64, s_depth=2)
    with contextlib.redirect_stdout(io.StringIO()):
        a = test_model(cubes, test_gt, gt_map, str(tmp_path), "ft.pkl", **kw)
        b = test_model_scene(scene, test_gt, gt_map, str(tmp_path), "ft.pkl", batch_size=256, **kw)
    print(f"[test_model / _scene] OA {a[0]:.3f} / {b[0]:.3f}")
    assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert a[4].shape == (H, W) and a[4].dtype == np.int64 and a[4].min() >= 1
    from hsimae_amd.finetune_train import scores
    masked = np.where(gt_map != 0, a[4], 0)
    h = scores(test_gt.reshape(-1), masked.reshape(-1))
    assert abs(a[0] - h[0]) < 1e-12 and abs(a[1] - h[1]) < 1e-12 and abs(a[2] - h[2]) < 1e-12 and np.allclose(a[3], h[3], atol=1e-12, rtol=0)
