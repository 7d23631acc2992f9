"""csrc/probe.hip on the device against tests/probe_ref.py: every stage of hsimae_probe_prepare / hsimae_probe_step through the C ABI
inside the bound of the fp64 restatement at the tile and segment edges, a 20-step trajectory, bit-identical repeats, the planted
clusters, the folded head inside the model, probe_scene and linear_probe_scene end to end, and refusals that write nothing."""
import contextlib
import ctypes as C
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import probe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
FILL = -7


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def guarded(n, dtype, fill=FILL):
    """(whole buffer, the n elements in its middle): GUARD elements of `fill` on either side must survive a call."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def intact(whole, fill=FILL):
    w = whole.cpu()
    return bool((w[:GUARD] == fill).all() and (w[-GUARD:] == fill).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_prepare(x, y, D, Cc, first, ldn=None):
    """x fp32 [n, ldx], y int64 [n] (host) -> dict of guarded device buffers after hsimae_probe_prepare."""
    from hsimae_amd import _lib
    n, ldx = x.shape
    Kp, ldn = D + 4, ldn or R.rup4(n)
    b = {"x": dev(x), "y": dev(y), "n": n, "Kp": Kp, "ldn": ldn}
    for key, size, dt in (("mean", D, torch.float32), ("rstd", D, torch.float32), ("xs", n * Kp, torch.float32),
                          ("xt", Kp * ldn, torch.float32), ("state", 8, torch.float64)):
        b[key + "_whole"], b[key] = guarded(size, dt)
    p = _lib.ProbePrepareParams(x=b["x"].data_ptr(), ldx=ldx, labels=b["y"].data_ptr(), n=n, D=D, C=Cc, first=first, eps=R.BN_EPS,
                                mean=b["mean"].data_ptr(), rstd=b["rstd"].data_ptr(), xs=b["xs"].data_ptr(), Kp=Kp,
                                xt=b["xt"].data_ptr(), ldn=ldn, state=b["state"].data_ptr())
    _lib.check(_lib.load().hsimae_probe_prepare(C.byref(p), stream()), "hsimae_probe_prepare")
    return b


def host_pre(b):
    n, Kp, ldn = b["n"], b["Kp"], b["ldn"]
    st = b["state"].cpu().numpy()
    return {"mean": b["mean"].cpu().numpy(), "rstd": b["rstd"].cpu().numpy(), "xs": b["xs"].view(n, Kp).cpu().numpy(),
            "xt": b["xt"].view(Kp, ldn).cpu().numpy(), "state": st.copy(), "bad": int(st[3]), "nv": int(st[4])}


def run_step(b, w, m, v, D, Cc, first, step, lr, hp, hist_len=None):
    """One hsimae_probe_step on the prepared buffers `b` from host w, m, v [64, Kp] -> dict of host arrays."""
    from hsimae_amd import _lib
    n, Kp, ldn = b["n"], b["Kp"], b["ldn"]
    S = (n + R.SEG - 1) // R.SEG
    o = {}
    for key, arr in (("w", w), ("m", m), ("v", v)):
        o[key + "_whole"], o[key] = guarded(R.ROWS * Kp, torch.float32)
        o[key].copy_(dev(arr).view(-1))
    for key, size, dt in (("gt", R.ROWS * ldn, torch.float32), ("scratch", S * R.ROWS * Kp, torch.float32),
                          ("loss_part", (n + 63) // 64, torch.float64), ("norm_part", (R.ROWS * Kp + 255) // 256, torch.float64),
                          ("hist", hist_len or step, torch.float32)):
        o[key + "_whole"], o[key] = guarded(size, dt)
    p = _lib.ProbeStepParams(xs=b["xs"].data_ptr(), xt=b["xt"].data_ptr(), Kp=Kp, ldn=ldn, labels=b["y"].data_ptr(), n=n, D=D, C=Cc,
                             first=first, w=o["w"].data_ptr(), m=o["m"].data_ptr(), v=o["v"].data_ptr(), gt=o["gt"].data_ptr(),
                             scratch=o["scratch"].data_ptr(), loss_part=o["loss_part"].data_ptr(), norm_part=o["norm_part"].data_ptr(),
                             lr=lr, weight_decay=hp["wd"], b1=hp["b1"], b2=hp["b2"], eps=hp["eps"], step=step,
                             state=b["state"].data_ptr(), loss_hist=o["hist"].data_ptr())
    _lib.check(_lib.load().hsimae_probe_step(C.byref(p), stream()), "hsimae_probe_step")
    got = {key: o[key].view(R.ROWS, Kp).cpu().numpy() for key in ("w", "m", "v")}
    got.update(gt=o["gt"].view(R.ROWS, ldn).cpu().numpy(), scratch=o["scratch"].view(S, R.ROWS, Kp).cpu().numpy(),
               state=b["state"].cpu().numpy(), hist=o["hist"].cpu().numpy(),
               intact=all(intact(o[k + "_whole"]) for k in ("w", "m", "v", "gt", "scratch", "loss_part", "norm_part", "hist")))
    return got


def run_logits(x, mean, rstd, w, D, Cc, first, ldz):
    from hsimae_amd import _lib
    n, ldx = x.shape
    xd, md, rd, wd = dev(x), dev(mean), dev(rstd), dev(w)
    zw, z = guarded(n * ldz, torch.float32)
    p = _lib.ProbeLogitsParams(x=xd.data_ptr(), ldx=ldx, mean=md.data_ptr(), rstd=rd.data_ptr(), w=wd.data_ptr(), Kp=D + 4, n=n, D=D,
                               C=Cc, first=first, z=z.data_ptr(), ldz=ldz)
    _lib.check(_lib.load().hsimae_probe_logits(C.byref(p), stream()), "hsimae_probe_logits")
    return zw, z.view(n, ldz).cpu().numpy()


def run_fold(w, mean, rstd, D, Cc, first, ldw):
    from hsimae_amd import _lib
    wd, md, rd = dev(w), dev(mean), dev(rstd)
    Ww, W = guarded(Cc * ldw, torch.float32)
    bw, b = guarded(Cc, torch.float32)
    p = _lib.ProbeFoldParams(w=wd.data_ptr(), Kp=D + 4, mean=md.data_ptr(), rstd=rd.data_ptr(), D=D, C=Cc, first=first,
                             weight=W.data_ptr(), ldw=ldw, bias=b.data_ptr())
    _lib.check(_lib.load().hsimae_probe_fold(C.byref(p), stream()), "hsimae_probe_fold")
    return Ww, W.view(Cc, ldw).cpu().numpy(), bw, b.cpu().numpy()


# ------------------------------------------------------------------ every stage through the C ABI
@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("D", R.DS)
def test_every_stage_lies_inside_the_bound_of_the_restatement(n, D):
    for ci, (Cc, first) in enumerate(R.CLASSES):
        pad = 4 * ((ci + n) % 3)                               # ldx = D, D + 4, D + 8; ldn and ldz padded with it
        x, y, w, m, v = R.step_case(n, D, Cc, first, ldx=D + pad, seed=ci)
        b = run_prepare(x, y, D, Cc, first, ldn=R.rup4(n) + pad)
        pre = host_pre(b)
        cp = R.check_prepare(pre, x, y, D, Cc, first)
        assert cp["ok"] and all(intact(b[k + "_whole"]) for k in ("mean", "rstd", "xs", "xt", "state")), (Cc, first, cp)
        if n >= 4:
            assert pre["bad"] == 1 and not pre["xs"][2].any() and not pre["xt"][:, 2].any()      # the bad label: counted, its row inert
        if D > 1 and pre["nv"]:
            assert not pre["xs"][:, 1].any() and pre["rstd"][1] == np.float32(1 / math.sqrt(R.f32(R.BN_EPS)))    # the constant column
        got = run_step(b, w, m, v, D, Cc, first, 3, R.HP["lr"], R.HP)
        cs = R.check_step(got, pre, y, w, m, v, D, Cc, first, 3, R.HP["lr"], R.HP)
        print(f"n {n} D {D} C {Cc} first {first}: " + " ".join(f"{k} {cs[k]:.3f}" for k in ("g", "loss", "scratch", "w", "m", "v", "norm")))
        assert cs["ok"] and got["intact"], (Cc, first, cs)
        assert got["hist"][2] == np.float32(got["state"][0]) and (got["hist"][:2] == FILL).all()     # loss_hist[step - 1] alone
        live = R.groups_of(D, D + 4, Cc, first).numpy() != 2
        for key, was in (("w", w), ("m", m), ("v", v)):        # rows outside [first, C) and the columns behind D: never written
            assert np.array_equal(got[key][~live], was[~live])
        g = got["gt"][:, :R.rup4(n)]
        ok = R.valid_of(y, first, Cc)
        assert not g[:first].any() and not g[Cc:].any() and not g[:, n:].any() and not g[:, :n][:, ~ok].any()
        assert (got["gt"][:, R.rup4(n):] == FILL).all()
        if Cc - first >= 3:                                     # the class without a member is trained all the same: p / nv > 0
            assert (g[Cc - 1, :n][ok] > 0).all()
        # the logits of the bank rows equal the forward's, and the fold reproduces them
        ldz = Cc + pad // 4
        zw, z = run_logits(x, pre["mean"], pre["rstd"], w, D, Cc, first, ldz)
        zref = R.forward_ref(R.operands(x[:, :D], np.ones(n, bool), pre["mean"], pre["rstd"])["xs"], w, y, first, Cc)
        assert intact(zw) and (z[:, Cc:] == FILL).all() and not z[:, :first].any() and np.isfinite(z[:, :Cc]).all()
        assert R.ratio(z[:, first:Cc], zref["z"][:, first:], zref["z_bound"][:, first:]) <= 1
        Ww, W, bw, bias = run_fold(w, pre["mean"], pre["rstd"], D, Cc, first, D + pad)
        W64, Wb, b64, bb = R.fold_ref(w, pre["mean"], pre["rstd"], D, Cc, first)
        assert intact(Ww) and intact(bw) and (W[:, D:] == FILL).all() and not W[:first, :D].any() and not bias[:first].any()
        assert R.ratio(W[:, :D], W64, Wb) <= 1 and R.ratio(bias, b64, bb) <= 1


def test_more_segments_than_one_pass_and_a_one_row_last_segment():
    """n = 1025: five segments, the last of one row (a chain of 4 with three zeros), 17 forward tiles."""
    n, D, Cc, first = 1025, 8, 5, 1
    x, y, w, m, v = R.step_case(n, D, Cc, first, seed=3)
    b = run_prepare(x, y, D, Cc, first)
    pre = host_pre(b)
    assert R.check_prepare(pre, x, y, D, Cc, first)["ok"]
    got = run_step(b, w, m, v, D, Cc, first, 1, R.HP["lr"], R.HP)
    cs = R.check_step(got, pre, y, w, m, v, D, Cc, first, 1, R.HP["lr"], R.HP)
    assert cs["ok"] and got["intact"] and got["scratch"].shape[0] == 5 and got["scratch"][4].any(), cs


# ------------------------------------------------------------------ the fit
def fit_on_device(x, y, Cc, first, T, hp, schedule="cosine"):
    from hsimae_amd import LinearProbe
    p = LinearProbe(Cc, first=first, max_iter=T, lr=hp["lr"], weight_decay=hp["wd"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"],
                    schedule=schedule)
    return p.fit(dev(x), dev(y))


def test_trajectory_of_20_steps_against_the_restatement():
    x, y = R.traj_case()
    D, Cc, first, T = 36, 8, 1, R.TRAJ_STEPS
    f = R.fit_ref(x, y, D, Cc, first, T, R.TRAJ_HP)
    e = R.emulate_fit(x, y, D, Cc, first, T, R.TRAJ_HP)
    gate = R.TRAJ_MARGIN * np.abs(e["w"][:Cc, :D + 1].astype(np.float64) - f["w"]).max()      # from the CPU emulation alone
    p = fit_on_device(x, y, Cc, first, T, R.TRAJ_HP)
    w = p.w.cpu().numpy()
    err = np.abs(w[:Cc, :D + 1].astype(np.float64) - f["w"]).max()
    hist = p.loss_history.cpu().numpy().astype(np.float64)
    print(f"device off the restatement by {err:.3g}, gate {gate:.3g} ({err / gate:.3f} of it); loss {hist[0]:.4f} -> {hist[-1]:.4f}")
    assert err <= gate and not w[Cc:].any() and not w[:first].any() and not w[:, D + 1:].any()
    # the start is uniform: every row's loss is log(sum of C - first ones) = ln(C - first), rounded once to fp32 for the history
    assert abs(hist[0] - math.log(Cc - first)) <= 2 * R.U * math.log(Cc - first) and hist[-1] < hist[0]
    loss_gate = R.TRAJ_MARGIN * np.abs(e["losses"] - f["losses"]).max() + R.U * f["losses"].max()
    assert np.abs(hist - f["losses"]).max() <= loss_gate
    assert float(p.grad_norm) == math.sqrt(p._state[2].item()) and float(p.loss) == p._state[0].item()
    assert p._state.cpu().tolist()[1] == T and p._state.cpu().tolist()[3:5] == [0, len(y)]
    p.check()


def test_two_fits_are_bit_identical_and_the_row_order_is_real():
    x, y = R.traj_case(n=600, D=32, seed=1)
    a, b = (fit_on_device(x, y, 8, 1, 10, R.TRAJ_HP) for _ in range(2))
    assert torch.equal(bits(a.w), bits(b.w)) and torch.equal(bits(a.loss_history), bits(b.loss_history))
    assert torch.equal(a._state, b._state) and torch.equal(bits(a.mean), bits(b.mean)) and torch.equal(bits(a.rstd), bits(b.rstd))
    perm = np.random.RandomState(2).permutation(600)
    c = fit_on_device(x[perm], y[perm], 8, 1, 10, R.TRAJ_HP)
    assert not torch.equal(bits(a.w), bits(c.w))                                          # the sums have an order


def test_planted_clusters_every_query_right():
    from hsimae_amd import LinearProbe
    bank, by, qs, qy = R.clusters()                          # 7 classes, D = 32, 140 bank rows, 1000 queries
    p = LinearProbe(8).fit(dev(bank), dev(by))
    lab = p.predict(dev(qs))
    z = p.logits(dev(qs)).cpu().numpy()
    hist = p.loss_history.cpu().numpy()
    top = np.sort(z[:, 1:], axis=1)
    print(f"loss {hist[0]:.4f} -> {hist[-1]:.4f}, smallest top-1/top-2 gap {(top[:, -1] - top[:, -2]).min():.3f}")
    assert lab.is_cuda and lab.dtype == torch.int64 and np.array_equal(lab.cpu().numpy(), qy)
    assert np.array_equal(1 + np.argmax(z[:, 1:], axis=1), qy) and not z[:, 0].any()
    assert abs(hist[0] - math.log(7)) <= 2 * R.U * math.log(7) and hist[-1] < hist[0]
    p.check()
    bad = by.copy()
    bad[5] = 0                                               # "unlabelled" in the bank: counted, and check() says so
    q = LinearProbe(8, max_iter=2).fit(dev(bank), dev(bad))
    with pytest.raises(RuntimeError, match="1 bank labels"):
        q.check()
    for args in ((dev(bank), dev(by[:-1])), (dev(bank)[:, :30], dev(by)), (dev(bank).double(), dev(by))):
        with pytest.raises((ValueError, TypeError)):
            LinearProbe(8).fit(*args)
    with pytest.raises(ValueError):
        p.logits(dev(qs)[:, :28])


# ------------------------------------------------------------------ the head in the model, probe_scene, linear_probe_scene
def tiny_hsivit(num_class=7, seed=0):
    """tests/test_gpu_knn.py's tiny model, built here: same shape, same seeds."""
    from hsimae_amd import HSIViT
    torch.manual_seed(seed)
    m = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=num_class, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, trunc_init=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    return m.cuda().eval()


def scene_23x19(seed=5, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((23, 19, 32)).astype(dtype)


def teacher_labels(feats, n_class, seed):
    """Labels 1 .. n_class - 1 a linear classifier can learn: the argmax of a random linear map of the standardised features."""
    f = feats.cpu().numpy().astype(np.float64)
    f = (f - f.mean(0)) / (f.std(0) + 1e-6)
    return 1 + np.argmax(f @ np.random.default_rng(seed).standard_normal((f.shape[1], n_class - 1)), axis=1)


def test_folded_head_in_the_model_agrees_with_the_probe():
    from hsimae_amd import LinearProbe
    m = tiny_hsivit(seed=2)
    scene = scene_23x19(seed=6)
    feats = m.scene_features(scene, batch_size=256)
    y = teacher_labels(feats, 7, seed=11)
    p = LinearProbe(7).fit(feats, dev(y))
    z = p.logits(feats).cpu().numpy().astype(np.float64)
    W, b = p.head()
    with torch.no_grad():
        m.cls_head.weight.copy_(W)
        m.cls_head.bias.copy_(b)
    lab, head_z = m.predict_scene(scene, batch_size=256, return_logits=True)
    bound = R.head_bound(feats.cpu().numpy(), W.cpu().numpy(), b.cpu().numpy())
    # z is the fp32 chain on the standardised rows, the head the folded product of raw rows: both within their bounds of the fp64
    # value of the folded head, whose own distance from z's fp64 value is the fold's rounding (U per weight: inside 2 UB)
    f64 = feats.cpu().numpy().astype(np.float64) @ W.cpu().numpy().astype(np.float64).T + b.cpu().numpy().astype(np.float64)
    x32 = feats.cpu().numpy()
    xs = R.operands(x32, np.ones(len(x32), bool), p.mean.cpu().numpy(), p.rstd.cpu().numpy())["xs"].astype(np.float64)
    # the probe's own logits against that product: the chain, the two roundings of every standardised feature, the fold's roundings
    zb = (R.gamma(xs.shape[1]) + 2 * R.U) * (np.abs(xs) @ np.abs(p.w.cpu().numpy()[:7].astype(np.float64)).T) + \
        R.U * (np.abs(x32.astype(np.float64)) @ np.abs(W.cpu().numpy().astype(np.float64)).T + np.abs(b.cpu().numpy().astype(np.float64)))
    worst = R.ratio(head_z.numpy()[:, 1:], f64[:, 1:], bound[:, 1:])
    both = R.ratio(head_z.numpy()[:, 1:], z[:, 1:], (bound + zb)[:, 1:])
    top = np.sort(z[:, 1:], axis=1)
    two = np.argsort(-z[:, 1:], axis=1)[:, :2] + 1
    rows = np.arange(z.shape[0])
    decided = top[:, -1] - top[:, -2] > 2 * (bound[rows, two[:, 0]] + bound[rows, two[:, 1]])
    print(f"head against the folded fp64 product {worst:.3f} of the bf16 bound, against the probe's logits {both:.3f}; "
          f"decided {decided.mean():.3f}, bound up to {bound[:, 1:].max():.3g}, gaps from {(top[:, -1] - top[:, -2]).min():.3g}")
    assert worst <= 1 and both <= 1
    assert decided.mean() >= 0.95
    res = m.classify_scene(scene, batch_size=256, views=(0,))
    want = 1 + np.argmax(z[:, 1:], axis=1)
    assert np.array_equal(res.labels.numpy().reshape(-1)[decided], want[decided])
    assert np.array_equal(lab.reshape(-1), res.labels.numpy().reshape(-1))


def test_probe_scene_is_the_composition_by_hand_bit_for_bit():
    from hsimae_amd import LinearProbe
    from hsimae_amd.finetune import SceneClassification
    scene = scene_23x19(seed=6)
    rng = np.random.default_rng(3)
    bank_pix = rng.choice(437, 90, replace=False)
    sub = rng.permutation(437)[:300]
    m, hand = tiny_hsivit(seed=2), tiny_hsivit(seed=2)
    bank_y = teacher_labels(hand.scene_features(scene, bank_pix, 256), 7, seed=12)
    kw = dict(max_iter=30, lr=2e-2)
    res = m.probe_scene(scene, bank_pix, bank_y, pixels=sub, batch_size=256, return_probs=True, **kw)
    assert isinstance(res, SceneClassification) and not res.labels.is_cuda and tuple(res.labels.shape) == (23, 19)
    p = LinearProbe(7, **kw).fit(hand.scene_features(scene, bank_pix, 256), dev(bank_y))
    W, b = p.head()
    with torch.no_grad():
        hand.cls_head.weight.copy_(W)
        hand.cls_head.bias.copy_(b)
    want = hand.classify_scene(scene, sub, batch_size=256, return_probs=True)
    for got, ref in zip(res, want):
        assert torch.equal(got, ref)
    lp = m.last_probe
    assert torch.equal(bits(lp.w), bits(p.w)) and torch.equal(bits(m.cls_head.weight.detach()), bits(W)) and lp.max_iter == 30
    assert torch.equal(bits(m.cls_head.bias.detach()), bits(b)) and float(lp.loss_history[-1]) < float(lp.loss_history[0])
    asked = np.zeros(437, bool)
    asked[sub] = True
    assert res.labels.reshape(-1)[asked].min() >= 1 and (res.labels.reshape(-1)[~asked] == 0).all()
    # on the device, all pixels, two bank views, two classification views
    d = m.probe_scene(torch.from_numpy(scene).cuda(), bank_pix, bank_y, bank_flips=(0, 3), views=(0, 1), batch_size=256, on_device=True,
                      max_iter=5)
    assert d.probs is None and all(t.is_cuda for t in d[:3]) and int(d.labels.min()) >= 1
    assert tuple(m.last_probe.loss_history.shape) == (5,) and int(m.last_probe._state[4].item()) == 180
    with pytest.raises(ValueError):
        m.probe_scene(scene, bank_pix, bank_y[:-1])
    with pytest.raises(ValueError):
        m.probe_scene(scene, bank_pix, bank_y, bank_flips="all")
    with pytest.raises(RuntimeError, match="bank labels"):
        m.probe_scene(scene, bank_pix, np.where(np.arange(90) == 4, 9, bank_y), max_iter=2)


def test_linear_probe_scene_scores_its_own_map_and_its_checkpoint_reloads(tmp_path):
    from hsimae_amd import HSIMAE, DualViT, HSIViT, linear_probe_scene, test_model_scene
    from hsimae_amd.finetune_train import scores
    kw = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=32, depth=3, num_heads=2, s_depth=2,
              trunc_init=True, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True)
    torch.manual_seed(4)
    d = quiet(DualViT, num_class=6, **kw)
    torch.manual_seed(5)
    mae = quiet(HSIMAE, **kw)
    torch.save(d.state_dict(), os.path.join(tmp_path, "ft.pkl"))
    torch.save(mae.state_dict(), os.path.join(tmp_path, "mae.pkl"))
    rng = np.random.default_rng(13)
    scene = scene_23x19(seed=14)
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    flat = gt.reshape(-1)
    train_index = np.flatnonzero((flat != 0) & (rng.random(437) < 0.3))
    train_labels = flat[train_index]
    test_gt = gt.copy()
    test_gt.reshape(-1)[train_index] = 0
    args = dict(depth=3, dim=32, s_depth=2, batch_size=256, max_iter=25)
    maps = {}
    for name in ("ft.pkl", "mae.pkl"):
        out = quiet(linear_probe_scene, scene, train_index, train_labels, test_gt, gt, os.path.join(tmp_path, name),
                    save_dir=str(tmp_path), **args)
        oa, aa, kappa, ca, pred = out
        assert pred.shape == gt.shape and pred.dtype == np.int64 and pred.min() >= 1 and pred.max() <= 5
        want = scores(test_gt.reshape(-1), np.where(gt == 0, 0, pred).reshape(-1))
        assert abs(oa - want[0]) <= 1e-12 and abs(aa - want[1]) <= 1e-12 and abs(kappa - want[2]) <= 1e-12
        assert np.allclose(ca, want[3], rtol=0, atol=1e-12)
        stem = name.replace(".pkl", "")
        sd = torch.load(os.path.join(tmp_path, stem + "_probe.pkl"), map_location="cpu")
        v = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=6, embed_dim=32, depth=3,
                  num_heads=2, s_depth=2, sep_pos_embed=True, use_learnable_pos_emb=False)
        assert list(sd) == list(v.state_dict()) and not sd["cls_head.weight"][0].any() and sd["cls_head.weight"][1:].any()
        v.load_state_dict(sd)                                                            # every key, every shape
        again = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), stem + "_probe.pkl", depth=3, dim=32, s_depth=2,
                      batch_size=256)
        assert np.array_equal(again[4], pred) and again[:3] == out[:3]
        maps[name] = pred
    assert not np.array_equal(maps["ft.pkl"], maps["mae.pkl"])                           # two encoders, two maps
    with pytest.raises(ValueError):
        linear_probe_scene(scene, train_index, train_labels, test_gt, gt, os.path.join(tmp_path, "ft.pkl"), save_images=True, **args)


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    from hsimae_amd import _lib
    lib = _lib.load()
    for what, got, want in R.refusals(lib, _lib):
        assert got == want, (what, got, want)
    n, D, Cc = 30, 12, 8
    x, y, w, m, v = R.step_case(n, D, Cc, 1)
    xd, yd = dev(x), dev(y)
    bufs = {k: guarded(size, dt) for k, size, dt in (("mean", D, torch.float32), ("rstd", D, torch.float32), ("xs", n * 16, torch.float32),
                                                      ("xt", 16 * 32, torch.float32), ("state", 8, torch.float64),
                                                      ("w", 64 * 16, torch.float32), ("gt", 64 * 32, torch.float32),
                                                      ("scratch", 64 * 16, torch.float32), ("part", 8, torch.float64),
                                                      ("z", n * Cc, torch.float32))}
    ptr = {k: t[1].data_ptr() for k, t in bufs.items()}
    pp = dict(x=xd.data_ptr(), ldx=D, labels=yd.data_ptr(), n=n, D=D, C=Cc, first=1, eps=1e-6, mean=ptr["mean"], rstd=ptr["rstd"],
              xs=ptr["xs"], Kp=16, xt=ptr["xt"], ldn=32, state=ptr["state"])
    for kw, code in ((dict(C=65), -2), (dict(eps=0.0), -1), (dict(ldn=28), -1), (dict(n=0), 0)):
        assert lib.hsimae_probe_prepare(C.byref(_lib.ProbePrepareParams(**dict(pp, **kw))), stream()) == code
    sp = dict(xs=ptr["xs"], xt=ptr["xt"], Kp=16, ldn=32, labels=yd.data_ptr(), n=n, D=D, C=Cc, first=1, w=ptr["w"], m=ptr["w"], v=ptr["w"],
              gt=ptr["gt"], scratch=ptr["scratch"], loss_part=ptr["part"], norm_part=ptr["part"], lr=0.01, weight_decay=1e-4, b1=0.9,
              b2=0.999, eps=1e-8, step=1, state=ptr["state"], loss_hist=None)
    for kw, code in ((dict(step=0), -1), (dict(b1=1.0), -1), (dict(C=65), -2), (dict(gt=None), -4), (dict(n=0), 0)):
        assert lib.hsimae_probe_step(C.byref(_lib.ProbeStepParams(**dict(sp, **kw))), stream()) == code
    lp = dict(x=xd.data_ptr(), ldx=D, mean=ptr["mean"], rstd=ptr["rstd"], w=ptr["w"], Kp=16, n=n, D=D, C=Cc, first=1, z=ptr["z"], ldz=Cc)
    for kw, code in ((dict(ldz=7), -1), (dict(first=8), -1), (dict(n=0), 0)):
        assert lib.hsimae_probe_logits(C.byref(_lib.ProbeLogitsParams(**dict(lp, **kw))), stream()) == code
    fp = dict(w=ptr["w"], Kp=16, mean=ptr["mean"], rstd=ptr["rstd"], D=D, C=Cc, first=1, weight=ptr["xs"], ldw=D, bias=ptr["z"])
    for kw, code in ((dict(ldw=8), -1), (dict(Kp=12), -1), (dict(bias=None), -4)):
        assert lib.hsimae_probe_fold(C.byref(_lib.ProbeFoldParams(**dict(fp, **kw))), stream()) == code
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        assert (whole == FILL).all(), k
