"""csrc/smooth.hip on the GPU: hsimae_prob_filter against the fp64 restatement and its derived bound (tests/smooth_ref.py) over the
whole case list through the C ABI with guarded buffers, twice bit for bit; the optional outputs; the planted scene; and the Python
layer: EdgeFilter.apply, smooth_classification, scene_guide and test_model_scene(smooth=..)."""
import contextlib
import ctypes as C
import io
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smooth_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
FILL = -7                                                  # what the outputs hold before a call


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def guarded(n, dtype, fill):
    """(whole buffer, the n elements in its middle): GUARD elements of `fill` on either side must survive a call."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def upload(case):
    """The case's inputs on the device, each in a buffer of exactly its size."""
    dev = {k: (None if case[k] is None else torch.from_numpy(np.ascontiguousarray(case[k])).cuda()) for k in ("probs", "row_of", "guide", "scale")}
    return dev


def run_filter(c, case, dev, conf=True, margin=True, probs=True):
    """One call on the current stream -> dict of (whole, inner) buffers: label, conf, margin, probs (or None)."""
    from hsimae_amd import _lib
    H, W, radius, Cc, first, G, form = c
    n, ldo = case["n"], case["ldo"]
    out = {"label": guarded(H * W, torch.int64, FILL), "conf": guarded(H * W, torch.float32, FILL) if conf else None,
           "margin": guarded(H * W, torch.float32, FILL) if margin else None,
           "probs": guarded(n * ldo, torch.float32, FILL) if probs else None}
    ptr = {k: (None if v is None else v[1].data_ptr()) for k, v in out.items()}
    p = _lib.ProbFilterParams(probs=dev["probs"].data_ptr(), ldp=case["ldp"], n=n, C=Cc, first=first, H=H, W=W,
                              row_of=_lib.ptr(dev["row_of"]), guide=_lib.ptr(dev["guide"]), G=max(G, 1), guide_scale=_lib.ptr(dev["scale"]),
                              radius=radius, a_s=case["a_s"], a_r=case["a_r"], out_probs=ptr["probs"], ldo=ldo,
                              label_map=ptr["label"], conf_map=ptr["conf"], margin_map=ptr["margin"])
    _lib.check(_lib.load().hsimae_prob_filter(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_prob_filter")
    return out


def guards_intact(out):
    for k, v in out.items():
        if v is not None:
            whole = v[0].cpu()
            assert (whole[:GUARD] == FILL).all() and (whole[-GUARD:] == FILL).all(), k


def per_pixel(out, ref, n, ldo, Cc):
    """What the call wrote, per pixel -> (out [H W, C], label, conf, margin); pixels without a row must hold the fill value
    in all three maps (they are returned as the restatement's zeros), and so must the pad columns of the probabilities and the rows
    that no pixel points to."""
    has, row = ref["has"], ref["row"]
    lm, cm, mm = (out[k][1].cpu().numpy() for k in ("label", "conf", "margin"))
    assert np.all(lm[~has] == FILL) and np.all(cm[~has] == FILL) and np.all(mm[~has] == FILL)
    pr = out["probs"][1].view(n, ldo).cpu().numpy()
    assert np.all(pr[:, Cc:] == FILL)
    used = np.zeros(n, bool)
    used[row[has]] = True
    assert np.all(pr[~used] == FILL)
    o = np.zeros((has.size, Cc), np.float32)
    o[has] = pr[row[has], :Cc]
    return o, np.where(has, lm, ref["label"]), np.where(has, cm, 0), np.where(has, mm, 0)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_prob_filter_lies_inside_the_bound_of_the_restatement(c):
    H, W, radius, Cc, first, G, form = c
    case = R.make_case(*c)
    ref = R.case_ref(c, case)
    dev = upload(case)
    out = run_filter(c, case, dev)
    guards_intact(out)
    got = per_pixel(out, ref, case["n"], case["ldo"], Cc)
    w = R.worst(got, ref, first)
    print(f"{R.case_id(c)}: err / bound: out {w['out']:.3f}, conf {w['conf']:.3f}, margin {w['margin']:.3f}; labels wrong "
          f"{w['wrong']}, share left open {w['open']:.5f}")
    assert w["zeros"] and w["wrong"] == 0
    assert w["out"] <= 1.0 and w["conf"] <= 1.0 and w["margin"] <= 1.0
    assert w["open"] <= 0.02
    # conf is the filtered probability AT the label that was written, bit for bit
    has = ref["has"]
    assert np.array_equal(got[2][has], got[0][np.flatnonzero(has), got[1][has]])
    again = run_filter(c, case, dev)
    for k in out:
        assert torch.equal(again[k][0].view(torch.int32), out[k][0].view(torch.int32)), k           # bit for bit


def test_optional_outputs_may_be_absent_in_every_combination():
    c = (17, 33, 3, 18, 1, 4, "subset")
    case = R.make_case(*c)
    dev = upload(case)
    full = run_filter(c, case, dev)
    for conf, margin, probs in itertools.product((False, True), repeat=3):
        out = run_filter(c, case, dev, conf=conf, margin=margin, probs=probs)
        guards_intact(out)
        for k in out:
            if out[k] is not None:
                assert torch.equal(out[k][0].view(torch.int32), full[k][0].view(torch.int32)), (k, conf, margin, probs)


def test_every_refusal_returns_its_code_and_writes_nothing():
    from hsimae_amd import _lib
    for what, got, want in R.refusals(_lib.load(), _lib):
        assert got == want, (what, got, want)
    c = (3, 2, 1, 18, 1, 1, "padded")
    case = R.make_case(*c)
    dev = upload(case)
    out = {k: guarded(64, torch.int64 if k == "label" else torch.float32, FILL) for k in ("label", "conf", "margin")}
    p = _lib.ProbFilterParams(probs=dev["probs"].data_ptr(), ldp=case["ldp"], n=6, C=18, first=1, H=3, W=2, guide=dev["guide"].data_ptr(),
                              G=1, guide_scale=dev["scale"].data_ptr(), radius=9, a_s=case["a_s"], a_r=case["a_r"],
                              label_map=out["label"][1].data_ptr(), conf_map=out["conf"][1].data_ptr(),
                              margin_map=out["margin"][1].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.load().hsimae_prob_filter(C.byref(p), stream) == -1                                  # radius 9
    p.radius, p.out_probs, p.ldo = 1, dev["probs"].data_ptr(), case["ldp"]
    assert _lib.load().hsimae_prob_filter(C.byref(p), stream) == -1                                  # in place
    p.out_probs, p.n = None, 0
    assert _lib.load().hsimae_prob_filter(C.byref(p), stream) == 0                                   # no pixel has a row
    torch.cuda.synchronize()
    for k, (whole, _) in out.items():
        assert (whole == FILL).all(), k


def test_the_planted_scene_is_repaired_on_the_device():
    from hsimae_amd import EdgeFilter
    s = R.planted_scene()
    H, W = s["H"], s["W"]
    probs, guide = torch.from_numpy(s["probs"]).cuda(), (torch.from_numpy(s["guide"]).cuda(), torch.from_numpy(s["scale"]).cuda())
    raw = 1 + probs[:, 1:].argmax(1).cpu().numpy()
    assert R.oa(raw, s["truth"]) < 0.8
    res = EdgeFilter(sigma_r=0.1).apply(probs, H, W, guide, return_probs=True)
    assert R.oa(res.labels.cpu().numpy(), s["truth"]) == 1.0
    ref = R.filter_ref(s["probs"], s["C"], 1, H, W, None, s["guide"], s["scale"], 3, R.coef(3.0), R.coef(0.1))
    w = R.worst((res.probs.cpu().numpy(), res.labels.reshape(-1).cpu().numpy(), res.confidence.reshape(-1).cpu().numpy(),
                 res.margin.reshape(-1).cpu().numpy()), ref, 1)
    assert w["all"] <= 1.0 and w["open"] == 0.0
    plain = EdgeFilter(sigma_r=None).apply(probs, H, W, None)
    assert R.oa(plain.labels.cpu().numpy(), s["truth"]) < 1.0
    print(f"planted scene on the device: OA raw {R.oa(raw, s['truth']):.4f}, guided 1.0, unguided "
          f"{R.oa(plain.labels.cpu().numpy(), s['truth']):.4f}; err / bound {w['all']:.3f}")


# ------------------------------------------------------------------ the Python layer
def tiny_dualvit(num_class=6, seed=4):
    from hsimae_amd import DualViT
    torch.manual_seed(seed)
    d = quiet(DualViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=num_class, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, trunc_init=True, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True)
    g = torch.Generator().manual_seed(seed + 8)
    with torch.no_grad():
        for n, p in d.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        d.cls_head.weight.copy_(0.2 * torch.randn(d.cls_head.weight.shape, generator=g))
    return d


def scene_23x19(seed=14):
    return np.random.default_rng(seed).standard_normal((23, 19, 32)).astype(np.float64)


def same(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                        y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_smooth_classification_is_edge_filter_apply_by_hand_and_apply_never_waits():
    from hsimae_amd import EdgeFilter, scene_guide, smooth_classification
    m = tiny_dualvit().cuda().eval()
    scene = torch.from_numpy(scene_23x19()).cuda()
    H, W = 23, 19
    guide = scene_guide(scene)
    assert guide[0].is_cuda and guide[0].dtype == torch.float32 and tuple(guide[0].shape) == (H, W, 1) and tuple(guide[1].shape) == (1,)
    filt = EdgeFilter(radius=2, sigma_s=2.0, sigma_r=0.3)
    for pix in (None, torch.tensor([436, 0, 18, 19, 200, 5, 418, 201, 219, 181])):
        res = m.classify_scene(scene, pixels=pix, batch_size=256, return_probs=True, on_device=True)
        before = [None if t is None else t.clone() for t in res]
        pix_d = None if pix is None else pix.cuda()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            by_hand = filt.apply(res.probs, H, W, guide, pixels=pix_d, first=1, return_probs=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got = smooth_classification(res, guide, pixels=pix, filt=filt, return_probs=True, on_device=True)
        assert all(t.is_cuda for t in got) and same(got, by_hand)
        assert same(res, before)                                                   # the input result is not modified
        host = smooth_classification(res, guide, pixels=pix, filt=filt)
        assert host.probs is None and not host.labels.is_cuda and torch.equal(host.labels, by_hand.labels.cpu())
        # against the restatement, from the device's own inputs
        n = res.probs.shape[0]
        row_of = None
        if pix is not None:
            row_of = np.full(H * W, -1, np.int32)
            row_of[pix.numpy()] = np.arange(n, dtype=np.int32)
        ref = R.filter_ref(res.probs.cpu().numpy(), 6, 1, H, W, row_of, guide[0].cpu().numpy(), guide[1].cpu().numpy(), 2, filt.a_s, filt.a_r)
        o = np.zeros((H * W, 6), np.float32)
        o[ref["has"]] = by_hand.probs.cpu().numpy()[ref["row"][ref["has"]]]
        w = R.worst((o, by_hand.labels.reshape(-1).cpu().numpy(), by_hand.confidence.reshape(-1).cpu().numpy(),
                     by_hand.margin.reshape(-1).cpu().numpy()), ref, 1)
        assert w["all"] <= 1.0, w
        rest = ~ref["has"]
        assert not by_hand.labels.reshape(-1).cpu().numpy()[rest].any() and not by_hand.confidence.reshape(-1).cpu().numpy()[rest].any()
    with pytest.raises(ValueError, match="return_probs=True"):
        smooth_classification(m.classify_scene(scene, batch_size=256, on_device=True), guide)


def test_scene_guide_is_the_leading_principal_components_scaled_to_their_range():
    import gwpca_ref
    from hsimae_amd import GWPCA, as_guide, scene_guide
    raw = gwpca_ref.graded(12, 11, 32, seed=6, group=1)
    ref = gwpca_ref.gwpca_ref(raw, 2, 1, False)
    guide, scale = scene_guide(raw, channels=2)
    assert torch.equal(guide, GWPCA(nc=2, group=1, whiten=False).fit_transform(raw, dtype=torch.float32))
    g = guide.cpu().numpy()
    err = gwpca_ref.component_err(g, ref["out"])
    lim = ref["bound"] + R.U * np.abs(ref["out"]).reshape(-1, 2).max(0)           # GWPCA's own bound + the rounding to fp32
    print(f"scene_guide: worst err / bound vs the GWPCA restatement {np.max(err / lim):.3f}")
    assert np.all(err <= lim)
    span = g.reshape(-1, 2).max(0) - g.reshape(-1, 2).min(0)
    assert np.all(np.abs(scale.cpu().numpy().astype(np.float64) * span - 1.0) <= 4 * R.U)      # one division on the device
    # an explicit guide goes through the same scaling; a constant channel gets scale 0
    bands = np.ascontiguousarray(raw[..., [3, 17]].astype(np.float32))
    bands[..., 1] = 2.5
    eg, es = as_guide(bands)
    assert torch.equal(eg.cpu(), torch.from_numpy(bands)) and es[1].item() == 0.0
    assert abs(es[0].item() * float(bands[..., 0].max() - bands[..., 0].min()) - 1.0) <= 4 * R.U


def test_test_model_scene_with_smoothing_scores_its_own_map_and_none_changes_nothing(tmp_path):
    from hsimae_amd import EdgeFilter, label_to_colormap, scene_guide, test_model_scene
    from hsimae_amd.finetune_train import scores
    import prob_ref
    d = tiny_dualvit()
    torch.save(d.state_dict(), os.path.join(tmp_path, "ft.pkl"))
    rng = np.random.default_rng(13)
    scene = scene_23x19()
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    test_gt = gt.copy()
    test_gt[rng.random(gt.shape) < 0.3] = 0
    kw = dict(depth=3, dim=32, s_depth=2, batch_size=256)
    base = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "ft.pkl", **kw)
    none = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "ft.pkl", smooth=None, **kw)
    assert base[:3] == none[:3] and np.array_equal(base[3], none[3]) and np.array_equal(base[4], none[4])
    assert not os.path.exists(os.path.join(tmp_path, "ft"))
    out = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "ft.pkl", smooth=True, save_images=True, **kw)
    assert out[4].shape == gt.shape and out[4].dtype == np.int64 and out[4].min() >= 1
    want = scores(test_gt.reshape(-1), np.where(gt == 0, 0, out[4]).reshape(-1))
    assert max(abs(a - b) for a, b in zip(out[:3], want[:3])) <= 1e-12 and np.abs(out[3] - want[3]).max() <= 1e-12
    tag = str(np.around(out[0] * 100, 2))
    folder = os.path.join(tmp_path, "ft")
    assert sorted(os.listdir(folder)) == sorted([f"ft_all_oa_{tag}.png", f"ft_oa_{tag}.png"])
    whole = prob_ref.decode_png(open(os.path.join(folder, f"ft_all_oa_{tag}.png"), "rb").read())
    masked = prob_ref.decode_png(open(os.path.join(folder, f"ft_oa_{tag}.png"), "rb").read())
    assert np.array_equal(whole, label_to_colormap(out[4])) and np.array_equal(masked, label_to_colormap(np.where(gt == 0, 0, out[4])))
    # the map is the default filter on classify_scene's probabilities, guided by the scene's first principal component
    from hsimae_amd import HSIViT
    v = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=6, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, sep_pos_embed=True, use_learnable_pos_emb=False).cuda()
    sd = v.state_dict()
    sd.update({k: t for k, t in torch.load(os.path.join(tmp_path, "ft.pkl"), map_location="cuda").items() if k in sd})
    v.load_state_dict(sd)
    v.eval()
    sc = torch.from_numpy(scene).cuda()
    res = v.classify_scene(sc, batch_size=256, return_probs=True, on_device=True)
    by_hand = EdgeFilter().apply(res.probs, 23, 19, scene_guide(sc))
    assert np.array_equal(out[4], by_hand.labels.cpu().numpy())
    assert not np.array_equal(out[4], base[4])                                     # (the filter did change this map)


def test_knn_and_probe_evaluations_take_the_same_option(tmp_path):
    """knn_eval_scene and linear_probe_scene with smooth=: None is the call without it, bit for bit; a filter (with and without
    range term) changes the map, and the scores returned are the scores of the map returned."""
    from hsimae_amd import EdgeFilter, knn_eval_scene, linear_probe_scene
    from hsimae_amd.finetune_train import scores
    d = tiny_dualvit()
    ckpt = os.path.join(tmp_path, "ft.pkl")
    torch.save(d.state_dict(), ckpt)
    rng = np.random.default_rng(13)
    scene = scene_23x19()
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    flat = gt.reshape(-1)
    train_index = np.flatnonzero((flat != 0) & (rng.random(437) < 0.3))
    train_labels = flat[train_index]
    test_gt = gt.copy()
    test_gt.reshape(-1)[train_index] = 0
    kw = dict(depth=3, dim=32, s_depth=2, batch_size=256)
    for fn, extra in ((knn_eval_scene, dict(k=5)), (linear_probe_scene, dict(max_iter=10))):
        base = quiet(fn, scene, train_index, train_labels, test_gt, gt, ckpt, **kw, **extra)
        none = quiet(fn, scene, train_index, train_labels, test_gt, gt, ckpt, smooth=None, **kw, **extra)
        assert base[:3] == none[:3] and np.array_equal(base[4], none[4])
        for filt in (EdgeFilter(radius=2), EdgeFilter(radius=2, sigma_r=None)):
            out = quiet(fn, scene, train_index, train_labels, test_gt, gt, ckpt, smooth=filt, **kw, **extra)
            assert out[4].shape == gt.shape and out[4].min() >= 1 and not np.array_equal(out[4], base[4])
            want = scores(test_gt.reshape(-1), np.where(gt == 0, 0, out[4]).reshape(-1))
            assert max(abs(a - b) for a, b in zip(out[:3], want[:3])) <= 1e-12 and np.abs(out[3] - want[3]).max() <= 1e-12
    with pytest.raises(TypeError):
        knn_eval_scene(scene, train_index, train_labels, test_gt, gt, ckpt, smooth="yes", **kw)
