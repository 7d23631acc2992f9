"""csrc/prob.hip on the GPU: hsimae_class_prob against the fp64 restatement and its derived bound (tests/prob_ref.py) over the
whole case list, with one view bit-identical to hsimae_class_argmax; DualViT.classify_scene against predict_scene and against
HSIViT.forward on flipped windows; test_model_scene with flip views and the reference's two pictures."""
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
import prob_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8
STALE, FILL = 0.5, -7                                      # what acc / the outputs hold before a call


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def guarded(n, dtype, fill):
    """(whole buffer, the n elements in its middle): GUARD elements of `fill` on either side must survive a call."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def run_prob(zs, Cc, first, H, W, p0=0, pixels=None, lda=None, ldp=None, conf=True, margin=True, probs=True):
    """One call per view on the current stream -> dict of (whole, inner) buffers: acc, label, conf, margin, probs (or None)."""
    from hsimae_amd import _lib
    V, N, ld = zs.shape
    lda, ldp = lda or Cc + 3, ldp or Cc + 5
    out = {"acc": guarded(N * lda, torch.float32, STALE), "label": guarded(H * W, torch.int64, FILL),
           "conf": guarded(H * W, torch.float32, FILL) if conf else None,
           "margin": guarded(H * W, torch.float32, FILL) if margin else None,
           "probs": guarded(N * ldp, torch.float32, FILL) if probs else None}
    ptr = {k: (None if v is None else v[1].data_ptr()) for k, v in out.items()}
    stream = torch.cuda.current_stream().cuda_stream
    for v in range(V):
        p = _lib.ClassProbParams(logits=zs[v].data_ptr(), ld=ld, N=N, C=Cc, first=first, view=v, n_views=V, acc=ptr["acc"], lda=lda,
                                 H=H, W=W, p0=p0, pixels=_lib.ptr(pixels), label_map=ptr["label"], conf_map=ptr["conf"],
                                 margin_map=ptr["margin"], probs=ptr["probs"], ldp=ldp)
        _lib.check(_lib.load().hsimae_class_prob(C.byref(p), stream), "hsimae_class_prob")
    out["lda"], out["ldp"] = lda, ldp
    return out


def guards_intact(out, N, Cc):
    for k in ("acc", "label", "conf", "margin", "probs"):
        if out[k] is None:
            continue
        whole = out[k][0].cpu()
        fill = STALE if k == "acc" else FILL
        assert (whole[:GUARD] == fill).all() and (whole[-GUARD:] == fill).all(), k
    assert (out["acc"][1].view(N, out["lda"])[:, Cc:] == STALE).all()
    if out["probs"] is not None:
        assert (out["probs"][1].view(N, out["ldp"])[:, Cc:] == FILL).all()


def in_row_order(out, row_of, ref, N, Cc, first):
    """The maps read back per row of the chunk -> (mean, label, conf, margin); a row whose pixel lies outside the map has
    nothing to read: it takes the restatement's values.  Also checks that nothing else in the maps was written."""
    mean = out["probs"][1].view(N, out["ldp"])[:, :Cc].cpu().numpy()
    label, conf, margin = ref["label"].copy(), ref["conf"].copy(), ref["margin"].copy()
    lm, cm, mm = (out[k][1].cpu().numpy() for k in ("label", "conf", "margin"))
    assert np.all(lm[row_of < 0] == FILL) and np.all(cm[row_of < 0] == FILL) and np.all(mm[row_of < 0] == FILL)
    pix = np.flatnonzero(row_of >= 0)
    assert np.all(lm[pix] != FILL)
    for px in pix:
        k = row_of[px]
        label[k], conf[k], margin[k] = lm[px], cm[px], mm[px]
    return mean, label, conf, margin


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_class_prob_lies_inside_the_bound_of_the_restatement(shape):
    from hsimae_amd import _lib
    N, Cc, ld = shape
    for first, V in itertools.product((0, 1), R.VIEWS):
        z = R.make_case(N, Cc, ld, first, V)
        ref = R.prob_ref(z, Cc, first)
        zs = torch.from_numpy(z).cuda()
        for name, H, W, p0, pixels in R.pixel_forms(N):
            pix_d = None if pixels is None else torch.from_numpy(pixels).cuda()
            out = run_prob(zs, Cc, first, H, W, p0, pix_d)
            guards_intact(out, N, Cc)
            got = in_row_order(out, R.rows_of_pixels(H, W, p0, pixels, N), ref, N, Cc, first)
            if name == "list" and N >= 6:                   # the repeated pixel: both of its rows hold the same logits
                got[1][N - 2], got[2][N - 2], got[3][N - 2] = got[1][N - 1], got[2][N - 1], got[3][N - 1]
            w = R.worst(got, z, Cc, first, ref)
            print(f"{shape} first {first} views {V} {name}: err / bound: mean {w['mean']:.3f}, conf {w['conf']:.3f}, "
                  f"margin {w['margin']:.3f}; labels wrong {w['wrong']}, share left open {w['open']:.5f}")
            assert w["zeros"] and w["wrong"] == 0
            assert w["mean"] <= 1.0 and w["conf"] <= 1.0 and w["margin"] <= 1.0
            assert w["open"] <= 1e-3
            acc = out["acc"][1].view(N, out["lda"])[:, :Cc].cpu().numpy()
            assert np.all(acc[:, :first] == 0)
            if V == 1:                                      # nothing but the softmax itself was stored
                assert np.array_equal(acc, got[0], equal_nan=True)
            if V == 1 and Cc <= 256:                        # hsimae_class_argmax's own limit
                whole, lab = guarded(H * W, torch.int64, FILL)
                sp = _lib.SceneParams(H=H, W=W, p0=p0, pixels=_lib.ptr(pix_d), N=N)
                _lib.check(_lib.load().hsimae_class_argmax(C.byref(sp), zs[0].data_ptr(), ld, Cc, first, lab.data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream), "hsimae_class_argmax")
                assert torch.equal(whole, out["label"][0])
            again = run_prob(zs, Cc, first, H, W, p0, pix_d)
            for k in ("acc", "label", "conf", "margin", "probs"):
                assert torch.equal(again[k][0].view(torch.int32), out[k][0].view(torch.int32)), k      # bit for bit, NaN included


def test_optional_outputs_may_be_absent_in_every_combination():
    N, Cc, ld, first, V = 65, 33, 48, 1, 3
    z = R.make_case(N, Cc, ld, first, V)
    zs = torch.from_numpy(z).cuda()
    H, W = 5, 15
    full = run_prob(zs, Cc, first, H, W, 3)
    for conf, margin, probs in itertools.product((False, True), repeat=3):
        out = run_prob(zs, Cc, first, H, W, 3, conf=conf, margin=margin, probs=probs)
        guards_intact(out, N, Cc)
        for k in ("acc", "label", "conf", "margin", "probs"):
            if out[k] is not None:
                assert torch.equal(out[k][0].view(torch.int32), full[k][0].view(torch.int32)), (k, conf, margin, probs)


def test_every_refusal_returns_its_code_and_writes_nothing():
    from hsimae_amd import _lib
    for what, got, want in R.refusals(_lib.load(), _lib):
        assert got == want, (what, got, want)
    zs = torch.from_numpy(R.make_case(5, 3, 16, 0, 1)).cuda()
    from hsimae_amd._lib import ClassProbParams
    out = {k: guarded(64, torch.int64 if k == "label" else torch.float32, FILL) for k in ("acc", "label", "conf", "margin", "probs")}
    p = ClassProbParams(logits=zs.data_ptr(), ld=16, N=0, C=3, first=0, view=0, n_views=1, acc=out["acc"][1].data_ptr(), lda=4, H=2,
                        W=4, label_map=out["label"][1].data_ptr(), conf_map=out["conf"][1].data_ptr(),
                        margin_map=out["margin"][1].data_ptr(), probs=out["probs"][1].data_ptr(), ldp=4)
    assert _lib.load().hsimae_class_prob(C.byref(p), torch.cuda.current_stream().cuda_stream) == 0      # N = 0
    p.N, p.view = 5, 1                                                                                     # view outside [0, n_views)
    assert _lib.load().hsimae_class_prob(C.byref(p), torch.cuda.current_stream().cuda_stream) == -1
    torch.cuda.synchronize()
    for k, (whole, _) in out.items():
        assert (whole == FILL).all(), k


# ------------------------------------------------------------------ classify_scene
def tiny_hsivit(num_class=7, seed=0):
    """tests/test_gpu_scene.py's tiny model, built here: same shape, same seeds."""
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
        m.cls_head.weight.copy_(0.2 * torch.randn(m.cls_head.weight.shape, generator=g))
    return m.cuda().eval()


def scene_23x19(seed=5, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((23, 19, 32)).astype(dtype)


def flipped_logits(m, scene, pix, views, bs):
    """HSIViT.forward on SceneCubes.gather(pixels, flips) windows, chunks of `bs` -> fp32 [V, n, num_class] (CPU)."""
    from hsimae_amd import SceneCubes
    cubes = SceneCubes(scene)
    out = []
    for v in views:
        rows = [m(cubes.gather(pix[k:k + bs], np.full(len(pix[k:k + bs]), v, np.uint8))).cpu() for k in range(0, len(pix), bs)]
        out.append(torch.cat(rows))
    cubes.check()
    return torch.stack(out).numpy()


def check_scene(res, logits, pix, H, W, nc, what):
    """res (a SceneClassification on the CPU) against the restatement of `logits` [V, n, nc] for the pixels `pix`."""
    ref = R.prob_ref(logits, nc, 1)
    lab, conf, margin = (t.reshape(-1).numpy() for t in (res.labels, res.confidence, res.margin))
    assert res.labels.dtype == torch.int64 and res.confidence.dtype == torch.float32 and res.margin.dtype == torch.float32
    assert tuple(res.labels.shape) == tuple(res.confidence.shape) == tuple(res.margin.shape) == (H, W)
    assert tuple(res.probs.shape) == (len(pix), nc) and res.probs.dtype == torch.float32
    w = R.worst((res.probs.numpy(), lab[pix], conf[pix], margin[pix]), logits, nc, 1, ref, planted=False)
    print(f"{what}: err / bound: mean {w['mean']:.3f}, conf {w['conf']:.3f}, margin {w['margin']:.3f}; labels wrong {w['wrong']}, "
          f"share left open {w['open']:.5f}")
    assert w["zeros"] and w["wrong"] == 0 and w["mean"] <= 1.0 and w["conf"] <= 1.0 and w["margin"] <= 1.0
    assert np.allclose(res.probs.numpy().sum(1), 1.0, atol=1e-5) and np.all(res.probs.numpy()[:, 0] == 0)
    rest = np.ones(H * W, bool)
    rest[pix] = False
    assert np.all(lab[rest] == 0) and np.all(conf[rest] == 0) and np.all(margin[rest] == 0)
    return w


def test_classify_scene_with_one_view_is_predict_scene_with_probabilities():
    m = tiny_hsivit()
    scene = scene_23x19()
    labels, logits = m.predict_scene(scene, batch_size=256, return_logits=True)
    res = m.classify_scene(scene, batch_size=256, return_probs=True)
    assert torch.equal(res.labels, labels)
    check_scene(res, logits.numpy()[None], np.arange(23 * 19), 23, 19, 7, "views=(0,)")
    assert m.classify_scene(scene, batch_size=256).probs is None
    # a subset of pixels (index list, any order), everything left on the device
    pix = torch.tensor([436, 0, 18, 19, 200, 5, 418])
    lab2, log2 = m.predict_scene(scene, pixels=pix, batch_size=256, return_logits=True)
    dev = m.classify_scene(torch.from_numpy(scene).cuda(), pixels=pix, batch_size=256, return_probs=True, on_device=True)
    assert all(t.is_cuda for t in dev)
    from hsimae_amd.finetune import SceneClassification
    res2 = SceneClassification(*(t.cpu() for t in dev))
    assert torch.equal(res2.labels, lab2)
    check_scene(res2, log2.numpy()[None], pix.numpy(), 23, 19, 7, "views=(0,), 7 pixels, on_device")


def test_classify_scene_averages_the_flip_views():
    m = tiny_hsivit(seed=3)
    scene = scene_23x19(seed=8)
    pix = np.arange(23 * 19)
    logits = flipped_logits(m, scene, pix, (0, 1, 2, 3), 256)
    assert not np.array_equal(logits[0], logits[1]) and not np.array_equal(logits[0], logits[2])      # the flips are seen
    res = m.classify_scene(scene, batch_size=256, views="flips", return_probs=True)
    check_scene(res, logits, pix, 23, 19, 7, "views='flips'")
    two = m.classify_scene(scene, batch_size=256, views=(3, 1), return_probs=True)
    check_scene(two, logits[[3, 1]], pix, 23, 19, 7, "views=(3, 1)")
    sub = np.array([436, 0, 18, 19, 200, 5, 418])
    res3 = m.classify_scene(scene, pixels=sub, batch_size=4, views="flips", return_probs=True)
    check_scene(res3, flipped_logits(m, scene, sub, (0, 1, 2, 3), 4), sub, 23, 19, 7, "views='flips', 7 pixels in chunks of 4")


def test_classify_scene_on_an_fp32_scene_smaller_than_the_pad():
    m = tiny_hsivit(seed=4)
    scene = np.random.default_rng(9).standard_normal((3, 5, 32)).astype(np.float32)
    pix = np.arange(15)
    res = m.classify_scene(scene, views="flips", return_probs=True)
    check_scene(res, flipped_logits(m, scene, pix, (0, 1, 2, 3), 15), pix, 3, 5, 7, "3 x 5 fp32 scene, views='flips'")
    one = m.classify_scene(scene, return_probs=True)
    assert torch.equal(one.labels, m.predict_scene(scene))


def test_classify_scene_refuses_bad_views():
    m = tiny_hsivit()
    for bad in ("all", (0, 0), (4,), ()):
        with pytest.raises(ValueError):
            m.classify_scene(scene_23x19(), views=bad)


# ------------------------------------------------------------------ test_model_scene: flip views and the pictures
def test_test_model_scene_with_flip_views_writes_the_reference_pictures(tmp_path):
    from hsimae_amd import DualViT, HSIViT, label_to_colormap, test_model, test_model_scene
    from hsimae_amd.finetune_train import _scene_scores
    torch.manual_seed(4)
    d = quiet(DualViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=6, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, trunc_init=True, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for n, p in d.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
        d.cls_head.weight.copy_(0.2 * torch.randn(d.cls_head.weight.shape, generator=g))
    torch.save(d.state_dict(), os.path.join(tmp_path, "ft.pkl"))
    rng = np.random.default_rng(13)
    scene = scene_23x19(seed=14)
    gt = rng.integers(0, 6, size=(23, 19))
    gt.reshape(-1)[:6] = np.arange(6)
    test_gt = gt.copy()
    test_gt[rng.random(gt.shape) < 0.3] = 0
    kw = dict(depth=3, dim=32, s_depth=2)

    def pictures(out, stem="ft"):
        tag = str(np.around(out[0] * 100, 2))
        folder = os.path.join(tmp_path, stem)
        assert sorted(os.listdir(folder)) == sorted([f"{stem}_all_oa_{tag}.png", f"{stem}_oa_{tag}.png"])
        whole = R.decode_png(open(os.path.join(folder, f"{stem}_all_oa_{tag}.png"), "rb").read())
        masked = R.decode_png(open(os.path.join(folder, f"{stem}_oa_{tag}.png"), "rb").read())
        assert np.array_equal(whole, label_to_colormap(out[4]))
        assert np.array_equal(masked, label_to_colormap(np.where(gt == 0, 0, out[4])))

    # the default call: what it returned before (predict_scene's map and its scores), and no picture
    base = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "ft.pkl", batch_size=256, **kw)
    assert not os.path.exists(os.path.join(tmp_path, "ft"))
    v = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=6, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, sep_pos_embed=True, use_learnable_pos_emb=False).cuda()
    sd = v.state_dict()
    sd.update({k: t for k, t in torch.load(os.path.join(tmp_path, "ft.pkl"), map_location="cuda").items() if k in sd})
    v.load_state_dict(sd)
    v.eval()
    pred = v.predict_scene(scene, batch_size=256, on_device=True)
    want = _scene_scores(pred, test_gt, gt, 6, torch.device("cuda:0"))
    assert base[:3] == want[:3] and np.array_equal(base[3], want[3]) and np.array_equal(base[4], pred.cpu().numpy())

    out = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "ft.pkl", batch_size=256, views="flips", save_images=True, **kw)
    pictures(out)
    assert out[4].shape == gt.shape and out[4].dtype == np.int64 and out[4].min() >= 1
    assert np.array_equal(out[4], v.classify_scene(scene, batch_size=256, views="flips").labels.numpy())
    want = _scene_scores(torch.from_numpy(out[4]).cuda(), test_gt, gt, 6, torch.device("cuda:0"))
    assert out[:3] == want[:3] and np.array_equal(out[3], want[3])

    # one view with pictures goes through classify_scene: the same map as the default call; test_model writes them too
    torch.save(d.state_dict(), os.path.join(tmp_path, "one.pkl"))
    one = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "one.pkl", batch_size=256, save_images=True, **kw)
    assert one[:3] == base[:3] and np.array_equal(one[4], base[4])
    pictures(one, "one")
    torch.save(d.state_dict(), os.path.join(tmp_path, "cubes.pkl"))
    data_cubes = [np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")[r:r + 9, c:c + 9] for r in range(23) for c in range(19)]
    cubes = quiet(test_model, data_cubes, test_gt, gt, str(tmp_path), "cubes.pkl", save_images=True, **kw)
    assert cubes[:3] == base[:3] and np.array_equal(cubes[4], base[4])
    pictures(cubes, "cubes")
