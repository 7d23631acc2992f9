"""Whole-scene inference on the GPU: hsimae_scene_windows against the windows recorded from the reference
(tests/golden/scene_windows.npz) and against hsimae_scene_batch, hsimae_class_argmax against torch.argmax, DualViT.predict_scene against HSIViT.forward on
windows built the reference's way, chunk invariance, the oracle at Base width, and test_model_scene against test_model."""
import contextlib
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import hsimae_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
FX = np.load(os.path.join(ROOT, "tests", "golden", "scene_windows.npz"))


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def rms_rel(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt() / b.double().pow(2).mean().sqrt())


def ref_windows(scene):
    """Utils/Preprocessing.py:208-213 (np.pad 'symmetric' + one 9 x 9 slice per pixel, row-major) and the fp32 cast of
    Model_Finetuning.py:49 -> [H*W, 9, 9, C] fp32."""
    H, W, _ = scene.shape
    pad = np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")
    return np.stack([pad[r:r + 9, c:c + 9] for r in range(H) for c in range(W)]).astype(np.float32)


def run_windows(scene, N, out, p0=0, pixels=None):
    from hsimae_amd import _lib
    H, W, Cb = scene.shape
    p = _lib.SceneParams(scene=scene.data_ptr(), scene_f64=int(scene.dtype == torch.float64), H=H, W=W, C=Cb, p0=p0,
                         pixels=_lib.ptr(pixels), N=N, out=out.data_ptr(), sn=out.stride(0), sb=out.stride(2), sh=out.stride(3),
                         sw=out.stride(4))
    _lib.check(_lib.load().hsimae_scene_windows(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_scene_windows")


@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("layout", ["band_fastest", "contiguous"])
def test_scene_windows_are_bit_exact_with_the_reference(tag, layout):
    scene = torch.from_numpy(FX[f"{tag}_scene"]).cuda()
    items = torch.from_numpy(FX[f"{tag}_items"])                        # [H*W, 1, C, 9, 9] fp32, HSIdataset's items
    H, W, Cb = scene.shape
    HW = H * W

    def buf(n):
        if layout == "band_fastest":                                    # the view HSIdataset / DeviceLoader deliver
            return torch.full((n, 9, 9, Cb), -1.0, device="cuda").permute(0, 3, 1, 2).unsqueeze(1)
        return torch.full((n, 1, Cb, 9, 9), -1.0, device="cuda")

    out = buf(HW)                                                       # range form, the whole scene
    run_windows(scene, HW, out)
    assert torch.equal(out.cpu(), items)
    out = buf(HW - 5)                                                   # range form from p0 = 3
    run_windows(scene, HW - 5, out, p0=3)
    assert torch.equal(out.cpu(), items[3:HW - 2])
    idx = torch.randperm(HW, generator=torch.Generator().manual_seed(1))[: HW - 4]
    idx = torch.cat([idx, idx[:3]])                                     # index-list form, any order, repeats allowed
    out = buf(idx.numel())
    run_windows(scene, idx.numel(), out, pixels=idx.cuda())
    assert torch.equal(out.cpu(), items[idx])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("Cb", [5, 8])                                  # scalar copy, 16-byte copy
def test_windows_and_batch_entry_points_cut_the_same_windows(Cb, dtype):
    """hsimae_scene_windows and hsimae_scene_batch run one cutter: on a 3 x 3 scene (narrower than the 4-pixel pad: the symmetric
    index wraps more than once) the same pixel list gives the same bits from both, and numpy's.  The last two pixels lie outside
    the scene: zero windows from both, `bad` from the batch entry point alone.  Nothing behind the window buffers is written."""
    from hsimae_amd import _lib
    scene = np.random.default_rng(Cb).standard_normal((3, 3, Cb)).astype(dtype)
    pad = np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")
    pix = [0, 4, 8, -1, 9]
    want = torch.zeros(5, 9, 9, Cb)
    for k, p in enumerate(pix[:3]):
        want[k] = torch.from_numpy(pad[p // 3:p // 3 + 9, p % 3:p % 3 + 9].astype(np.float32))
    scene_d, pix_d, n = torch.from_numpy(scene).cuda(), torch.tensor(pix).cuda(), 5 * 81 * Cb
    got = []
    for batch in (False, True):
        big = torch.full((n + 64,), -7.0, device="cuda")
        out = big[:n].view(5, 9, 9, Cb).permute(0, 3, 1, 2).unsqueeze(1)                # band-fastest, as the loaders deliver
        if batch:
            items, bad = torch.arange(5).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda")
            p = _lib.SceneBatchParams(scene=scene_d.data_ptr(), scene_f64=int(dtype == np.float64), H=3, W=3, C=Cb,
                                      items=items.data_ptr(), N=5, n_items=5, pixels=pix_d.data_ptr(), out=out.data_ptr(),
                                      sn=out.stride(0), sb=out.stride(2), sh=out.stride(3), sw=out.stride(4), bad=bad.data_ptr())
            _lib.check(_lib.load().hsimae_scene_batch(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_scene_batch")
            assert int(bad.item()) == 1
        else:
            run_windows(scene_d, 5, out, pixels=pix_d)
        assert (big[n:] == -7).all(), "canary behind the windows overwritten"
        got.append(big[:n].view(5, 9, 9, Cb).cpu())
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))
    assert torch.equal(got[0].view(torch.int32), want.view(torch.int32))
    assert (got[0][3:] == 0).all() and (got[1][3:] == 0).all()


def run_argmax(logits, H, W, labels, first=1, pixels=None, p0=0):
    from hsimae_amd import _lib
    p = _lib.SceneParams(H=H, W=W, p0=p0, pixels=_lib.ptr(pixels), N=logits.shape[0])
    _lib.check(_lib.load().hsimae_class_argmax(C.byref(p), logits.data_ptr(), logits.stride(0), logits.shape[1], first,
                                               labels.data_ptr(), torch.cuda.current_stream().cuda_stream), "hsimae_class_argmax")


def test_class_argmax_matches_torch_argmax_with_ties_and_nans():
    g = torch.Generator().manual_seed(3)
    N, nc = 1500, 17
    full = torch.randn(N, nc + 3, generator=g)                          # rows 20 floats apart: a strided [N, 17] view
    x = full[:, :nc]
    x[100:200, 5] = x[100:200, 9] = x[100:200].max(1).values + 1       # planted two-way ties
    x[200:260, 1:] = 0.25                                               # all equal
    x[300:340, 7] = float("nan")                                        # one NaN
    x[340:380, 3] = x[340:380, 12] = float("nan")                       # two NaNs: the first wins
    x[380:400, 0] = float("nan")                                        # NaN outside the searched range (column 0)
    x[400:420, 1] = float("nan")                                        # NaN in the first searched column
    x[420:440, nc - 1] = float("inf")
    want = 1 + torch.argmax(x[:, 1:], 1)
    xd = full.cuda()[:, :nc]
    H, W = 50, 40
    labels = torch.full((H * W,), -7, dtype=torch.int64, device="cuda")
    run_argmax(xd, H, W, labels, p0=200)                                # range form: map[200 + n]
    lab = labels.cpu()
    assert torch.equal(lab[200:200 + N], want)
    assert (lab[:200] == -7).all() and (lab[200 + N:] == -7).all()
    idx = torch.randperm(H * W, generator=g)[:N]                        # index-list form
    labels.fill_(-7)
    run_argmax(xd, H, W, labels, pixels=idx.cuda())
    lab = labels.cpu()
    assert torch.equal(lab[idx], want)
    rest = torch.ones(H * W, dtype=torch.bool)
    rest[idx] = False
    assert (lab[rest] == -7).all()
    labels.fill_(-7)                                                    # first = 0: plain argmax
    run_argmax(xd, H, W, labels, first=0)
    assert torch.equal(labels.cpu()[:N], torch.argmax(x, 1))


def tiny_hsivit(num_class=7, seed=0):
    from hsimae_amd import HSIViT
    torch.manual_seed(seed)
    m = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=num_class, embed_dim=32, depth=3,
              num_heads=2, s_depth=2, trunc_init=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                               # non-degenerate biases / LayerNorms / head
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
        m.cls_head.weight.copy_(0.2 * torch.randn(m.cls_head.weight.shape, generator=g))
    return m.cuda().eval()


def scene_23x19(seed=5, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((23, 19, 32)).astype(dtype)


def test_predict_scene_equals_hsivit_forward_on_reference_windows():
    m = tiny_hsivit()
    scene = scene_23x19()
    labels, logits = m.predict_scene(scene, batch_size=256, return_logits=True)
    x = torch.from_numpy(ref_windows(scene)).cuda().permute(0, 3, 1, 2).unsqueeze(1)
    ref = torch.cat([m(x[k:k + 256]).cpu() for k in range(0, x.shape[0], 256)])
    assert labels.shape == (23, 19) and labels.dtype == torch.int64
    assert logits.shape == ref.shape and torch.equal(logits, ref)      # same kernels, same chunk shapes
    assert torch.equal(labels.reshape(-1), 1 + torch.argmax(ref[:, 1:], 1))
    # a subset of pixels (index list, any order): their logits in that order, their labels in place, 0 elsewhere
    pix = torch.tensor([436, 0, 18, 19, 200, 5, 418])
    lab2, log2 = m.predict_scene(torch.from_numpy(scene).cuda(), pixels=pix, batch_size=256, return_logits=True)
    assert rms_rel(log2, ref[pix]) < 1e-5
    want = torch.zeros(23 * 19, dtype=torch.int64)
    want[pix] = 1 + torch.argmax(log2[:, 1:], 1)
    assert torch.equal(lab2.reshape(-1), want)


def test_predict_scene_is_chunk_invariant():
    m = tiny_hsivit(seed=2)
    scene = scene_23x19(seed=6, dtype=np.float32)
    la, ga = m.predict_scene(scene, batch_size=97, return_logits=True)
    lb, gb = m.predict_scene(scene, batch_size=4096, return_logits=True)
    assert rms_rel(ga, gb) < 1e-3
    top2 = torch.topk(gb[:, 1:], 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-2 * gb.abs().max(1).values
    assert clear.float().mean() > 0.5
    assert torch.equal(la.reshape(-1)[clear], lb.reshape(-1)[clear])


def test_scene_pass_handles_a_one_pixel_chunk_tail():
    """50 pixels in chunks of 7: seven whole chunks and a last one of a single pixel (ScenePass.chunks).  A chunk of one and a
    call of one launch the same shapes, so the tail's rows equal the same call made on that pixel alone, bit for bit."""
    m = tiny_hsivit(seed=3)
    scene = torch.from_numpy(scene_23x19(seed=7)).cuda()
    pix = torch.randperm(23 * 19, generator=torch.Generator().manual_seed(8))[:50]
    assert m._scene_chunk(7) == 7 and pix.numel() % 7 == 1
    rest = torch.ones(23 * 19, dtype=torch.bool)
    rest[pix] = False

    feats = m.scene_features(scene, pix, batch_size=7).cpu()
    assert feats.shape == (50, 4 * 32) and torch.isfinite(feats).all()
    assert torch.equal(feats[49:], m.scene_features(scene, pix[49:], batch_size=7).cpu())

    got = m.classify_scene(scene, pix, batch_size=7, views=(0, 3), return_probs=True)      # on_device=False: raises if `bad` is set
    one = m.classify_scene(scene, pix[49:], batch_size=7, views=(0, 3), return_probs=True)
    assert got.probs.shape == (50, 7) and torch.equal(got.probs[49:], one.probs)
    for a, b in zip(got[:3], one[:3]):                                  # labels, confidence, margin of that pixel
        assert a.shape == (23, 19) and torch.equal(a.reshape(-1)[pix[49:]], b.reshape(-1)[pix[49:]])
        assert torch.isfinite(a.double()).all() and (a.reshape(-1)[rest] == 0).all()
        assert (b.reshape(-1)[torch.arange(23 * 19) != pix[49]] == 0).all()
    assert torch.isfinite(got.probs).all() and (got.labels.reshape(-1)[pix] >= 1).all()

    bank = pix[:20]
    knn = m.knn_scene(scene, bank, 1 + torch.arange(20) % 6, pixels=pix, k=5, batch_size=7, return_probs=True, on_device=True)
    m.last_knn.check()                                                  # no index outside the bank, no bad label
    assert torch.isfinite(knn.probs).all() and (knn.labels.reshape(-1).cpu()[rest] == 0).all()
    assert (knn.labels.reshape(-1).cpu()[pix] >= 1).all()


def test_predict_scene_base_width_against_oracle():
    from hsimae_amd import HSIViT
    cfg = O.OracleConfig(bands=32)
    state = O.init_state(cfg, seed=9, std=0.02)
    g = torch.Generator().manual_seed(10)
    state["cls_head.weight"] = torch.randn(10, 128 * 4, generator=g) * 0.02
    state["cls_head.bias"] = torch.randn(10, generator=g) * 0.05
    v = quiet(HSIViT, img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, num_class=10, embed_dim=128, depth=12,
              num_heads=8, s_depth=9, trunc_init=True)
    model_dict = v.state_dict()
    model_dict.update({k: t for k, t in state.items() if k in model_dict})
    v.load_state_dict(model_dict)
    v = v.cuda().eval()
    scene = np.random.default_rng(11).random((31, 27, 32))
    pix = np.concatenate([np.arange(0, 31 * 27, 29), [26, 27, 31 * 27 - 1]])
    labels, logits = v.predict_scene(scene, pixels=pix, return_logits=True)
    x = torch.from_numpy(ref_windows(scene)[pix]).permute(0, 3, 1, 2).unsqueeze(1).contiguous()
    ref, _ = O.dualvit_classify(state, cfg, x)
    assert rms_rel(logits, ref) < 1e-2
    assert torch.equal(labels.reshape(-1)[torch.from_numpy(pix)], 1 + torch.argmax(logits[:, 1:], 1))


def test_test_model_scene_returns_what_test_model_returns(tmp_path):
    from hsimae_amd import DualViT, test_model, test_model_scene
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
    gt.reshape(-1)[:6] = np.arange(6)                                   # every class present
    test_gt = gt.copy()
    test_gt[rng.random(gt.shape) < 0.3] = 0
    data_cubes = [np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")[r:r + 9, c:c + 9] for r in range(23) for c in range(19)]   # fp64, as get_data_set_dual gives them
    kw = dict(depth=3, dim=32, s_depth=2)
    a = quiet(test_model, data_cubes, test_gt, gt, str(tmp_path), "ft.pkl", **kw)
    b = quiet(test_model_scene, scene, test_gt, gt, str(tmp_path), "ft.pkl", batch_size=256, **kw)
    assert a[:3] == b[:3]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert b[4].shape == gt.shape and b[4].min() >= 1
