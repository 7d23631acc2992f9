"""csrc/recon.hip and hsimae_amd/recon.py on the device: hsimae_recon_accumulate bit for bit against the sequential fp32 replay of
tests/recon_ref.py, hsimae_recon_finish inside the bounds derived there, and reconstruct_scene / recon_eval_scene /
mask_pretraining(val_scene=) against the by-hand pipeline of their parts."""
import contextlib
import ctypes as C
import functools
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import recon_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16
FILL = -7


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def guarded(n, dtype, fill=FILL, inner=0):
    """(whole buffer, the n elements in its middle set to `inner`): GUARD elements of `fill` on either side must survive."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    whole[GUARD:GUARD + n] = inner
    return whole, whole[GUARD:GUARD + n]


def intact(whole, fill=FILL):
    w = whole.cpu()
    return bool((w[:GUARD] == fill).all() and (w[-GUARD:] == fill).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ hsimae_recon_accumulate
SHAPES = [(9, 9, 8, 9), (5, 3, 8, 9), (13, 10, 16, 9), (20, 23, 24, 4), (12, 12, 200, 5)]


@functools.lru_cache(maxsize=None)
def windows(shape):
    """The synthetic windows of a shape and the replay of one and of two passes over them (computed once, never modified)."""
    H, W, Cb, stride = shape
    scene, rows, cols, pred, mask = R.make_windows(H, W, Cb, stride, seed=sum(shape))
    acc, cnt = np.zeros((H, W, Cb), np.float32), np.zeros((H, W, Cb), np.int32)
    R.accumulate(pred, mask, rows, cols, 0, H, W, acc, cnt)
    one = (acc.copy(), cnt.copy())
    R.accumulate(pred, mask, rows, cols, 0, H, W, acc, cnt)
    for a in (scene, rows, cols, pred, mask, acc, cnt) + one:
        a.setflags(write=False)
    return scene, rows, cols, pred, mask, one, (acc, cnt)


def run_accumulate(shape, chunk, passes=1):
    """-> (sum whole, sum, cnt whole, cnt) after `passes` passes in chunks of `chunk` windows through the C ABI."""
    from hsimae_amd import _lib
    H, W, Cb, _ = shape
    _, rows, cols, pred, mask, _, _ = windows(shape)
    n_win = pred.shape[0]
    rows_d, cols_d = torch.from_numpy(rows.copy()).cuda(), torch.from_numpy(cols.copy()).cuda()
    pred_d, mask_d = torch.from_numpy(pred.copy()).cuda(), torch.from_numpy(mask.copy()).cuda()
    sw, s = guarded(H * W * Cb, torch.float32)
    cw, c = guarded(H * W * Cb, torch.int32)
    for _ in range(passes):
        for w0 in range(0, n_win, chunk):
            n = min(chunk, n_win - w0)
            p = _lib.ReconAccumulateParams(pred_img=pred_d[w0:w0 + n].data_ptr(), mask_img=mask_d[w0:w0 + n].data_ptr(), n=n, w0=w0,
                                           rows=rows_d.data_ptr(), nrows=len(rows), cols=cols_d.data_ptr(), ncols=len(cols),
                                           H=H, W=W, C=Cb, sum=s.data_ptr(), cnt=c.data_ptr())
            _lib.check(_lib.load().hsimae_recon_accumulate(C.byref(p), stream()), "hsimae_recon_accumulate")
    return sw, s, cw, c


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accumulate_equals_the_sequential_replay_bit_for_bit(shape):
    """Chunks of 1, 3, 7 and all windows (they cut the window rows), one and two passes; NaN sits in pred under mask 0 and at every
    reflected position and must never surface; the canaries around sum and cnt survive; two runs agree bit for bit."""
    _, rows, cols, pred, _, one, two = windows(shape)
    n_win = pred.shape[0]
    assert np.isfinite(one[0]).all() and np.isnan(pred).any()
    for chunk in sorted({1, 3, 7, n_win}):
        for passes, (want_s, want_c) in ((1, one), (2, two)):
            sw, s, cw, c = run_accumulate(shape, chunk, passes)
            assert intact(sw) and intact(cw), (chunk, passes)
            assert np.array_equal(c.cpu().numpy(), want_c.reshape(-1)), (chunk, passes)
            assert np.array_equal(s.cpu().numpy().view(np.int32), want_s.reshape(-1).view(np.int32)), (chunk, passes)
    again = run_accumulate(shape, 3, 2)
    assert torch.equal(bits(again[1]), bits(s)) and torch.equal(again[3], c)
    print(f"{shape}: {n_win} windows ({len(rows)} x {len(cols)}), up to {int(one[1].max())} reconstructions per voxel")


# ------------------------------------------------------------------ hsimae_recon_finish
def run_finish(scene, acc, cnt, want=("recon", "cover", "rmse", "sam")):
    from hsimae_amd import _lib
    H, W, Cb = scene.shape
    s_d, a_d, c_d = (torch.from_numpy(np.array(a, order="C")).cuda() for a in (scene, acc, cnt))      # (copies: the cached ones are read-only)
    sizes = dict(recon=(H * W * Cb, torch.float32), cover=(H * W, torch.int32), rmse=(H * W, torch.float32), sam=(H * W, torch.float32))
    out = {k: guarded(*sizes[k], inner=FILL) for k in want}
    out["stats"] = guarded(4, torch.float64, inner=FILL)
    out["partials"] = guarded(4 * _lib.RECON_GRID, torch.float64, inner=FILL)
    p = _lib.ReconFinishParams(scene=s_d.data_ptr(), scene_f64=int(scene.dtype == np.float64), H=H, W=W, C=Cb, sum=a_d.data_ptr(),
                               cnt=c_d.data_ptr(), partials=out["partials"][1].data_ptr(), stats=out["stats"][1].data_ptr(),
                               **{k: out[k][1].data_ptr() for k in want})
    _lib.check(_lib.load().hsimae_recon_finish(C.byref(p), stream()), "hsimae_recon_finish")
    assert all(intact(w) for w, _ in out.values())
    return {k: v.cpu().numpy() for k, (_, v) in out.items()}


def check_finish(got, ref, tag):
    H, W = ref["cover"].shape
    assert np.array_equal(got["recon"].view(np.int32), ref["recon"].reshape(-1).view(np.int32)), tag
    assert np.array_equal(got["cover"], ref["cover"].reshape(-1)), tag
    worst = {}
    for k in ("rmse", "sam"):
        worst[k] = float(np.max(np.abs(got[k].astype(np.float64) - ref[k].reshape(-1)) / ref["b_" + k].reshape(-1)))
    assert got["stats"][1] == ref["stats"][1] and got["stats"][3] == ref["stats"][3], tag
    for j in (0, 2):
        worst[f"stats[{j}]"] = float(abs(got["stats"][j] - ref["stats"][j]) / ref["b_stats"][j])
    print(f"{tag}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0, (tag, worst)


@pytest.mark.parametrize("shape", [s[:3] for s in SHAPES], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_finish_lies_inside_the_bound_on_every_pixel(shape, dtype):
    H, W, Cb = shape
    scene, acc, cnt, special = R.make_sums(H, W, Cb, seed=H + W)
    scene = scene.astype(dtype)
    ref = R.finish(scene, acc, cnt)
    got = run_finish(scene, acc, cnt)
    check_finish(got, ref, f"{shape} {np.dtype(dtype).name}")
    # no band reconstructed, both norms zero, one norm zero, identical spectra, spectra two ulps apart
    assert got["cover"][special["empty"]] == 0 and got["rmse"][special["empty"]] == 0 and got["sam"][special["empty"]] == 0
    assert got["rmse"][special["both_zero"]] == 0 and got["sam"][special["both_zero"]] == 0
    assert got["sam"][special["one_zero"]] == np.float32(np.pi / 2)
    assert got["rmse"][special["same"]] == 0 and got["sam"][special["same"]] == 0 and got["cover"][special["same"]] == Cb - 1
    assert 0 < got["sam"][special["near"]] < 1e-6
    # two runs agree bit for bit; every optional output may be absent and stats does not change
    again = run_finish(scene, acc, cnt)
    assert all(np.array_equal(again[k].view(np.int32), got[k].view(np.int32)) for k in ("recon", "cover", "rmse", "sam"))
    for want in ((), ("rmse",), ("cover", "sam"), ("recon",)):
        part = run_finish(scene, acc, cnt, want)
        assert np.array_equal(part["stats"].view(np.int64), got["stats"].view(np.int64)), want
        assert all(np.array_equal(part[k].view(np.int32), got[k].view(np.int32)) for k in want)


def test_seventy_thousand_pixels_run_past_both_grid_caps():
    """70 000 x 1 x 8: 70 000 workgroups of work for the accumulate (its launch stops at 65 536) and 17 500 quads of pixels for the
    finish (1 024 workgroups): the stride loops of both."""
    shape = (70000, 1, 8, 9)
    scene, rows, cols, pred, mask, one, _ = windows(shape)
    sw, s, cw, c = run_accumulate(shape, pred.shape[0])
    assert intact(sw) and intact(cw)
    assert np.array_equal(c.cpu().numpy(), one[1].reshape(-1))
    assert np.array_equal(s.cpu().numpy().view(np.int32), one[0].reshape(-1).view(np.int32))
    check_finish(run_finish(scene, one[0], one[1]), R.finish(scene, one[0], one[1]), "70000x1x8")


def test_an_accumulated_nan_shows_in_its_pixel_and_in_stats():
    scene, acc, cnt, special = R.make_sums(9, 9, 8, seed=2)
    px = next(p for p in range(81) if p not in special.values())
    acc = acc.copy()
    acc.reshape(-1, 8)[px, 3] = np.nan
    cnt.reshape(-1, 8)[px, 3] = 1
    got = run_finish(scene, acc, cnt)
    assert np.isnan(got["rmse"][px]) and np.isnan(got["sam"][px]) and np.isnan(got["recon"].reshape(-1, 8)[px, 3])
    assert np.isnan(got["stats"][0]) and np.isnan(got["stats"][2]) and got["stats"][3] == (cnt.reshape(-1, 8).max(axis=1) > 0).sum()
    others = np.arange(81) != px
    assert np.isfinite(got["rmse"][others]).all() and np.isfinite(got["sam"][others]).all()


# ------------------------------------------------------------------ reconstruct_scene, recon_eval_scene, mask_pretraining
KW = dict(img_size=9, patch_size=3, in_chans=1, bands=32, b_patch_size=8, embed_dim=32, depth=3, num_heads=2, s_depth=2,
          trunc_init=True, decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=4, norm_pix_loss=True)


def tiny(kind, seed=0):
    """The tiny configuration of the scene tests (tests/test_gpu_knn.py), as an HSIMAE or a DualViT."""
    import hsimae_amd
    torch.manual_seed(seed)
    m = quiet(hsimae_amd.DualViT, num_class=6, **KW) if kind == "dualvit" else quiet(hsimae_amd.HSIMAE, **KW)
    return m.cuda().eval()


def scene_23x19(seed=5, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((23, 19, 32)).astype(dtype)


@pytest.mark.parametrize("kind", ["hsimae", "dualvit"])
def test_reconstruct_scene_is_the_by_hand_pipeline_bit_for_bit(kind):
    from hsimae_amd import HSIMAE, SceneCubes, SceneReconstruction, reconstruct_scene
    m = tiny(kind)
    m.want_recons = False
    scene = scene_23x19()
    H, W, Cb, stride, bs, passes, ratio = 23, 19, 32, 4, 7, 2, 0.75
    random.seed(3)
    gen = torch.Generator(device="cuda").manual_seed(11)
    res = reconstruct_scene(m, scene, mask_ratio=ratio, stride=stride, passes=passes, generator=gen, batch_size=bs)
    assert isinstance(res, SceneReconstruction) and not any(t.is_cuda for t in res) and m.want_recons is False
    # by hand: the same seeds, SceneCubes.gather -> HSIMAE.forward -> numpy replay
    rows, cols = R.centres(H, stride), R.centres(W, stride)
    items = (rows[:, None].astype(np.int64) * W + cols[None, :]).reshape(-1)
    cubes = SceneCubes(scene, pixels=items)
    random.seed(3)
    gen = torch.Generator(device="cuda").manual_seed(11)
    acc, cnt = np.zeros((H, W, Cb), np.float32), np.zeros((H, W, Cb), np.int32)
    T, L = m.input_size[0], m.input_size[1] ** 2
    m.want_recons = True
    loss_sum = 0.0
    with torch.no_grad():
        for _ in range(passes):
            grid = m.get_dim_patches(T, L, ratio)
            for w0 in range(0, len(items), bs):
                n = min(bs, len(items) - w0)
                win = cubes.gather(np.arange(w0, w0 + n))
                n1 = torch.rand(n, T, device="cuda", generator=gen)
                n2 = torch.rand(n, L, device="cuda", generator=gen)
                loss, pred, mask = HSIMAE.forward(m, win, ratio, noise=(n1, n2), grid=grid)
                R.accumulate(pred[:, 0].cpu().numpy(), mask[:, 0].cpu().numpy(), rows, cols, w0, H, W, acc, cnt)
                loss_sum += float(loss.double().item()) * n
    cubes.check()
    assert np.array_equal(res.count.numpy(), cnt) and cnt.max() >= 2 * 4
    ref = R.finish(scene, acc, cnt)
    got = dict(recon=res.recon.numpy().reshape(-1), cover=res.cover.numpy().reshape(-1), rmse=res.rmse.numpy().reshape(-1),
               sam=res.sam.numpy().reshape(-1),
               stats=np.array([float(res.mse) * ref["stats"][1], ref["stats"][1], float(res.mean_sam) * ref["stats"][3], ref["stats"][3]]))
    ref["b_stats"] = ref["b_stats"] + 4 * R.U * np.abs(ref["stats"])          # the division and this test's product back
    check_finish(got, ref, f"reconstruct_scene {kind}")
    want_loss = loss_sum / (passes * len(items))
    assert abs(float(res.loss) - want_loss) <= 2.0 ** -24 * abs(want_loss) and res.loss.dtype == torch.float32
    peak = float(scene.max() - scene.min())
    assert abs(float(res.psnr) - 10 * np.log10(peak * peak / float(res.mse))) <= 1e-12 * abs(float(res.psnr))
    assert abs(float(res.coverage) - (cnt > 0).sum() / cnt.size) <= 1e-15
    # two passes raise the coverage (stride 9: interior pixels lie in one window)
    cover = []
    for p in (1, 2):
        random.seed(3)
        r = reconstruct_scene(m, scene, stride=9, passes=p, generator=torch.Generator(device="cuda").manual_seed(11), batch_size=bs,
                              return_recon=False)
        assert r.recon is None
        cover.append(float(r.coverage))
    print(f"{kind}: psnr {float(res.psnr):.2f} dB, mean sam {float(res.mean_sam):.3f} rad, coverage {cover[0]:.3f} -> {cover[1]:.3f}")
    assert 0.5 < cover[0] < cover[1] <= 1.0


def test_reconstruct_scene_on_the_device_issues_no_host_wait():
    from hsimae_amd import reconstruct_scene
    m = tiny("hsimae", seed=2)
    scene = torch.from_numpy(scene_23x19(seed=7)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    random.seed(1)
    first = reconstruct_scene(m, scene, stride=5, generator=gen, batch_size=9, on_device=True)      # first use allocates
    torch.cuda.synchronize()
    gen.manual_seed(1)
    random.seed(1)
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = reconstruct_scene(m, scene, stride=5, generator=gen, batch_size=9, on_device=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in res) and res.mse.dim() == 0 and res.mse.dtype == torch.float64
    assert all(torch.equal(a, b) for a, b in zip(first, res))                                       # and the same seeds, the same bits


def test_recon_eval_scene_loads_both_kinds_of_checkpoint(tmp_path):
    from hsimae_amd import DualViT, HSIMAE, recon_eval_scene
    torch.manual_seed(4)
    d = quiet(DualViT, num_class=6, **KW)
    torch.manual_seed(5)
    mae = quiet(HSIMAE, **KW)
    torch.save(d.state_dict(), os.path.join(tmp_path, "ft.pkl"))
    torch.save(mae.state_dict(), os.path.join(tmp_path, "mae.pkl"))
    scene = scene_23x19(seed=14)
    args = dict(depth=3, dim=32, s_depth=2, dec_depth=1, dec_dim=32, stride=5, seed=9, batch_size=16)
    out = {name: quiet(recon_eval_scene, scene, os.path.join(tmp_path, name), **args) for name in ("ft.pkl", "mae.pkl")}
    for r in out.values():
        assert not any(t.is_cuda for t in r) and tuple(r.recon.shape) == (23, 19, 32) and tuple(r.sam.shape) == (23, 19)
        assert np.isfinite(float(r.psnr)) and 0 < float(r.mean_sam) < np.pi and 0.5 < float(r.coverage) <= 1
    assert not torch.equal(out["ft.pkl"].recon, out["mae.pkl"].recon)                                # two models, two cubes
    # the pretraining checkpoint: what reconstruct_scene gives on the model itself with the same seeds
    again = quiet(recon_eval_scene, scene, os.path.join(tmp_path, "mae.pkl"), **args)
    assert all(torch.equal(a, b) for a, b in zip(again, out["mae.pkl"]))
    from hsimae_amd import reconstruct_scene
    random.seed(9)
    own = reconstruct_scene(mae.cuda().eval(), scene, stride=5, generator=torch.Generator(device="cuda").manual_seed(9), batch_size=16)
    assert torch.equal(bits(own.recon), bits(out["mae.pkl"].recon)) and torch.equal(own.count, out["mae.pkl"].count)


def test_mask_pretraining_with_a_validation_scene_writes_the_new_keys_and_leaves_the_run_alone(tmp_path, monkeypatch):
    import hsimae_amd
    from hsimae_amd.pretrain import seed_everything
    from test_gpu_train import KW as LOOP_KW, cubes
    monkeypatch.setenv("HSIMAE_DETERMINISTIC", "1")
    val = np.random.default_rng(8).random((14, 12, 32)).astype(np.float32)
    lines = []
    kw = dict(LOOP_KW, log=lambda *s: lines.append(" ".join(map(str, s))))
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "val")
    seed_everything(0)
    _, l0 = hsimae_amd.mask_pretraining(cubes(), d0, "m.pkl", epochs=2, **kw)
    seed_everything(0)
    _, l1 = hsimae_amd.mask_pretraining(cubes(), d1, "m.pkl", epochs=2, val_scene=val, val_every=1, **kw)
    # the training run does not notice the validation: the same losses and the same weights, bit for bit
    assert l0 == l1
    a, b = torch.load(os.path.join(d0, "m.pkl")), torch.load(os.path.join(d1, "m.pkl"))
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    plain = np.load(os.path.join(d0, "train_log.npy"), allow_pickle=True)
    assert plain.shape[0] == 2 and np.allclose(np.array(list(plain[0]), dtype=np.float64), l0)       # the file as it always was
    log = np.load(os.path.join(d1, "train_log.npy"), allow_pickle=True).item()
    assert sorted(log) == ["epoch_loss", "val_epoch", "val_loss", "val_mean_sam", "val_mse"]
    assert log["epoch_loss"] == l1 and log["val_epoch"] == [0, 1] and len(log["val_mse"]) == len(log["val_mean_sam"]) == 2
    assert all(np.isfinite(v) and v > 0 for v in log["val_mse"] + log["val_mean_sam"])
    assert sum("scene reconstruction mse" in s for s in lines) == 2
    seed_everything(0)
    _, _ = hsimae_amd.mask_pretraining(cubes(), str(tmp_path / "every2"), "m.pkl", epochs=2, val_scene=val, val_every=2, **kw)
    assert np.load(os.path.join(tmp_path, "every2", "train_log.npy"), allow_pickle=True).item()["val_epoch"] == [1]
