"""Fine-tuning from the scene on the GPU: hsimae_scene_batch against numpy's own pad / slice / flip / cast, SceneCubes +
DeviceLoader against the batches recorded from the reference's HSIdataset + DataLoader (tests/golden/scene_batches.npz) and
against the existing HSIdataset, dual_branch_finetuning_scene against dual_branch_finetuning, and what the datasets allocate.
Every comparison is for equality."""
import contextlib
import ctypes as C
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
FX = np.load(os.path.join(ROOT, "tests", "golden", "scene_batches.npz"))
CANARY = 64

SCENES = {"3x5x8_f32": ((3, 5, 8), np.float32),         # smaller than the 4-pixel pad
          "10x7x32_f64": ((10, 7, 32), np.float64),     # 16-byte path, fp64 -> fp32
          "13x11x6_f32": ((13, 11, 6), np.float32)}     # C % 4 != 0: scalar path
_scene_cache = {}


def scene_and_windows(name):
    """(scene, windows [H*W, 9, 9, C] in the scene's dtype): np.pad 'symmetric' + one slice per pixel, computed once."""
    if name not in _scene_cache:
        shape, dt = SCENES[name]
        scene = np.random.default_rng(len(name) + shape[0]).standard_normal(shape).astype(dt)
        pad = np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")
        win = np.stack([pad[r:r + 9, c:c + 9] for r in range(shape[0]) for c in range(shape[1])])
        win.setflags(write=False)
        _scene_cache[name] = (scene, win, torch.from_numpy(scene).cuda())
    return _scene_cache[name]


def np_items(win, pixels, flips):
    """The reference's item: flip along w (bit 0), flip along h (bit 1), cast to fp32 -> [n, 1, C, 9, 9]."""
    out = []
    for p, f in zip(pixels, flips):
        w = win[p]
        if f & 1:
            w = np.flip(w, 1)
        if f & 2:
            w = np.flip(w, 0)
        out.append(w.astype(np.float32))
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).unsqueeze(1)


def run_batch(scene_d, items, n_items, pixels=None, labels=None, flips=None, layout="band_fastest", bad=None):
    """One hsimae_scene_batch call on fresh buffers with canaries behind them -> (x, y, bad), all on the host."""
    from hsimae_amd import _lib
    H, W, Cb = scene_d.shape
    n = len(items)
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a, dtype=dt)).cuda()   # noqa: E731
    items_d, pix_d, lab_d, fl_d = dev(items, np.int64), dev(pixels, np.int64), dev(labels, np.int64), dev(flips, np.uint8)
    big = torch.full((n * 81 * Cb + CANARY,), -7.0, device="cuda")
    flat = big[:n * 81 * Cb]
    out = flat.view(n, 9, 9, Cb).permute(0, 3, 1, 2).unsqueeze(1) if layout == "band_fastest" else flat.view(n, 1, Cb, 9, 9)
    ybig = torch.full((n + CANARY,), -7, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda") if bad is None else bad
    p = _lib.SceneBatchParams(scene=scene_d.data_ptr(), scene_f64=int(scene_d.dtype == torch.float64), H=H, W=W, C=Cb,
                              items=items_d.data_ptr(), N=n, n_items=n_items, pixels=_lib.ptr(pix_d), labels=_lib.ptr(lab_d),
                              flips=_lib.ptr(fl_d), out=out.data_ptr(), sn=out.stride(0), sb=out.stride(2), sh=out.stride(3),
                              sw=out.stride(4), y=None if labels is None else ybig.data_ptr(), bad=bad.data_ptr())
    _lib.check(_lib.load().hsimae_scene_batch(C.byref(p), torch.cuda.current_stream().cuda_stream), "hsimae_scene_batch")
    assert (big[n * 81 * Cb:] == -7).all() and (ybig[n:] == -7).all(), "canary behind out / y overwritten"
    if labels is None:
        assert (ybig == -7).all()
    return out.cpu(), ybig[:n].cpu(), int(bad.item())


@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("tables", ["none", "labels", "pixels+labels", "pixels"])
@pytest.mark.parametrize("layout", ["band_fastest", "contiguous"])
@pytest.mark.parametrize("name", list(SCENES))
def test_kernel_equals_numpy_pad_slice_flip_cast(name, layout, tables, N):
    scene, win, scene_d = scene_and_windows(name)
    H, W, _ = scene.shape
    rng = np.random.default_rng(N + len(tables))
    if "pixels" in tables:                                              # a table of pixels in any order, with repeats
        pixels = rng.integers(0, H * W, size=37)
        pixels[:4] = [0, W - 1, (H - 1) * W, H * W - 1]                 # the four corners
    else:
        pixels = None
    n_items = H * W if pixels is None else len(pixels)
    labels = rng.integers(0, 9, size=n_items) if "labels" in tables else None
    items = rng.integers(0, n_items, size=N)                            # N = 257 > n_items: repeated items
    items[-1] = n_items - 1
    flips = (np.arange(N) + 1) % 4 if N > 1 else np.array([3])          # all four values
    for fl in ((flips, None) if N > 1 else (flips,)):
        x, y, bad = run_batch(scene_d, items, n_items, pixels, labels, fl, layout)
        pix = items if pixels is None else pixels[items]
        want = np_items(win, pix, np.zeros(N, dtype=np.uint8) if fl is None else fl)
        assert x.dtype == torch.float32 and torch.equal(x, want)
        assert bad == 0
        if labels is not None:
            assert torch.equal(y, torch.from_numpy(labels[items]))
        x2, y2, _ = run_batch(scene_d, items, n_items, pixels, labels, fl, layout)      # a second run: the same bits
        assert torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(y, y2)


@pytest.mark.parametrize("layout", ["band_fastest", "contiguous"])
@pytest.mark.parametrize("name", list(SCENES))
def test_out_of_range_item_or_pixel_is_flagged_zeroed_and_not_read(name, layout):
    scene, win, scene_d = scene_and_windows(name)
    H, W, _ = scene.shape
    rng = np.random.default_rng(7)
    pixels = rng.integers(0, H * W, size=20)
    labels = rng.integers(1, 9, size=20)
    items = rng.integers(0, 20, size=40)
    flips = rng.integers(0, 4, size=40).astype(np.uint8)
    good_x = np_items(win, pixels[items], flips)
    # out-of-range ITEMS (passed as data, with valid tables), then an out-of-range PIXEL in the table
    for bad_items, bad_pixels in (({5: 20, 17: -1, 33: 2 ** 40}, {}), ({}, {3: H * W}), ({}, {3: -1}), ({}, {3: 2 ** 33 + 1})):
        it, px = items.copy(), pixels.copy()
        for k, v in bad_items.items():
            it[k] = v
        for k, v in bad_pixels.items():
            px[k] = v
        hit = torch.tensor([k in bad_items or int(it[k]) in bad_pixels for k in range(40)])
        assert hit.any() and not hit.all()
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        x, y, bad = run_batch(scene_d, it, 20, px, labels, flips, layout, bad=flag)
        assert bad == 1
        assert (x[hit] == 0).all() and (y[hit] == -1).all()
        assert torch.equal(x[~hit], good_x[~hit]) and torch.equal(y[~hit], torch.from_numpy(labels[items])[~hit])
        _, _, bad = run_batch(scene_d, items, 20, pixels, labels, flips, layout, bad=flag)     # a clean call never clears it
        assert bad == 1
    # without tables the item is the pixel: the same check applies to it
    it = np.array([0, H * W, 3, -5, H * W - 1])
    x, _, bad = run_batch(scene_d, it, H * W, None, None, None, layout)
    assert bad == 1 and (x[[1, 3]] == 0).all() and torch.equal(x[[0, 2, 4]], np_items(win, [0, 3, H * W - 1], [0, 0, 0]))


def test_scene_cubes_python_surface():
    from hsimae_amd import SceneCubes
    scene, win, scene_d = scene_and_windows("10x7x32_f64")
    ds = SceneCubes(scene_d, pixels=[69, 0, 12], gt=[2, 1, 3], train=True)
    assert ds.scene.data_ptr() == scene_d.data_ptr() and len(ds) == 3
    x, y = ds.gather([2, 2, 0], flips=[0, 3, 1])
    assert x.shape == (3, 1, 32, 9, 9) and x.stride(2) == 1 and y.dtype == torch.int64       # band-fastest view
    assert torch.equal(x.cpu(), np_items(win, [12, 12, 69], [0, 3, 1])) and y.tolist() == [3, 3, 2]
    random.seed(3)
    xi, yi = ds[1]
    random.seed(3)
    f = (1 if random.random() < 0.5 else 0) | (2 if random.random() < 0.5 else 0)
    assert xi.shape == (1, 32, 9, 9) and torch.equal(xi.cpu(), np_items(win, [0], [f])[0]) and int(yi) == 1
    ds.train = False
    state = random.getstate()
    assert torch.equal(ds.batch([0])[0].cpu(), np_items(win, [69], [0])) and random.getstate() == state   # eval: no draws
    ds.check()
    whole = SceneCubes(scene, device="cuda:0")                          # a host scene is uploaded; item i is pixel i
    assert len(whole) == 70 and torch.equal(whole.gather([69, 5]).cpu(), np_items(win, [69, 5], [0, 0]))
    whole.gather([70])
    with pytest.raises(RuntimeError, match="outside"):
        whole.check()
    whole.check()                                                       # reported once


def loaders(scene_d, H, W):
    from hsimae_amd import DeviceLoader, SceneCubes, unlabeled_pixels
    train = SceneCubes(scene_d, FX["loop_tr_i"], FX["loop_tr_y"], train=True)
    unl = SceneCubes(scene_d, unlabeled_pixels(H, W), train=True)
    val = SceneCubes(scene_d, FX["loop_va_i"], FX["loop_va_y"])
    train_dl = DeviceLoader(train, batch_size=3, shuffle=True)
    unl_bs = int(np.ceil(len(unl) / len(train_dl)) / 2)
    return train_dl, DeviceLoader(unl, batch_size=unl_bs, shuffle=True), DeviceLoader(val, batch_size=512, shuffle=False), unl_bs


def test_loaders_reproduce_the_reference_loops_batches_and_rng_positions():
    from hsimae_amd.pretrain import seed_everything
    scene = FX["A_scene"]
    H, W, Cb = scene.shape
    train_dl, unl_dl, val_dl, unl_bs = loaders(torch.from_numpy(scene).cuda(), H, W)
    assert unl_bs == int(FX["loop_unl_bs"]) and len(train_dl) == int(FX["loop_iters"]) and len(val_dl) == int(FX["loop_val_iters"])

    def same(x, key):
        want = torch.from_numpy(FX[key])
        assert x.dtype == want.dtype and x.shape == want.shape and torch.equal(x.cpu(), want), key

    for epoch in range(2):
        seed_everything(42 + epoch); labeled_iter = iter(train_dl)      # `stable(loader, 42 + epoch)`, both before any batch
        seed_everything(42 + epoch); unlabeled_iter = iter(unl_dl)
        for k in range(len(train_dl)):
            x, y = next(labeled_iter)
            x_u = next(unlabeled_iter)
            same(x, f"loop_e{epoch}_tr_x{k}"); same(y, f"loop_e{epoch}_tr_y{k}"); same(x_u, f"loop_e{epoch}_un_x{k}")
        seed_everything(42 + epoch)
        n_val = 0
        for k, (x, y) in enumerate(val_dl):
            same(x, f"loop_e{epoch}_va_x{k}"); same(y, f"loop_e{epoch}_va_y{k}")
            n_val += 1
        assert n_val == int(FX["loop_val_iters"])
        assert random.random() == float(FX[f"loop_e{epoch}_pyrand"])
        assert torch.equal(torch.rand(1), torch.from_numpy(FX[f"loop_e{epoch}_torchrand"]))
    for dl in (train_dl, unl_dl, val_dl):
        dl.dataset.check()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_unlabeled_set_equals_the_reference_tiles(tag):
    from hsimae_amd import SceneCubes, unlabeled_pixels
    scene = FX[f"{tag}_scene"]
    ds = SceneCubes(scene, unlabeled_pixels(scene.shape[0], scene.shape[1]))
    want = torch.tensor(FX[f"{tag}_cubes2"], dtype=torch.float32).permute(0, 3, 1, 2).unsqueeze(1)   # Model_Finetuning.py:54-55
    assert len(ds) == len(want) and torch.equal(ds.gather(list(range(len(ds)))).cpu(), want)
    ds.check()


def test_rank_path_of_the_device_loader():
    from hsimae_amd import DeviceLoader, SceneCubes
    scene, win, scene_d = scene_and_windows("10x7x32_f64")
    pix, lab = np.arange(0, 70, 3), np.arange(24) % 4
    ds = SceneCubes(scene_d, pix, lab, train=True)
    torch.manual_seed(1); random.seed(1)
    whole = [(x.cpu(), y.cpu()) for x, y in DeviceLoader(ds, batch_size=8, shuffle=True)]
    for rank in range(2):
        torch.manual_seed(1); random.seed(1)
        part = [(x.cpu(), y.cpu()) for x, y in DeviceLoader(ds, batch_size=4, shuffle=True, rank=rank, world=2)]
        assert len(part) == len(whole)
        for (x, y), (gx, gy) in zip(part, whole):
            assert torch.equal(x, gx[4 * rank:4 * rank + 4]) and torch.equal(y, gy[4 * rank:4 * rank + 4])


def test_gather_equals_the_existing_hsidataset_on_numpy_windows():
    from hsimae_amd import SceneCubes
    from hsimae_amd.finetune_train import HSIdataset
    scene, win, scene_d = scene_and_windows("10x7x32_f64")
    rng = np.random.default_rng(2)
    pix, lab = rng.permutation(70)[:30], rng.integers(0, 5, size=30)
    old = HSIdataset([win[p] for p in pix], lab, train=True)
    new = SceneCubes(scene_d, pix, lab, train=True)
    idx = rng.integers(0, 30, size=45)
    random.seed(9)
    ox, oy = old.batch(idx)
    after = random.random()
    random.seed(9)
    nx, ny = new.batch(idx)
    assert random.random() == after                                     # the same draws
    assert nx.shape == ox.shape and torch.equal(nx, ox) and torch.equal(ny, oy)
    old.train = new.train = False
    assert torch.equal(new.batch(idx)[0], old.batch(idx)[0])


def test_norm_and_split_of_get_scene_set_dual(tmp_path):
    from hsimae_amd import get_scene_set_dual
    for tag in ("A", "B"):
        raw, gt = FX[f"{tag}_scene"], FX[f"{tag}_gt"]
        np.save(tmp_path / "d.npy", raw); np.save(tmp_path / "g.npy", gt); np.save(tmp_path / "m.npy", FX[f"{tag}_mask"])
        np.random.seed(int(FX[f"{tag}_percent_seed"]))
        idx, lab, scene, test_gt, gt_raw = get_scene_set_dual(str(tmp_path / "d.npy"), str(tmp_path / "g.npy"), percent=0.3, GWPCA=False)
        assert np.array_equal(idx, FX[f"{tag}_percent_train_index"]) and np.array_equal(lab, FX[f"{tag}_percent_train_labels"])
        assert np.array_equal(test_gt, FX[f"{tag}_percent_test_gt"]) and np.array_equal(gt_raw, gt)
        assert scene.is_cuda and scene.dtype == torch.from_numpy(raw).dtype and np.array_equal(scene.cpu().numpy(), raw)
        idx, _, scene, _, _ = get_scene_set_dual(raw, gt, mask=str(tmp_path / "m.npy"), norm=True, GWPCA=False)
        assert np.array_equal(idx, FX[f"{tag}_mask_train_index"])
        want = (raw - np.min(raw)) / (np.max(raw) - np.min(raw))       # Utils/Preprocessing.py:195-198, in the scene's dtype
        assert want.dtype == raw.dtype and np.array_equal(scene.cpu().numpy(), want)


def test_three_datasets_on_a_shared_scene_allocate_only_their_tables():
    from hsimae_amd import SceneCubes, unlabeled_pixels
    H, W, Cb = 96, 80, 32
    scene_d = torch.rand(H, W, Cb, dtype=torch.float64, device="cuda")   # 1.9 MB: a copy would show
    rng = np.random.default_rng(0)
    tr, va, unl = rng.permutation(H * W)[:300], rng.permutation(H * W)[:200], unlabeled_pixels(H, W)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    sets = [SceneCubes(scene_d, tr, tr % 5, train=True), SceneCubes(scene_d, unl, train=True), SceneCubes(scene_d, va, va % 5)]
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    tables = 8 * (2 * len(tr) + len(unl) + 2 * len(va))
    print(f"[scene datasets] {grown} bytes allocated for {tables} bytes of tables; the scene has {scene_d.numel() * 8}")
    assert all(s.scene.data_ptr() == scene_d.data_ptr() for s in sets)
    assert grown <= tables + (1 << 20)


def toy_scene():
    """The separable toy classes of tests/test_gpu_dualvit.py (a spectral ramp per class + noise) as an 18 x 18 x 32 scene of
    6 x 6 single-class blocks."""
    rng = np.random.default_rng(0)
    bands, classes = 32, 3
    ramp = np.linspace(0, 1, bands, dtype=np.float32)
    gt_map = (1 + (np.arange(18)[:, None] // 6 + np.arange(18)[None, :] // 6) % classes).astype(np.int64)
    scene = np.empty((18, 18, bands), dtype=np.float32)
    for c in range(1, classes + 1):
        base = 0.25 + 0.2 * c * ramp if c % 2 else 0.75 - 0.2 * c * ramp
        scene[gt_map == c] = base
    scene = np.clip(scene + 0.05 * rng.standard_normal(scene.shape).astype(np.float32), 0, 1)
    labeled = np.sort(np.concatenate([rng.permutation(np.flatnonzero(gt_map.reshape(-1) == c))[:32] for c in range(1, classes + 1)]))
    return scene, labeled, gt_map.reshape(-1)[labeled]


def run_both_loops(out_dir):
    """Both fine-tuning runs from the same seeds; the checkpoints land in out_dir, the losses and scores in results.pt."""
    from hsimae_amd import dual_branch_finetuning, dual_branch_finetuning_scene
    from hsimae_amd.scene_data import tile_origins
    scene, labeled, gt = toy_scene()
    pad = np.pad(scene, ((4, 4), (4, 4), (0, 0)), "symmetric")
    data_cubes = np.stack([pad[r:r + 9, c:c + 9] for r in range(18) for c in range(18)])
    data_cubes_2 = np.stack([scene[r:r + 9, c:c + 9] for r in tile_origins(18) for c in tile_origins(18)])
    kw = dict(lr=2e-3, wd=5e-3, depth=4, dim=64, dec_depth=1, dec_dim=32, s_depth=2, epochs=3, mask_ratio=0.5, lamda=5, batch_size=16,
              log=lambda *_: None)
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(0); np.random.seed(0); random.seed(0)
        a = dual_branch_finetuning(data_cubes, list(labeled), data_cubes_2, gt, out_dir, "cubes.pkl", **kw)
        torch.manual_seed(0); np.random.seed(0); random.seed(0)
        b = dual_branch_finetuning_scene(scene, list(labeled), gt, out_dir, "scene.pkl", **kw)
    torch.save({"cubes": a, "scene": b}, os.path.join(out_dir, "results.pt"))


def test_scene_loop_equals_the_cube_loop_bit_for_bit(tmp_path):
    """dual_branch_finetuning on numpy-built data_cubes / data_cubes_2 against dual_branch_finetuning_scene on the scene: the
    loss lists, the validation scores and every tensor of the checkpoints are compared for equality (no margin).
    The two runs share one child process of their own: a training run leaves process-wide state behind (the library's table
    of arenas a forward has filled, the caching allocator's blocks) that the tests after this one should not inherit."""
    import subprocess
    env = dict(os.environ, HSIMAE_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = torch.load(os.path.join(str(tmp_path), "results.pt"), weights_only=False)
    a, b = res["cubes"], res["scene"]
    print(f"[loop equality] train loss {a[1]} / {b[1]}, val loss {a[2]} / {b[2]}")
    assert a[1] == b[1] and a[2] == b[2]
    assert a[0][:3] == b[0][:3] and np.array_equal(a[0][3], b[0][3])
    sa, sb = (torch.load(os.path.join(str(tmp_path), n), map_location="cpu") for n in ("cubes.pkl", "scene.pkl"))
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert np.isfinite(a[1]).all() and np.isfinite(a[2]).all()


if __name__ == "__main__":
    run_both_loops(sys.argv[1])
