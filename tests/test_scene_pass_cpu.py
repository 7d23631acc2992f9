"""The host side every whole-scene entry point shares (hsimae_amd/scene_pass.py: largest_chunk, pixel_indices, as_scene) and the
one checkpoint loader of the evaluation wrappers (checkpoint.load_matching).  Nothing here needs a GPU: hsimae_workspace_bytes
and the model's config are host code."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from test_scene_cpu import tiny_hsivit  # noqa: E402


@pytest.fixture(scope="module")
def sizing():
    """(lib, cfg, (T, L), bytes(n, grid)) of the tiny HSIViT (bands 32, dim 32, depth 2)."""
    from hsimae_amd import _lib
    m = tiny_hsivit()
    lib, cfg = _lib.load(), m._config()
    grid = (m.input_size[0], m.input_size[1] ** 2)
    assert grid == (4, 9)

    def nbytes(n, g=grid):
        return lib.hsimae_workspace_bytes(C.byref(cfg), n, g[0], g[1])
    return lib, cfg, grid, nbytes


def test_largest_chunk_fits_the_budget_and_the_caps(sizing):
    from hsimae_amd.scene_pass import largest_chunk
    lib, cfg, grid, nbytes = sizing
    budget = nbytes(5)
    assert nbytes(6) > budget > 0
    assert largest_chunk(lib, cfg, [grid], 8192, budget) == 5
    assert largest_chunk(lib, cfg, [grid], 3, budget) == 3
    assert largest_chunk(lib, cfg, [grid], 8192, 0) == 1                # never below 1
    assert largest_chunk(lib, cfg, [grid], 8192, budget, cap=2) == 2
    assert largest_chunk(lib, cfg, [grid], 8192, budget, cap=100) == 5


def test_largest_chunk_with_two_grids_is_the_smaller_of_the_two(sizing):
    from hsimae_amd.scene_pass import largest_chunk
    lib, cfg, grid, nbytes = sizing
    small = (2, 3)
    budget = nbytes(5)
    a, b = largest_chunk(lib, cfg, [grid], 8192, budget), largest_chunk(lib, cfg, [small], 8192, budget)
    assert a == 5 and b > a                                             # fewer tokens per window: more windows fit
    assert largest_chunk(lib, cfg, [grid, small], 8192, budget) == min(a, b)
    assert largest_chunk(lib, cfg, [small, grid], 8192, budget) == min(a, b)


def test_largest_chunk_equals_a_linear_scan(sizing):
    from hsimae_amd.scene_pass import largest_chunk
    lib, cfg, grid, nbytes = sizing
    for n in range(1, 13):
        budget = nbytes(n)
        for batch_size in (1, 7, 12, 40):
            fits = [k for k in range(1, batch_size + 1) if 0 <= nbytes(k) <= budget]
            assert largest_chunk(lib, cfg, [grid], batch_size, budget) == max(fits, default=1), (n, batch_size)


def test_scene_chunk_wrappers_are_largest_chunk(sizing):
    from hsimae_amd import HSIMAE
    from hsimae_amd.recon import _recon_chunk
    from hsimae_amd.scene_pass import largest_chunk
    lib, cfg, grid, _ = sizing
    m = tiny_hsivit()
    assert m._scene_chunk(37) == largest_chunk(lib, cfg, [grid], 37, m.SCENE_WORKSPACE_BUDGET) == 37
    mae = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=16, b_patch_size=8, embed_dim=64, depth=2, num_heads=4, s_depth=1,
                 decoder_embed_dim=48, decoder_depth=1, decoder_num_heads=6)
    assert _recon_chunk(mae, 0.75, 4096, 11) == 11 and _recon_chunk(mae, 0.75, 6, 11) == 6


def test_pixel_indices_accepts_integer_lists_arrays_and_tensors():
    from hsimae_amd.scene_pass import pixel_indices
    for given in ([3, 0, 19], np.array([3, 0, 19], dtype=np.int32), torch.tensor([3, 0, 19], dtype=torch.int64)):
        p = pixel_indices(given, 20)
        assert p.dtype == torch.int64 and p.device.type == "cpu" and p.is_contiguous() and p.tolist() == [3, 0, 19]
    p = pixel_indices(torch.arange(0, 20, 2)[::2], 20)                  # a strided view comes back contiguous
    assert p.is_contiguous() and p.tolist() == [0, 4, 8, 12, 16]
    p = pixel_indices([], 20, allow_empty=True)
    assert p.dtype == torch.int64 and p.numel() == 0
    assert pixel_indices(torch.zeros(0, dtype=torch.int32), 20).numel() == 0        # allow_empty is the default


def test_pixel_indices_refuses_what_is_no_pixel_list():
    from hsimae_amd.scene_pass import pixel_indices
    for bad in (np.array([0.5]), torch.tensor([1.0, 2.0]), np.array([True, False]), np.zeros((2, 2), dtype=np.int64), 3):
        with pytest.raises(ValueError, match="integer"):
            pixel_indices(bad, 20)
    for bad in ([-1], [0, 20], torch.tensor([5, 20])):
        with pytest.raises(ValueError, match="out of range"):
            pixel_indices(bad, 20)
    with pytest.raises(ValueError, match="fit_pixels: pixel index out of range"):
        pixel_indices([20], 20, what="fit_pixels")
    with pytest.raises(ValueError, match="init must be a non-empty 1-D array of integer"):
        pixel_indices([], 20, what="init", allow_empty=False)
    with pytest.raises(ValueError, match="integer"):
        pixel_indices(torch.zeros(0, dtype=torch.int64), 20, allow_empty=False)
    assert pixel_indices([19], 20, allow_empty=False).tolist() == [19]


def test_as_scene_checks_and_keeps_a_tensor_in_place():
    from hsimae_amd.scene_data import device_scene
    from hsimae_amd.scene_pass import as_scene
    with pytest.raises(ValueError, match="H, W, C"):
        as_scene(np.zeros((20, 32), dtype=np.float32))
    with pytest.raises(ValueError, match="float32 or float64"):
        as_scene(np.zeros((4, 5, 32), dtype=np.int32))
    with pytest.raises(ValueError, match="float32 or float64"):
        as_scene(torch.zeros(4, 5, 32, dtype=torch.float16))
    for shape in ((0, 5, 32), (4, 0, 32), (4, 5, 0)):
        with pytest.raises(ValueError, match="empty scene"):
            as_scene(np.zeros(shape, dtype=np.float64))
    with pytest.raises(ValueError, match="H, W, C"):                    # scene_data's checks are these
        device_scene(np.zeros((20, 32), dtype=np.float32), "cpu")
    t = torch.zeros(4, 5, 32, dtype=torch.float64)
    s = as_scene(t)
    assert s.data_ptr() == t.data_ptr() and s.shape == t.shape and s.dtype == t.dtype
    v = torch.zeros(5, 4, 32).transpose(0, 1)                           # a view is not copied either
    assert as_scene(v).data_ptr() == v.data_ptr() and as_scene(v).stride() == v.stride()
    a = np.arange(4 * 5 * 8, dtype=np.float32).reshape(4, 5, 8)
    assert torch.equal(as_scene(a), torch.from_numpy(a)) and torch.equal(as_scene(a[:, ::-1]), torch.from_numpy(a).flip(1))


def test_scene_array_adds_the_models_checks_to_as_scene():
    from hsimae_amd.finetune import scene_array
    s, H, W, Cb = scene_array(np.zeros((4, 5, 32), dtype=np.float32), 32, 1)
    assert (H, W, Cb) == (4, 5, 32) and tuple(s.shape) == (4, 5, 32)
    with pytest.raises(ValueError, match="multiple of 8"):
        scene_array(np.zeros((4, 5, 12), dtype=np.float32), 12, 1)
    with pytest.raises(ValueError, match="bands=32"):
        scene_array(np.zeros((4, 5, 16), dtype=np.float32), 32, 1)
    with pytest.raises(ValueError, match="batch_size"):
        scene_array(np.zeros((4, 5, 32), dtype=np.float32), 32, 0)
    with pytest.raises(ValueError, match="empty scene"):
        scene_array(np.zeros((0, 5, 32), dtype=np.float32), 32, 1)


def test_cluster_scene_checks_the_scene_then_the_device():
    m = tiny_hsivit()
    good = np.zeros((4, 5, 32), dtype=np.float32)
    with pytest.raises(ValueError, match="out of range"):
        m.cluster_scene(good, 3, pixels=[0, 20])
    for features in ("encoder", "spectra"):                             # the spectra take any band count, but a scene it must be
        with pytest.raises(ValueError, match="H, W, C"):
            m.cluster_scene(np.zeros((20, 32), dtype=np.float32), 3, features=features)
        with pytest.raises(ValueError, match="float32 or float64"):
            m.cluster_scene(np.zeros((4, 5, 32), dtype=np.int32), 3, features=features)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.cluster_scene(good, 3, features=features, fit_pixels=[0, 1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.cluster_scene(np.zeros((4, 5, 13), dtype=np.float32), 3, features="spectra")


def tiny_net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2)).train()


def test_load_matching_filters_by_key_and_on_request_by_shape(tmp_path):
    from hsimae_amd.checkpoint import load_matching
    src = tiny_net(1).state_dict()
    extra = dict(src, **{"2.weight": torch.ones(2, 2)})                 # a key the model does not have
    del extra["1.bias"]                                                 # ... and one it has that the file lacks
    wrong = dict(src, **{"1.weight": torch.ones(5, 3)})                 # a tensor of another shape
    torch.save(extra, tmp_path / "extra.pkl")
    torch.save(wrong, tmp_path / "wrong.pkl")
    for match_shapes in (True, False):
        m = tiny_net(2)
        init = {k: v.clone() for k, v in m.state_dict().items()}
        assert load_matching(m, tmp_path / "extra.pkl", "cpu", match_shapes) is m and not m.training
        got = m.state_dict()
        assert set(got) == set(init)
        assert all(torch.equal(got[k], src[k]) for k in got if k != "1.bias") and torch.equal(got["1.bias"], init["1.bias"])
        assert not torch.equal(got["0.weight"], init["0.weight"])
    m = tiny_net(2)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    load_matching(m, tmp_path / "wrong.pkl", "cpu", match_shapes=True)
    got = m.state_dict()
    assert torch.equal(got["1.weight"], init["1.weight"])               # the mismatched tensor keeps its initial value
    assert all(torch.equal(got[k], src[k]) for k in got if k != "1.weight")
    m = tiny_net(2)
    with pytest.raises(RuntimeError, match="size mismatch"):
        load_matching(m, tmp_path / "wrong.pkl", "cpu", match_shapes=False)
