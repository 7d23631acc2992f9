"""Fine-tuning from the scene on CPU: the host arithmetic of hsimae_amd.scene_data (tile origins, the unlabeled set's centre
pixels, the train / test split) against the records made by the reference (tests/golden/make_golden_scene_batches.py), and
the declaration, export and argument refusals of hsimae_scene_batch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FX = np.load(os.path.join(ROOT, "tests", "golden", "scene_batches.npz"))


def test_tile_origins_equal_the_reference_record():
    from hsimae_amd.scene_data import tile_origins
    at = 0
    for L, n in zip(FX["origins_length"], FX["origins_count"]):
        want = FX["origins_cat"][at:at + n]
        at += n
        got = tile_origins(int(L))
        assert got.dtype == np.int64 and np.array_equal(got, want), (L, got, want)
    assert at == len(FX["origins_cat"])
    for L, want in ((9, [0]), (10, [0, 1]), (19, [0, 9, 10]), (30, [0, 9, 18, 21])):
        assert tile_origins(L).tolist() == want


@pytest.mark.parametrize("L", range(9, 41))
def test_tiles_cover_the_axis(L):
    from hsimae_amd.scene_data import tile_origins
    o = tile_origins(L)
    assert o[0] == 0 and o[-1] == L - 9
    assert np.all(np.diff(o[:-1]) == 9) and (len(o) == 1 or 0 < o[-1] - o[-2] <= 9)
    covered = np.zeros(L, dtype=bool)
    for a in o:
        covered[a:a + 9] = True
    assert covered.all()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_unlabeled_pixels_are_the_centres_of_the_reference_tiles(tag):
    from hsimae_amd.scene_data import unlabeled_pixels
    scene = FX[f"{tag}_scene"]
    H, W, _ = scene.shape
    got = unlabeled_pixels(H, W)
    assert got.dtype == np.int64 and np.array_equal(got, FX[f"{tag}_unl_centres"])
    # ... and the unpadded tile around such a centre is the recorded data_cubes_2 item
    for p, tile in zip(got, FX[f"{tag}_cubes2"]):
        r, c = divmod(int(p), W)
        assert np.array_equal(scene[r - 4:r + 5, c - 4:c + 5], tile)


def test_unlabeled_pixels_refuse_a_scene_smaller_than_a_tile():
    from hsimae_amd.scene_data import unlabeled_pixels
    for H, W in ((8, 20), (20, 8), (3, 5)):
        with pytest.raises(ValueError, match="smaller"):
            unlabeled_pixels(H, W)
    assert unlabeled_pixels(9, 9).tolist() == [4 * 9 + 4]


@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("mode", ["num", "percent", "mask"])
def test_split_labeled_equals_the_reference_record(tag, mode):
    from hsimae_amd.scene_data import split_labeled
    kw = {"num": dict(num=2), "percent": dict(percent=0.3), "mask": dict(mask=FX[f"{tag}_mask"])}[mode]
    np.random.seed(int(FX[f"{tag}_{mode}_seed"]))
    train_index, train_labels, test_gt = split_labeled(FX[f"{tag}_gt"], **kw)
    after = np.random.rand()
    assert np.array_equal(train_index, FX[f"{tag}_{mode}_train_index"])            # the reference's encounter order
    assert np.array_equal(train_labels, FX[f"{tag}_{mode}_train_labels"])
    assert test_gt.shape == FX[f"{tag}_gt"].shape and np.array_equal(test_gt, FX[f"{tag}_{mode}_test_gt"])
    assert after == float(FX[f"{tag}_{mode}_rand"])                                 # one permutation drawn, or none (mask)
    assert len(train_index) > 0 and np.all(FX[f"{tag}_gt"].reshape(-1)[train_index] == train_labels)


def loop_split(gt, percent=None, num=None):
    """Utils/Preprocessing.py:243-269 as a plain walk over the shuffled pixels (the form split_labeled vectorises)."""
    gt = np.asarray(gt).reshape(-1)
    n_classes = int(gt.max()) + 1
    shuffled = np.random.permutation(np.arange(len(gt)))
    count = np.array([np.sum(gt == c) for c in range(n_classes)])
    quota = np.ceil(count * percent) if percent else np.where(count == num, num - 5, num)
    seen, train = np.zeros(n_classes), []
    for p in shuffled:
        c = gt[p]
        if c:
            seen[c] += 1
            if seen[c] <= quota[c]:
                train.append(p)
    return np.array(train, dtype=np.int64)


def test_split_labeled_keeps_the_num_minus_5_quirk_and_equals_the_walk():
    from hsimae_amd.scene_data import split_labeled
    gt = np.zeros(400, dtype=np.int64)
    gt[:7] = 1                                                          # exactly num pixels: quota num - 5 = 2
    gt[7:30] = 2
    gt[30:36] = 3                                                       # fewer than num: all of them
    gt[36:200] = 4
    gt = np.random.default_rng(1).permutation(gt).reshape(20, 20)
    np.random.seed(11)
    idx, lab, test_gt = split_labeled(gt, num=7)
    assert np.bincount(lab, minlength=5).tolist() == [0, 2, 7, 6, 7]
    assert np.array_equal(test_gt.reshape(-1) == 0, (gt.reshape(-1) == 0) | np.isin(np.arange(400), idx))
    np.random.seed(11)
    assert np.array_equal(idx, loop_split(gt, num=7))
    for seed, pc in ((12, 0.1), (13, 0.5), (14, 1.0)):
        np.random.seed(seed)
        idx, _, _ = split_labeled(gt, percent=pc)
        np.random.seed(seed)
        assert np.array_equal(idx, loop_split(gt, percent=pc))
    with pytest.raises(AssertionError):                                 # a class of 0 .. max is missing
        split_labeled(np.array([[0, 1, 3]]), num=1)
    with pytest.raises(AssertionError):
        split_labeled(gt, mask=np.ones(5))
    with pytest.raises(ValueError):
        split_labeled(gt)


def test_spilt_dataset_on_the_index_list_equals_the_reference_record():
    """Model_Finetuning.py:111: the reference splits the labeled INDEX list; dual_branch_finetuning_scene does the same."""
    from hsimae_amd.finetune_train import spilt_dataset
    np.random.seed(int(FX["loop_split_seed"]))
    tr_i, tr_y, va_i, va_y = spilt_dataset(list(FX["A_percent_train_index"]), FX["A_percent_train_labels"], training_ratio=0.5)
    assert np.random.rand() == float(FX["loop_split_rand"])
    for got, key in ((tr_i, "loop_tr_i"), (tr_y, "loop_tr_y"), (va_i, "loop_va_i"), (va_y, "loop_va_y")):
        assert np.array_equal(np.asarray(got), FX[key]), key


def test_python_argument_refusals():
    from hsimae_amd.scene_data import SceneCubes, get_scene_set_dual
    good = np.zeros((9, 10, 8), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="patch_size"):
        get_scene_set_dual(good, np.zeros((9, 10), dtype=np.int64), patch_size=7, num=1, GWPCA=False)
    with pytest.raises(ValueError, match="H, W, C"):
        SceneCubes(np.zeros((9, 10), dtype=np.float32))
    with pytest.raises(ValueError, match="float32 or float64"):
        SceneCubes(np.zeros((9, 10, 8), dtype=np.int32))
    with pytest.raises(ValueError, match="out of range"):
        SceneCubes(good, pixels=[0, 90])
    with pytest.raises(ValueError, match="out of range"):
        SceneCubes(good, pixels=[-1])
    with pytest.raises(ValueError, match="integer"):
        SceneCubes(good, pixels=np.array([0.5]))
    with pytest.raises(ValueError, match="labels for"):
        SceneCubes(good, pixels=[0, 1], gt=[1])
    with pytest.raises(ValueError, match="labels for"):
        SceneCubes(good, gt=[1, 2])
    with pytest.raises(RuntimeError, match="GPU"):                      # valid arguments, no device: no CPU fallback
        SceneCubes(good, pixels=[0, 1], gt=[1, 2], device="cpu")


def test_header_library_and_bindings_have_the_entry_point_under_abi_108():
    import hsimae_amd
    from hsimae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hsimae_hip.h")).read()
    assert re.search(r"\bint hsimae_scene_batch\(const hsimae_scene_batch_params\* p, void\* stream\);", hdr)
    lib = _lib.load()
    assert "hsimae_scene_batch" in _lib.SYMBOLS and lib.hsimae_scene_batch is not None
    assert lib.hsimae_version() == 108 == _lib.ABI_VERSION
    # the ctypes mirror has the header's fields, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} hsimae_scene_batch_params;", hdr).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?=,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.SceneBatchParams._fields_]
    for name in ("SceneCubes", "get_scene_set_dual", "split_labeled", "tile_origins", "unlabeled_pixels", "dual_branch_finetuning_scene"):
        assert callable(getattr(hsimae_amd, name))


def test_scene_batch_refusals_need_no_gpu():
    from hsimae_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float64)                          # host memory: every call below returns before a launch
    a = buf.data_ptr()
    ENULL, EDIMS, EALIGN = -4, -1, -3

    def call(**over):
        kw = dict(scene=a, scene_f64=0, H=4, W=5, C=8, items=a, N=3, n_items=20, pixels=None, labels=None, flips=None, out=a,
                  sn=648, sb=1, sh=72, sw=8, y=None, bad=a)
        kw.update(over)
        return lib.hsimae_scene_batch(C.byref(_lib.SceneBatchParams(**kw)), None)

    assert lib.hsimae_scene_batch(None, None) == ENULL
    assert call(bad=None) == ENULL
    for name in ("scene", "items", "out"):
        assert call(**{name: None}) == ENULL
    assert call(labels=a) == ENULL                                      # labels without y
    assert call(y=a) == ENULL                                           # y without labels
    for name in ("H", "W", "C"):
        assert call(**{name: 0}) == EDIMS and call(**{name: -3}) == EDIMS
    assert call(N=-1) == EDIMS
    assert call(n_items=-1) == EDIMS
    assert call(scene=a + 2) == EALIGN
    assert call(scene=a + 4, scene_f64=1) == EALIGN
    for name in ("items", "pixels"):
        assert call(**{name: a + 4}) == EALIGN
    assert call(labels=a + 4, y=a) == EALIGN and call(labels=a, y=a + 4) == EALIGN
    assert call(out=a + 2) == EALIGN and call(bad=a + 2) == EALIGN
    assert call(N=0) == 0 and call(N=0, scene=None, items=None, out=None) == 0
    assert not buf.any()                                                # N = 0 wrote nothing (and nothing else ran)
