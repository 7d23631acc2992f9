"""bench.py host logic without a GPU: the --dump-outputs writer (budget, seeded samples) and the argument checks."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_stays_within_64_mb_with_seeded_samples(tmp_path):
    """Outputs of the huge model's size (pred / mask 32 M floats each, 67 M gradient elements): every file float32, 64 MB in all,
    small arrays whole, large ones sampled at the same positions in every call, pred and mask at the same positions."""
    g = torch.Generator().manual_seed(0)
    model = torch.nn.Module()
    model.big = torch.nn.Parameter(torch.zeros(8192, 8192))
    model.small = torch.nn.Parameter(torch.zeros(64))
    model.frozen = torch.nn.Parameter(torch.zeros(3))                 # no .grad: nothing written
    model.big.grad = torch.randn(8192, 8192, generator=g)
    model.small.grad = torch.randn(64, generator=g)
    pred = torch.randn(4096, 1, 96, 9, 9, generator=g)
    mask = (pred > 0).float()
    loss = torch.tensor(0.5)
    for tag in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / tag), loss, pred, mask, model) == 5
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grad.big.npy", "grad.small.npy", "loss.npy", "mask.npy", "pred.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    a = {f: np.load(tmp_path / "a" / f) for f in files}
    b = {f: np.load(tmp_path / "b" / f) for f in files}
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[f], b[f]) for f in files)
    assert float(a["loss.npy"]) == 0.5
    assert np.array_equal(a["grad.small.npy"], model.small.grad.numpy())
    assert a["pred.npy"].size == bench.DUMP_IMG_ELEMS and np.array_equal(a["mask.npy"], (a["pred.npy"] > 0).astype(np.float32))
    assert 0 < a["grad.big.npy"].size <= bench.DUMP_GRAD_ELEMS and a["grad.big.npy"].ndim == 1
    assert np.isin(a["grad.big.npy"], model.big.grad.numpy()).all()


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
