"""bench.py on one GPU: the one-line JSON contract of the driver and the roofline objects it carries."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    d = json.loads(lines[-1])                                     # the LAST line of stdout is the JSON line
    assert sum(l.lstrip().startswith("{") for l in lines) == 1
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "patches/s" and d["dtype"] == "bf16" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] in ("mfma", "hbm") and rf["unit"] in ("TFLOP/s", "GB/s") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    # per-kernel and per-group evidence: the dominant encoder kernels, the decoder group and one fused decoder Block
    for k in ("roofline_kernel", "roofline_kernel_hbm", "roofline_decoder", "roofline_decoder_block", "encoder_mfma_frac", "step_ms"):
        assert k in d, k
    # the line says what library produced it (VERDICT r05 "Next round" 5): the shipped one, built from these sources, no variant switch
    b = d["build"]
    assert b["variant"] == [] and b["variant_bits"] == 0 and b["default_flags"] is True and b["matches_sources"] is True
    blk = d["roofline_decoder_block"]
    assert 50 < blk["fwd_us"] < 1000 and 100 < blk["bwd_us"] < 3000 and 0 < blk["frac"] < 1


@pytest.mark.gpu
def test_bench_data_parallel_line_carries_the_self_check():
    """`bench.py --verify` (on with --full whenever the reducer runs): the 1-rank RCCL path (`--force-ddp`: real all-reduces of
    every bucket) must report a consistent step — the bucketed, backward-overlapped reduction equals one plain all-reduce of the
    same step's local gradients — and list the buckets it issued."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--force-ddp", "--full",
                        "--no-extras"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.lstrip().startswith("{")][-1])
    assert d["dp_consistent"] is True, d.get("dp_verify")
    v = d["dp_verify"]
    assert v["ranks"] == 1 and v["matches_single_collective"] is True and len(v["buckets"]) >= 3
    assert sum(hi - lo for lo, hi in v["buckets"]) * 4 == d["comm"]["bytes"]


@pytest.mark.gpu
def test_plain_bench_is_lean_and_dumps_the_same_outputs_run_after_run(tmp_path):
    """A plain run times the steps and prints the line, nothing after them (the replay / CPU legs are --full only).
    `--dump-outputs DIR` writes what the last timed step returned (loss, pred, mask, every parameter gradient) as float32 .npy
    within 64 MB; two runs with the same arguments see the same inputs, so the mask is bit-identical and the rest agrees up to
    summation order."""
    import numpy as np
    runs = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert sum(l.lstrip().startswith("{") for l in lines) == 1
        d = json.loads(lines[-1])
        assert d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "bf16" and d["ms_per_step"] > 0
        for k in ("roofline_kernel", "roofline_decoder", "encoder_mfma_frac", "optimizer_step_ms", "input_pipeline", "cpu_baseline",
                  "comm", "dp_verify"):
            assert k not in d, k
        files = sorted(os.listdir(tmp_path / tag))
        assert sum(os.path.getsize(tmp_path / tag / f) for f in files) <= 64 << 20
        out = {f[:-4]: np.load(tmp_path / tag / f) for f in files}
        assert all(a.dtype == np.float32 for a in out.values())
        # 533 parameters; mask_token is never used (kept for the state-dict format) and gets no gradient
        assert {"loss", "pred", "mask"} <= set(out) and sum(k.startswith("grad.") for k in out) == 532 and "grad.mask_token" not in out
        assert abs(float(out["loss"]) - d["loss"]) <= 1e-5 * abs(d["loss"]) + 1e-6        # (the line rounds to 6 decimals)
        runs.append(out)
    a, b = runs
    assert a.keys() == b.keys()
    assert np.array_equal(a["mask"], b["mask"]) and set(np.unique(a["mask"])) <= {0.0, 1.0}
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-5 * abs(float(a["loss"]))
    assert np.allclose(a["pred"], b["pred"], rtol=1e-4, atol=1e-5)
    for k in a:
        if k.startswith("grad."):
            assert np.isfinite(a[k]).all(), k
            assert np.linalg.norm(a[k] - b[k]) <= 1e-3 * np.linalg.norm(a[k]) + 1e-12, k
