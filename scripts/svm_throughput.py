"""Timings of the RBF support-vector classifier (csrc/svm.hip, hsimae_amd/svm.py) on one MI355X, for profiles/EXPERIMENTS.md.

Synthetic 610 x 340 x 32 scene with 16 classes (Gaussian class signatures plus noise):
  (a) one RBFSVM.fit at banks of 640 and 4,300 rows (spectra), with the solver's iteration counts;
  (b) RBFSVM.fit_reference (both grid stages: 35 + 225 points) at 640 rows; with --sklearn the same grid through sklearn on the
      host's CPUs, when sklearn imports;
  (c) svm_scene pixels/s for spectra and for encoder features, next to knn_scene in the same process;
  (d) --profile: only (a) and the spectra half of (c), for a `rocprofv3 --kernel-trace --stats -- python scripts/svm_throughput.py
      --profile` run of its own.
Prints one JSON line per item.  Usage: python scripts/svm_throughput.py [--profile] [--sklearn] [--skip-search] [--sklearn-only: no GPU, (b)'s sklearn half alone]"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hsimae_amd import HSIViT, RBFSVM  # noqa: E402

H, W, BANDS, CLASSES = 610, 340, 32, 16


def scene_and_labels(seed=0):
    rng = np.random.RandomState(seed)
    truth = rng.randint(1, CLASSES + 1, (H // 10 + 1, W // 10 + 1)).repeat(10, 0).repeat(10, 1)[:H, :W]
    sig = rng.standard_normal((CLASSES + 1, BANDS))
    return (sig[truth] + 0.8 * rng.standard_normal((H, W, BANDS))).astype(np.float32), truth


def bank_of(truth, per_class, seed=1):
    rng = np.random.RandomState(seed)
    flat = truth.reshape(-1)
    pix = np.concatenate([rng.choice(np.flatnonzero(flat == c), per_class, replace=False) for c in range(1, CLASSES + 1)])
    return pix, flat[pix]


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return min(ts), out


def solver_slope(rows, truth):
    """Time per SMO iteration of ONE two-class problem, as the slope between max_iter = 200 and 1,200 (C = 2^9 and eps = 1e-12 keep it
    running on rows whose sides ignore their classes), for n = 80, 538 and 4,096 variables: the launch and everything outside the loop cancel."""
    import ctypes as C
    from hsimae_amd import _lib
    for per_class in (40, 269, 2048):
        x = rows[:2 * per_class].contiguous()                  # the first pixels, dealt to the two sides whatever their class:
        #                                                        a problem that does not converge within the iterations timed
        M = int(x.shape[0])
        K = torch.empty(1, M, M, dtype=torch.float32, device="cuda")
        ss = torch.empty(M, dtype=torch.float32, device="cuda")
        g = _lib.SvmGramParams(x=x.data_ptr(), ldx=x.stride(0), M=M, D=BANDS, n_gamma=1, gamma=(C.c_float * 16)(1.0 / BANDS), K=K.data_ptr(),
                               ldk=M, sumsq=ss.data_ptr())
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().hsimae_svm_gram(C.byref(g), st), "hsimae_svm_gram")
        table = torch.tensor([[0, np.float64(512.0).view(np.int64), 0, per_class, per_class, M - per_class, 0, 0]], dtype=torch.int64).cuda()
        alpha, grad = torch.zeros(M, dtype=torch.float64, device="cuda"), torch.zeros(M, dtype=torch.float64, device="cuda")
        state = torch.zeros(8, dtype=torch.float64, device="cuda")
        out = {}
        for iters in (200, 1200):
            p = _lib.SvmSolveParams(K=K.data_ptr(), ldk=M, M=M, n_k=1, table=table.data_ptr(), n_problems=1, resume=0, max_iter=iters,
                                    eps=1e-12, alpha=alpha.data_ptr(), grad=grad.data_ptr(), alpha_len=M, state=state.data_ptr())
            t, _ = timed(lambda: _lib.check(_lib.load().hsimae_svm_solve(C.byref(p), st), "hsimae_svm_solve"), reps=5)
            out[iters] = (t, float(state[0].item()))
        (t1, i1), (t2, i2) = out[200], out[1200]
        print(json.dumps({"item": "solver_slope", "n": M, "iterations": [i1, i2], "ms": [1e3 * t1, 1e3 * t2],
                          "us_per_iteration": 1e6 * (t2 - t1) / max(1.0, i2 - i1)}))


def sklearn_grid(xs, y):
    """The reference's two stages and its refit through sklearn on this host's CPU, scored as the reference scores."""
    try:
        from sklearn.svm import SVC
    except ImportError:
        print(json.dumps({"item": "sklearn_grid", "skipped": "sklearn does not import here"}))
        return
    from hsimae_amd.finetune_train import scores, spilt_dataset
    from hsimae_amd.svm import reference_grid
    np.random.seed(0)
    t0, n = time.perf_counter(), 0
    best = (1.0, 1.0)
    for stage in (reference_grid(), None):
        cs, gs = stage if stage else reference_grid(*best)
        tr, _, va, _ = spilt_dataset(np.arange(y.size), y, training_ratio=0.5)
        top = 0.0
        for cc in cs:
            for gg in gs:
                pred = SVC(C=cc, gamma=gg, kernel="rbf").fit(xs[tr], y[tr]).predict(xs[va])
                metric = sum(scores(y[va], pred)[:3])                               # OA + AA + kappa, the reference's score
                n += 1
                if metric > top:
                    top, best = metric, (cc, gg)
    SVC(C=best[0], gamma=best[1], kernel="rbf").fit(xs[tr], y[tr])                   # the refit on the training half
    print(json.dumps({"item": "sklearn_grid", "rows": int(y.size), "fits": n + 1, "s": time.perf_counter() - t0, "C": best[0],
                      "gamma": best[1], "cpus_available": len(os.sched_getaffinity(0)), "note": "libsvm runs one thread per fit"}))


def main():
    profile, with_sklearn, skip_search = (f in sys.argv for f in ("--profile", "--sklearn", "--skip-search"))
    scene, truth = scene_and_labels()
    if "--sklearn-only" in sys.argv:                                                 # no GPU needed: (b)'s comparison alone
        pix, y = bank_of(truth, 40)
        return sklearn_grid(scene.reshape(-1, BANDS)[pix].astype(np.float64), y)
    rows = torch.from_numpy(scene.reshape(-1, BANDS)).cuda()
    for per_class in (40, 269):                                                      # (a): 640 and 4,304 rows
        pix, y = bank_of(truth, per_class)
        x, yd = rows[torch.from_numpy(pix).cuda()], torch.from_numpy(y).cuda()
        svm = RBFSVM(CLASSES + 1, C=8.0, gamma=1.0 / BANDS)
        t, _ = timed(lambda: svm.fit(x, yd))
        it = svm.iterations.cpu().numpy()
        print(json.dumps({"item": "fit", "rows": int(x.shape[0]), "ms": 1e3 * t, "iterations_max": float(it.max()),
                          "iterations_sum": float(it.sum()), "support": int(svm.n_support.sum()),
                          "us_per_iteration_of_the_longest_problem": 1e6 * t / max(1.0, float(it.max()))}))
    solver_slope(rows, truth)
    pix, y = bank_of(truth, 40)
    x = rows[torch.from_numpy(pix).cuda()]
    if not profile and not skip_search:                                              # (b)
        np.random.seed(0)
        svm = RBFSVM(CLASSES + 1)
        t0 = time.perf_counter()
        c, g, _ = svm.fit_reference(x, y)
        torch.cuda.synchronize()
        print(json.dumps({"item": "fit_reference", "rows": 640, "s": time.perf_counter() - t0, "C": c, "gamma": g}))
        if with_sklearn:
            sklearn_grid(x.cpu().numpy().astype(np.float64), y)
    torch.manual_seed(0)                                                             # (c)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIViT(img_size=9, patch_size=3, in_chans=1, bands=BANDS, b_patch_size=8, num_class=CLASSES + 1, embed_dim=96, depth=12,
                   num_heads=6, s_depth=6, sep_pos_embed=True, use_learnable_pos_emb=False).cuda().eval()
    dscene = torch.from_numpy(scene).cuda()
    kinds = [("svm_scene spectra", lambda: m.svm_scene(dscene, pix, y, features="spectra", C=8.0, gamma=1.0 / BANDS, on_device=True))]
    if not profile:
        kinds += [("svm_scene encoder", lambda: m.svm_scene(dscene, pix, y, features="encoder", C=8.0, gamma="scale", on_device=True)),
                  ("knn_scene", lambda: m.knn_scene(dscene, pix, y, on_device=True))]
    for name, fn in kinds:
        t, _ = timed(fn, reps=2)
        print(json.dumps({"item": name, "bank": 640, "s": t, "pixels_per_s": H * W / t}))


if __name__ == "__main__":
    main()
