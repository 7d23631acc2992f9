"""Records sklearn's SVC(kernel='rbf', decision_function_shape='ovo') on the inputs of tests/test_gpu_svm.py and
tests/test_svm_bound_cpu.py -> tests/golden/svm_cases.npz.  The inputs are regenerated from seeds (tests/svm_ref.py: clusters);
only sklearn's outputs are stored.  Run from the repository root: python tests/golden/make_golden_svm.py (needs scikit-learn;
the tests themselves do not).

Per case c7 / c16 (Gaussian clusters, D = 32, gamma = 1 / D, C = 8, 20 bank rows per class, 200 queries), at tol = 1e-3 ("t3")
and tol = 1e-10 ("t10"): dual_coef_, intercept_, support_, decision values and labels on the queries; dd_max = the largest
|d_t3 - d_t10|.  For c7 a 3 x 3 grid search as the reference's parameter_selection runs it (spilt_dataset after
np.random.seed(GRID_SEED), tol = 1e-3 fits, OA + AA + kappa on the validation half): the split, the score table, the winner,
and per grid point the tol = 1e-10 decision values on the validation rows with that point's dd_max."""
import itertools
import os
import sys

import numpy as np
from sklearn import metrics
from sklearn.svm import SVC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import svm_ref as R  # noqa: E402

CASES = {"c7": 7, "c16": 16}
D, GAMMA, C, Q = 32, 1.0 / 32, 8.0, 200
GRID_SEED = 123
GRID_CS = [0.5, 8.0, 128.0]
GRID_GAMMAS = [2.0 ** -7, 2.0 ** -5, 2.0 ** -3]


def fit(x, y, c, g, tol):
    return SVC(C=c, gamma=g, kernel="rbf", tol=tol, decision_function_shape="ovo").fit(x, y)


def main():
    from hsimae_amd.finetune_train import spilt_dataset
    out = {}
    for name, n in CASES.items():
        bank, by, qs, _ = R.clusters(n, D=D, Q=Q)
        x, q = bank.astype(np.float64), qs.astype(np.float64)
        d = {}
        for tag, tol in (("t3", 1e-3), ("t10", 1e-10)):
            m = fit(x, by, C, GAMMA, tol)
            d[tag] = m.decision_function(q)
            out[f"{name}_{tag}_dual_coef"] = m.dual_coef_
            out[f"{name}_{tag}_intercept"] = m.intercept_
            out[f"{name}_{tag}_support"] = m.support_.astype(np.int32)
            out[f"{name}_{tag}_labels"] = m.predict(q).astype(np.int64)
        out[f"{name}_t10_decision"] = d["t10"]
        out[f"{name}_t3_decision"] = d["t3"].astype(np.float32)
        out[f"{name}_dd_max"] = np.float64(np.abs(d["t3"] - d["t10"]).max())
    bank, by, _, _ = R.clusters(7, D=D, Q=Q)
    np.random.seed(GRID_SEED)
    tr, _, va, _ = spilt_dataset(np.arange(by.size), by, training_ratio=0.5)
    tr, va = np.asarray(tr, np.int64), np.asarray(va, np.int64)
    x = bank.astype(np.float64)
    table = np.zeros((len(GRID_CS), len(GRID_GAMMAS)))
    dec10, ddm = [], []
    for (ci, c), (gi, g) in itertools.product(enumerate(GRID_CS), enumerate(GRID_GAMMAS)):
        m3, m10 = fit(x[tr], by[tr], c, g, 1e-3), fit(x[tr], by[tr], c, g, 1e-10)
        pred = m3.predict(x[va])
        table[ci, gi] = (metrics.accuracy_score(by[va], pred) + np.mean(metrics.recall_score(by[va], pred, average=None)) +
                         metrics.cohen_kappa_score(by[va], pred))
        dec10.append(m10.decision_function(x[va]))
        ddm.append(np.abs(m3.decision_function(x[va]) - dec10[-1]).max())
    best = (0.0, 0.0, 0.0)
    for (ci, c), (gi, g) in itertools.product(enumerate(GRID_CS), enumerate(GRID_GAMMAS)):
        if table[ci, gi] > best[2]:
            best = (c, g, table[ci, gi])
    out.update(grid_tr=tr, grid_va=va, grid_table=table, grid_winner=np.array(best), grid_t10_decision=np.stack(dec10),
               grid_dd_max=np.array(ddm), grid_cs=np.array(GRID_CS), grid_gammas=np.array(GRID_GAMMAS))
    path = os.path.join(HERE, "svm_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in ("c7_dd_max", "c16_dd_max", "grid_table", "grid_winner", "grid_dd_max"):
        print(k, out[k])


if __name__ == "__main__":
    main()
