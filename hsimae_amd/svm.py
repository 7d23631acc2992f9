"""RBF support-vector classification of feature rows on the device (csrc/svm.hip): `RBFSVM`, `reference_grid`.

sklearn's `SVC(kernel='rbf')` / libsvm's C-SVC, one-vs-one: the baseline hyperspectral papers report next to their deep models
(the reference's Compared_Methods/svm_rbf.py), and the non-linear counterpart of the linear probe on frozen encoder features.
Four kinds of launches: the kernel matrices (hsimae_svm_gram), every two-class problem of every (C, gamma) point in ONE launch
(hsimae_svm_solve: SMO with second-order working-set selection, one workgroup per problem), the compact model (hsimae_svm_pack)
and the prediction (hsimae_svm_predict).  Nothing here waits for the host except gamma="scale" (one number read in fit()), check(), and grid_search() /
fit_reference(): the reference's split runs on the host, so labels given as a device tensor are copied back once, and all
scores are read once.

The `probs` / confidence / margin of a prediction are VOTE SHARES: the fraction of the pairwise contests a class won.  They are
not Platt probabilities (Platt scaling is not implemented).
"""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import torch

from . import _lib
from .classify import ScoreMeter, _labels
from .knn import _features

MAX_ROWS = 8192                     # HSIMAE_SVM_MAX_ROWS: rows of a bank (one Gram matrix; alpha and G of one problem live in LDS)
MAX_GAMMAS = 16                     # HSIMAE_SVM_MAX_GAMMAS: kernel matrices of one hsimae_svm_gram call
MAX_REAL_CLASSES = 32               # HSIMAE_SVM_MAX_CLASSES: 496 pairs of decision sums for 64 query rows fill the LDS
GRAM_BUDGET_BYTES = 2 << 30         # the Gram stack n_gamma * M * ldk * 4 of one call; above it grid_search / fit raise
STATE = 8


def reference_grid(best_c=None, best_g=None):
    """The reference's two grid stages as data (Compared_Methods/svm_rbf.py:48-66) -> (Cs, gammas).  Without arguments stage 1:
    C = 2^-3, 2^-1, .., 2^9 and gamma = 2^-5, 2^-3, .., 2^3; with the stage-1 winner stage 2: the winner times
    2^-1.75, 2^-1.5, .., 2^1.75 on both axes."""
    if best_c is None and best_g is None:
        return [float(np.power(2.0, i)) for i in range(-3, 10, 2)], [float(np.power(2.0, i)) for i in range(-5, 4, 2)]
    steps = [-1.75 + 0.25 * i for i in range(15)]
    return [float(best_c * np.power(2.0, i)) for i in steps], [float(best_g * np.power(2.0, i)) for i in steps]


def pick_winner(Cs, gammas, table):
    """The reference's rule on a score table [len(Cs), len(gammas)] of OA + AA + kappa: visit itertools.product(Cs, gammas) in
    order, start from 0, only a strict improvement replaces the incumbent -> (C, gamma, score); (0, 0, 0) when nothing is > 0."""
    best = (0, 0, 0)
    for (ci, c), (gi, g) in itertools.product(enumerate(Cs), enumerate(gammas)):
        if table[ci][gi] > best[2]:
            best = (c, g, float(table[ci][gi]))
    return best


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _Bank:
    """The rows sorted by class (stable), the class ranges, and the Gram stack for a list of gammas: what fits share."""

    def __init__(self, features, labels, first, n_real):
        x = _features(features, "features")
        M, D = int(x.shape[0]), int(x.shape[1])
        if not 2 <= M <= MAX_ROWS:
            raise ValueError(f"between 2 and {MAX_ROWS} bank rows are served, got {M}")
        y = _labels(labels, "labels", x.device).reshape(-1)
        if y.numel() != M:
            raise ValueError(f"{y.numel()} labels for {M} rows")
        key = y - first
        wrong = (key < 0) | (key >= n_real)
        key = torch.where(wrong, torch.full_like(key, n_real), key)                  # bad rows behind every class: in no problem
        self.bad = wrong.any()
        key, self.order = torch.sort(key, stable=True)
        self.x = x[self.order].contiguous()
        self.labels = key + first
        self.counts = (key[:, None] == torch.arange(n_real, device=x.device)[None, :]).sum(0)
        self.starts = torch.cumsum(self.counts, 0) - self.counts
        self.M, self.D, self.dev, self.n_real = M, D, x.device, n_real
        self.ldk = (M + 3) // 4 * 4

    def scale_gamma(self):
        """sklearn's gamma='scale' = 1 / (D * Var(X)), the variance over all entries, in fp64 on the device; ONE host wait."""
        var = float(self.x.double().var(unbiased=False).item())
        return 1.0 / (self.D * var) if var > 0 else 1.0

    def gram(self, gammas):
        g = [float(v) for v in gammas]
        if not 1 <= len(g) <= MAX_GAMMAS:
            raise ValueError(f"between 1 and {MAX_GAMMAS} gammas per Gram stack, got {len(g)}")
        if len(g) * self.M * self.ldk * 4 > GRAM_BUDGET_BYTES:
            raise ValueError(f"the Gram stack of {len(g)} x {self.M} x {self.ldk} floats is above the budget of {GRAM_BUDGET_BYTES} bytes")
        K = torch.empty(len(g), self.M, self.ldk, dtype=torch.float32, device=self.dev)
        self.sumsq = torch.empty(self.M, dtype=torch.float32, device=self.dev)
        p = _lib.SvmGramParams(x=self.x.data_ptr(), ldx=self.x.stride(0), M=self.M, D=self.D, n_gamma=len(g),
                               gamma=(C.c_float * 16)(*g), K=K.data_ptr(), ldk=self.ldk, sumsq=self.sumsq.data_ptr())
        with torch.cuda.device(self.dev):
            _lib.check(_lib.load().hsimae_svm_gram(C.byref(p), _stream(self.dev)), "hsimae_svm_gram")
        return K

    def table(self, Cs, n_gamma):
        """The problems of itertools.product(Cs, range(n_gamma)) x the class pairs, built on the device -> int64 [n, 8]."""
        n = self.n_real
        ia, ib = torch.triu_indices(n, n, 1, device=self.dev)
        P = int(ia.numel())
        na, nb = self.counts[ia], self.counts[ib]
        off = torch.cumsum(na + nb, 0) - (na + nb)
        span = (n - 1) * self.M                                                     # alphas of one model at most
        rows = []
        for m, (c, g) in enumerate(itertools.product(Cs, range(n_gamma))):
            cc = torch.full((P,), float(c), dtype=torch.float64, device=self.dev).view(torch.int64)
            rows.append(torch.stack([torch.full_like(ia, g), cc, self.starts[ia], na, self.starts[ib], nb, off + m * span,
                                     torch.zeros_like(ia)], 1))
        return torch.cat(rows).contiguous(), P, span


class RBFSVM:
    """C-SVC with the kernel exp(-gamma ||x - x'||^2), one-vs-one, libsvm's decision rule (a pair (a, b), a < b, votes for a
    when its decision value is > 0; ties in the vote go to the lower class).  Classes are [first, num_class); with first = 1
    class 0 is "unlabelled" and never predicted.  `gamma="scale"` is sklearn's 1 / (D * Var(X)): fit() then reads one number
    from the device, its only host wait; a float gamma waits for nothing.  Banks of at most 8192 rows and 32 real classes."""

    def __init__(self, num_class, first=1, C=1.0, gamma="scale", eps=1e-3, max_iter=1_000_000):
        self.num_class, self.first = int(num_class), int(first)
        self.n_real = self.num_class - self.first
        if self.first < 0 or not 2 <= self.n_real <= MAX_REAL_CLASSES:
            raise ValueError(f"between 2 and {MAX_REAL_CLASSES} classes in [first, num_class) are served, got first={first}, num_class={num_class}")
        self.C, self.gamma, self.eps, self.max_iter = float(C), gamma, float(eps), int(max_iter)
        if not self.C > 0 or not self.eps > 0 or self.max_iter < 0:
            raise ValueError("C and eps must be positive, max_iter >= 0")
        if gamma != "scale" and not float(gamma) > 0:
            raise ValueError(f"gamma must be 'scale' or a positive number, got {gamma}")
        self.model = None

    # ------------------------------------------------------------------ launches
    def _solve(self, bank, K, table, alpha_len):
        n = int(table.shape[0])
        alpha = torch.zeros(alpha_len, dtype=torch.float64, device=bank.dev)
        grad = torch.zeros(alpha_len, dtype=torch.float64, device=bank.dev)
        state = torch.zeros(n, STATE, dtype=torch.float64, device=bank.dev)
        p = _lib.SvmSolveParams(K=K.data_ptr(), ldk=bank.ldk, M=bank.M, n_k=int(K.shape[0]), table=table.data_ptr(), n_problems=n,
                                resume=0, max_iter=self.max_iter, eps=self.eps, alpha=alpha.data_ptr(), grad=grad.data_ptr(),
                                alpha_len=alpha_len, state=state.data_ptr())
        with torch.cuda.device(bank.dev):
            _lib.check(_lib.load().hsimae_svm_solve(C.byref(p), _stream(bank.dev)), "hsimae_svm_solve")
        return alpha, state

    def _pack(self, bank, table, first_problem, alpha, state, gamma):
        dev, M, D, n = bank.dev, bank.M, bank.D, self.n_real
        P = n * (n - 1) // 2
        m = {"sv_index": torch.zeros(M, dtype=torch.int32, device=dev), "sv_start": torch.zeros(n + 1, dtype=torch.int32, device=dev),
             "coef": torch.zeros(n - 1, M, dtype=torch.float32, device=dev), "rho": torch.zeros(P, dtype=torch.float32, device=dev),
             "sv": torch.zeros(M, D, dtype=torch.float32, device=dev), "sv_sumsq": torch.zeros(M, dtype=torch.float32, device=dev),
             "gamma": float(gamma), "state": state[first_problem:first_problem + P], "M": M, "D": D}
        p = _lib.SvmPackParams(table=table.data_ptr(), first_problem=first_problem, n_class=n, alpha=alpha.data_ptr(),
                               alpha_len=alpha.numel(), state=state.data_ptr(), x=bank.x.data_ptr(), ldx=bank.x.stride(0), M=M, D=D,
                               sumsq=bank.sumsq.data_ptr(), sv_index=m["sv_index"].data_ptr(), sv_start=m["sv_start"].data_ptr(),
                               coef=m["coef"].data_ptr(), ldc=M, rho=m["rho"].data_ptr(), sv=m["sv"].data_ptr(), ldsv=D,
                               sv_sumsq=m["sv_sumsq"].data_ptr())
        with torch.cuda.device(dev):
            _lib.check(_lib.load().hsimae_svm_pack(C.byref(p), _stream(dev)), "hsimae_svm_pack")
        return m

    def _predict(self, m, x, H, W, p0, pixels, label_map, conf_map, margin_map, probs, decision, outside=None):
        n = self.n_real
        p = _lib.SvmPredictParams(q=x.data_ptr(), ldq=x.stride(0) if x.shape[0] > 1 else x.shape[1], Q=x.shape[0], D=m["D"],
                                  sv=m["sv"].data_ptr(), ldsv=m["D"], sv_sumsq=m["sv_sumsq"].data_ptr(), sv_start=m["sv_start"].data_ptr(),
                                  S_max=m["M"], coef=m["coef"].data_ptr(), ldc=m["M"], rho=m["rho"].data_ptr(), n_class=n, first=self.first,
                                  gamma=m["gamma"], H=H, W=W, p0=p0, pixels=_lib.ptr(pixels), label_map=label_map.data_ptr(),
                                  conf_map=_lib.ptr(conf_map), margin_map=_lib.ptr(margin_map), probs=_lib.ptr(probs), ldp=self.num_class,
                                  decision=_lib.ptr(decision), ldd=n * (n - 1) // 2, outside=_lib.ptr(outside))
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().hsimae_svm_predict(C.byref(p), _stream(x.device)), "hsimae_svm_predict")

    # ------------------------------------------------------------------ public
    def fit(self, features, labels):
        """Fit on fp32 rows [M, D] (D % 4 == 0) and integer labels [M] in [first, num_class).  The rows are sorted by class
        (stable); a label outside the classes or an empty class is reported by check()."""
        with torch.no_grad():
            bank = _Bank(features, labels, self.first, self.n_real)
            gamma = bank.scale_gamma() if self.gamma == "scale" else float(self.gamma)
            K = bank.gram([gamma])
            table, P, span = bank.table([self.C], 1)
            alpha, state = self._solve(bank, K, table, span)
            self.model = self._pack(bank, table, 0, alpha, state, gamma)
        self.bank, self.gamma_, self.alpha, self.table = bank, gamma, alpha, table
        return self

    @property
    def n_support(self):
        """int32 [real classes] on the device: support rows per class."""
        s = self._fitted()["sv_start"]
        return s[1:] - s[:-1]

    @property
    def iterations(self):
        return self._fitted()["state"][:, 0]

    @property
    def dual_gap(self):
        """fp64 [pairs] on the device: G_max - G_min of every problem when it stopped (below eps when it converged)."""
        return self._fitted()["state"][:, 2]

    def _fitted(self):
        if self.model is None:
            raise RuntimeError("RBFSVM: call fit() first")
        return self.model

    def _queries(self, features):
        m = self._fitted()
        x = _features(features, "features")
        if x.device != m["sv"].device:
            raise RuntimeError(f"hsimae_amd runs on MI355X only (no CPU fallback): features are on {x.device}, the model on {m['sv'].device}")
        if x.shape[1] != m["D"]:
            raise ValueError(f"features have {x.shape[1]} columns, the model {m['D']}")
        return m, x

    def decision_function(self, features):
        """-> fp32 [Q, pairs] on the device: libsvm's one-vs-one decision values, pairs (0, 1), (0, 2), .., (1, 2), .. of the
        real classes; > 0 votes for the lower class of the pair."""
        m, x = self._queries(features)
        Q, n = int(x.shape[0]), self.n_real
        dec = torch.zeros(Q, n * (n - 1) // 2, dtype=torch.float32, device=x.device)
        if Q:
            self._predict(m, x, 1, Q, 0, None, torch.zeros(Q, dtype=torch.int64, device=x.device), None, None, None, dec)
        return dec

    def predict_into(self, features, H, W, pixels, label_map, conf_map=None, margin_map=None, probs=None):
        """Classify the rows of `features` and write label (int64, first + class), the winner's vote share and its lead over
        the runner-up at `pixels` (int64 device tensor, one per row; None: row order) of the [H * W] maps and, in row order,
        the vote shares into probs [Q, num_class].  Vote shares, not Platt probabilities."""
        m, x = self._queries(features)
        if x.shape[0]:
            self._predict(m, x, H, W, 0, pixels, label_map, conf_map, margin_map, probs, None)

    def predict(self, features, return_probs=False):
        """-> (labels int64 [Q], confidence fp32 [Q], margin fp32 [Q]) and with return_probs=True also probs fp32
        [Q, num_class]: the share of the pairwise contests every class won (columns below `first` are 0; vote shares, not
        Platt probabilities); confidence is the winner's share, margin its lead over the runner-up."""
        m, x = self._queries(features)
        Q, dev = int(x.shape[0]), x.device
        labels = torch.zeros(Q, dtype=torch.int64, device=dev)
        conf = torch.zeros(Q, dtype=torch.float32, device=dev)
        margin = torch.zeros(Q, dtype=torch.float32, device=dev)
        probs = torch.empty(Q, self.num_class, dtype=torch.float32, device=dev) if return_probs else None
        if Q:
            self._predict(m, x, 1, Q, 0, None, labels, conf, margin, probs, None)
        return (labels, conf, margin, probs) if return_probs else (labels, conf, margin)

    def check(self):
        """Raise if a label of the last fit was outside [first, num_class), a class had no row, or a problem did not converge
        within max_iter (one small copy)."""
        m = self._fitted()
        host = torch.cat([m["state"][:, 1], self.bank.bad.double().reshape(1), (self.bank.counts == 0).any().double().reshape(1)]).cpu()
        if host[-2]:
            raise RuntimeError(f"RBFSVM: a label was outside [{self.first}, {self.num_class})")
        if host[-1] or bool((host[:-2] == -2).any()):
            raise RuntimeError("RBFSVM: a class has no row")
        if bool((host[:-2] != 1).any()):
            raise RuntimeError(f"RBFSVM: {int((host[:-2] != 1).sum())} of {host.numel() - 2} problems did not converge in {self.max_iter} iterations")

    # ------------------------------------------------------------------ the reference's grid search
    def grid_search(self, features, labels, Cs, gammas, val_ratio=0.5, keep_models=False):
        """The reference's parameter_selection: split the rows per class with finetune_train.spilt_dataset (numpy's global
        generator, as there), fit every (C, gamma) on the training half -- one Gram stack per 16 gammas and ONE solver launch
        for all points and pairs --, score the validation half by OA + AA + kappa (ScoreMeter), read all scores once, and
        return the reference's winner (pick_winner).  Labels must be first .. num_class - 1 with first = 1, as the split
        requires.  keep_models=True keeps every point's packed model on the device as `self.last_search` [(C, gamma, model)] in
        visiting order (off by default: at an encoder bank that is gigabytes).
        -> (C, gamma, score table fp64 [len(Cs), len(gammas)], (training rows, validation rows))."""
        from .finetune_train import spilt_dataset
        Cs, gammas = [float(c) for c in Cs], [float(g) for g in gammas]
        x = _features(features, "features")
        y_host = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64).reshape(-1)
        tr, _, va, _ = spilt_dataset(np.arange(y_host.size), y_host - (self.first - 1), training_ratio=1 - val_ratio)
        tr, va = np.asarray(tr, np.int64), np.asarray(va, np.int64)
        table = self._search(x, y_host, tr, va, Cs, gammas, keep_models)
        c, g, _ = pick_winner(Cs, gammas, table)
        return c, g, table, (tr, va)

    def _search(self, x, y_host, tr, va, Cs, gammas, keep_models=False):
        dev = x.device
        with torch.no_grad():
            tr_d, va_d = torch.from_numpy(tr).to(dev), torch.from_numpy(va).to(dev)
            bank = _Bank(x[tr_d], y_host[tr], self.first, self.n_real)
            xv = x[va_d].contiguous()
            yv = torch.from_numpy(y_host[va]).to(dev)
            pred = torch.zeros(len(va), dtype=torch.int64, device=dev)
            outs, self.last_search = [], []                       # last_search: (C, gamma, packed model) in visiting order
            for g0 in range(0, len(gammas), MAX_GAMMAS):
                gs = gammas[g0:g0 + MAX_GAMMAS]
                K = bank.gram(gs)
                tab, P, span = bank.table(Cs, len(gs))
                alpha, state = self._solve(bank, K, tab, span * len(Cs) * len(gs))
                for m, (c, gi) in enumerate(itertools.product(range(len(Cs)), range(len(gs)))):
                    model = self._pack(bank, tab, m * P, alpha, state, gs[gi])
                    self._predict(model, xv, 1, len(va), 0, None, pred, None, None, None, None)
                    meter = ScoreMeter(self.num_class, dev)
                    meter.update(yv, pred)
                    _lib.check(_lib.load().hsimae_scores(meter.cm.data_ptr(), meter.num_class, meter._out.data_ptr(), _stream(dev)),
                               "hsimae_scores")
                    outs.append((c, g0 + gi, meter._out))
                    if keep_models:
                        self.last_search.append((Cs[c], gs[gi], model))
            host = torch.stack([o[2][:3] for o in outs]).cpu().numpy()               # the one read
        table = np.zeros((len(Cs), len(gammas)))
        for (c, g, _), s in zip(outs, host):
            table[c, g] = s[0] + s[1] + s[2]
        return table

    def fit_reference(self, features, labels):
        """The reference's svm_rbf.train: stage 1 (7 x 5), stage 2 (15 x 15 around the stage-1 winner; each stage draws its own
        split), then a refit at the winner on the TRAINING HALF of the stage-2 split -- not on the whole bank: the reference's
        quirk, kept.  Sets C and gamma.  -> (C, gamma, stage-2 score table)."""
        c, g, _, _ = self.grid_search(features, labels, *reference_grid())
        if not c > 0 or not g > 0:
            raise RuntimeError("RBFSVM.fit_reference: no point of the first grid stage scored above 0 on the validation half, so there "
                               "is no winner to build the second stage around")
        c, g, table, (tr, _) = self.grid_search(features, labels, *reference_grid(c, g))
        if not c > 0 or not g > 0:
            raise RuntimeError("RBFSVM.fit_reference: no point of the second grid stage scored above 0 on the validation half")
        self.C, self.gamma = float(c), float(g)
        x = _features(features, "features")
        y = _labels(labels, "labels", x.device).reshape(-1)
        idx = torch.from_numpy(tr).to(x.device)
        self.fit(x[idx], y[idx])
        return c, g, table
