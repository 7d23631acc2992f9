"""Linear probe on frozen features, trained and applied on the device (csrc/probe.hip): `LinearProbe`.

The evaluation masked-autoencoder work reports first (He et al. 2022, MAE's linear probing): a linear classifier on the frozen
encoder's features, here on the cached pooled rows `scene_features` returns, so a step costs a [n, D] x [D, C] product each way and
never touches the encoder.  The features are standardised per column (MAE's BatchNorm1d(affine=False, eps=1e-6) ahead of the
linear layer), the bias is one more column, and training is full-batch AdamW with decoupled decay (none on the bias):
hsimae_probe_prepare once, then hsimae_probe_step per iteration (four launches), all on the current stream.  fit() never waits for
the host; the kernels use no atomics and every sum has a fixed order, so two fits are bit-identical.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .classify import _labels
from .knn import MAX_BANK, _features

MAX_PROBE_CLASSES = _lib.PROBE_ROWS
SCHEDULES = ("cosine", "constant")


class LinearProbe:
    """Multinomial logistic regression over the classes [first, num_class) on fp32 rows [n, D] on a GPU (D % 4 == 0, D <= 4096,
    n <= 2^20, num_class <= 64).  With first = 1 class 0 is "unlabelled": never trained, never predicted.
    fit() issues exactly `max_iter` full-batch AdamW steps; the learning rate of step t = 0 .. max_iter - 1 is computed on the host,
    lr * 1/2 (1 + cos(pi t / max_iter)) for schedule="cosine", lr for "constant", and passed as a launch argument.
    A bank label outside [first, num_class) makes its row inert (it enters no statistic, loss or gradient) and is counted:
    check() raises on it.  The defaults are MAE's recipe scaled to a small bank, not tuned on a real scene.
    After fit(), all on the features' device: w fp32 [64, D + 4] (the standardised operand's weights, bias in column D), mean and rstd
    fp32 [D], loss_history fp32 [max_iter] (the mean cross-entropy before each update), grad_norm (0-d fp64: ||dW|| of the last
    step), loss (0-d fp64: loss_history's last entry in fp64)."""

    QUERY_CHUNK_ROWS = 1 << 20

    def __init__(self, num_class, first=1, max_iter=100, lr=1e-2, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8,
                 schedule="cosine", bn_eps=1e-6):
        self.num_class, self.first, self.max_iter = int(num_class), int(first), int(max_iter)
        if not 2 <= self.num_class <= MAX_PROBE_CLASSES:
            raise ValueError(f"between 2 and {MAX_PROBE_CLASSES} classes are served, got {num_class}")
        if not 0 <= self.first < self.num_class:
            raise ValueError(f"first must lie in [0, {self.num_class}), got {first}")
        if self.max_iter < 1:
            raise ValueError(f"max_iter must be >= 1, got {max_iter}")
        self.lr, self.weight_decay, self.eps, self.bn_eps = float(lr), float(weight_decay), float(eps), float(bn_eps)
        if not (self.lr >= 0 and math.isfinite(self.lr)) or not (self.weight_decay >= 0 and math.isfinite(self.weight_decay)):
            raise ValueError(f"lr and weight_decay must be finite and >= 0, got {lr} and {weight_decay}")
        if not (self.eps >= 0 and math.isfinite(self.eps)) or not (self.bn_eps > 0 and math.isfinite(self.bn_eps)):
            raise ValueError(f"eps must be finite and >= 0 and bn_eps finite and > 0, got {eps} and {bn_eps}")
        self.betas = tuple(float(b) for b in betas)
        if len(self.betas) != 2 or not all(0 <= b < 1 for b in self.betas):
            raise ValueError(f"betas must be two numbers in [0, 1), got {betas}")
        if schedule not in SCHEDULES:
            raise ValueError(f"schedule must be one of {SCHEDULES}, got {schedule!r}")
        self.schedule = schedule
        self.w = self.mean = self.rstd = self.loss_history = self._state = None

    def lr_at(self, t):
        """The learning rate of step t (0-based), as fit() passes it."""
        return self.lr * 0.5 * (1.0 + math.cos(math.pi * t / self.max_iter)) if self.schedule == "cosine" else self.lr

    @staticmethod
    def _stream(dev):
        return torch.cuda.current_stream(dev).cuda_stream

    @staticmethod
    def _ld(t):
        return t.stride(0) if t.shape[0] > 1 else t.shape[1]

    # ------------------------------------------------------------------ public
    def fit(self, features, labels):
        x = _features(features, "features")
        n, D, dev = int(x.shape[0]), int(x.shape[1]), x.device
        if not 1 <= n <= MAX_BANK:
            raise ValueError(f"the bank must hold between 1 and {MAX_BANK} rows, got {n}")
        y = _labels(labels, "labels", dev).reshape(-1)
        if y.numel() != n:
            raise ValueError(f"{y.numel()} labels for {n} bank rows")
        Kp, ldn, rows = D + 4, (n + 3) // 4 * 4, _lib.PROBE_ROWS
        segs = (n + _lib.PROBE_SEG - 1) // _lib.PROBE_SEG
        lib = _lib.load()
        with torch.no_grad(), torch.cuda.device(dev):
            f32 = dict(dtype=torch.float32, device=dev)
            f64 = dict(dtype=torch.float64, device=dev)
            mean, rstd = torch.empty(D, **f32), torch.empty(D, **f32)
            xs, xt = torch.empty(n, Kp, **f32), torch.empty(Kp, ldn, **f32)
            state = torch.zeros(_lib.PROBE_STATE, **f64)
            w, m, v = (torch.zeros(rows, Kp, **f32) for _ in range(3))
            gt, scratch = torch.empty(rows, ldn, **f32), torch.empty(segs, rows, Kp, **f32)
            loss_part, norm_part = torch.empty((n + 63) // 64, **f64), torch.empty((rows * Kp + 255) // 256, **f64)
            hist = torch.zeros(self.max_iter, **f32)
            stream = self._stream(dev)
            pp = _lib.ProbePrepareParams(x=x.data_ptr(), ldx=self._ld(x), labels=y.data_ptr(), n=n, D=D, C=self.num_class,
                                         first=self.first, eps=self.bn_eps, mean=mean.data_ptr(), rstd=rstd.data_ptr(),
                                         xs=xs.data_ptr(), Kp=Kp, xt=xt.data_ptr(), ldn=ldn, state=state.data_ptr())
            _lib.check(lib.hsimae_probe_prepare(C.byref(pp), stream), "hsimae_probe_prepare")
            sp = _lib.ProbeStepParams(xs=xs.data_ptr(), xt=xt.data_ptr(), Kp=Kp, ldn=ldn, labels=y.data_ptr(), n=n, D=D,
                                      C=self.num_class, first=self.first, w=w.data_ptr(), m=m.data_ptr(), v=v.data_ptr(),
                                      gt=gt.data_ptr(), scratch=scratch.data_ptr(), loss_part=loss_part.data_ptr(),
                                      norm_part=norm_part.data_ptr(), lr=self.lr, weight_decay=self.weight_decay, b1=self.betas[0],
                                      b2=self.betas[1], eps=self.eps, step=1, state=state.data_ptr(), loss_hist=hist.data_ptr())
            for t in range(self.max_iter):
                sp.lr, sp.step = self.lr_at(t), t + 1
                _lib.check(lib.hsimae_probe_step(C.byref(sp), stream), "hsimae_probe_step")
            self.w, self.mean, self.rstd, self.loss_history, self._state = w, mean, rstd, hist, state
        return self

    @property
    def loss(self):
        return None if self._state is None else self._state[0]

    @property
    def grad_norm(self):
        return None if self._state is None else self._state[2].sqrt()

    def _queries(self, features):
        if self.w is None:
            raise RuntimeError("LinearProbe: call fit() first")
        x = _features(features, "features")
        if x.device != self.w.device:
            raise RuntimeError(f"hsimae_amd runs on MI355X only (no CPU fallback): features are on {x.device}, the probe on "
                               f"{self.w.device}")
        if x.shape[1] != self.mean.shape[0]:
            raise ValueError(f"features have {x.shape[1]} columns, the probe {self.mean.shape[0]}")
        return x

    def logits(self, features):
        """-> fp32 [Q, num_class]: the rows standardised by the bank's statistics, times w; columns below `first` are 0."""
        x = self._queries(features)
        Q, D, dev = int(x.shape[0]), int(x.shape[1]), x.device
        z = torch.empty(Q, self.num_class, dtype=torch.float32, device=dev)
        with torch.no_grad(), torch.cuda.device(dev):
            for k0 in range(0, Q, self.QUERY_CHUNK_ROWS):
                part = x[k0:k0 + self.QUERY_CHUNK_ROWS]
                p = _lib.ProbeLogitsParams(x=part.data_ptr(), ldx=self._ld(x), mean=self.mean.data_ptr(), rstd=self.rstd.data_ptr(),
                                           w=self.w.data_ptr(), Kp=D + 4, n=int(part.shape[0]), D=D, C=self.num_class,
                                           first=self.first, z=z[k0:].data_ptr(), ldz=self.num_class)
                _lib.check(_lib.load().hsimae_probe_logits(C.byref(p), self._stream(dev)), "hsimae_probe_logits")
        return z

    def predict(self, features):
        """-> labels int64 [Q] = first + argmax of the logits over [first, num_class) (hsimae_class_argmax: ties to the lower)."""
        z = self.logits(features)
        Q, dev = int(z.shape[0]), z.device
        labels = torch.zeros(Q, dtype=torch.int64, device=dev)
        with torch.no_grad(), torch.cuda.device(dev):
            for k0 in range(0, Q, 1 << 30):
                n = min(1 << 30, Q - k0)
                sp = _lib.SceneParams(H=1, W=n, C=1, p0=0, N=n)
                _lib.check(_lib.load().hsimae_class_argmax(C.byref(sp), z[k0:].data_ptr(), self.num_class, self.num_class, self.first,
                                                           labels[k0:].data_ptr(), self._stream(dev)), "hsimae_class_argmax")
        return labels

    def head(self):
        """-> (weight fp32 [num_class, D], bias fp32 [num_class]): the probe in terms of the raw features (hsimae_probe_fold), what
        a model's `cls_head` takes; rows below `first` are 0."""
        if self.w is None:
            raise RuntimeError("LinearProbe: call fit() first")
        D, dev = int(self.mean.shape[0]), self.w.device
        weight = torch.empty(self.num_class, D, dtype=torch.float32, device=dev)
        bias = torch.empty(self.num_class, dtype=torch.float32, device=dev)
        with torch.no_grad(), torch.cuda.device(dev):
            p = _lib.ProbeFoldParams(w=self.w.data_ptr(), Kp=D + 4, mean=self.mean.data_ptr(), rstd=self.rstd.data_ptr(), D=D,
                                     C=self.num_class, first=self.first, weight=weight.data_ptr(), ldw=D, bias=bias.data_ptr())
            _lib.check(_lib.load().hsimae_probe_fold(C.byref(p), self._stream(dev)), "hsimae_probe_fold")
        return weight, bias

    def check(self):
        """Raise if the bank held a label outside [first, num_class) (one small copy, the only wait)."""
        if self._state is not None:
            bad = int(self._state[3].item())
            if bad:
                raise RuntimeError(f"LinearProbe: {bad} bank labels were outside [{self.first}, {self.num_class})")
