"""Weighted k-NN classification of frozen features on the device (csrc/knn.hip): `KNNClassifier`.

The evaluation a pretrained encoder gets without fine-tuning (Wu et al. 2018; DINO's `knn_classifier`): L2-normalised features,
the k most similar rows of a labelled bank, every neighbour voting for its class with weight exp(similarity / T).  Three
launches per chunk of queries (hsimae_row_normalize, hsimae_knn_topk, hsimae_knn_vote); the [Q, M] similarity matrix is never
written to memory.  Nothing here waits for the host except fit()'s one check of the labels and check().
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .classify import MAX_CLASSES, _labels, _need_cuda

MAX_K = 64              # hsimae_knn_topk: one list entry per lane
MAX_BANK = 1 << 20
MAX_DIM = 4096


def _features(t, what):
    """fp32 [n, D] on a GPU, D % 4 == 0, rows 16-byte aligned: used as it is when it already is all that."""
    _need_cuda(t, what)
    if t.dim() != 2:
        raise ValueError(f"{what} must be [n, D], got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    D = int(t.shape[1])
    if D < 4 or D % 4 or D > MAX_DIM:
        raise ValueError(f"{what} has {D} columns: a multiple of 4 between 4 and {MAX_DIM} is served")
    t = t.detach()
    if t.shape[0] and (t.stride(1) != 1 or t.stride(0) < D or t.stride(0) % 4 or t.data_ptr() % 16):
        t = t.contiguous()
    return t


class KNNClassifier:
    """k-NN over cosine similarity with DINO's defaults: the `k` nearest bank rows vote with weight exp(sim / temperature).
    Classes are [first, num_class); with first = 1 class 0 is "unlabelled" and never predicted.  Everything stays on the
    features' device and nothing waits for the host after fit()."""

    QUERY_CHUNK_BYTES = 64 << 20          # the normalised copy of the queries is at most this large

    def __init__(self, k=20, temperature=0.07, num_class=None, first=1):
        self.k, self.first = int(k), int(first)
        if not 1 <= self.k <= MAX_K:
            raise ValueError(f"k between 1 and {MAX_K} is served, got {k}")
        self.temperature = float(temperature)
        if not self.temperature > 0 or self.temperature == float("inf"):
            raise ValueError(f"temperature must be a positive number, got {temperature}")
        self.num_class = None if num_class is None else int(num_class)
        if self.first < 0:
            raise ValueError(f"first must be >= 0, got {first}")
        self.bank = self.labels = self._bad = None

    # ------------------------------------------------------------------ the three launches
    @staticmethod
    def _stream(dev):
        return torch.cuda.current_stream(dev).cuda_stream

    def _normalized(self, x):
        out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        p = _lib.RowNormalizeParams(x=x.data_ptr(), ld=x.stride(0) if x.shape[0] > 1 else x.shape[1], N=x.shape[0], D=x.shape[1],
                                    out=out.data_ptr(), ldo=x.shape[1])
        _lib.check(_lib.load().hsimae_row_normalize(C.byref(p), self._stream(x.device)), "hsimae_row_normalize")
        return out

    def _topk(self, qn, idx, sim):
        b = self.bank
        p = _lib.KnnTopkParams(q=qn.data_ptr(), ldq=qn.shape[1], bank=b.data_ptr(), ldb=b.shape[1], Q=qn.shape[0], M=b.shape[0],
                               D=b.shape[1], k=self.k, idx=idx.data_ptr(), sim=sim.data_ptr())
        _lib.check(_lib.load().hsimae_knn_topk(C.byref(p), self._stream(b.device)), "hsimae_knn_topk")

    def _vote(self, idx, sim, n, H, W, p0, pixels_ptr, label_map, conf_map, margin_map, probs_ptr):
        p = _lib.KnnVoteParams(idx=idx.data_ptr(), sim=sim.data_ptr(), Q=n, k=self.k, M=self.bank.shape[0],
                               bank_labels=self.labels.data_ptr(), C=self.num_class, first=self.first,
                               inv_temperature=1.0 / self.temperature, H=H, W=W, p0=p0, pixels=pixels_ptr,
                               label_map=label_map.data_ptr(), conf_map=_lib.ptr(conf_map), margin_map=_lib.ptr(margin_map),
                               probs=probs_ptr, ldp=self.num_class, bad=self._bad.data_ptr())
        _lib.check(_lib.load().hsimae_knn_vote(C.byref(p), self._stream(self.bank.device)), "hsimae_knn_vote")

    # ------------------------------------------------------------------ public
    def fit(self, features, labels):
        """Store the normalised bank fp32 [M, D] and its labels int64 [M] on the features' device.  Refuses a label outside
        [first, num_class) here (one host check); num_class=None takes the largest label + 1."""
        x = _features(features, "features")
        M = int(x.shape[0])
        if not self.k <= M <= MAX_BANK:
            raise ValueError(f"the bank must hold between k={self.k} and {MAX_BANK} rows, got {M}")
        y = _labels(labels, "labels", x.device).reshape(-1)
        if y.numel() != M:
            raise ValueError(f"{y.numel()} labels for {M} bank rows")
        lo, hi = (int(v) for v in torch.stack([y.min(), y.max()]).tolist())          # the one wait
        nc = hi + 1 if self.num_class is None else self.num_class
        if not 2 <= nc <= MAX_CLASSES or self.first >= nc:
            raise ValueError(f"between 2 and {MAX_CLASSES} classes with first={self.first} below them are served, got {nc}")
        if lo < self.first or hi >= nc:
            raise ValueError(f"bank labels must lie in [{self.first}, {nc}): min {lo}, max {hi}")
        self.num_class = nc
        with torch.cuda.device(x.device):
            self.bank, self.labels = self._normalized(x), y
            self._bad = torch.zeros(1, dtype=torch.int32, device=x.device)
        return self

    def _queries(self, features):
        if self.bank is None:
            raise RuntimeError("KNNClassifier: call fit() first")
        x = _features(features, "features")
        if x.device != self.bank.device:
            raise RuntimeError(f"hsimae_amd runs on MI355X only (no CPU fallback): features are on {x.device}, the bank on {self.bank.device}")
        if x.shape[1] != self.bank.shape[1]:
            raise ValueError(f"features have {x.shape[1]} columns, the bank {self.bank.shape[1]}")
        return x, max(64, self.QUERY_CHUNK_BYTES // (4 * int(x.shape[1])))

    def neighbours(self, features):
        """-> (idx int32 [Q, k], sim fp32 [Q, k]): the k most similar bank rows of every query, best first; equal similarities
        by ascending bank index."""
        x, chunk = self._queries(features)
        Q = int(x.shape[0])
        with torch.no_grad(), torch.cuda.device(x.device):
            idx = torch.empty(Q, self.k, dtype=torch.int32, device=x.device)
            sim = torch.empty(Q, self.k, dtype=torch.float32, device=x.device)
            for k0 in range(0, Q, chunk):
                self._topk(self._normalized(x[k0:k0 + chunk]), idx[k0:k0 + chunk], sim[k0:k0 + chunk])
        return idx, sim

    def predict_into(self, features, H, W, pixels, label_map, conf_map=None, margin_map=None, probs=None):
        """normalise -> top-k -> vote for the rows of `features`, written at `pixels` (int64 device tensor, one per row) of the
        [H * W] maps and, in row order, into probs [Q, num_class]."""
        x, chunk = self._queries(features)
        Q = int(x.shape[0])
        with torch.no_grad(), torch.cuda.device(x.device):
            idx = torch.empty(min(chunk, Q), self.k, dtype=torch.int32, device=x.device)
            sim = torch.empty(min(chunk, Q), self.k, dtype=torch.float32, device=x.device)
            for k0 in range(0, Q, chunk):
                n = min(chunk, Q - k0)
                self._topk(self._normalized(x[k0:k0 + n]), idx, sim)
                self._vote(idx, sim, n, H, W, k0 if pixels is None else 0, None if pixels is None else pixels.data_ptr() + 8 * k0,
                           label_map, conf_map, margin_map, None if probs is None else probs.data_ptr() + 4 * self.num_class * k0)

    def predict(self, features, return_probs=False):
        """-> (labels int64 [Q], confidence fp32 [Q], margin fp32 [Q]) and with return_probs=True also probs fp32 [Q, num_class]
        (columns below `first` are 0): the weighted vote of every query's k nearest bank rows."""
        x, _ = self._queries(features)
        Q, dev = int(x.shape[0]), x.device
        labels = torch.zeros(Q, dtype=torch.int64, device=dev)
        conf = torch.zeros(Q, dtype=torch.float32, device=dev)
        margin = torch.zeros(Q, dtype=torch.float32, device=dev)
        probs = torch.empty(Q, self.num_class, dtype=torch.float32, device=dev) if return_probs else None
        if Q:
            self.predict_into(x, 1, Q, None, labels, conf, margin, probs)
        return (labels, conf, margin, probs) if return_probs else (labels, conf, margin)

    def check(self):
        """Raise if a vote since the last check() met a neighbour whose label was outside [first, num_class) (one small copy;
        fit() has checked the labels, so this cannot happen unless the bank was changed behind its back)."""
        if self._bad is not None and int(self._bad.item()):
            self._bad.zero_()
            raise RuntimeError(f"KNNClassifier: a bank label was outside [{self.first}, {self.num_class})")
