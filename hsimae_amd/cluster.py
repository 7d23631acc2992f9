"""Unsupervised land-cover maps: k-means on frozen features on the device (csrc/kmeans.hip), and what scores such a map.

  KMeans(n_clusters, metric)   Lloyd's algorithm with hsimae_kmeans_assign / hsimae_kmeans_update: every round is two calls on the
      current stream and `fit` issues exactly `max_iter` of them without waiting for the host.  Lloyd at a fixed point is
      idempotent and the kernels are deterministic (no atomics), so the rounds after convergence change nothing, bit for bit; how
      many rounds changed a label is counted on the device (`n_iter_`).
  hungarian_max / cluster_mapping / purity / nmi / ari   the host side of the evaluation, in fp64 numpy on the small
      (class, cluster) contingency table (ScoreMeter counts it on the device): the one-to-one matching of clusters to classes that
      maximises the matches, and the partition scores of the unsupervised HSI literature.  Neither scipy nor sklearn is imported.

k-means++ seeding is out of scope: `n_init` restarts of the random seeding cover the need.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from .knn import _features

MAX_CLUSTERS = 1024
METRICS = ("cosine", "euclidean")

# what DualViT.cluster_scene returns
SceneClustering = collections.namedtuple("SceneClustering", ["labels", "score", "margin", "centroids", "counts", "inertia", "n_iter"])


class KMeans:
    """k-means over fp32 rows [N, D] on a GPU (D % 4 == 0, D <= 4096, 1 <= n_clusters <= 1024).
    metric="cosine": spherical k-means, rows and centroids L2-normalised (one hsimae_row_normalize copy of the features), the
    score of a row is its cosine similarity to the centroid.  metric="euclidean": the features as they are, score = x . c -
    1/2 ||c||^2 (the argmax is the nearest centroid).  Labels are first .. first + n_clusters - 1 (first = 1 leaves 0 for
    "not asked", as the scene maps do).
    init="random": n_clusters distinct rows drawn with torch.randperm(N, generator=generator) on the CPU generator (stream-
    reproducible); a tensor [n_clusters, D]: the seed centroids.  Either way the centroids are seeded by one update over the seed
    rows, so they are normalised / biased by the code the later rounds use.
    n_init > 1: that many seedings (a given tensor is used for each, so only "random" gains from it); the run with the lowest
    final inertia is kept, which costs one host read per restart.  With n_init = 1 fit() never waits for the host.
    An empty cluster keeps its centroid; `empty_` counts them after the last round.
    After fit(), all on the features' device: centroids fp32 [K, D], counts int64 [K], labels_ int64 [N], inertia_ (0-d fp64: the sum
    of squared distances of the last update, to the centroids its labels were assigned against: at the fixed point the final
    inertia), n_iter_ (0-d int64: rounds that changed a label), empty_ (0-d int64)."""

    CHUNK_BYTES = 64 << 20          # predict_into: the normalised copy of a chunk of rows is at most this large

    def __init__(self, n_clusters, metric="cosine", max_iter=20, n_init=1, init="random", generator=None, first=1):
        self.n_clusters, self.max_iter, self.n_init, self.first = int(n_clusters), int(max_iter), int(n_init), int(first)
        if not 1 <= self.n_clusters <= MAX_CLUSTERS:
            raise ValueError(f"between 1 and {MAX_CLUSTERS} clusters are served, got {n_clusters}")
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        if self.max_iter < 1 or self.n_init < 1:
            raise ValueError(f"max_iter and n_init must be >= 1, got {max_iter} and {n_init}")
        if self.first < 0:
            raise ValueError(f"first must be >= 0, got {first}")
        if isinstance(init, str):
            if init != "random":
                raise ValueError(f'init must be "random" or a tensor [n_clusters, D], got {init!r} (k-means++ is not served)')
        elif not isinstance(init, torch.Tensor):
            raise TypeError(f'init must be "random" or a tensor [n_clusters, D], got {type(init).__name__}')
        self.metric, self.init, self.generator = metric, init, generator
        self.centroids = self.bias = self.counts = self.labels_ = self.inertia_ = self.n_iter_ = self.empty_ = self._state = None

    # ------------------------------------------------------------------ the launches
    @staticmethod
    def _stream(dev):
        return torch.cuda.current_stream(dev).cuda_stream

    @staticmethod
    def _ld(t):
        return t.stride(0) if t.shape[0] > 1 else t.shape[1]

    def _normalized(self, x):
        out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        p = _lib.RowNormalizeParams(x=x.data_ptr(), ld=self._ld(x), N=x.shape[0], D=x.shape[1], out=out.data_ptr(), ldo=x.shape[1])
        _lib.check(_lib.load().hsimae_row_normalize(C.byref(p), self._stream(x.device)), "hsimae_row_normalize")
        return out

    def _rows(self, x):
        return self._normalized(x) if self.metric == "cosine" else x

    def _assign(self, x, n, c, bias, H, W, p0, pixels_ptr, labels, score, margin, changed):
        p = _lib.KmeansAssignParams(x=x.data_ptr(), ldx=self._ld(x), c=c.data_ptr(), ldc=c.shape[1], bias=_lib.ptr(bias), N=n,
                                    K=self.n_clusters, D=c.shape[1], first=self.first, H=H, W=W, p0=p0, pixels=pixels_ptr,
                                    labels=labels.data_ptr(), score=_lib.ptr(score), margin=_lib.ptr(margin), changed=_lib.ptr(changed))
        _lib.check(_lib.load().hsimae_kmeans_assign(C.byref(p), self._stream(c.device)), "hsimae_kmeans_assign")

    def _update(self, x, labels, w, changed):
        c = w["c"]
        p = _lib.KmeansUpdateParams(x=x.data_ptr(), ldx=self._ld(x), labels=labels.data_ptr(), N=x.shape[0], K=self.n_clusters,
                                    D=c.shape[1], first=self.first, normalize=int(self.metric == "cosine"), c=c.data_ptr(),
                                    ldc=c.shape[1], bias=_lib.ptr(w["bias"]), counts=w["counts"].data_ptr(), sums=w["sums"].data_ptr(),
                                    changed=_lib.ptr(changed), scratch=w["scratch"].data_ptr(), state=w["state"].data_ptr())
        _lib.check(_lib.load().hsimae_kmeans_update(C.byref(p), self._stream(c.device)), "hsimae_kmeans_update")

    def _run(self, xs, seeds):
        """One seeding and max_iter rounds on the current stream -> the run's tensors; nothing waits for the host."""
        K, (N, D), dev = self.n_clusters, xs.shape, xs.device
        w = {"c": torch.zeros(K, D, dtype=torch.float32, device=dev),
             "bias": torch.zeros(K, dtype=torch.float32, device=dev) if self.metric == "euclidean" else None,
             "counts": torch.zeros(K, dtype=torch.int64, device=dev), "sums": torch.zeros(K, D, dtype=torch.float64, device=dev),
             "scratch": torch.zeros(K * ((D + 63) // 64) + 1, dtype=torch.float64, device=dev),
             "state": torch.zeros(_lib.KMEANS_STATE, dtype=torch.float64, device=dev),
             "labels": torch.zeros(N, dtype=torch.int64, device=dev)}
        changed = torch.zeros(_lib.KMEANS_GRID, dtype=torch.int32, device=dev)
        # seeding: every centroid is the mean of one row (labels first .. first + K - 1), normalised or biased as later rounds do
        self._update(seeds, torch.arange(self.first, self.first + K, dtype=torch.int64, device=dev), w, None)
        for _ in range(self.max_iter):
            self._assign(xs, N, w["c"], w["bias"], 1, N, 0, None, w["labels"], None, None, changed)
            self._update(xs, w["labels"], w, changed)
        self._assign(xs, N, w["c"], w["bias"], 1, N, 0, None, w["labels"], None, None, None)   # labels of the final centroids
        return w

    # ------------------------------------------------------------------ public
    def fit(self, features):
        x = _features(features, "features")
        N, D, K, dev = int(x.shape[0]), int(x.shape[1]), self.n_clusters, x.device
        if N < 1:
            raise ValueError("features has no rows")
        if N >= 1 << 31:
            raise ValueError(f"fewer than 2^31 rows are served, got {N}")
        given = None
        if isinstance(self.init, torch.Tensor):
            given = _features(self.init, "init")
            if tuple(given.shape) != (K, D):
                raise ValueError(f"init must be [{K}, {D}], got {tuple(given.shape)}")
            if given.device != dev:
                raise RuntimeError(f"hsimae_amd runs on MI355X only (no CPU fallback): init is on {given.device}, the features on {dev}")
        elif K > N:
            raise ValueError(f"{K} distinct seed rows cannot be drawn from {N} rows")
        with torch.no_grad(), torch.cuda.device(dev):
            xs = self._rows(x)
            best = best_inertia = None
            for _ in range(self.n_init):
                if given is not None:
                    seeds = given
                else:
                    seeds = xs[torch.randperm(N, generator=self.generator)[:K].to(dev)]
                w = self._run(xs, seeds)
                if self.n_init == 1:
                    best = w
                    break
                inertia = float(w["state"][0].item())              # the one host read of a restart
                if best is None or inertia < best_inertia or (best_inertia != best_inertia and inertia == inertia):
                    best, best_inertia = w, inertia
            self.centroids, self.bias, self.counts, self.labels_, self._state = best["c"], best["bias"], best["counts"], best["labels"], best["state"]
            self.inertia_ = self._state[0]
            self.n_iter_, self.empty_ = self._state[2].to(torch.int64), self._state[3].to(torch.int64)
        return self

    def _queries(self, features):
        if self.centroids is None:
            raise RuntimeError("KMeans: call fit() first")
        x = _features(features, "features")
        if x.device != self.centroids.device:
            raise RuntimeError(f"hsimae_amd runs on MI355X only (no CPU fallback): features are on {x.device}, the centroids on "
                               f"{self.centroids.device}")
        if x.shape[1] != self.centroids.shape[1]:
            raise ValueError(f"features have {x.shape[1]} columns, the centroids {self.centroids.shape[1]}")
        return x, max(64, self.CHUNK_BYTES // (4 * int(x.shape[1])))

    def predict_into(self, features, H, W, pixels, label_map, score_map=None, margin_map=None):
        """The label, best score and margin (best - second best score) of the rows of `features`, written at `pixels` (int64
        device tensor, one per row; None: row order) of the [H * W] maps, in chunks of rows."""
        x, chunk = self._queries(features)
        Q = int(x.shape[0])
        with torch.no_grad(), torch.cuda.device(x.device):
            for k0 in range(0, Q, chunk):
                n = min(chunk, Q - k0)
                self._assign(self._rows(x[k0:k0 + n]), n, self.centroids, self.bias, H, W, k0 if pixels is None else 0,
                             None if pixels is None else pixels.data_ptr() + 8 * k0, label_map, score_map, margin_map, None)

    def predict(self, features):
        """-> (labels int64 [Q], score fp32 [Q], margin fp32 [Q]) on the features' device."""
        x, _ = self._queries(features)
        Q, dev = int(x.shape[0]), x.device
        labels = torch.zeros(Q, dtype=torch.int64, device=dev)
        score = torch.zeros(Q, dtype=torch.float32, device=dev)
        margin = torch.zeros(Q, dtype=torch.float32, device=dev)
        if Q:
            self.predict_into(x, 1, Q, None, labels, score, margin)
        return labels, score, margin

    def fit_predict(self, features):
        return self.fit(features).labels_


# ---------------------------------------------------------------------- the host side of the evaluation (fp64 numpy)
def hungarian_max(table):
    """The one-to-one assignment of rows to columns that maximises the sum of table[row, col] (Kuhn-Munkres with potentials,
    O(n^3)); a rectangular table is zero-padded to a square.  -> (rows, cols): min(table.shape) pairs, rows ascending."""
    t = np.asarray(table, np.float64)
    if t.ndim != 2 or not t.size:
        raise ValueError(f"table must be a non-empty 2-D array, got shape {t.shape}")
    nr, nc = t.shape
    n = max(nr, nc)
    profit = np.zeros((n, n))
    profit[:nr, :nc] = t
    cost = np.zeros((n + 1, n + 1))
    cost[1:, 1:] = profit.max() - profit
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)       # p[col] = the row matched to it (1-based, 0: none)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0] - u[i0] - v
            free = ~used
            free[0] = False
            better = free & (cur < minv)
            minv[better], way[better] = cur[better], j0
            cand = np.where(free, minv, np.inf)
            j1 = int(np.argmin(cand))
            delta = cand[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    rows, cols = p[1:] - 1, np.arange(n)
    keep = (rows < nr) & (cols < nc)
    order = np.argsort(rows[keep], kind="stable")
    return rows[keep][order], cols[keep][order]


def cluster_mapping(table):
    """table[class, cluster] = labelled pixels of that class in that cluster -> class index of every cluster: the matching that
    maximises the matched pixels (hungarian_max); a cluster left unmatched (more clusters than classes) takes its majority
    class (ties: the lower class)."""
    t = np.asarray(table, np.float64)
    out = np.argmax(t, axis=0)
    rows, cols = hungarian_max(t)
    out[cols] = rows
    return out


def purity(table):
    t = np.asarray(table, np.float64)
    return float(t.max(axis=0).sum() / t.sum())


def _entropy(counts):
    q = counts[counts > 0] / counts.sum()
    return float(-(q * np.log(q)).sum())


def nmi(table):
    """Normalised mutual information of the two partitions, arithmetic-mean normalisation: I / ((H_class + H_cluster) / 2); 1
    when both partitions have a single part."""
    t = np.asarray(table, np.float64)
    n = t.sum()
    a, b = t.sum(1), t.sum(0)
    hc, hk = _entropy(a), _entropy(b)
    if hc == 0.0 and hk == 0.0:
        return 1.0
    nz = t > 0
    mi = float((t[nz] / n * (np.log(t[nz] * n) - np.log(np.outer(a, b)[nz]))).sum())
    return float(min(1.0, max(0.0, mi) / ((hc + hk) / 2)))


def ari(table):
    """Adjusted Rand index (Hubert & Arabie 1985) from the contingency table; 1 when the denominator vanishes (both partitions
    trivial)."""
    t = np.asarray(table, np.float64)
    n = t.sum()
    pairs = lambda x: float((x * (x - 1) / 2).sum())                      # noqa: E731
    s, sa, sb, tot = pairs(t), pairs(t.sum(1)), pairs(t.sum(0)), n * (n - 1) / 2
    expected = sa * sb / tot if tot else 0.0
    denom = (sa + sb) / 2 - expected
    return 1.0 if denom == 0 else float((s - expected) / denom)
