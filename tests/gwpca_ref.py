"""fp64 restatement of group-wise PCA and a per-component error bound (tests/test_gwpca_cpu.py, tests/test_gpu_gwpca.py,
tests/golden/make_golden_gwpca.py).  A plain module, not a conftest.

The restatement (numpy, float64), written from the definition and not from the reference's code:
    x = (X - min X) / (max X - min X) over the whole scene; bands split by recursive halving (c -> c // 2, c - c // 2,
    group // 2 times); per group of width w, n = H * W, k = nc // group:
    mean; C = D^T D / (n - 1) with D = x - mean, accumulated centred in a second pass; (lambda, V) = eigh(C), descending,
    negative lambda clipped to 0; each retained v_j signed so that its entry of largest magnitude (first on a tie) is
    positive; y_j = D v_j, with whitening divided by max(sqrt(lambda_j), eps).

The bound.  Two correct fp64 implementations of the above differ by
 (i)   the rounding of the mean and of the covariance sums,
 (ii)  the eigen-solver's backward error,
 (iii) the roundings of the projection itself.
(i) and (ii) are a perturbation dC of C.  To first order it moves v_k by sum_{j != k} (v_j^T dC v_k) / (lambda_k - lambda_j) v_j
and lambda_k by v_k^T dC v_k, and |v_j^T dC v_k| <= ||dC||_2.  With s_k the whitening scale (1 without whitening):

    |dy_k(p)| <= ||dC|| * sum_{j != k} |D_p . v_j| / (|lambda_k - lambda_j| s_k)        (eigenvector)
               + ||dC|| * |y_k(p)| / (2 lambda_k)                    [whitening only]  (eigenvalue under the square root)
               + [(w + 4) u sum_i |D_pi| |v_ik| + sqrt(w) dmean] / s_k                  (projection, mean)

and the bound of component k is the maximum over the pixels p of the right-hand side (each |D_p . v_j| replaced by its
maximum over p).  The sum runs over ALL eigenvalues of the group, retained or not; its largest term is
||dC|| / gap_k * max|y|-sized, i.e. the bound scales with 2^-53 lambda_1 / gap_k max|y_k|, gap_k the distance from lambda_k
to its nearest neighbour.  Constants, u = 2^-53:

    ||dC||  = u * (C_SUM * sqrt(n) * trace C  +  C_EIG * sqrt(w) * lambda_1  +  2 trace C)
    dmean   = u * (C_SUM * sqrt(n) + 4) * max|X| / (max X - min X)

 * C_SUM * sqrt(n): a sum of n terms accumulated in any order has the deterministic bound n u sum|terms|; its roundings are
   of either sign, and the probabilistic form sqrt(n) u (Higham & Mary 2019) is what tests/gemm_ref.py uses for the same
   reason.  |dC_ij| <= sqrt(n) u sqrt(C_ii C_jj), so ||dC||_2 <= ||dC||_F <= sqrt(n) u trace C.  C_SUM = 1.
   The mean may be formed from the raw sums, (sum X / n - min) / range, which scales its rounding by max|X| / range.
 * C_EIG * sqrt(w): a Jacobi sweep applies w - 1 rotations to every matrix entry, each with a rounding of u ||C||; over the
   at most 10 sweeps a converged solve takes that is a random walk of 10 w steps, <= 4 sqrt(10 w) u ||C|| < 13 sqrt(w) u
   lambda_1.  LAPACK's own backward error is of the same form.  C_EIG = 13.
 * 2 trace C: the solver stops at an off-diagonal norm of 2^-52 trace C.
The bound is derived, not tuned; the tests print the worst err / bound they meet.
"""
import numpy as np

U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)
C_SUM = 1.0
C_EIG = 13.0
BLOCK = 4096            # pixels per partial sum of the restatement's own two passes


def groups(bands, group=4):
    """[(start, end)] of the contiguous band groups: every range halved (c -> c // 2, c - c // 2), group // 2 times."""
    out = [(0, int(bands))]
    for _ in range(group // 2):
        nxt = []
        for a, e in out:
            m = a + (e - a) // 2
            nxt += [(a, m), (m, e)]
        out = nxt
    return out


def normalise(X):
    X = np.asarray(X)
    x = X.reshape(-1, X.shape[-1]).astype(np.float64)
    mn, mx = x.min(), x.max()
    return (x - mn) / (mx - mn), float(mn), float(mx)


def centred_cov(x, order=None, drop=None):
    """Mean and covariance of the rows of x [n, w]: two passes, partial sums of BLOCK rows.  order: a row permutation (another
    summation order); drop: a slice of rows left out of the covariance pass (a planted fault)."""
    n, w = x.shape
    xs = x if order is None else x[order]
    mu = np.zeros(w)
    for i in range(0, n, BLOCK):
        mu += xs[i:i + BLOCK].sum(0)
    mu /= n
    Cm = np.zeros((w, w))
    for i in range(0, n, BLOCK):
        d = xs[i:i + BLOCK] - mu
        if drop is not None:
            keep = np.ones(len(d), bool)
            keep[max(drop.start - i, 0):max(drop.stop - i, 0)] = False
            d = d[keep]
        Cm += d.T @ d
    return mu, Cm / (n - 1)


def eig_desc(Cm, k):
    """All eigenvalues descending (clipped at 0) and the k leading eigenvectors as rows, signed: largest |entry| positive."""
    lam, V = np.linalg.eigh(Cm)
    lam, V = lam[::-1].copy(), V[:, ::-1]
    Vt = V.T.copy()
    arg = np.abs(Vt).argmax(1)                       # first index on a tie
    Vt *= np.where(Vt[np.arange(len(Vt)), arg] < 0, -1.0, 1.0)[:, None]
    return np.maximum(lam, 0.0), Vt[:k], Vt


def whiten_scale(lam_k, whiten):
    return np.maximum(np.sqrt(lam_k), EPS) if whiten else np.ones_like(lam_k)


def gwpca_ref(X, nc=32, group=4, whiten=True, order=None):
    """-> dict: out [H, W, nc] fp64; min, max; mean [C]; lam [C] (all eigenvalues, per group descending); comps (list of [k, w]);
    bound [nc] (per component, absolute, on `out`); mean_bound (scalar), lam_bound [C]; gap_rel, lam_rel [nc] (the fixture
    condition: gap_k / lambda_k and lambda_k / lambda_1 of every retained component)."""
    X = np.asarray(X)
    H, W, Cb = X.shape
    x, mn, mx = normalise(X)
    n, k = x.shape[0], nc // group
    amp = float(np.abs(X.astype(np.float64)).max() / (mx - mn)) if mx > mn else np.inf
    dmean = U * (C_SUM * np.sqrt(n) + 4.0) * amp
    out, means, lams, comps, bound, lam_bound, gap_rel, lam_rel = [], [], [], [], [], [], [], []
    for a, e in groups(Cb, group):
        w = e - a
        mu, Cm = centred_cov(x[:, a:e], order)
        lam, Vk, Vall = eig_desc(Cm, k)
        D = x[:, a:e] - mu
        s = whiten_scale(lam[:k], whiten)
        y = D @ Vk.T / s
        dC = U * (C_SUM * np.sqrt(n) * np.trace(Cm) + C_EIG * np.sqrt(w) * lam[0] + 2.0 * np.trace(Cm))
        proj_all = np.abs(D @ Vall.T).max(0)                          # max_p |D_p . v_j|, every j
        b = np.zeros(k)
        for c in range(k):
            diff = np.abs(lam[c] - np.delete(lam, c))
            b[c] = dC * np.sum(np.delete(proj_all, c) / diff) / s[c]
            if whiten:
                b[c] += dC * np.abs(y[:, c]).max() / (2.0 * lam[c])
            b[c] += ((w + 4) * U * (np.abs(D) @ np.abs(Vk[c])).max() + np.sqrt(w) * dmean) / s[c]
            gap_rel.append(diff.min() / lam[c])
            lam_rel.append(lam[c] / lam[0])
        out.append(y); means.append(mu); lams.append(lam); comps.append(Vk); bound.append(b)
        lam_bound.append(np.full(w, dC))
    return {"out": np.concatenate(out, 1).reshape(H, W, nc), "min": mn, "max": mx, "mean": np.concatenate(means),
            "lam": np.concatenate(lams), "comps": comps, "bound": np.concatenate(bound), "mean_bound": dmean,
            "lam_bound": np.concatenate(lam_bound), "gap_rel": np.array(gap_rel), "lam_rel": np.array(lam_rel)}


def component_err(a, b):
    """max over the pixels of |a - b| per component: [nc]."""
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).reshape(-1, a.shape[-1]).max(0)


def graded(H, W, Cb, seed, group=4, ratio=0.55, k=14, dtype=np.float64):
    """A raw scene whose groups each hold min(k, w) orthogonal spectral patterns with variances ratio^j on a pedestal: every
    retained eigenvalue is well separated (the fixture condition), values in about [1000, 5000]."""
    r = np.random.RandomState(seed)
    X = np.zeros((H * W, Cb))
    for a, e in groups(Cb, group):
        Q, _ = np.linalg.qr(r.randn(e - a, min(k, e - a)))
        s = ratio ** (0.5 * np.arange(Q.shape[1]))
        X[:, a:e] = (r.rand(H * W, Q.shape[1]) - 0.5) * s @ Q.T + 0.2 * r.rand(e - a)
    return (4000.0 * X + 1000.0).reshape(H, W, Cb).astype(dtype)
