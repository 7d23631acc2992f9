"""numpy restatement of csrc/recon.hip (hsimae_recon_accumulate / hsimae_recon_finish, include/hsimae_hip.h) and the bounds the
GPU is held to.

accumulate   replayed sequentially in fp32 in the stated order (windows ascending, one add per voxel and window).  fp32 addition
             is exact arithmetic followed by one rounding, the same in numpy and on the device: the GPU must match BIT FOR BIT.
finish       in fp64 from the SAME fp32 inputs.  r = sum / (float)cnt is one IEEE fp32 division: under the project's flags (-O3,
             no fast-math; hipcc's -fhip-fp32-correctly-rounded-divide-sqrt is on by default) it is correctly rounded, as
             numpy's float32 division is, so `recon` must be bit-equal and the division contributes 0 to the bounds below.
             With u = 2^-53 (fp64 unit roundoff), per pixel with m reconstructed bands:
  se      m products (r - x)^2, each (1 + 2u) at most (the difference of two fp32 values rounds once when their exponents are far
          apart, the square once; fma only removes roundings), added in any order: relative (m + 1) u.  se / m: + u.  sqrt is
          correctly rounded in fp64 (IEEE): halves what came before, + u.  rmse_fp64 is therefore within (m / 2 + 3) u relative,
          for the device and for this file alike, so the two differ by at most (m + 6) u |rmse|; the final fp32 rounding adds
          2^-24 |rmse| (and 2^-149 absolute where the result is subnormal).
  sam     nr, nx: relative (m / 2 + 2) u each by the argument above.  The unit vectors p = r / nr, q = x / nx are therefore off by
          at most e_u = (m / 2 + 3) u in norm.  A = |p - q|, B = |p + q|: each is off by at most 2 e_u from the vectors and
          (m / 2 + 2) u (A or B) from its own subtraction / sum / sqrt.  With A^2 + B^2 = 4 the angle t = atan2(A, B) moves by at most
          (|dA| B + |dB| A) / 4 <= (|dA| + |dB|) / 2, so sam = 2 t by |dA| + |dB| <= 4 e_u + (m / 2 + 2) u (A + B)
          <= (2 m + 12) u + 3 (m / 2 + 2) u = (3.5 m + 18) u absolute.  atan2 in fp64: AMD's device library documents 2 ulp = 4 u
          relative; numpy's libm atan2 is below 1 ulp.  Device and this file together: 2 (3.5 m + 18) u + 6 u |sam|, then the fp32
          rounding 2^-24 |sam| (+ 2^-149).  r == x bit for bit gives A = 0 and sam = 0 exactly.
  stats   sums of n non-negative fp64 terms in a fixed order: relative (n - 1) u on top of the terms' own errors.  The counts
          (stats[1], stats[3]) are integers below 2^53: exact.
No constant here is measured.
"""
import numpy as np

U = 2.0 ** -53
GRID = 1024                 # HSIMAE_RECON_GRID


def centres(L, s):
    """The window centres along an axis of length L for stride s, from the issue's words (not from hsimae_amd.recon)."""
    out = []
    c = min(4, L - 1)
    while c <= L - 1:
        out.append(c)
        c += s
    if out[-1] + 4 < L - 1:
        out.append(L - 1)
    return np.array(out, dtype=np.int32)


def sym(q, n):
    m = q % (2 * n)
    return m if m < n else 2 * n - 1 - m


# ------------------------------------------------------------------ accumulate
def accumulate(pred, mask, rows, cols, w0, H, W, acc, cnt, fault=None):
    """In place: acc fp32 [H][W][C], cnt int32 [H][W][C] after the chunk pred / mask fp32 [n][C][9][9] holding the windows
    w0 .. w0 + n - 1.  Windows ascending; within a window every voxel is touched once, so the slab update is the sequential
    replay.  `fault` plants one of the mistakes test_recon_bound_cpu.py lists."""
    n = pred.shape[0]
    ncols = len(cols)
    order = range(n - 1, -1, -1) if fault == "descending" else range(n)
    with np.errstate(invalid="ignore"):
        for k in order:
            ir, ic = divmod(w0 + k, ncols)
            r0, c0 = int(rows[ir]) - 4, int(cols[ic]) - 4
            if fault == "reflected":                    # every position lands somewhere, through the pad's own index map
                for i in range(9):
                    for j in range(9):
                        r, c = sym(r0 + i, H), sym(c0 + j, W)
                        on = mask[k, :, i, j] != 0
                        acc[r, c, on] = (acc[r, c, on] + pred[k, on, i, j]).astype(np.float32)
                        cnt[r, c, on] += 1
                continue
            i0, i1 = max(0, -r0), min(9, H - r0)
            j0, j1 = max(0, -c0), min(9, W - c0)
            p = pred[k, :, i0:i1, j0:j1].transpose(1, 2, 0)
            on = mask[k, :, i0:i1, j0:j1].transpose(1, 2, 0) != 0
            a = acc[r0 + i0:r0 + i1, c0 + j0:c0 + j1]
            q = cnt[r0 + i0:r0 + i1, c0 + j0:c0 + j1]
            if fault == "multiply":
                a[...] = (a + p * on.astype(np.float32)).astype(np.float32)
            else:
                a[on] = (a[on] + p[on]).astype(np.float32)
            if fault == "no_increment":
                q[on] = 1
            else:
                q[on] += 1


def make_windows(H, W, C, stride, seed):
    """A synthetic forward output over the whole window grid of an H x W x C scene: -> scene fp64 [H][W][C], rows, cols, pred,
    mask fp32 [nwin][C][9][9].  pred is the scene's window times (1 + 5 % noise); mask is 0 / 1 per (window, band octet, 3 x 3
    patch) as the model masks; NaN sits in pred wherever mask is 0 and at EVERY reflected position (whatever its mask)."""
    rng = np.random.default_rng(seed)
    scene = rng.uniform(0.05, 1.0, size=(H, W, C))
    rows, cols = centres(H, stride), centres(W, stride)
    nwin = len(rows) * len(cols)
    tok = rng.random((nwin, C // 8, 3, 3)) < 0.6
    mask = np.repeat(np.repeat(np.repeat(tok, 8, axis=1), 3, axis=2), 3, axis=3).astype(np.float32)
    w = np.arange(nwin)
    r = rows[w // len(cols)].astype(np.int64)[:, None] - 4 + np.arange(9)            # [nwin][9]
    c = cols[w % len(cols)].astype(np.int64)[:, None] - 4 + np.arange(9)
    inside = ((r >= 0) & (r < H))[:, :, None] & ((c >= 0) & (c < W))[:, None, :]
    mr, mc = r % (2 * H), c % (2 * W)
    sr, sc = np.where(mr < H, mr, 2 * H - 1 - mr), np.where(mc < W, mc, 2 * W - 1 - mc)
    cube = scene[sr[:, :, None], sc[:, None, :]].transpose(0, 3, 1, 2)                # [nwin][C][9][9]
    pred = (cube * (1 + 0.05 * rng.standard_normal(cube.shape))).astype(np.float32)
    pred[np.broadcast_to(~inside[:, None], pred.shape)] = np.nan
    pred[mask == 0] = np.nan
    return scene, rows, cols, pred, mask


# ------------------------------------------------------------------ finish
def finish(scene, acc, cnt, fault=None):
    """fp64 restatement -> dict(recon fp32, cover int32, rmse, sam fp64 [H][W], stats fp64 [4], and the absolute bounds
    b_rmse, b_sam [H][W], b_stats [4] of the module docstring)."""
    x = scene.astype(np.float32)
    on = cnt > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        r32 = np.where(on, acc / cnt.astype(np.float32), np.float32(0) if fault == "no_fill" else x).astype(np.float32)
    m = on.sum(axis=2).astype(np.int32)
    r, xd = r32.astype(np.float64), x.astype(np.float64)
    sel = np.ones_like(on) if fault == "all_bands" else on
    with np.errstate(invalid="ignore", divide="ignore"):
        se = np.where(on, (r - xd) ** 2, 0.0).sum(axis=2)
        rmse = np.where(m > 0, np.sqrt(se / np.where(m > 0, scene.shape[2] if fault == "div_C" else m, 1)), 0.0)
        nr = np.sqrt(np.where(sel, r * r, 0.0).sum(axis=2))
        nx = np.sqrt(np.where(sel, xd * xd, 0.0).sum(axis=2))
        p, q = r / nr[..., None], xd / nx[..., None]
        if fault == "acos":
            sam = np.arccos(np.clip(np.where(sel, p * q, 0.0).sum(axis=2), -1.0, 1.0))
        else:
            A = np.sqrt(np.where(sel, (p - q) ** 2, 0.0).sum(axis=2))
            B = np.sqrt(np.where(sel, (p + q) ** 2, 0.0).sum(axis=2))
            sam = 2.0 * np.arctan2(A, B)
    zr, zx = nr == 0, nx == 0
    sam = np.where(zr & zx, 0.0, np.where(zr | zx, np.pi / 2, sam))
    sam = np.where(m > 0, sam, 0.0)
    have = m > 0
    npix = int(have.sum())
    stats = np.array([se[have].sum(), float(m[have].sum()), sam[have].sum(), float(npix)])
    md = m.astype(np.float64)
    b_rmse = np.abs(rmse) * (2.0 ** -24 + (md + 6) * U) + 2.0 ** -149
    b_sam_64 = 2 * (3.5 * md + 18) * U + 6 * U * np.abs(sam)
    b_sam = b_sam_64 + np.abs(sam) * 2.0 ** -24 + 2.0 ** -149
    mmax = float(md.max()) if md.size else 0.0
    b_stats = np.array([abs(stats[0]) * (2 * (mmax + 1) + 2 * npix) * U, 0.0,
                        float(b_sam_64[have].sum()) + abs(stats[2]) * 2 * npix * U, 0.0])
    return dict(recon=r32, cover=m, rmse=rmse, sam=sam, stats=stats, b_rmse=b_rmse, b_sam=b_sam, b_stats=b_stats)


def _tree(v):
    """The xor tree over the last axis (64 lanes): partner lane ^ 1, ^ 2, .. ^ 32."""
    idx = np.arange(64)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[..., idx ^ s]
    return v[..., 0]


def _lanes(t, on):
    """Lane-strided fp64 sums of t [npix][C] over the bands with `on`: lane l adds b = l, l + 64, .. in order; then the tree."""
    npix, C = t.shape
    lanes = np.zeros((npix, 64))
    for b0 in range(0, C, 64):
        w = min(64, C - b0)
        lanes[:, :w] = lanes[:, :w] + np.where(on[:, b0:b0 + w], t[:, b0:b0 + w], 0.0)
    return _tree(lanes)


def finish_emulated(scene, acc, cnt):
    """The device's own sequence in numpy: fp32 division, fp64 lane-strided sums, the xor tree, the per-wave / per-workgroup /
    final order of stats, the fp32 roundings of the maps.  (numpy has no fma: products round once more than the device's.)"""
    H, W, C = scene.shape
    x = scene.astype(np.float32).reshape(-1, C)
    k = cnt.reshape(-1, C)
    on = k > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        r32 = np.where(on, acc.reshape(-1, C) / k.astype(np.float32), x).astype(np.float32)
        r, xd = r32.astype(np.float64), x.astype(np.float64)
        m = on.sum(axis=1)
        se, rr, xx = _lanes((r - xd) ** 2, on), _lanes(r * r, on), _lanes(xd * xd, on)
        rmse = np.where(m > 0, np.sqrt(se / np.maximum(m, 1)), 0.0)
        nr, nx = np.sqrt(rr), np.sqrt(xx)
        p, q = r / nr[:, None], xd / nx[:, None]
        sam = 2.0 * np.arctan2(np.sqrt(_lanes((p - q) ** 2, on)), np.sqrt(_lanes((p + q) ** 2, on)))
    sam = np.where((nr == 0) & (nx == 0), 0.0, np.where((nr == 0) | (nx == 0), 1.5707963267948966, sam))
    sam = np.where(m > 0, sam, 0.0)
    npix = H * W
    G = min((npix + 3) // 4, GRID)
    stats = np.zeros(4)
    for j, v in enumerate((np.where(m > 0, se, 0.0), m.astype(np.float64), sam, (m > 0).astype(np.float64))):
        steps = -(-npix // (4 * G))
        pad = np.zeros(steps * 4 * G)
        pad[:npix] = v
        waves = np.zeros(4 * G)
        for t in range(steps):
            waves = waves + pad[t * 4 * G:(t + 1) * 4 * G]
        wv = waves.reshape(G, 4)
        blocks = ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]
        lanes = np.zeros(64)
        for g0 in range(0, G, 64):
            w = min(64, G - g0)
            lanes[:w] = lanes[:w] + blocks[g0:g0 + w]
        stats[j] = _tree(lanes)
    return dict(recon=r32.reshape(H, W, C), cover=m.reshape(H, W).astype(np.int32), rmse=rmse.astype(np.float32).reshape(H, W),
                sam=sam.astype(np.float32).reshape(H, W), stats=stats)


def make_sums(H, W, C, seed):
    """Finish inputs with every special pixel: -> scene fp64, acc fp32, cnt int32, and the flat indices of the special pixels
    dict(empty=, both_zero=, one_zero=, same=, near=).  The rest: counts 0 .. 3 per voxel, acc = cnt x the scene within 5 %."""
    rng = np.random.default_rng(seed)
    scene = rng.uniform(0.05, 1.0, size=(H, W, C))
    cnt = rng.integers(0, 4, size=(H, W, C)).astype(np.int32)
    acc = (scene * cnt * (1 + 0.05 * rng.standard_normal((H, W, C)))).astype(np.float32)
    flat_s, flat_a, flat_c = scene.reshape(-1, C), acc.reshape(-1, C), cnt.reshape(-1, C)
    pick = rng.permutation(H * W)[:5] if H * W >= 5 else np.arange(0)
    names = ["empty", "both_zero", "one_zero", "same", "near"]
    special = {}
    for name, px in zip(names, pick):
        special[name] = int(px)
        if name == "empty":
            flat_c[px] = 0
            flat_a[px] = 0
        elif name == "both_zero":
            flat_c[px] = 2
            flat_a[px] = 0
            flat_s[px] = 0.0
        elif name == "one_zero":
            flat_c[px] = 1
            flat_a[px] = 0
        elif name == "same":
            flat_c[px] = 1
            flat_c[px, 0] = 0                             # one band never reconstructed: it must not matter
            flat_a[px] = flat_s[px].astype(np.float32)
        elif name == "near":                              # the angle a good model lands at: two bands one ulp off
            flat_c[px] = 1
            a = flat_s[px].astype(np.float32)
            a[:2] = np.nextafter(a[:2], np.float32(2))
            flat_a[px] = a
    acc[cnt == 0] = 0
    return scene, acc, cnt, special
