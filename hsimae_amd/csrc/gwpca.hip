// Group-wise PCA of a raw scene (Utils/GroupWisePCA.py `applyGWPCA`): x = (X - min X) / (max X - min X) over the whole
// [H][W][C] array, the band axis halved `group / 2` times into contiguous groups, and per group a (whitened) PCA with
// nc / group components, concatenated into [H][W][nc].  fp64 throughout; an fp32 scene is widened exactly on load.
//
// What is computed is the exact PCA (what scikit-learn >= 1.5 does for every scene: `covariance_eigh` when n >= 10 w, LAPACK
// `full` otherwise; the reference pins 1.3, whose `auto` sends a large scene through the randomized solver, an approximation
// of the same decomposition).  The covariance is accumulated CENTRED, in a second pass after the mean, not as the
// reference's X^T X - n mean mean^T: for data in [0, 1] mean^2 is 10-100 x the variance and that subtraction is where the
// reference loses its digits.  No floating-point atomics: every reduction goes through a per-workgroup slab that is combined
// in a fixed order, so two runs are bit-identical.
//
//   1. gw_range_sums  one read of the scene: min, max, per-band sum of the RAW values          -> slab1 [nb1][C + 2]
//      gw_model_head  min, max, mean[b] = (sum_b / n - min) / (max - min), the group offsets   (one workgroup)
//   2. gw_gram        pixel tiles of normalised, centred rows staged in LDS; every 16 x 16 tile of every group's D^T D on
//                     v_mfma_f64_16x16x4_f64 (4 pixels per issue), all groups from one read     -> slab2 [nb2][sum w^2]
//      gw_gram_sum    slab2 summed in block order, / (n - 1), mirrored to the full symmetric matrix
//   3. gw_eig         one workgroup per group: cyclic Jacobi in round-robin order on the w x w matrix in LDS, until the
//                     off-diagonal norm is <= 2^-52 trace or GW_MAX_SWEEPS sweeps have run (so NaN input terminates too);
//                     sort, sign (largest-magnitude entry positive, first on a tie), clip, 1 / max(sqrt(lambda), eps)
//                     folded into the projection matrix
//   4. gw_project     y = (x - mean_g) P_g for all groups from one read, [H][W][nc] written with 16-byte stores
//
// max X == min X and non-finite input cannot be detected without a host wait; as in the reference the output is then NaN.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int GW_MAXG = 4;            // groups
constexpr int GW_MAXW = 128;          // widest group the eigen-solver's LDS holds (128 x 129 fp64 = 129 KB of 160 KB)
constexpr int GW_MAX_SWEEPS = 30;     // converged scenes need 6-10; the cap is what ends the loop on NaN / Inf input
constexpr int GW_EIG_THREADS = 512;
constexpr int GW_STAGE_BYTES = 32 * 1024;   // LDS of one staged pixel tile (gram / project): 4 workgroups per CU

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct GwPlan {
    int64_t n;                        // pixels
    int C, ngroups, k, nc, whiten;    // k = nc / group components per group
    int off[GW_MAXG + 1];             // band offsets of the groups
    int sq[GW_MAXG + 1];              // prefix sums of w_g^2 (offsets into the covariance block)
    int wmax, wmin;
    int S, nb1;                       // range/sums: pixel slices per workgroup iteration, workgroups
    int ld2, P2, nb2, npairs, nacc;   // gram: LDS row stride, pixels per tile, workgroups, 16 x 16 tile pairs, per-wave accumulators
    int ld4, P4, nb4, proj_lds;       // project
    int v_lds;                        // eigen-solve: eigenvectors next to the matrix in LDS (m <= 92), else in the workspace
};

struct GwModel {
    double* minmax; double* mean; double* lambda; double* proj; int32_t* goff;
};

int gw_plan(const hsimae_gwpca_params& p, GwPlan& pl) {
    if (p.H <= 0 || p.W <= 0 || p.C <= 0 || p.nc <= 0) return HS_EDIMS;
    pl.n = (int64_t)p.H * p.W;
    if (pl.n < 2) return HS_EDIMS;
    if (p.group != 1 && p.group != 2 && p.group != 4) return HS_EUNSUPPORTED;
    if (p.nc % p.group) return HS_EDIMS;
    pl.C = p.C; pl.ngroups = p.group; pl.nc = p.nc; pl.k = p.nc / p.group; pl.whiten = p.whiten ? 1 : 0;
    // split_data: every range (a, e) -> (a, a + (e - a) / 2), (a + (e - a) / 2, e), group / 2 times
    int cur[GW_MAXG + 1] = {0, p.C}, ncur = 1;
    for (int it = 0; it < p.group / 2; ++it) {
        int nxt[GW_MAXG + 1];
        for (int g = 0; g < ncur; ++g) { nxt[2 * g] = cur[g]; nxt[2 * g + 1] = cur[g] + (cur[g + 1] - cur[g]) / 2; }
        nxt[2 * ncur] = p.C;
        ncur *= 2;
        for (int g = 0; g <= ncur; ++g) cur[g] = nxt[g];
    }
    pl.wmax = 0; pl.wmin = p.C; pl.npairs = 0;
    for (int g = 0; g <= GW_MAXG; ++g) { pl.off[g] = p.C; pl.sq[g] = 0; }
    for (int g = 0; g < ncur; ++g) {
        const int w = cur[g + 1] - cur[g];
        pl.off[g] = cur[g];
        pl.sq[g + 1] = pl.sq[g] + w * w;
        pl.wmax = w > pl.wmax ? w : pl.wmax;
        pl.wmin = w < pl.wmin ? w : pl.wmin;
        const int T = (w + 15) / 16;
        pl.npairs += T * (T + 1) / 2;
    }
    for (int g = ncur; g <= GW_MAXG; ++g) { pl.off[g] = p.C; pl.sq[g] = pl.sq[ncur]; }
    if (pl.k > pl.wmin || pl.k > pl.n) return HS_EDIMS;
    if (pl.wmax > GW_MAXW) return HS_EUNSUPPORTED;
    // 1: S pixel slices of C threads each (C >= 256: one slice, two bands per thread; C <= 512 follows from wmax <= 128)
    pl.S = p.C >= 256 ? 1 : 256 / p.C;
    int64_t nb = (pl.n + (int64_t)pl.S * 16 - 1) / ((int64_t)pl.S * 16);
    pl.nb1 = (int)(nb < 1 ? 1 : nb > 1024 ? 1024 : nb);
    // 2: row stride = 16 mod 32 doubles (the 4 pixel rows of one MFMA operand read land on disjoint banks), >= C + 16 so
    //    that a 16-band tile that overhangs the last group reads zeros
    pl.ld2 = (p.C + 16 + 31) / 32 * 32 + 16;
    int P = GW_STAGE_BYTES / 8 / pl.ld2 / 4 * 4;
    pl.P2 = P < 4 ? 4 : P > 64 ? 64 : P;
    const int64_t tiles2 = (pl.n + pl.P2 - 1) / pl.P2;
    int64_t cap = (int64_t)(64 << 20) / (8 * (int64_t)pl.sq[ncur]);          // the slab stays below 64 MB
    cap = cap < 1 ? 1 : cap > 512 ? 512 : cap;
    pl.nb2 = (int)(tiles2 < cap ? tiles2 : cap);
    const int need = (pl.npairs + 3) / 4;
    pl.nacc = need <= 1 ? 1 : need <= 3 ? 3 : need <= 5 ? 5 : need <= 10 ? 10 : need <= 18 ? 18 : 36;
    // 4
    pl.ld4 = p.C | 1;
    P = GW_STAGE_BYTES / 8 / pl.ld4;
    pl.P4 = P < 1 ? 1 : P > 64 ? 64 : P;
    const int64_t tiles4 = (pl.n + pl.P4 - 1) / pl.P4;
    pl.nb4 = (int)(tiles4 < 2048 ? tiles4 : 2048);
    pl.proj_lds = (int64_t)p.C * pl.k * 8 <= 24 * 1024;
    const int m = pl.wmax + (pl.wmax & 1);
    pl.v_lds = m <= 92;                                  // 2 x 92 x 93 fp64 + the static arrays < 160 KB
    return HS_OK;
}

// min / max that keep a NaN once they have met one (numpy's amin / amax), so that a scene holding a NaN comes out all NaN
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// ---------------------------------------------------------------------------------------------- 1. range and band sums
template <typename T>
__global__ __launch_bounds__(256) void gw_range_sums_kernel(const T* __restrict__ x, GwPlan pl, double* __restrict__ slab) {
    __shared__ double red[512], rmin[256], rmax[256];
    const int t = threadIdx.x, C = pl.C, S = pl.S;
    const int s = S == 1 ? 0 : t / C, b = S == 1 ? t : t - s * C;
    const bool on = s < S && b < C, on2 = S == 1 && b + 256 < C;
    const int64_t rows = (pl.n + gridDim.x - 1) / gridDim.x;           // a contiguous run of pixels per workgroup
    const int64_t r0 = rows * blockIdx.x, r1 = r0 + rows < pl.n ? r0 + rows : pl.n;
    double a0 = 0.0, a1 = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    if (on) {
#pragma unroll 4
        for (int64_t r = r0 + s; r < r1; r += S) {
            const double v = (double)x[r * C + b];
            a0 += v; mn = nan_min(mn, v); mx = nan_max(mx, v);
            if (on2) {
                const double u = (double)x[r * C + b + 256];
                a1 += u; mn = nan_min(mn, u); mx = nan_max(mx, u);
            }
        }
    }
    red[t] = a0; red[256 + t] = a1; rmin[t] = mn; rmax[t] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { rmin[t] = nan_min(rmin[t], rmin[t + h]); rmax[t] = nan_max(rmax[t], rmax[t + h]); }
        __syncthreads();
    }
    double* o = slab + (int64_t)blockIdx.x * (C + 2);
    if (t == 0) { o[0] = rmin[0]; o[1] = rmax[0]; }
    if (s == 0 && b < C) {
        double sum = 0.0;
        for (int q = 0; q < S; ++q) sum += red[q * C + b];              // slices in order
        o[2 + b] = sum;
        if (on2) o[2 + b + 256] = red[256 + t];
    }
}

__global__ __launch_bounds__(256) void gw_model_head_kernel(const double* __restrict__ slab, GwPlan pl, GwModel m) {
    __shared__ double rmin[256], rmax[256];
    const int t = threadIdx.x, C = pl.C, nb = pl.nb1;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (int q = t; q < nb; q += 256) { mn = nan_min(mn, slab[(int64_t)q * (C + 2)]); mx = nan_max(mx, slab[(int64_t)q * (C + 2) + 1]); }
    rmin[t] = mn; rmax[t] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { rmin[t] = nan_min(rmin[t], rmin[t + h]); rmax[t] = nan_max(rmax[t], rmax[t + h]); }
        __syncthreads();
    }
    mn = rmin[0]; mx = rmax[0];
    if (t == 0) { m.minmax[0] = mn; m.minmax[1] = mx; }
    if (t <= GW_MAXG) m.goff[t] = pl.off[t];
    for (int b = t; b < C; b += 256) {
        double sum = 0.0;
        for (int q = 0; q < nb; ++q) sum += slab[(int64_t)q * (C + 2) + 2 + b];     // workgroups in order
        m.mean[b] = (sum / (double)pl.n - mn) / (mx - mn);
    }
}

// a tile of P pixels, normalised and centred, into LDS rows of `ld` doubles; pixels past the scene's end are zero rows
template <typename T>
__device__ __forceinline__ void gw_stage(const T* __restrict__ x, int64_t p0, int P, const GwPlan& pl, int ld, double mn, double rng,
                                         const double* mean, double* tile) {
    const int C = pl.C;
    for (int e = threadIdx.x; e < P * C; e += 256) {
        const int p = e / C, c = e - p * C;
        double v = 0.0;
        if (p0 + p < pl.n) v = ((double)x[(p0 + p) * C + c] - mn) / rng - mean[c];
        tile[p * ld + c] = v;
    }
}

// ---------------------------------------------------------------------------------------------- 2. centred Gram
// D[i][j] += sum over 4 pixels q of A[i][q] B[q][j]; lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], one fp64 each, and
// D[(l >> 4) + 4 r][l & 15] in result register r (NOT the 4 (l >> 4) + r of the other 16 x 16 forms).
template <typename T, int NACC>
__global__ __launch_bounds__(256) void gw_gram_kernel(const T* __restrict__ x, GwPlan pl, GwModel m, double* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) double gsm[];
    __shared__ int pr_row[GW_MAXG * 36], pr_col[GW_MAXG * 36], pr_g[GW_MAXG * 36];
    double* mean = gsm;                                   // [C]
    double* tile = gsm + ((pl.C + 1) & ~1);               // [P2][ld2]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, ld = pl.ld2, P = pl.P2;
    for (int c = t; c < pl.C; c += 256) mean[c] = m.mean[c];
    for (int e = t; e < P * ld; e += 256) tile[e] = 0.0;  // the pad columns stay zero
    if (t < pl.npairs) {
        int i = t, g = 0;
        for (;; ++g) {
            const int Tg = (pl.off[g + 1] - pl.off[g] + 15) / 16, cnt = Tg * (Tg + 1) / 2;
            if (i < cnt) break;
            i -= cnt;
        }
        const int Tg = (pl.off[g + 1] - pl.off[g] + 15) / 16;
        int ti = 0;
        while (i >= Tg - ti) { i -= Tg - ti; ++ti; }      // upper triangle, row by row: (ti, ti + i)
        pr_row[t] = 16 * ti; pr_col[t] = 16 * (ti + i); pr_g[t] = g;
    }
    const double mn = m.minmax[0], rng = m.minmax[1] - mn;
    __syncthreads();
    int prow[NACC], pcol[NACC];
    f64x4 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const int pi = wave + 4 * a;
        const bool ok = pi < pl.npairs;
        prow[a] = ok ? pl.off[pr_g[pi]] + pr_row[pi] : 0;
        pcol[a] = ok ? pl.off[pr_g[pi]] + pr_col[pi] : 0;
        acc[a] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    const int64_t tiles = (pl.n + P - 1) / P;
    for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        __syncthreads();                                  // the previous tile has been consumed
        gw_stage(x, tl * P, P, pl, ld, mn, rng, mean, tile);
        __syncthreads();
        for (int s4 = 0; s4 < P; s4 += 4) {
            const double* rp = tile + (s4 + (lane >> 4)) * ld + (lane & 15);
#pragma unroll
            for (int a = 0; a < NACC; ++a)
                if (wave + 4 * a < pl.npairs)             // wave-uniform
                    acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(rp[prow[a]], rp[pcol[a]], acc[a], 0, 0, 0);
        }
    }
    double* o = slab + (int64_t)blockIdx.x * pl.sq[pl.ngroups];
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const int pi = wave + 4 * a;
        if (pi >= pl.npairs) continue;
        const int g = pr_g[pi], w = pl.off[g + 1] - pl.off[g], j = pr_col[pi] + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = pr_row[pi] + (lane >> 4) + 4 * r;
            if (i < w && j < w) o[pl.sq[g] + i * w + j] = acc[a][r];
        }
    }
}

__global__ __launch_bounds__(256) void gw_gram_sum_kernel(const double* __restrict__ slab, GwPlan pl, double* __restrict__ cov) {
    const int e = blockIdx.x * 256 + threadIdx.x, G2 = pl.sq[pl.ngroups];
    if (e >= G2) return;
    int g = 0;
    while (e >= pl.sq[g + 1]) ++g;
    const int w = pl.off[g + 1] - pl.off[g], q = e - pl.sq[g];
    int i = q / w, j = q - i * w;
    if ((i >> 4) > (j >> 4)) { const int h = i; i = j; j = h; }          // only tiles on or above the diagonal were computed
    const double* src = slab + pl.sq[g] + i * w + j;
    double sum = 0.0;
    for (int b = 0; b < pl.nb2; ++b) sum += src[(int64_t)b * G2];        // workgroups in order
    cov[e] = sum / (double)(pl.n - 1);
}

// ---------------------------------------------------------------------------------------------- 3. eigen-solve
// Two-sided cyclic Jacobi, round-robin ordering: m / 2 disjoint rotations per step, m - 1 steps per sweep (m = w rounded up
// to even; the pad row / column is zero, so its rotations are the identity).  Per step: (a) one thread per pair computes
// (c, s, t) from A[p][p], A[q][q], A[p][q]; (b) every 2 x 2 block A[{p,q}][{p',q'}] with pair <= pair' takes J^T . J' and is
// written with its mirror image (A stays exactly symmetric), and rows p, q of V^T take the rotation.
__global__ __launch_bounds__(GW_EIG_THREADS) void gw_eig_kernel(const double* __restrict__ cov, GwPlan pl, GwModel mo, double* vws) {
    extern __shared__ __attribute__((aligned(16))) double esm[];
    __shared__ double cc[GW_MAXW / 2], ss[GW_MAXW / 2], tt[GW_MAXW / 2], red[2 * GW_EIG_THREADS], lam[GW_MAXW], sgn[GW_MAXW], scl[GW_MAXW];
    __shared__ int ip[GW_MAXW / 2], iq[GW_MAXW / 2], src[GW_MAXW], done;
    const int g = blockIdx.x, t = threadIdx.x, NT = GW_EIG_THREADS;
    const int g0 = pl.off[g], w = pl.off[g + 1] - g0, m = w + (w & 1), h = m / 2, lda = m | 1;
    double* A = esm;                                                    // [m][lda]
    double* V = pl.v_lds ? esm + m * lda : vws + (int64_t)g * GW_MAXW * GW_MAXW;   // V^T: row j = eigenvector j, [m][ldv]
    const int ldv = pl.v_lds ? lda : m;
    for (int e = t; e < m * m; e += NT) {
        const int i = e / m, j = e - i * m;
        A[i * lda + j] = (i < w && j < w) ? cov[pl.sq[g] + i * w + j] : 0.0;
        V[i * ldv + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int sweep = 0; sweep < GW_MAX_SWEEPS; ++sweep) {
        double off2 = 0.0, tr = 0.0;
        for (int e = t; e < w * w; e += NT) {
            const int i = e / w, j = e - i * w;
            const double a = A[i * lda + j];
            if (i == j) tr += a; else off2 += a * a;
        }
        red[t] = off2; red[NT + t] = tr;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (t < s) { red[t] += red[t + s]; red[NT + t] += red[NT + t + s]; }
            __syncthreads();
        }
        if (t == 0) {
            const double thr = 0x1p-52 * red[NT];
            done = red[0] <= thr * thr;                                 // false for NaN: the sweep cap ends the loop then
        }
        __syncthreads();
        if (done) break;
        for (int r = 0; r < m - 1; ++r) {
            if (t < h) {
                int p = t == 0 ? m - 1 : (r + t) % (m - 1), q = (r + m - 1 - t) % (m - 1);
                if (p > q) { const int u = p; p = q; q = u; }
                const double apq = A[p * lda + q], app = A[p * lda + p], aqq = A[q * lda + q];
                double c = 1.0, s = 0.0, tn = 0.0;
                if (apq != 0.0) {
                    const double th = (aqq - app) / (2.0 * apq);
                    tn = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(tn * tn + 1.0);
                    s = tn * c;
                }
                ip[t] = p; iq[t] = q; cc[t] = c; ss[t] = s; tt[t] = tn;
            }
            __syncthreads();
            for (int e = t; e < h * h; e += NT) {
                const int k = e / h, k2 = e - k * h;
                if (k > k2) continue;
                const int p = ip[k], q = iq[k];
                if (k == k2) {
                    const double apq = A[p * lda + q], tn = tt[k];
                    A[p * lda + p] -= tn * apq;
                    A[q * lda + q] += tn * apq;
                    A[p * lda + q] = 0.0;
                    A[q * lda + p] = 0.0;
                    continue;
                }
                const int p2 = ip[k2], q2 = iq[k2];
                const double c = cc[k], s = ss[k], c2 = cc[k2], s2 = ss[k2];
                const double b00 = A[p * lda + p2], b01 = A[p * lda + q2], b10 = A[q * lda + p2], b11 = A[q * lda + q2];
                const double r00 = c * b00 - s * b10, r01 = c * b01 - s * b11, r10 = s * b00 + c * b10, r11 = s * b01 + c * b11;
                const double n00 = c2 * r00 - s2 * r01, n01 = s2 * r00 + c2 * r01, n10 = c2 * r10 - s2 * r11, n11 = s2 * r10 + c2 * r11;
                A[p * lda + p2] = n00; A[p * lda + q2] = n01; A[q * lda + p2] = n10; A[q * lda + q2] = n11;
                A[p2 * lda + p] = n00; A[q2 * lda + p] = n01; A[p2 * lda + q] = n10; A[q2 * lda + q] = n11;
            }
            for (int e = t; e < h * m; e += NT) {
                const int k = e / m, j = e - k * m;
                const int p = ip[k], q = iq[k];
                const double c = cc[k], s = ss[k], vp = V[p * ldv + j], vq = V[q * ldv + j];
                V[p * ldv + j] = c * vp - s * vq;
                V[q * ldv + j] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
    // descending order (ties, and NaN, by index: a total order whatever the values)
    if (t < w) lam[t] = A[t * lda + t];
    __syncthreads();
    if (t < w) {
        const double lt = lam[t];
        int rank = 0;
        for (int i = 0; i < w; ++i) rank += (lam[i] > lt) || (!(lam[i] < lt) && i < t);
        src[rank] = t;
    }
    __syncthreads();
    if (t < w) {
        const int j = src[t];
        double l = lam[j];
        if (l < 0.0) l = 0.0;                                           // a NaN stays a NaN
        mo.lambda[g0 + t] = l;
        int arg = 0;
        double best = fabs(V[j * ldv]);
        for (int i = 1; i < w; ++i) {
            const double a = fabs(V[j * ldv + i]);
            if (a > best) { best = a; arg = i; }
        }
        sgn[t] = V[j * ldv + arg] < 0.0 ? -1.0 : 1.0;
        double sc = sqrt(l);
        if (sc < 0x1p-52) sc = 0x1p-52;                                 // scale[scale < eps] = eps
        scl[t] = pl.whiten ? 1.0 / sc : 1.0;
    }
    __syncthreads();
    const int k = pl.k;
    for (int e = t; e < w * k; e += NT) {
        const int i = e / k, j = e - i * k;
        mo.proj[(int64_t)(g0 + i) * k + j] = sgn[j] * V[src[j] * ldv + i] * scl[j];
    }
}

// ---------------------------------------------------------------------------------------------- 4. projection
template <typename O, int NV> struct GwStore;
template <> struct GwStore<double, 1> { static __device__ __forceinline__ void st(double* o, const double* v) { o[0] = v[0]; } };
template <> struct GwStore<float, 1> { static __device__ __forceinline__ void st(float* o, const double* v) { o[0] = (float)v[0]; } };
template <> struct GwStore<double, 2> {
    static __device__ __forceinline__ void st(double* o, const double* v) { *reinterpret_cast<double2*>(o) = make_double2(v[0], v[1]); }
};
template <> struct GwStore<float, 4> {
    static __device__ __forceinline__ void st(float* o, const double* v) {
        *reinterpret_cast<float4*>(o) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);   // v_cvt_f32_f64: nearest even
    }
};

template <typename T, typename O, int NV>
__global__ __launch_bounds__(256) void gw_project_kernel(const T* __restrict__ x, GwPlan pl, GwModel m, O* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double psm[];
    double* mean = psm;                                   // [C]
    double* tile = psm + ((pl.C + 1) & ~1);               // [P4][ld4]
    double* pl_proj = tile + ((pl.P4 * pl.ld4 + 1) & ~1); // [C][k] when it fits
    const int t = threadIdx.x, ld = pl.ld4, P = pl.P4, k = pl.k, nc = pl.nc, per = nc / NV;
    for (int c = t; c < pl.C; c += 256) mean[c] = m.mean[c];
    const double* proj = m.proj;
    if (pl.proj_lds) {
        for (int e = t; e < pl.C * k; e += 256) pl_proj[e] = m.proj[e];
        proj = pl_proj;
    }
    const double mn = m.minmax[0], rng = m.minmax[1] - mn;
    __syncthreads();
    const int64_t tiles = (pl.n + P - 1) / P;
    for (int64_t tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
        __syncthreads();
        gw_stage(x, tl * P, P, pl, ld, mn, rng, mean, tile);
        __syncthreads();
        for (int e = t; e < P * per; e += 256) {
            const int p = e / per, co = (e - p * per) * NV;
            const int64_t pix = tl * P + p;
            if (pix >= pl.n) break;
            const int g = co / k, j = co - g * k, g0 = pl.off[g], w = pl.off[g + 1] - g0;
            const double* d = tile + p * ld + g0;
            const double* pj = proj + (int64_t)g0 * k + j;
            double acc[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = 0.0;
            for (int i = 0; i < w; ++i) {
                const double di = d[i];
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] = fma(di, pj[i * k + v], acc[v]);
            }
            GwStore<O, NV>::st(out + pix * nc + co, acc);
        }
    }
}

GwModel gw_model(const hsimae_gwpca_params& p) { return GwModel{p.minmax, p.mean, p.lambda, p.proj, p.group_off}; }

int gw_check(const hsimae_gwpca_params& p, GwPlan& pl) {
    const int rc = gw_plan(p, pl);
    if (rc) return rc;
    if (!p.scene || !p.minmax || !p.mean || !p.lambda || !p.proj || !p.group_off) return HS_ENULL;
    if (reinterpret_cast<uintptr_t>(p.scene) & (p.scene_f64 ? 7 : 3)) return HS_EALIGN;
    if ((reinterpret_cast<uintptr_t>(p.minmax) | reinterpret_cast<uintptr_t>(p.mean) | reinterpret_cast<uintptr_t>(p.lambda) |
         reinterpret_cast<uintptr_t>(p.proj)) & 7) return HS_EALIGN;
    if (reinterpret_cast<uintptr_t>(p.group_off) & 3) return HS_EALIGN;
    return HS_OK;
}

// workspace carve, in doubles: slab1 | slab2 | cov | V^T of every group
struct GwCarve { int64_t slab1, slab2, cov, vt, total; };
GwCarve gw_carve(const GwPlan& pl) {
    GwCarve c;
    const int64_t G2 = pl.sq[pl.ngroups];
    c.slab1 = 0;
    c.slab2 = c.slab1 + (int64_t)pl.nb1 * (pl.C + 2);
    c.cov = c.slab2 + (int64_t)pl.nb2 * G2;
    c.vt = c.cov + G2;
    c.total = c.vt + (int64_t)pl.ngroups * GW_MAXW * GW_MAXW;
    return c;
}

template <typename T, int NACC>
void launch_gram(const T* x, const GwPlan& pl, const GwModel& m, double* slab, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((gw_gram_kernel<T, NACC>), dim3(pl.nb2), dim3(256), lds, s, x, pl, m, slab);
}
template <typename T>
void dispatch_gram(const T* x, const GwPlan& pl, const GwModel& m, double* slab, hipStream_t s) {
    const size_t lds = 8 * (size_t)(((pl.C + 1) & ~1) + pl.P2 * pl.ld2);
    switch (pl.nacc) {
        case 1: launch_gram<T, 1>(x, pl, m, slab, lds, s); break;
        case 3: launch_gram<T, 3>(x, pl, m, slab, lds, s); break;
        case 5: launch_gram<T, 5>(x, pl, m, slab, lds, s); break;
        case 10: launch_gram<T, 10>(x, pl, m, slab, lds, s); break;
        case 18: launch_gram<T, 18>(x, pl, m, slab, lds, s); break;
        default: launch_gram<T, 36>(x, pl, m, slab, lds, s); break;
    }
}

template <typename T, typename O, int NV>
void launch_project(const T* x, const GwPlan& pl, const GwModel& m, O* out, hipStream_t s) {
    const size_t lds = 8 * (size_t)(((pl.C + 1) & ~1) + ((pl.P4 * pl.ld4 + 1) & ~1) + (pl.proj_lds ? pl.C * pl.k : 0));
    hipLaunchKernelGGL((gw_project_kernel<T, O, NV>), dim3(pl.nb4), dim3(256), lds, s, x, pl, m, out);
}
template <typename T>
void dispatch_project(const T* x, const GwPlan& pl, const GwModel& m, void* out, int out_f64, hipStream_t s) {
    if (out_f64) {
        if (pl.k % 2 == 0) launch_project<T, double, 2>(x, pl, m, static_cast<double*>(out), s);
        else launch_project<T, double, 1>(x, pl, m, static_cast<double*>(out), s);
    } else {
        if (pl.k % 4 == 0) launch_project<T, float, 4>(x, pl, m, static_cast<float*>(out), s);
        else launch_project<T, float, 1>(x, pl, m, static_cast<float*>(out), s);
    }
}

}  // namespace

int64_t hs_gwpca_workspace_bytes(const hsimae_gwpca_params& p) {
    GwPlan pl;
    const int rc = gw_plan(p, pl);
    if (rc) return rc;
    return 8 * gw_carve(pl).total;
}

int hs_gwpca_fit(const hsimae_gwpca_params& p, void* workspace, hipStream_t s) {
    GwPlan pl;
    const int rc = gw_check(p, pl);
    if (rc) return rc;
    if (!workspace) return HS_ENULL;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return HS_EALIGN;
    const GwCarve cv = gw_carve(pl);
    double* ws = static_cast<double*>(workspace);
    const GwModel m = gw_model(p);
    if (p.scene_f64) hipLaunchKernelGGL(gw_range_sums_kernel<double>, dim3(pl.nb1), dim3(256), 0, s, static_cast<const double*>(p.scene), pl, ws + cv.slab1);
    else hipLaunchKernelGGL(gw_range_sums_kernel<float>, dim3(pl.nb1), dim3(256), 0, s, static_cast<const float*>(p.scene), pl, ws + cv.slab1);
    hipLaunchKernelGGL(gw_model_head_kernel, dim3(1), dim3(256), 0, s, ws + cv.slab1, pl, m);
    if (p.scene_f64) dispatch_gram(static_cast<const double*>(p.scene), pl, m, ws + cv.slab2, s);
    else dispatch_gram(static_cast<const float*>(p.scene), pl, m, ws + cv.slab2, s);
    hipLaunchKernelGGL(gw_gram_sum_kernel, dim3((pl.sq[pl.ngroups] + 255) / 256), dim3(256), 0, s, ws + cv.slab2, pl, ws + cv.cov);
    const int mm = pl.wmax + (pl.wmax & 1);
    const size_t lds = 8 * (size_t)(mm * (mm | 1)) * (pl.v_lds ? 2 : 1);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gw_eig_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(gw_eig_kernel, dim3(pl.ngroups), dim3(GW_EIG_THREADS), lds, s, ws + cv.cov, pl, m, ws + cv.vt);
    return (int)hipGetLastError();
}

int hs_gwpca_apply(const hsimae_gwpca_params& p, void* out, int out_f64, hipStream_t s) {
    GwPlan pl;
    const int rc = gw_check(p, pl);
    if (rc) return rc;
    if (!out) return HS_ENULL;
    if (reinterpret_cast<uintptr_t>(out) & 15) return HS_EALIGN;
    const GwModel m = gw_model(p);
    if (p.scene_f64) dispatch_project(static_cast<const double*>(p.scene), pl, m, out, out_f64, s);
    else dispatch_project(static_cast<const float*>(p.scene), pl, m, out, out_f64, s);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(gwpca)
