// Linear probe on frozen features on the device (hsimae_probe_prepare, hsimae_probe_step, hsimae_probe_logits, hsimae_probe_fold;
// include/hsimae_hip.h): multinomial logistic regression over the classes [first, C) on per-column standardised fp32 rows, the bias
// as column D of the operand (feature 1), full-batch AdamW with decoupled decay (none on the bias column).  Kp = D + 4; w, m, v are
// fp32 [64][Kp]; rows outside [first, C) and columns behind D are never written.
//
//   probe_stats_kernel        one thread per column d: over the valid rows (label in [first, C)) in ascending order, fp64 from 0:
//                             sum += x_id; mu = sum / nv; ss = fma(x_id - mu, x_id - mu, ss); mean = fp32(mu), rstd = fp32(1 /
//                             sqrt(ss / nv + eps)).  One more workgroup (one wave) counts the invalid labels: lane l takes the rows
//                             l, l + 64, .., then the xor tree; it writes the state block {0, 0, 0, bad, nv, 0, 0, 0}.
//   probe_standardize_kernel  one thread per (row i < roundup(n, 4), column k < Kp): fl(fl(x - mean) * rstd), 1 at k = D, 0 behind D,
//                             0 for an invalid row and for i >= n; written to xs[i][k] (i < n) and xt[k][i].
//   probe_forward_kernel      a workgroup (4 waves) owns 64 rows: the exact-fp32 dot tile of dot_tile.h against the 64 rows of w, the
//                             k-ordered fmaf chain from +0 over 0 .. Kp - 1; the block is handed over through LDS.  TRAIN: wave v
//                             takes the rows 16 v .. 16 v + 15 in order: row_softmax_stats / row_exp over [first, C), p = e * (1 /
//                             sum), g = (p - [c = y]) * fp32(1 / nv) back into the block (0 outside [first, C), for an invalid row and
//                             past n); the row's loss log(sum) - (z_y - m) in fp64 is added in row order, the waves' sums in wave
//                             order: loss_part[workgroup].  The block leaves transposed: gt[c][i].  Otherwise (hsimae_probe_logits)
//                             the rows of x are standardised while they are staged and the block leaves as z[i][c], 0 for c < first.
//   probe_grad_kernel         workgroup (64 columns k of Kp, segment s of HSIMAE_PROBE_SEG rows): the same tile with A = rows of gt,
//                             B = rows of xt, the chain running over the segment's rows i ascending from +0 -> scratch[s][c][k].
//   probe_update_kernel       one thread per (c, k): dW = scratch[0] + scratch[1] + .. in ascending s; adamw_one (optim.h) with weight
//                             decay 0 at k = D; block_sum (optim.h) of dW^2 in fp64 -> norm_part[workgroup].
//   probe_finish_kernel       one wave: lane l adds the partials l, l + 64, .. in order, the xor tree adds the lanes (loss, then
//                             dW^2): state = {loss / nv, step, ||dW||^2, bad, nv, 0, 0, 0}, loss_hist[step - 1].
//   probe_fold_kernel         one wave per class c: weight[c][d] = fl(w[c][d] * rstd[d]); lane 0 forms bias[c] = fp32(w[c][D] - sum_d
//                             w[c][d] mean[d] rstd[d]) in fp64 over ascending d from 0; rows below `first` are 0.
//
// Refusals (hs_probe_*, before any launch, so a refusal writes nothing): HS_EDIMS for n < 0, D <= 0, D % 4, C < 2, first outside
// [0, C), Kp != D + 4, a leading dimension below its width, eps / step / the optimizer's numbers out of range; HS_EUNSUPPORTED for
// C > 64, D > 4096, n > 2^20; HS_ENULL for a required pointer NULL with n > 0; HS_EALIGN for a matrix off 16 bytes or with a leading
// dimension that is no multiple of 4, another pointer off its element.  n = 0 -> HS_OK, no launch.
//
// No atomics anywhere, no barrier across workgroups, no flag: launches are ordered by the stream, every sum has one fixed order
// that does not depend on the grid (the segment length is a constant): two runs are bit-identical.
#include "common.h"
#include "dot_tile.h"
#include "kernels.h"
#include "optim.h"
#include "row_wave.h"

namespace {

constexpr int PB_ROWS = HSIMAE_PROBE_ROWS;
constexpr int PB_SEG = HSIMAE_PROBE_SEG;
constexpr int PB_MAXN = 1 << 20;
constexpr int PB_BATCH = 16;                  // rows in flight per column of probe_stats_kernel
static_assert(PB_ROWS == TB && PB_SEG % KS == 0, "one column of dot tiles; a segment is whole K-slabs");

__device__ __forceinline__ bool label_ok(int64_t y, int first, int C) { return y >= first && y < C; }

// the operand of one feature: two fp32 roundings
__device__ __forceinline__ float standardized(float x, float mean, float rstd) { return (x - mean) * rstd; }

__global__ __launch_bounds__(64) void probe_stats_kernel(hsimae_probe_prepare_params p) {
    const int lane = threadIdx.x, n = p.n;
    if (blockIdx.x + 1 == gridDim.x) {                                         // the census and the state block
        long long bad = 0;
        for (int i = lane; i < n; i += 64) bad += !label_ok(p.labels[i], p.first, p.C);
        bad = tree_sum(bad);
        if (lane < HSIMAE_PROBE_STATE) p.state[lane] = lane == 3 ? (double)bad : lane == 4 ? (double)(n - bad) : 0.0;
        return;
    }
    const int d = blockIdx.x * 64 + lane;
    const bool live = d < p.D;
    const float* xc = p.x + (live ? d : 0);                                    // (a lane past D reads column 0 and drops it)
    double sum = 0.0, ss = 0.0;
    long long nv = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const double mu = pass && nv ? sum / (double)nv : 0.0;
        for (int i0 = 0; i0 < n; i0 += PB_BATCH) {                             // ascending rows, PB_BATCH loads in flight
            float v[PB_BATCH];
            bool ok[PB_BATCH];
#pragma unroll
            for (int u = 0; u < PB_BATCH; ++u) {
                const int i = i0 + u < n ? i0 + u : n - 1;
                v[u] = xc[(int64_t)i * p.ldx];
                ok[u] = i0 + u < n && label_ok(p.labels[i], p.first, p.C);
            }
#pragma unroll
            for (int u = 0; u < PB_BATCH; ++u)
                if (ok[u]) {
                    if (pass) { const double c = (double)v[u] - mu; ss = fma(c, c, ss); }
                    else { sum += (double)v[u]; ++nv; }
                }
        }
    }
    if (live) {
        p.mean[d] = nv ? (float)(sum / (double)nv) : 0.f;
        p.rstd[d] = nv ? (float)(1.0 / sqrt(ss / (double)nv + (double)p.eps)) : 0.f;
    }
}

__global__ __launch_bounds__(256) void probe_standardize_kernel(hsimae_probe_prepare_params p) {
    const int Kp = p.Kp, n4 = (p.n + 3) & ~3;
    const int64_t total = (int64_t)n4 * Kp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / Kp), k = (int)(e % Kp);
        float v = 0.f;
        if (i < p.n && label_ok(p.labels[i], p.first, p.C)) {
            if (k < p.D) v = standardized(p.x[(int64_t)i * p.ldx + k], p.mean[k], p.rstd[k]);
            else if (k == p.D) v = 1.f;
        }
        if (i < p.n) p.xs[(int64_t)i * Kp + k] = v;
        p.xt[(int64_t)k * p.ldn + i] = v;
    }
}

// what the forward tile needs, from either entry point
struct ForwardArgs {
    const float* a; int lda, DA;                 // the rows: xs (DA = Kp) or raw x (DA = D)
    const float *mean, *rstd;                    // raw rows only
    const float* w; int Kp, n, D, C, first;
    const int64_t* labels; const double* state; float* gt; int ldn; double* loss_part;       // TRAIN
    float* z; int ldz;                                                                       // logits
};

// raw feature rows into the operand while they are staged: column k of this thread's pieces is k0 + 4 c4 + j
struct Standardize {
    const float *mean, *rstd; int D;
    __device__ __forceinline__ void operator()(SlabRegs& s, int k0) const {
        const int k = k0 + 4 * (threadIdx.x & 7);
        if (k < D) {
            const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + k), rs = *reinterpret_cast<const f32x4*>(rstd + k);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < 4; ++j) s.v[h][j] = standardized(s.v[h][j], mu[j], rs[j]);
        } else if (k == D) {
            s.v[0][0] = 1.f; s.v[1][0] = 1.f;                                  // (the fetch left zeros behind D)
        }
    }
};

template <bool TRAIN>
__global__ __launch_bounds__(256) void probe_forward_kernel(ForwardArgs p) {
    __shared__ float slabs[2][TQ][SLD];          // the two operands' slabs; after the last slab the block P lies over them
    float (*Xs)[SLD] = slabs[0], (*Ws)[SLD] = slabs[1];
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(&slabs[0][0][0]);       // [row][class]
    __shared__ double Lw[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * TQ;
    SlabRegs rx = fetch_slab(p.a, i0, p.n, p.lda, 0, p.DA), rw = fetch_slab(p.w, 0, PB_ROWS, p.Kp, 0, p.Kp);
    f32x16 acc;
    if (TRAIN) {
        acc = dot_tile(Xs, Ws, rx, rw, p.a, i0, p.n, p.lda, p.w, 0, PB_ROWS, p.Kp, p.Kp);
    } else {
        const Standardize stage{p.mean, p.rstd, p.D};
        stage(rx, 0);
        acc = dot_tile_staged(Xs, Ws, rx, rw, p.a, i0, p.n, p.lda, p.DA, p.w, 0, PB_ROWS, p.Kp, p.Kp, stage);
    }
    hand_over(P, acc);
    if (!TRAIN) {
        for (int e = threadIdx.x; e < TQ * PB_ROWS; e += 256) {
            const int r = e >> 6, c = e & 63;
            if (i0 + r < p.n && c < p.C) p.z[(i0 + r) * p.ldz + c] = c < p.first ? 0.f : P[r][c];
        }
        return;
    }
    const double nv = p.state[4];
    const float inv_n = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
    const bool live = lane >= p.first && lane < p.C;                           // lane = the class of this lane's column
    double loss = 0.0;
    for (int r = wave * 16; r < wave * 16 + 16; ++r) {                         // wave-uniform
        const int64_t i = i0 + r;
        const int64_t y = i < p.n ? p.labels[i] : -1;
        float g = 0.f;
        if (label_ok(y, p.first, p.C)) {
            float m, sum;
            row_softmax_stats(P[r], p.first, p.C, lane, m, sum);
            const float inv = 1.f / sum;
            if (live) g = (row_exp(P[r][lane], m) * inv - (lane == (int)y ? 1.f : 0.f)) * inv_n;
            loss += log((double)sum) - ((double)P[r][(int)y] - (double)m);
        }
        P[r][lane] = g;                                                        // (the wave has read the row: LDS keeps program order)
    }
    if (lane == 0) Lw[wave] = loss;
    __syncthreads();
    if (threadIdx.x == 0) p.loss_part[blockIdx.x] = ((Lw[0] + Lw[1]) + Lw[2]) + Lw[3];
    const int n4 = (p.n + 3) & ~3;
    for (int e = threadIdx.x; e < TQ * PB_ROWS; e += 256) {                    // transposed: a wave writes 64 consecutive rows i
        const int c = e >> 6, r = e & 63;
        if (i0 + r < n4) p.gt[(int64_t)c * p.ldn + i0 + r] = P[r][c];
    }
}

__global__ __launch_bounds__(256) void probe_grad_kernel(hsimae_probe_step_params p) {
    __shared__ float slabs[2][TQ][SLD];
    float (*Gs)[SLD] = slabs[0], (*Xs)[SLD] = slabs[1];
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(&slabs[0][0][0]);       // [class][column]
    const int k0 = blockIdx.x * TB, s = blockIdx.y, n4 = (p.n + 3) & ~3;
    const int len = min(PB_SEG, n4 - s * PB_SEG);                              // a multiple of 4
    const float *G = p.gt + (int64_t)s * PB_SEG, *X = p.xt + (int64_t)s * PB_SEG;
    SlabRegs rg = fetch_slab(G, 0, PB_ROWS, p.ldn, 0, len), rx = fetch_slab(X, k0, p.Kp, p.ldn, 0, len);
    const f32x16 acc = dot_tile(Gs, Xs, rg, rx, G, 0, PB_ROWS, p.ldn, X, k0, p.Kp, p.ldn, len);
    hand_over(P, acc);
    float* out = p.scratch + (int64_t)s * PB_ROWS * p.Kp;
    for (int e = threadIdx.x; e < PB_ROWS * TB; e += 256) {
        const int c = e >> 6, k = k0 + (e & 63);
        if (k < p.Kp) out[(int64_t)c * p.Kp + k] = P[c][e & 63];
    }
}

__global__ __launch_bounds__(256) void probe_update_kernel(hsimae_probe_step_params p, float inv_bc1, float inv_sqrt_bc2) {
    const int e = blockIdx.x * 256 + threadIdx.x, c = e / p.Kp, k = e % p.Kp;
    const int S = (p.n + PB_SEG - 1) / PB_SEG;
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    if (c >= p.first && c < p.C && k <= p.D) {
        const int64_t stride = (int64_t)PB_ROWS * p.Kp;
        const float* part = p.scratch + e;
        float dw = part[0];
        for (int s = 1; s < S; ++s) dw += part[s * stride];
        adamw_one(p.w[e], dw, p.m[e], p.v[e], p.lr, k == p.D ? 0.f : p.weight_decay, p.b1, p.b2, p.eps, inv_bc1, inv_sqrt_bc2, 1.f);
        sq[0] = sq64(dw);
    }
    block_sum(p.norm_part + blockIdx.x, sq);
}

__global__ __launch_bounds__(64) void probe_finish_kernel(hsimae_probe_step_params p) {
    const int lane = threadIdx.x, tiles = (p.n + TQ - 1) / TQ, groups = (PB_ROWS * p.Kp + 255) / 256;
    double loss = 0.0, sq = 0.0;
    for (int g = lane; g < tiles; g += 64) loss += p.loss_part[g];
    for (int g = lane; g < groups; g += 64) sq += p.norm_part[g];
    loss = tree_sum(loss);
    sq = tree_sum(sq);
    if (lane == 0) {
        const double nv = p.state[4];
        const double mean = nv > 0.0 ? loss / nv : 0.0;
        p.state[0] = mean;
        p.state[1] = (double)p.step;
        p.state[2] = sq;
        p.state[5] = p.state[6] = p.state[7] = 0.0;
        if (p.loss_hist) p.loss_hist[p.step - 1] = (float)mean;
    }
}

__global__ __launch_bounds__(64) void probe_fold_kernel(hsimae_probe_fold_params p) {
    const int lane = threadIdx.x, c = blockIdx.x, D = p.D;
    const bool real = c >= p.first;
    const float* w = p.w + (int64_t)c * p.Kp;
    for (int d = lane; d < D; d += 64) p.weight[(int64_t)c * p.ldw + d] = real ? w[d] * p.rstd[d] : 0.f;
    if (lane == 0) {
        double acc = 0.0;
        if (real)
            for (int d = 0; d < D; ++d) acc += (double)w[d] * (double)p.mean[d] * (double)p.rstd[d];
        p.bias[c] = real ? (float)((double)w[D] - acc) : 0.f;
    }
}

// the checks every entry point shares: the problem's size, then the limits
int shape_refusal(int n, int D, int C, int first, int Kp) {
    if (n < 0 || D <= 0 || D % 4 || C < 2 || first < 0 || first >= C || Kp != D + 4) return HS_EDIMS;
    if (C > PB_ROWS || D > 4096 || n > PB_MAXN) return HS_EUNSUPPORTED;
    return HS_OK;
}
inline bool in01(float b) { return b >= 0.f && b < 1.f; }

}  // namespace

int hs_probe_prepare(const hsimae_probe_prepare_params& p, hipStream_t s) {
    if (const int rc = shape_refusal(p.n, p.D, p.C, p.first, p.Kp)) return rc;
    if (p.ldx < p.D || p.ldn < ((p.n + 3) & ~3) || !(p.eps > 0.f) || std::isinf(p.eps)) return HS_EDIMS;
    if (p.n > 0 && (!p.x || !p.labels || !p.mean || !p.rstd || !p.xs || !p.xt || !p.state)) return HS_ENULL;
    if (misaligned(p.x, 15) || misaligned(p.xs, 15) || misaligned(p.xt, 15) || p.ldx % 4 || p.ldn % 4 || misaligned(p.labels, 7) ||
        misaligned(p.mean, 15) || misaligned(p.rstd, 15) || misaligned(p.state, 7)) return HS_EALIGN;
    if (p.n == 0) return HS_OK;
    hipLaunchKernelGGL(probe_stats_kernel, dim3((unsigned)((p.D + 63) / 64 + 1)), dim3(64), 0, s, p);
    const int64_t total = (int64_t)((p.n + 3) & ~3) * p.Kp;
    hipLaunchKernelGGL(probe_standardize_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_probe_step(const hsimae_probe_step_params& p, hipStream_t s) {
    if (const int rc = shape_refusal(p.n, p.D, p.C, p.first, p.Kp)) return rc;
    if (p.ldn < ((p.n + 3) & ~3) || p.step < 1 || !(p.lr >= 0.f) || !(p.weight_decay >= 0.f) || !(p.eps >= 0.f) || !in01(p.b1) ||
        !in01(p.b2)) return HS_EDIMS;
    if (p.n > 0 && (!p.xs || !p.xt || !p.labels || !p.w || !p.m || !p.v || !p.gt || !p.scratch || !p.loss_part || !p.norm_part ||
                    !p.state)) return HS_ENULL;
    if (misaligned(p.xs, 15) || misaligned(p.xt, 15) || misaligned(p.w, 15) || misaligned(p.gt, 15) || p.ldn % 4 ||
        misaligned(p.labels, 7) || misaligned(p.m, 3) || misaligned(p.v, 3) || misaligned(p.scratch, 3) || misaligned(p.loss_part, 7) ||
        misaligned(p.norm_part, 7) || misaligned(p.state, 7) || misaligned(p.loss_hist, 3)) return HS_EALIGN;
    if (p.n == 0) return HS_OK;
    float inv_bc1, inv_sqrt_bc2;
    bias_corrections(p.b1, p.b2, p.step, inv_bc1, inv_sqrt_bc2);
    ForwardArgs f{};
    f.a = p.xs; f.lda = p.Kp; f.DA = p.Kp; f.w = p.w; f.Kp = p.Kp; f.n = p.n; f.D = p.D; f.C = p.C; f.first = p.first;
    f.labels = p.labels; f.state = p.state; f.gt = p.gt; f.ldn = p.ldn; f.loss_part = p.loss_part;
    const unsigned tiles = (unsigned)((p.n + TQ - 1) / TQ), segs = (unsigned)((p.n + PB_SEG - 1) / PB_SEG);
    hipLaunchKernelGGL(probe_forward_kernel<true>, dim3(tiles), dim3(256), 0, s, f);
    hipLaunchKernelGGL(probe_grad_kernel, dim3((unsigned)((p.Kp + TB - 1) / TB), segs), dim3(256), 0, s, p);
    hipLaunchKernelGGL(probe_update_kernel, dim3((unsigned)((PB_ROWS * p.Kp + 255) / 256)), dim3(256), 0, s, p, inv_bc1, inv_sqrt_bc2);
    hipLaunchKernelGGL(probe_finish_kernel, dim3(1), dim3(64), 0, s, p);
    return (int)hipGetLastError();
}

int hs_probe_logits(const hsimae_probe_logits_params& p, hipStream_t s) {
    if (const int rc = shape_refusal(p.n, p.D, p.C, p.first, p.Kp)) return rc;
    if (p.ldx < p.D || p.ldz < p.C) return HS_EDIMS;
    if (p.n > 0 && (!p.x || !p.mean || !p.rstd || !p.w || !p.z)) return HS_ENULL;
    if (misaligned(p.x, 15) || misaligned(p.w, 15) || misaligned(p.mean, 15) || misaligned(p.rstd, 15) || p.ldx % 4 ||
        misaligned(p.z, 3)) return HS_EALIGN;
    if (p.n == 0) return HS_OK;
    ForwardArgs f{};
    f.a = p.x; f.lda = p.ldx; f.DA = p.D; f.mean = p.mean; f.rstd = p.rstd; f.w = p.w; f.Kp = p.Kp; f.n = p.n; f.D = p.D; f.C = p.C;
    f.first = p.first; f.z = p.z; f.ldz = p.ldz;
    hipLaunchKernelGGL(probe_forward_kernel<false>, dim3((unsigned)((p.n + TQ - 1) / TQ)), dim3(256), 0, s, f);
    return (int)hipGetLastError();
}

int hs_probe_fold(const hsimae_probe_fold_params& p, hipStream_t s) {
    if (const int rc = shape_refusal(0, p.D, p.C, p.first, p.Kp)) return rc;
    if (p.ldw < p.D) return HS_EDIMS;
    if (!p.w || !p.mean || !p.rstd || !p.weight || !p.bias) return HS_ENULL;
    if (misaligned(p.w, 3) || misaligned(p.mean, 3) || misaligned(p.rstd, 3) || misaligned(p.weight, 3) || misaligned(p.bias, 3))
        return HS_EALIGN;
    hipLaunchKernelGGL(probe_fold_kernel, dim3((unsigned)p.C), dim3(64), 0, s, p);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(probe)
