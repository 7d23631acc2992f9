// RBF support-vector classifier on the device (hsimae_svm_gram, hsimae_svm_solve, hsimae_svm_pack, hsimae_svm_predict;
// include/hsimae_hip.h states every sequence): the baseline hyperspectral papers report next to their deep models, sklearn's
// SVC(kernel='rbf') / libsvm's C-SVC, one-vs-one.
//
//   svm_sumsq_kernel    one workgroup per 64 rows: the dot tile of the rows with themselves, its diagonal is n_t = dot_tt.
//   svm_gram_kernel     one workgroup per 64 x 64 tile on or above the diagonal: the dot tile, d2 = fmaf(-2, dot, n_t + n_s) clamped
//                       at 0, K = exp2(-(gamma log2 e) d2) for every gamma, written at (t, s) and (s, t); the diagonal is the constant 1.
//   svm_solve_kernel    one workgroup per problem of the table: SMO with second-order working-set selection, alpha and G fp64 in
//                       LDS, four barriers per iteration, two kernel rows read per iteration.  Every fp64 operation is one IEEE
//                       operation (contraction is off for this file), every argmax goes by argd_better.
//   svm_pack_kernel     one workgroup per class: its support rows in ascending order behind those of the classes before it (which
//                       it counts itself: no workgroup waits for another), coefficients, rows and norms gathered.
//   svm_predict_kernel  a workgroup owns 64 query rows and walks the support rows in tiles of 64: dot tile -> kernel values in
//                       LDS -> per (row, pair) one fmaf chain in ascending support order; then votes, shares, maps.
//
// No atomics anywhere; every output element has one owner and one order: two runs are bit-identical.
#include "common.h"
#include "dot_tile.h"
#include "kernels.h"
#include "row_wave.h"

#pragma clang fp contract(off)

namespace {

constexpr int SVM_LDS_MAX = 160 * 1024;      // what a gfx950 workgroup may hold
constexpr int SVM_SCRATCH = 128;             // bytes of reduction scratch of the solver
constexpr double SVM_TAU = 1e-12;
static_assert(16 * HSIMAE_SVM_MAX_ROWS + SVM_SCRATCH <= SVM_LDS_MAX, "alpha and G of the largest problem fit the LDS");
constexpr int SVM_SLAB_FLOATS = 2 * TQ * SLD;
constexpr int SVM_CS = 36;                   // HSIMAE_SVM_MAX_CLASSES + 1 class starts, padded
static_assert(4 * (SVM_SLAB_FLOATS + TQ + SVM_CS + 64 * (HSIMAE_SVM_MAX_CLASSES * (HSIMAE_SVM_MAX_CLASSES - 1) / 2)) <= SVM_LDS_MAX,
              "slabs, query norms and the decision sums of the most classes fit the LDS");
static_assert(HSIMAE_SVM_MAX_CLASSES * 64 <= SVM_SLAB_FLOATS, "the votes fit over the slabs");

// launch with dynamic LDS of any size up to the workgroup's limit.  The opt-in belongs to the (kernel, device) pair and costs a
// host call only: it is made before every launch, and its error is the call's.
template <auto Kernel, class Args>
int svm_launch(dim3 grid, size_t lds, hipStream_t s, const Args& a) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SVM_LDS_MAX);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
    hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, s, a);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------ Gram
// K from a dot product and the two squared norms, for g2 = fl(gamma log2 e)
__device__ __forceinline__ float svm_d2(float dot, float nt, float ns) {
    const float d2 = fmaf(-2.f, dot, nt + ns);
    return d2 < 0.f ? 0.f : d2;                                       // a NaN stays
}
__device__ __forceinline__ float svm_kernel_value(float d2, float g2) { return __builtin_amdgcn_exp2f((-g2) * d2); }

__global__ __launch_bounds__(256) void svm_sumsq_kernel(hsimae_svm_gram_params p) {
    __shared__ float slabs[2][TQ][SLD];
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(&slabs[0][0][0]);
    const int64_t a0 = (int64_t)blockIdx.x * TQ;
    const int64_t hi = a0 + TQ < p.M ? a0 + TQ : p.M;                 // the tile alone: nothing is prefetched behind it
    SlabRegs ra = fetch_slab(p.x, a0, hi, p.ldx, 0, p.D), rb = ra;
    const f32x16 acc = dot_tile(slabs[0], slabs[1], ra, rb, p.x, a0, hi, p.ldx, p.x, a0, hi, p.ldx, p.D);
    hand_over(P, acc);
    const int t = threadIdx.x;
    if (t < TQ && a0 + t < p.M) p.sumsq[a0 + t] = P[t][t];
}

__global__ __launch_bounds__(256) void svm_gram_kernel(hsimae_svm_gram_params p) {
    if (blockIdx.x < blockIdx.y) return;                              // below the diagonal: the tile above writes it
    __shared__ float slabs[2][TQ][SLD];
    __shared__ float nA[TQ], nB[TQ];
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(&slabs[0][0][0]);
    const int64_t M = p.M, a0 = (int64_t)blockIdx.y * TQ, b0 = (int64_t)blockIdx.x * TQ;
    const int64_t ahi = a0 + TQ < M ? a0 + TQ : M, bhi = b0 + TQ < M ? b0 + TQ : M;
    const int tid = threadIdx.x;
    if (tid < TQ) nA[tid] = a0 + tid < M ? p.sumsq[a0 + tid] : 0.f;
    else if (tid < 2 * TQ) nB[tid - TQ] = b0 + tid - TQ < M ? p.sumsq[b0 + tid - TQ] : 0.f;
    SlabRegs ra = fetch_slab(p.x, a0, ahi, p.ldx, 0, p.D), rb = fetch_slab(p.x, b0, bhi, p.ldx, 0, p.D);
    const f32x16 acc = dot_tile(slabs[0], slabs[1], ra, rb, p.x, a0, ahi, p.ldx, p.x, b0, bhi, p.ldx, p.D);
    hand_over(P, acc);
    const bool diag = a0 == b0;
    for (int g = 0; g < p.n_gamma; ++g) {
        const float g2 = p.gamma[g] * HS_LOG2E;
        float* Kg = p.K + (int64_t)g * M * p.ldk;
        for (int e = tid; e < TQ * TB; e += 256) {                   // (t, s): rows of the tile along s
            const int r = e >> 6, c = e & 63;
            if (a0 + r >= M || b0 + c >= M) continue;
            const int lo = diag && c < r ? c : r, hi = diag && c < r ? r : c;      // a diagonal tile reads its upper half only
            const float v = diag && r == c ? 1.f : svm_kernel_value(svm_d2(P[lo][hi], nA[lo], nB[hi]), g2);
            Kg[(a0 + r) * p.ldk + b0 + c] = v;
        }
        if (diag) continue;
        for (int e = tid; e < TQ * TB; e += 256) {                   // (s, t): the same values, rows along t
            const int c = e >> 6, r = e & 63;
            if (a0 + r >= M || b0 + c >= M) continue;
            Kg[(b0 + c) * p.ldk + a0 + r] = svm_kernel_value(svm_d2(P[r][c], nA[r], nB[c]), g2);
        }
    }
}

// ------------------------------------------------------------------ solver
// (value, index) of the better of two argmax candidates: index < 0 is "none"; a larger value wins, of equals the lower index,
// a NaN never wins.  (common.h's arg_better is this rule for fp32 with the NaN clause the other way round: there a NaN wins.)
__device__ __forceinline__ void argd_better(double& v, int& i, double v2, int i2) {
    const bool take = i2 >= 0 && !__builtin_isnan(v2) && (i < 0 || v2 > v || (v2 == v && i2 < i));
    if (take) { v = v2; i = i2; }
}
struct TreeArgD { static __device__ __forceinline__ void f(double& v, int& i, double v2, int i2) { argd_better(v, i, v2, i2); } };
struct TreeMaxD { static __device__ __forceinline__ void f(double& a, double b) { if (b > a) a = b; } };     // a NaN never enters
// the threads' candidates into the workgroup's: the xor tree over the lanes, then the four waves in ascending order
__device__ __forceinline__ void block_argmax(double& v, int& i, double* sv, int* si) {
    wave_tree<TreeArgD>(v, i);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sv[wave] = v; si[wave] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int w = 1; w < 4; ++w) argd_better(v, i, sv[w], si[w]);
}

__global__ __launch_bounds__(256) void svm_solve_kernel(hsimae_svm_solve_params p) {
    extern __shared__ double svm_lds[];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const hsimae_svm_problem T = p.table[r];
    double* st = p.state + r * HSIMAE_SVM_STATE;
    const int64_t M = p.M;
    const bool refused = T.k_index < 0 || T.k_index >= p.n_k || T.a0 < 0 || T.na < 0 || T.b0 < 0 || T.nb < 0 || T.na > M || T.nb > M ||
                         T.a0 > M - T.na || T.b0 > M - T.nb || T.na + T.nb > M || T.out_offset < 0 ||
                         T.out_offset > p.alpha_len - (T.na + T.nb) || !(T.C > 0.0) || T.C > 1.7e308;
    if (refused) {
        if (tid < HSIMAE_SVM_STATE) st[tid] = tid == 1 ? -1.0 : 0.0;
        return;
    }
    const int na = (int)T.na, n = (int)(T.na + T.nb), ncap = p.M;
    const double Cc = T.C, eps = p.eps;
    double* alpha = svm_lds;
    double* G = svm_lds + ncap;
    double* sv1 = G + ncap;                       // [4] pass 1: values
    double* sm2 = sv1 + 4;                        // [4] pass 1: the maximum over I_low
    double* sv2 = sm2 + 4;                        // [4] pass 2: values
    int* si1 = reinterpret_cast<int*>(sv2 + 4);   // [4]
    int* si2 = si1 + 4;                           // [4]
    double* ga = p.alpha + T.out_offset;
    double* gg = p.grad + T.out_offset;
    const double before = p.resume ? st[0] : 0.0;
    if (T.na == 0 || T.nb == 0) {
        for (int t = tid; t < n; t += 256) { ga[t] = 0.0; gg[t] = -1.0; }
        if (tid < HSIMAE_SVM_STATE) st[tid] = tid == 1 ? -2.0 : 0.0;
        return;
    }
    for (int t = tid; t < n; t += 256) {
        alpha[t] = p.resume ? ga[t] : 0.0;
        G[t] = p.resume ? gg[t] : -1.0;
    }
    __syncthreads();
    const float* Kb = p.K + T.k_index * M * p.ldk;
    const int64_t a0 = T.a0, bshift = T.b0 - T.na;                    // bank row of local t: a0 + t, or b0 + (t - na)
    const double inf = __builtin_inf();
    int it = 0, conv = 0;
    double gap = 0.0;
    for (;;) {
        // 1. i and the stopping gap
        double gmax = 0.0, m2 = -inf;
        int i = -1;
        for (int t = tid; t < n; t += 256) {
            const bool pos = t < na;
            const double a = alpha[t], yg = pos ? G[t] : -G[t];
            const bool ub = a >= Cc, lb = a <= 0.0;
            if (pos ? !ub : !lb) argd_better(gmax, i, -yg, t);
            if ((pos ? !lb : !ub) && yg > m2) m2 = yg;
        }
        wave_tree<TreeMaxD>(m2);
        if ((tid & 63) == 0) sm2[tid >> 6] = m2;
        block_argmax(gmax, i, sv1, si1);
        m2 = sm2[0];
        for (int w = 1; w < 4; ++w) if (sm2[w] > m2) m2 = sm2[w];
        m2 = m2 + 0.0;                                                // a maximum of -0 and +0 is +0 whichever lane held it
        gap = i < 0 ? -inf : gmax + m2;
        if (i < 0 || gap < eps) { conv = 1; break; }
        if (it >= p.max_iter) break;
        // 2. j
        const float* Ki = Kb + (i < na ? a0 + i : bshift + i) * p.ldk;
        double best = 0.0;
        int j = -1;
        for (int t = tid; t < n; t += 256) {
            const bool pos = t < na;
            const double a = alpha[t], yg = pos ? G[t] : -G[t];
            const bool ub = a >= Cc, lb = a <= 0.0;
            if (pos ? lb : ub) continue;                              // not in I_low
            const double b = gmax + yg;
            if (!(b > 0.0)) continue;
            double q = 2.0 - 2.0 * (double)Ki[pos ? a0 + t : bshift + t];
            if (!(q > 0.0)) q = SVM_TAU;
            argd_better(best, j, (b * b) / q, t);
        }
        block_argmax(best, j, sv2, si2);
        if (j < 0) { conv = 1; break; }
        // 3. the two-variable update, by every thread alike
        const float* Kj = Kb + (j < na ? a0 + j : bshift + j) * p.ldk;
        const bool ipos = i < na, jpos = j < na;
        const double oi = alpha[i], oj = alpha[j], gi = G[i], gj = G[j];
        double quad = 2.0 - 2.0 * (double)Ki[jpos ? a0 + j : bshift + j];
        if (!(quad > 0.0)) quad = SVM_TAU;
        double ai = oi, aj = oj;
        if (ipos != jpos) {
            const double delta = (-gi - gj) / quad, diff = ai - aj;
            ai = ai + delta; aj = aj + delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
            if (diff > 0.0) { if (ai > Cc) { ai = Cc; aj = Cc - diff; } }          // C_i = C_j: diff > C_i - C_j is diff > 0
            else { if (aj > Cc) { aj = Cc; ai = Cc + diff; } }
        } else {
            const double delta = (gi - gj) / quad, sum = ai + aj;
            ai = ai - delta; aj = aj + delta;
            if (sum > Cc) { if (ai > Cc) { ai = Cc; aj = sum - Cc; } }
            else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
            if (sum > Cc) { if (aj > Cc) { aj = Cc; ai = sum - Cc; } }
            else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
        }
        const double di = ai - oi, dj = aj - oj;
        __syncthreads();                                              // everybody has read alpha and G of i and j
        // 4. the gradient
        for (int t = tid; t < n; t += 256) {
            const bool pos = t < na;
            const int64_t col = pos ? a0 + t : bshift + t;
            const double ki = (double)Ki[col], kj = (double)Kj[col];
            const double qi = pos == ipos ? ki : -ki, qj = pos == jpos ? kj : -kj;
            G[t] = G[t] + (qi * di + qj * dj);
        }
        if (tid == 0) { alpha[i] = ai; alpha[j] = aj; }
        ++it;
        __syncthreads();
    }
    for (int t = tid; t < n; t += 256) { ga[t] = alpha[t]; gg[t] = G[t]; }
    if (tid == 0) {                                                   // libsvm's calculate_rho and the counts, t ascending
        double ub = inf, lb = -inf, sum_free = 0.0;
        int nfree = 0, nsv = 0, nbound = 0;
        bool finite = true;
        for (int t = 0; t < n; ++t) {
            const bool pos = t < na;
            const double a = alpha[t], yg = pos ? G[t] : -G[t];
            if (!(a - a == 0.0) || !(yg - yg == 0.0)) finite = false;         // a NaN or an infinity in alpha or G
            if (a > 0.0) ++nsv;
            if (a >= Cc) {
                ++nbound;
                if (!pos) ub = yg < ub ? yg : ub; else lb = yg > lb ? yg : lb;
            } else if (a <= 0.0) {
                if (pos) ub = yg < ub ? yg : ub; else lb = yg > lb ? yg : lb;
            } else {
                ++nfree;
                sum_free = sum_free + yg;
            }
        }
        const double rho = nfree > 0 ? sum_free / (double)nfree : (ub + lb) / 2.0;
        st[0] = before + (double)it; st[1] = finite ? (double)conv : -3.0; st[2] = gap; st[3] = (double)nsv; st[4] = (double)nbound; st[5] = rho;
        st[6] = 0.0; st[7] = 0.0;
    }
}

// ------------------------------------------------------------------ pack
__device__ __forceinline__ int pair_index(int a, int b, int nc) { return a * nc - a * (a + 1) / 2 + (b - a - 1); }

struct SvmPairs {
    const hsimae_svm_problem* tab; int nc;
    __device__ __forceinline__ const hsimae_svm_problem& pair(int a, int b) const { return tab[pair_index(a, b, nc)]; }
    // the bank rows of class c: from its first pair
    __device__ __forceinline__ int64_t start(int c) const { return c < nc - 1 ? pair(c, c + 1).a0 : pair(c - 1, c).b0; }
    __device__ __forceinline__ int64_t count(int c) const { return c < nc - 1 ? pair(c, c + 1).na : pair(c - 1, c).nb; }
    // alpha of row t of class c in its pair with class o
    __device__ __forceinline__ double alpha_of(const double* alpha, int c, int o, int64_t t) const {
        if (c < o) return alpha[pair(c, o).out_offset + t];
        const hsimae_svm_problem& T = pair(o, c);
        return alpha[T.out_offset + T.na + t];
    }
    __device__ __forceinline__ bool is_sv(const double* alpha, int c, int64_t t) const {
        bool any = false;
        for (int o = 0; o < nc; ++o)
            if (o != c && alpha_of(alpha, c, o, t) > 0.0) any = true;
        return any;
    }
};

__global__ __launch_bounds__(256) void svm_pack_kernel(hsimae_svm_pack_params p) {
    __shared__ int wave_n[4];
    __shared__ int list_pos[256], list_row[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nc = p.n_class, c = blockIdx.x;
    const int P = nc * (nc - 1) / 2;
    const SvmPairs S{p.table + p.first_problem, nc};
    const int64_t M = p.M;
    // the table must describe nc disjoint ascending classes inside the bank and alpha ranges inside the buffer
    int wrong = 0;
    for (int a = 0; a < nc; ++a) {
        const int64_t s0 = S.start(a), n0 = S.count(a);
        if (s0 < 0 || n0 < 0 || n0 > M || s0 > M - n0) { wrong = 1; continue; }
        if (a + 1 < nc && s0 + n0 > S.start(a + 1)) wrong = 1;
    }
    for (int q = tid; q < P; q += 256) {
        int a = 0, rest = q;
        while (rest >= nc - 1 - a) { rest -= nc - 1 - a; ++a; }
        const int b = a + 1 + rest;
        const hsimae_svm_problem& T = S.pair(a, b);
        if (T.a0 != S.start(a) || T.na != S.count(a) || T.b0 != S.start(b) || T.nb != S.count(b) || T.out_offset < 0 ||
            T.na < 0 || T.nb < 0 || T.na + T.nb > M || T.out_offset > p.alpha_len - (T.na + T.nb) ||
            p.state[(p.first_problem + q) * HSIMAE_SVM_STATE + 1] == -1.0) wrong = 1;
    }
    if (__syncthreads_or(wrong)) {
        if (c == 0) for (int k = tid; k <= nc; k += 256) p.sv_start[k] = 0;
        return;
    }
    if (c == 0) for (int q = tid; q < P; q += 256) p.rho[q] = (float)p.state[(p.first_problem + q) * HSIMAE_SVM_STATE + 5];
    // the support rows of the classes before this one
    int mine = 0;
    for (int k = 0; k < c; ++k) {
        const int64_t nk = S.count(k);
        for (int64_t t = tid; t < nk; t += 256) mine += S.is_sv(p.alpha, k, t) ? 1 : 0;
    }
    mine = tree_sum(mine);
    if (lane == 0) wave_n[wave] = mine;
    __syncthreads();
    int at = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    __syncthreads();
    if (tid == 0) p.sv_start[c] = at;
    const int64_t r0 = S.start(c), ncls = S.count(c);
    for (int64_t t0 = 0; t0 < ncls; t0 += 256) {
        const int64_t t = t0 + tid;
        const bool sv = t < ncls && S.is_sv(p.alpha, c, t);
        const unsigned long long mask = __ballot(sv);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int pos = at + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += wave_n[w];
        const int found = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        if (sv) {
            list_pos[pos - at] = pos;
            list_row[pos - at] = (int)(r0 + t);
            p.sv_index[pos] = (int)(r0 + t);
            p.sv_sumsq[pos] = p.sumsq[r0 + t];
            for (int j = 0; j < nc - 1; ++j) {
                const int o = j < c ? j : j + 1;
                const double a = S.alpha_of(p.alpha, c, o, t);
                p.coef[(int64_t)j * p.ldc + pos] = (float)(c < o ? a : -a);
            }
        }
        __syncthreads();
        for (int k = 0; k < found; ++k) {
            const float* src = p.x + (int64_t)list_row[k] * p.ldx;
            float* dst = p.sv + (int64_t)list_pos[k] * p.ldsv;
            for (int d = tid; d < p.D; d += 256) dst[d] = src[d];
        }
        at += found;
        __syncthreads();
    }
    if (c == nc - 1 && tid == 0) p.sv_start[nc] = at;
}

// ------------------------------------------------------------------ predict
__global__ __launch_bounds__(256) void svm_predict_kernel(hsimae_svm_predict_params p) {
    extern __shared__ float svm_f[];                                  // all of it dynamic: the opt-in covers the whole workgroup limit
    float (*Qs)[SLD] = reinterpret_cast<float (*)[SLD]>(svm_f);
    float (*Bs)[SLD] = reinterpret_cast<float (*)[SLD]>(svm_f + TQ * SLD);
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(svm_f);
    int* votes = reinterpret_cast<int*>(svm_f);                      // [class][row], over the slabs once the tiles are done
    float* qn = svm_f + SVM_SLAB_FLOATS;
    int* cs = reinterpret_cast<int*>(qn + TQ);                        // [SVM_CS] where each class starts among the support rows
    float* dec = qn + TQ + SVM_CS;                                    // [pair][row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = p.D, nc = p.n_class;
    const int NP = nc * (nc - 1) / 2;
    int S = p.sv_start[nc];
    S = S < 0 ? 0 : (S > p.S_max ? p.S_max : S);
    if (tid <= nc) { const int v = p.sv_start[tid]; cs[tid] = v < 0 ? 0 : (v > S ? S : v); }
    const float g2 = p.gamma * HS_LOG2E;
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t qtiles = ((int64_t)p.Q + TQ - 1) / TQ;
    int out_count = 0;
    for (int64_t qt = blockIdx.x; qt < qtiles; qt += gridDim.x) {
        const int64_t q0 = qt * TQ;
        __syncthreads();                                              // the votes of the tile before are read
        for (int rr = 0; rr < 16; ++rr) {                             // the query rows' squared norms, one wave per row
            const int row = wave * 16 + rr;
            float ss = 0.f;
            if (q0 + row < p.Q) {                                     // wave-uniform
                const float* x = p.q + (q0 + row) * p.ldq;
                for (int c = lane; c < D; c += 64) ss = fmaf(x[c], x[c], ss);
                ss = tree_sum(ss);
            }
            if (lane == 0) qn[row] = ss;
        }
        for (int e = tid; e < NP * TQ; e += 256) dec[e] = 0.f;
        SlabRegs rq = fetch_slab(p.q, q0, p.Q, p.ldq, 0, D), rb = fetch_slab(p.sv, 0, S, p.ldsv, 0, D);
        for (int j0 = 0; j0 < S; j0 += TB) {
            const f32x16 acc = dot_tile(Qs, Bs, rq, rb, p.q, q0, p.Q, p.ldq, p.sv, j0, S, p.ldsv, D);
            hand_over(P, acc);
            const int jend = j0 + TB < S ? j0 + TB : S;
            for (int e = tid; e < TQ * TB; e += 256) {
                const int r = e >> 6, c = e & 63;
                if (j0 + c < jend) P[r][c] = svm_kernel_value(svm_d2(P[r][c], qn[r], p.sv_sumsq[j0 + c]), g2);
            }
            __syncthreads();
            int q = 0;
            for (int a = 0; a < nc; ++a)
                for (int b = a + 1; b < nc; ++b, ++q) {
                    if ((q & 3) != wave) continue;                    // wave-uniform: this wave's pairs
                    const int alo = cs[a] > j0 ? cs[a] : j0, ahi = cs[a + 1] < jend ? cs[a + 1] : jend;
                    const int blo = cs[b] > j0 ? cs[b] : j0, bhi = cs[b + 1] < jend ? cs[b + 1] : jend;
                    if (alo >= ahi && blo >= bhi) continue;
                    float d = dec[q * TQ + lane];
                    const float* ca = p.coef + (int64_t)(b - 1) * p.ldc;
                    const float* cb = p.coef + (int64_t)a * p.ldc;
                    for (int s = alo; s < ahi; ++s) d = fmaf(ca[s], P[lane][s - j0], d);
                    for (int s = blo; s < bhi; ++s) d = fmaf(cb[s], P[lane][s - j0], d);
                    dec[q * TQ + lane] = d;
                }
        }
        __syncthreads();                                              // the sums are whole, P is read
        if (wave == 0) {
            const int64_t r = q0 + lane;
            const bool valid = r < p.Q;
            for (int c = 0; c < nc; ++c) votes[c * TQ + lane] = 0;
            int q = 0;
            for (int a = 0; a < nc; ++a)
                for (int b = a + 1; b < nc; ++b, ++q) {
                    const float d = dec[q * TQ + lane] - p.rho[q];
                    if (p.decision && valid) p.decision[r * p.ldd + q] = d;
                    votes[(d > 0.f ? a : b) * TQ + lane] += 1;
                }
            int best = 0, bv = votes[lane];
            for (int c = 1; c < nc; ++c) { const int v = votes[c * TQ + lane]; if (v > bv) { bv = v; best = c; } }
            int second = -1;
            for (int c = 0; c < nc; ++c) { const int v = votes[c * TQ + lane]; if (c != best && v > second) second = v; }
            const float fp = (float)NP, top = (float)bv / fp, sec = (float)second / fp;
            if (valid) {
                if (p.probs) {
                    float* pr = p.probs + r * p.ldp;
                    for (int c = 0; c < p.first; ++c) pr[c] = 0.f;
                    for (int c = 0; c < nc; ++c) pr[p.first + c] = (float)votes[c * TQ + lane] / fp;
                }
                const int64_t pix = row_pixel(p.pixels, p.p0, r, HW);
                write_maps(p.label_map, p.conf_map, p.margin_map, pix, p.first + best, top, sec, false);
                out_count += __popcll(__ballot(pix < 0));
            }
        }
    }
    if (p.outside) {
        if (tid == 0) p.outside[blockIdx.x] = out_count;
        if (blockIdx.x == 0) for (int g = gridDim.x + tid; g < HSIMAE_SVM_GRID; g += 256) p.outside[g] = 0;
    }
}

bool positive_finite(double v) { return v > 0.0 && v <= 1.7e308; }

}  // namespace

int hs_svm_gram(const hsimae_svm_gram_params& p, hipStream_t s) {
    if (p.M < 0 || p.D <= 0 || p.D % 4 || p.ldx < p.D || p.ldk < p.M || p.n_gamma < 1) return HS_EDIMS;
    if (p.M > HSIMAE_SVM_MAX_ROWS || p.D > 4096 || p.n_gamma > HSIMAE_SVM_MAX_GAMMAS) return HS_EUNSUPPORTED;
    for (int g = 0; g < p.n_gamma; ++g)
        if (!(p.gamma[g] > 0.f) || p.gamma[g] > 3.0e38f) return HS_EDIMS;
    if (p.M > 0 && (!p.x || !p.K || !p.sumsq)) return HS_ENULL;
    if (misaligned(p.x, 15) || p.ldx % 4 || misaligned(p.K, 3) || misaligned(p.sumsq, 3)) return HS_EALIGN;
    if (p.M == 0) return HS_OK;
    const unsigned T = (unsigned)((p.M + TQ - 1) / TQ);
    hipLaunchKernelGGL(svm_sumsq_kernel, dim3(T), dim3(256), 0, s, p);
    hipLaunchKernelGGL(svm_gram_kernel, dim3(T, T), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_svm_solve(const hsimae_svm_solve_params& p, hipStream_t s) {
    if (p.n_problems < 0 || p.M < 1 || p.ldk < p.M || p.n_k < 1 || p.max_iter < 0 || !positive_finite(p.eps) || p.alpha_len < 0)
        return HS_EDIMS;
    if (p.M > HSIMAE_SVM_MAX_ROWS) return HS_EUNSUPPORTED;
    if (p.n_problems > 0 && (!p.K || !p.table || !p.alpha || !p.grad || !p.state)) return HS_ENULL;
    if (misaligned(p.K, 3) || misaligned(p.table, 7) || misaligned(p.alpha, 7) || misaligned(p.grad, 7) || misaligned(p.state, 7))
        return HS_EALIGN;
    if (p.n_problems == 0) return HS_OK;
    return svm_launch<svm_solve_kernel>(dim3((unsigned)p.n_problems), (size_t)16 * p.M + SVM_SCRATCH, s, p);
}

int hs_svm_pack(const hsimae_svm_pack_params& p, hipStream_t s) {
    if (p.first_problem < 0 || p.n_class < 2 || p.M < 1 || p.D <= 0 || p.ldx < p.D || p.ldsv < p.D || p.ldc < p.M || p.alpha_len < 0)
        return HS_EDIMS;
    if (p.n_class > HSIMAE_SVM_MAX_CLASSES || p.M > HSIMAE_SVM_MAX_ROWS) return HS_EUNSUPPORTED;
    if (!p.table || !p.alpha || !p.state || !p.x || !p.sumsq || !p.sv_index || !p.sv_start || !p.coef || !p.rho || !p.sv || !p.sv_sumsq)
        return HS_ENULL;
    if (misaligned(p.table, 7) || misaligned(p.alpha, 7) || misaligned(p.state, 7) || misaligned(p.x, 3) || misaligned(p.sumsq, 3) ||
        misaligned(p.sv_index, 3) || misaligned(p.sv_start, 3) || misaligned(p.coef, 3) || misaligned(p.rho, 3) || misaligned(p.sv, 3) ||
        misaligned(p.sv_sumsq, 3)) return HS_EALIGN;
    hipLaunchKernelGGL(svm_pack_kernel, dim3((unsigned)p.n_class), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_svm_predict(const hsimae_svm_predict_params& p, hipStream_t s) {
    if (p.Q < 0 || p.D <= 0 || p.D % 4 || p.ldq < p.D || p.ldsv < p.D || p.S_max < 0 || p.ldc < p.S_max || p.n_class < 2 || p.first < 0 ||
        p.H <= 0 || p.W <= 0 || !(p.gamma > 0.f) || p.gamma > 3.0e38f) return HS_EDIMS;
    if (p.n_class > HSIMAE_SVM_MAX_CLASSES || p.D > 4096 || p.S_max > HSIMAE_SVM_MAX_ROWS) return HS_EUNSUPPORTED;
    const int NP = p.n_class * (p.n_class - 1) / 2;
    if ((p.probs && p.ldp < p.first + p.n_class) || (p.decision && p.ldd < NP)) return HS_EDIMS;
    if (p.Q > 0 && (!p.q || !p.sv || !p.sv_sumsq || !p.sv_start || !p.coef || !p.rho || !p.label_map)) return HS_ENULL;
    if (misaligned(p.q, 15) || misaligned(p.sv, 15) || p.ldq % 4 || p.ldsv % 4 || misaligned(p.sv_sumsq, 3) || misaligned(p.sv_start, 3) ||
        misaligned(p.coef, 3) || misaligned(p.rho, 3) || misaligned(p.pixels, 7) || misaligned(p.label_map, 7) ||
        misaligned(p.conf_map, 3) || misaligned(p.margin_map, 3) || misaligned(p.probs, 3) || misaligned(p.decision, 3) ||
        misaligned(p.outside, 3)) return HS_EALIGN;
    if (p.Q == 0) return HS_OK;
    const int64_t tiles = ((int64_t)p.Q + TQ - 1) / TQ;
    const size_t lds = sizeof(float) * (size_t)(SVM_SLAB_FLOATS + TQ + SVM_CS + TQ * NP);
    return svm_launch<svm_predict_kernel>(dim3((unsigned)(tiles < HSIMAE_SVM_GRID ? tiles : HSIMAE_SVM_GRID)), lds, s, p);
}

HS_UNIT_VARIANT_BITS(svm)
