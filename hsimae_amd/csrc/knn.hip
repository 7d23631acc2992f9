// k-NN evaluation of frozen features on the device (hsimae_row_normalize, hsimae_knn_topk, hsimae_knn_vote; include/hsimae_hip.h):
// what lies between "pooled feature of every pixel" and "label of every pixel" when a pretrained encoder is judged without
// fine-tuning (Wu et al. 2018; DINO's knn_classifier).
//
//   row_normalize_kernel  one wave per row: ss = lane-strided fmaf(x, x, ss) over the columns l, l + 64, .., the xor tree over the
//                         64 lanes, n = sqrtf(ss), r = 1 / fmaxf(n, 1e-12f), out = x * r (F.normalize's rule: a zero row gives
//                         zeros).  In place is allowed: a lane re-reads only what it writes itself.
//   knn_topk_kernel       a workgroup (4 waves) owns 64 query rows and walks the bank in tiles of 64 rows in ascending index.
//                         Per tile: K-slabs of 32 columns of both operands staged in LDS, every wave one 32 x 32 block of exact
//                         fp32 dot products on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain from +0: k = 0, 1, .., D - 1 for
//                         every output, wherever its bank row sits in the tile), the 64 x 64 block handed over through LDS, then
//                         every wave updates the running top-k lists of its 16 query rows (LDS, rank = lane): a candidate enters
//                         while the list is short, and once it is full only if it beats the k-th entry strictly; equal ones stay
//                         behind the earlier index.  A NaN orders below every number.  The [Q, M] matrix exists only as that
//                         64 x 64 block; the only global writes are idx and sim.
//   knn_vote_kernel       one wave per row: lane j holds neighbour j (rank order), w_j = exp2(((sim_j - sim_0) inv_T) log2 e),
//                         lane l holds the classes first + l, first + l + 64, ..: score_c = the w_j of class c added in rank
//                         order from 0, total = lane-strided sum and the xor tree, p_c = score_c * (1 / total); label, confidence
//                         and margin by wave_argmax, row_runner_up and write_maps (row_wave.h), as class_prob_kernel's.
//
// No atomics anywhere; a row is touched by one wave: two runs are bit-identical.
#include "common.h"
#include "dot_tile.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int KNN_MAXK = 64;          // one list entry per lane
constexpr int KNN_MAXC = 1024;
constexpr int KNN_MAXNB = 2048;       // workgroups at most: a stride loop beyond (rows of normalize / vote, query tiles of top-k)
// the slabs, the 64 x 64 dot tile, beats() and the row norm: dot_tile.h (shared with kmeans.hip)

__global__ __launch_bounds__(256) void row_normalize_kernel(hsimae_row_normalize_params p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = p.D;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.N; r += (int64_t)gridDim.x * 4) {       // wave-uniform
        const float* x = p.x + r * p.ld;
        float* o = p.out + r * p.ldo;
        float n;
        const float rn = row_inv_norm(x, D, lane, n);
        for (int c = lane; c < D; c += 64) o[c] = x[c] * rn;
        if (p.norms && lane == 0) p.norms[r] = n;
    }
}

// the value lane `l` holds, l wave-uniform
__device__ __forceinline__ int lane_of(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_of(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }

__global__ __launch_bounds__(256) void knn_topk_kernel(hsimae_knn_topk_params p) {
    __shared__ float slabs[2][TQ][SLD];          // the two operands' slabs; after a tile's last slab the block P lies over them
    float (*Qs)[SLD] = slabs[0], (*Bs)[SLD] = slabs[1];
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(&slabs[0][0][0]);       // the tile's dot products [query][bank row]
    __shared__ float Ls[TQ][KNN_MAXK];           // running lists, rank = column
    __shared__ int Li[TQ][KNN_MAXK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = p.k, D = p.D;
    const int64_t qtiles = ((int64_t)p.Q + TQ - 1) / TQ;
    for (int64_t qt = blockIdx.x; qt < qtiles; qt += gridDim.x) {
        const int64_t q0 = qt * TQ;
        SlabRegs rq = fetch_slab(p.q, q0, p.Q, p.ldq, 0, D), rb = fetch_slab(p.bank, 0, p.M, p.ldb, 0, D);
        for (int64_t j0 = 0; j0 < p.M; j0 += TB) {
            const f32x16 acc = dot_tile(Qs, Bs, rq, rb, p.q, q0, p.Q, p.ldq, p.bank, j0, p.M, p.ldb, D);
            hand_over(P, acc);
            // the lists of this wave's 16 rows; before this tile every row holds min(k, j0) entries
            const int len0 = j0 < k ? (int)j0 : k;
            const bool valid = j0 + lane < p.M;
            for (int rr = 0; rr < 16; ++rr) {
                const int row = wave * 16 + rr;
                if (q0 + row >= p.Q) break;                                // wave-uniform
                const float c = P[row][lane];
                int len = len0;
                float kth = len == k ? Ls[row][k - 1] : 0.f;
                unsigned long long mask = __ballot(valid && (len < k || beats(c, kth)));
                if (!mask) continue;
                float ls = Ls[row][lane];                                  // lanes >= len: not yet meaningful, never read as entries
                int lx = Li[row][lane];
                while (mask) {
                    const int b = __ffsll((long long)mask) - 1;            // ascending bank index
                    mask &= mask - 1;
                    const float s = lane_of(c, b);
                    if (len == k && !beats(s, kth)) continue;
                    const int at = __popcll(__ballot(lane < len && !beats(s, ls)));        // the entries that stay in front: a prefix
                    const float us = __shfl_up(ls, 1);
                    const int ux = __shfl_up(lx, 1);
                    if (lane > at) { ls = us; lx = ux; }
                    if (lane == at) { ls = s; lx = (int)(j0 + b); }
                    if (len < k) ++len;
                    kth = lane_of(ls, k - 1);
                }
                Ls[row][lane] = ls;
                Li[row][lane] = lx;
            }
        }
        for (int rr = 0; rr < 16; ++rr) {
            const int row = wave * 16 + rr;
            if (q0 + row >= p.Q) break;
            if (lane < k) {
                p.idx[(q0 + row) * k + lane] = Li[row][lane];
                p.sim[(q0 + row) * k + lane] = Ls[row][lane];
            }
        }
    }
}

__global__ __launch_bounds__(256) void knn_vote_kernel(hsimae_knn_vote_params p) {
    __shared__ float Sc[4][KNN_MAXC];            // per wave: the scores, then the probabilities; a lane re-reads only its own
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = p.k, C = p.C, first = p.first;
    const int64_t HW = (int64_t)p.H * p.W;
    float* sc = Sc[wave];
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.Q; r += (int64_t)gridDim.x * 4) {       // wave-uniform
        int nb = -1;
        float s = 0.f;
        if (lane < k) { nb = p.idx[r * k + lane]; s = p.sim[r * k + lane]; }
        int64_t lab = first;
        bool wrong = false;
        if (lane < k) {
            wrong = nb < 0 || nb >= p.M;
            if (!wrong) { lab = p.bank_labels[nb]; wrong = lab < first || lab >= C; }
        }
        const bool bad = __ballot(wrong) != 0;
        const float s0 = lane_of(s, 0);
        const float w = __builtin_amdgcn_exp2f(((s - s0) * p.inv_temperature) * HS_LOG2E);
        const int cls = (int)lab;
        float sum = 0.f;
        for (int c = first + lane; c - lane < C; c += 64) {                                        // whole rounds: every lane takes part
            float a = 0.f;
            for (int j = 0; j < k; ++j) {                                                          // rank order
                const float wj = lane_of(w, j);
                if (lane_of(cls, j) == c) a += wj;
            }
            if (c < C) { sc[c] = a; sum += a; }
        }
        const float rs = 1.f / tree_sum(sum);
        float key = -__builtin_inff();
        int best = 0x7fffffff;
        if (p.probs) for (int c = lane; c < first; c += 64) p.probs[r * p.ldp + c] = 0.f;
        for (int c = first + lane; c < C; c += 64) {                                               // ascending: first of a tie stays
            const float pc = bad ? 0.f : sc[c] * rs;
            sc[c] = pc;
            if (p.probs) p.probs[r * p.ldp + c] = pc;
            arg_better(key, best, pc, c);
        }
        wave_argmax(key, best);
        float second = row_runner_up(sc, 1.f, first, C, lane, best);
        if (bad) { best = 0; key = second = 0.f; }                                                 // label 0, confidence and margin 0
        const int64_t pix = row_pixel(p.pixels, p.p0, r, HW);
        if (lane == 0) {
            if (bad) *p.bad = 1;
            write_maps(p.label_map, p.conf_map, p.margin_map, pix, best, key, second, C - first == 1);
        }
    }
}

}  // namespace

int hs_row_normalize(const hsimae_row_normalize_params& p, hipStream_t s) {
    if (p.N < 0 || p.D < 0 || p.ld < p.D || p.ldo < p.D) return HS_EDIMS;
    if (p.N > 0 && p.D > 0 && (!p.x || !p.out)) return HS_ENULL;
    if (misaligned(p.x, 3) || misaligned(p.out, 3) || misaligned(p.norms, 3)) return HS_EALIGN;
    if (p.N == 0 || p.D == 0) return HS_OK;
    hipLaunchKernelGGL(row_normalize_kernel, dim3(rows_grid(p.N, KNN_MAXNB)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_knn_topk(const hsimae_knn_topk_params& p, hipStream_t s) {
    if (p.Q < 0 || p.M < 0 || p.D <= 0 || p.D % 4 || p.k < 1 || p.ldq < p.D || p.ldb < p.D) return HS_EDIMS;
    if (p.k > KNN_MAXK || p.M > (1 << 20) || p.D > 4096) return HS_EUNSUPPORTED;
    if (p.k > p.M) return HS_EDIMS;
    if (p.Q > 0 && (!p.q || !p.bank || !p.idx || !p.sim)) return HS_ENULL;
    if (misaligned(p.q, 15) || misaligned(p.bank, 15) || p.ldq % 4 || p.ldb % 4 || misaligned(p.idx, 3) || misaligned(p.sim, 3))
        return HS_EALIGN;
    if (p.Q == 0) return HS_OK;
    const int64_t tiles = ((int64_t)p.Q + TQ - 1) / TQ;
    hipLaunchKernelGGL(knn_topk_kernel, dim3((unsigned)(tiles < KNN_MAXNB ? tiles : KNN_MAXNB)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_knn_vote(const hsimae_knn_vote_params& p, hipStream_t s) {
    if (p.Q < 0 || p.M < 1 || p.k < 1 || p.C < 2 || p.first < 0 || p.first >= p.C || (p.probs && p.ldp < p.C) || p.H <= 0 || p.W <= 0 ||
        !(p.inv_temperature > 0.f) || p.inv_temperature > 3.0e38f) return HS_EDIMS;
    if (p.k > KNN_MAXK || p.C > KNN_MAXC) return HS_EUNSUPPORTED;
    if (p.Q > 0 && (!p.idx || !p.sim || !p.bank_labels || !p.label_map || !p.bad)) return HS_ENULL;
    if (misaligned(p.idx, 3) || misaligned(p.sim, 3) || misaligned(p.bank_labels, 7) || misaligned(p.pixels, 7) ||
        misaligned(p.label_map, 7) || misaligned(p.conf_map, 3) || misaligned(p.margin_map, 3) || misaligned(p.probs, 3) ||
        misaligned(p.bad, 3)) return HS_EALIGN;
    if (p.Q == 0) return HS_OK;
    hipLaunchKernelGGL(knn_vote_kernel, dim3(rows_grid(p.Q, KNN_MAXNB)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(knn)
