// k-means on frozen features on the device (hsimae_kmeans_assign, hsimae_kmeans_update; include/hsimae_hip.h): Lloyd's algorithm
// over fp32 rows x [N, D] and K centroids c [K, D], one formulation for both metrics: score(i, k) = x_i . c_k - bias_k, label =
// argmax.  Euclidean: bias_k = 1/2 ||c_k||^2.  Cosine (spherical k-means): unit rows, unit centroids, bias NULL = 0.
//
//   kmeans_assign_kernel  a workgroup (4 waves) owns 64 rows of x and walks the centroids in tiles of 64 in ascending index, as
//                         knn_topk_kernel walks its bank: the same K-slabs in LDS and the same exact-fp32 dot tile (dot_tile.h).
//                         Per tile the 64 x 64 block is handed over through LDS with the tile's biases beside it; lane (row, part)
//                         scans its 16 columns: score = dot - bias (one rounding), and keeps best, best index and second best in
//                         registers across all tiles.  The four parts of a row are merged once, after the last tile (lane ^ 16,
//                         ^ 32).  A strictly better score wins, equal scores stay with the lower index, a NaN beats nothing.
//                         A row's label is compared with the value already in the map before it is overwritten; the workgroup's
//                         count of changed rows goes to changed[workgroup], workgroup 0 zeroes the entries no workgroup owns.
//   kmeans_sums_kernel    one wave per (cluster, 64-column slab): it scans all labels in windows of 2,048 (32 loads per lane in
//                         flight), ballots compact the window's members into an ascending list in LDS, and lane l adds column
//                         64 slab + l of every member row in ascending row order into one fp64 sum (32 rows in flight), and
//                         (x - c_old)^2 into the inertia partial beside it.
//                         The wave of slab 0 writes the count; the wave (0, 0) also counts the labels that name no cluster.
//   kmeans_finish_kernel  one wave per cluster: c = fp32(sum / count), for cosine normalised in place by row_normalize_kernel's
//                         rule (row_inv_norm), bias = fp32(1/2 sum c^2) with the sum in fp64; an empty cluster is not touched.
//                         One more workgroup adds the state block from what the earlier launches left: inertia, changed,
//                         iterations, empty, bad.
//
// No atomics anywhere; every output element is one chain in a fixed order: two runs are bit-identical, whatever the grid.
#include "common.h"
#include "dot_tile.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int KM_MAXK = 1024;
constexpr int KM_NONE = 0x7fffffff;           // "no centroid yet": loses every tie on the index

// the better of two scores under beats(): a number over a NaN, the larger number
__device__ __forceinline__ float better_of(float a, float b) { return beats(b, a) ? b : a; }

// (best score, its centroid, second best score) of the centroids seen so far, and f, the merge of another such triple into it
// (the form wave_tree takes); merging is order-free: ties go by the index
struct Best {
    float b; int i; float b2;
    static __device__ __forceinline__ void f(float& b, int& i, float& b2, float s, int si, float s2) {
        const bool take = beats(s, b) || (!beats(b, s) && si < i);
        if (take) { b2 = better_of(s2, b); b = s; i = si; }
        else b2 = better_of(b2, s);
    }
};

__global__ __launch_bounds__(256) void kmeans_assign_kernel(hsimae_kmeans_assign_params p) {
    __shared__ float slabs[2][TQ][SLD];          // the two operands' slabs; after a tile's last slab the block P lies over them
    float (*Xs)[SLD] = slabs[0], (*Cs)[SLD] = slabs[1];
    float (*P)[PLD] = reinterpret_cast<float (*)[PLD]>(&slabs[0][0][0]);       // the tile's dot products [row][centroid]
    __shared__ float Bt[TB];                     // the tile's biases
    __shared__ int Ch[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = p.K, D = p.D;
    const int row = wave * 16 + (lane & 15), part = lane >> 4;                 // bank (row + 16 part + c) % 32: no conflict
    const float qnan = __builtin_nanf("");
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t tiles = ((int64_t)p.N + TQ - 1) / TQ;
    int changed = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t i0 = t * TQ;
        SlabRegs rx = fetch_slab(p.x, i0, p.N, p.ldx, 0, D), rc = fetch_slab(p.c, 0, K, p.ldc, 0, D);
        Best best{qnan, KM_NONE, qnan};
        for (int j0 = 0; j0 < K; j0 += TB) {
            const f32x16 acc = dot_tile(Xs, Cs, rx, rc, p.x, i0, p.N, p.ldx, p.c, j0, K, p.ldc, D);
            // (dot_tile's barriers: the readers of the previous tile's Bt are done; hand_over's: Bt is whole with P)
            if (threadIdx.x < TB) Bt[threadIdx.x] = (p.bias && j0 + (int)threadIdx.x < K) ? p.bias[j0 + threadIdx.x] : 0.f;
            hand_over(P, acc);
#pragma unroll 4
            for (int c = 0; c < 16; ++c) {
                const int col = part * 16 + c, j = j0 + col;
                const float s = P[row][col] - Bt[col];
                Best::f(best.b, best.i, best.b2, j < K ? s : qnan, j < K ? j : KM_NONE, qnan);
            }
        }
        wave_tree<Best, 16>(best.b, best.i, best.b2);                          // the row's four parts: lane ^ 16, ^ 32
        const int64_t i = i0 + row;
        if (part == 0 && i < p.N) {
            const int64_t pix = row_pixel(p.pixels, p.p0, i, HW);
            if (pix >= 0) {
                const int64_t lab = (int64_t)p.first + best.i;
                if (p.changed) changed += p.labels[pix] != lab;
                p.labels[pix] = lab;
                if (p.score) p.score[pix] = best.b;
                if (p.margin) p.margin[pix] = K == 1 ? best.b : best.b - best.b2;
            }
        }
    }
    if (p.changed) {                                                           // the same in every thread
        changed = tree_sum(changed);
        if (lane == 0) Ch[wave] = changed;
        __syncthreads();
        if (threadIdx.x == 0) p.changed[blockIdx.x] = Ch[0] + Ch[1] + Ch[2] + Ch[3];
        if (blockIdx.x == 0)
            for (int g = gridDim.x + threadIdx.x; g < HSIMAE_KMEANS_GRID; g += 256) p.changed[g] = 0;
    }
}

__device__ __forceinline__ int slabs_of(int D) { return (D + 63) / 64; }

constexpr int KM_CHUNKS = 32;                 // a window is 32 chunks of 64 labels
constexpr int KM_WIN = 64 * KM_CHUNKS;
constexpr int KM_BATCH = 32;                  // member rows in flight per wave

__global__ __launch_bounds__(64) void kmeans_sums_kernel(hsimae_kmeans_update_params p) {
    __shared__ int list[KM_WIN];                 // the window's members (row - window start), ascending
    const int lane = threadIdx.x, nslab = slabs_of(p.D);
    const int k = blockIdx.x / nslab, slab = blockIdx.x % nslab;               // one wave per workgroup: uniform
    const int col = slab * 64 + lane;
    const bool live = col < p.D;
    const bool census = blockIdx.x == 0;
    const int64_t lo = p.first, hi = (int64_t)p.first + p.K, want = lo + k;
    const float cold = live ? p.c[(int64_t)k * p.ldc + col] : 0.f;
    const float* xc = p.x + (live ? col : 0);                                  // (a lane past D reads column 0 and drops it)
    const unsigned long long below = (1ull << lane) - 1;
    double sum = 0.0, ine = 0.0;
    int64_t cnt = 0, nbad = 0;
    for (int64_t w0 = 0; w0 < p.N; w0 += KM_WIN) {
        int64_t lab[KM_CHUNKS];
#pragma unroll
        for (int ch = 0; ch < KM_CHUNKS; ++ch) {                               // all of the window's labels in flight
            const int64_t i = w0 + ch * 64 + lane;
            lab[ch] = i < p.N ? p.labels[i] : lo - 1;                          // past the end: nobody's member, and not counted
        }
        int n = 0;
#pragma unroll
        for (int ch = 0; ch < KM_CHUNKS; ++ch) {
            const bool valid = w0 + ch * 64 + lane < p.N;
            const bool mem = lab[ch] == want;
            const unsigned long long mask = __ballot(mem);
            if (census) nbad += __popcll(__ballot(valid && (lab[ch] < lo || lab[ch] >= hi)));
            if (mem) list[n + __popcll(mask & below)] = ch * 64 + lane;
            n += __popcll(mask);
        }
        cnt += n;
        __syncthreads();                                                       // (one wave: orders the list's writes and reads)
        for (int j = 0; j < n; j += KM_BATCH) {                                // ascending row index, KM_BATCH rows in flight
            float v[KM_BATCH];
#pragma unroll
            for (int u = 0; u < KM_BATCH; ++u) {
                const int r = __builtin_amdgcn_readfirstlane(list[j + u < n ? j + u : n - 1]);
                v[u] = xc[(w0 + r) * p.ldx];
            }
#pragma unroll
            for (int u = 0; u < KM_BATCH; ++u)
                if (j + u < n) {
                    sum += (double)v[u];
                    const double d = (double)v[u] - (double)cold;
                    ine = fma(d, d, ine);
                }
        }
        __syncthreads();                                                       // before the next window's list
    }
    if (live) p.sums[(int64_t)k * p.D + col] = sum;
    else ine = 0.0;
    ine = tree_sum(ine);
    if (lane == 0) {
        p.scratch[blockIdx.x] = ine;
        if (slab == 0) p.counts[k] = cnt;
        if (census) p.scratch[(int64_t)p.K * nslab] = (double)nbad;
    }
}

__global__ __launch_bounds__(256) void kmeans_finish_kernel(hsimae_kmeans_update_params p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = p.D, K = p.K;
    if (blockIdx.x + 1 < gridDim.x) {
        const int k = blockIdx.x * 4 + wave;                                   // wave-uniform
        if (k >= K) return;
        const int64_t cnt = p.counts[k];
        if (cnt == 0) return;                                                  // an empty cluster keeps centroid and bias
        float* c = p.c + (int64_t)k * p.ldc;
        const double* sum = p.sums + (int64_t)k * D;
        const double n = (double)cnt;
        for (int d = lane; d < D; d += 64) c[d] = (float)(sum[d] / n);
        if (p.normalize) {                                                     // in place: a lane re-reads only what it wrote
            float norm;
            const float rn = row_inv_norm(c, D, lane, norm);
            for (int d = lane; d < D; d += 64) c[d] = c[d] * rn;
        }
        if (p.bias) {
            double ss = 0.0;
            for (int d = lane; d < D; d += 64) ss = fma((double)c[d], (double)c[d], ss);
            ss = tree_sum(ss);
            if (lane == 0) p.bias[k] = (float)(0.5 * ss);
        }
        return;
    }
    if (wave) return;                                                          // the state block: one wave
    const int parts = K * slabs_of(D);
    double ine = 0.0;
    for (int g = lane; g < parts; g += 64) ine += p.scratch[g];
    ine = tree_sum(ine);
    long long changed = 0, empty = 0;
    if (p.changed) for (int g = lane; g < HSIMAE_KMEANS_GRID; g += 64) changed += p.changed[g];
    for (int k = lane; k < K; k += 64) empty += p.counts[k] == 0;
    wave_tree<TreeAdd>(changed, empty);
    if (lane == 0) {
        p.state[0] = ine;
        p.state[1] = (double)changed;
        p.state[2] = p.state[2] + (changed > 0 ? 1.0 : 0.0);
        p.state[3] = (double)empty;
        p.state[4] = p.scratch[parts];
        p.state[5] = p.state[6] = p.state[7] = 0.0;
    }
}

}  // namespace

int hs_kmeans_assign(const hsimae_kmeans_assign_params& p, hipStream_t s) {
    if (p.N < 0 || p.K < 1 || p.D <= 0 || p.D % 4 || p.first < 0 || p.ldx < p.D || p.ldc < p.D || p.H <= 0 || p.W <= 0) return HS_EDIMS;
    if (p.K > KM_MAXK || p.D > 4096) return HS_EUNSUPPORTED;
    if (p.N > 0 && (!p.x || !p.c || !p.labels)) return HS_ENULL;
    if (misaligned(p.x, 15) || misaligned(p.c, 15) || p.ldx % 4 || p.ldc % 4 || misaligned(p.bias, 3) || misaligned(p.pixels, 7) ||
        misaligned(p.labels, 7) || misaligned(p.score, 3) || misaligned(p.margin, 3) || misaligned(p.changed, 3)) return HS_EALIGN;
    if (p.N == 0) return HS_OK;
    const int64_t tiles = ((int64_t)p.N + TQ - 1) / TQ;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)(tiles < HSIMAE_KMEANS_GRID ? tiles : HSIMAE_KMEANS_GRID)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_kmeans_update(const hsimae_kmeans_update_params& p, hipStream_t s) {
    if (p.N < 0 || p.K < 1 || p.D <= 0 || p.D % 4 || p.first < 0 || p.ldx < p.D || p.ldc < p.D) return HS_EDIMS;
    if (p.K > KM_MAXK || p.D > 4096) return HS_EUNSUPPORTED;
    if (p.N > 0 && (!p.x || !p.labels || !p.c || !p.counts || !p.sums || !p.scratch || !p.state)) return HS_ENULL;
    if (misaligned(p.x, 15) || misaligned(p.c, 15) || p.ldx % 4 || p.ldc % 4 || misaligned(p.labels, 7) || misaligned(p.bias, 3) ||
        misaligned(p.counts, 7) || misaligned(p.sums, 7) || misaligned(p.changed, 3) || misaligned(p.scratch, 7) ||
        misaligned(p.state, 7)) return HS_EALIGN;
    if (p.N == 0) return HS_OK;
    hipLaunchKernelGGL(kmeans_sums_kernel, dim3((unsigned)(p.K * ((p.D + 63) / 64))), dim3(64), 0, s, p);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)((p.K + 3) / 4 + 1)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(kmeans)
