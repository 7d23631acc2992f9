// Superpixels and object-level class maps (hsimae_slic, hsimae_segment_vote; include/hsimae_hip.h): SLIC (Achanta et al., TPAMI
// 2012) in gSLIC's gather form (Ren and Reid 2011) over a scene's guide image, and the vote of every superpixel over the class
// probabilities of its pixels.  The definition (grid, initial centres, distance, tie and NaN rules, the order of every sum) is
// stated in the header and restated in fp64 in tests/slic_ref.py.
//
//   slic_init_kernel     one lane per centre: the grid centres (no gradient perturbation).
//   slic_round_kernel    one workgroup per centre k, a stride loop where there are more centres than workgroups.  The old centres
//                        of the 5 x 5 cells around k are staged in LDS; the 256 lanes walk the pixels of k's region (the pixels
//                        whose home cell is one of the 3 x 3 around k: at most 96 x 96, 24 x 24 at size 8), recompute each
//                        pixel's nine-candidate argmin (slic_nearest, the ONE place a winner is decided) and leave a byte per
//                        pixel in LDS: "k won it".  Then one lane per scene row adds the members' features and coordinates in
//                        fp64 along ascending x, and one lane per output slot adds the row partials in ascending y: the fixed
//                        order numpy repeats bit for bit.  The mean is divided once in fp64 and rounded to fp32 once; a centre
//                        without a pixel keeps its bits.  A round reads one centre buffer and writes the other: one launch per
//                        round, no label round trip, at the price of nine distance evaluations per pixel and centre.
//                        The FINAL pass is the same kernel instantiated with FINAL = true: a pixel's label and distance are written by the
//                        workgroup of the centre that won it (every pixel has exactly one), the integer member count is the
//                        centre's `counts` entry, and no centre moves.
//   segment_vote_kernel  one workgroup per segment over the same region: the index of the row of `probs` behind every member pixel
//                        is staged in LDS, the class sums follow in slabs of 8 classes in the same fixed order (mode 0), or every classified
//                        member's own argmax is counted per class (mode 1: integer counts, exact in any order).  Wave 0 takes the
//                        argmax and the runner-up of the segment's vector (row_wave.h), and the workgroup writes the three maps.
//
// No atomics, no grid-wide barrier, no host wait: every output element has one writer, two runs are bit-identical.
// LDS: 96 * 8 doubles + 96 ints, + the 25 staged centres and one byte per region pixel (slic: 8 KB at size 8, 16 KB at size 32),
// + the segment's vector and one int per region pixel (vote: 9 KB at size 8 and 17 columns, at most 48 KB).  These are latency-bound kernels of a few lanes per scene row; what bounds a
// round is written down with its measurement in profiles/EXPERIMENTS.md.
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int SLIC_MAXG = 4;
constexpr int SLIC_MINS = 2, SLIC_MAXS = 32;
constexpr int SLIC_MAXR = 3 * SLIC_MAXS;       // rows (and columns) of a region at most
constexpr int SLIC_GRID = 4096;                // workgroups at most: the kernels stride over the rest of the centres
constexpr int SLIC_SLAB = 8;                   // classes per slab of the vote: the fp64 accumulators a lane holds
constexpr int SLIC_MAXC = 1024;
constexpr int SLIC_CW = 8;                     // floats per centre: G features, y, x, pad

struct SlicGrid { int H, W, ny, nx, K, R3; };          // R3 = 3 size: the rows (columns) of a region at most
inline SlicGrid slic_grid(int H, int W, int S) {
    const int ny = (H + S - 1) / S, nx = (W + S - 1) / S;
    return {H, W, ny, nx, ny * nx, 3 * S};
}

// the home cell of coordinate v along an axis of L pixels and n cells, and the first coordinate whose home cell is c
__device__ __forceinline__ int home_cell(int v, int n, int L) { return (int)((int64_t)v * n / L); }
__device__ __forceinline__ int cell_lo(int c, int n, int L) { return (int)(((int64_t)c * L + n - 1) / n); }

// the pixels whose home cell is one of the 3 x 3 around cell (i, j): rows [y0, y0 + rh), columns [x0, x0 + rw).  A cell has at most
// ceil(H / ny) <= size rows, so rh, rw <= 3 size: the LDS of both kernels is sized for that, and the min() keeps it so
struct Region { int y0, x0, rh, rw; };
__device__ __forceinline__ Region region_of(int i, int j, const SlicGrid& g) {
    Region r;
    r.y0 = cell_lo(i > 0 ? i - 1 : 0, g.ny, g.H);
    r.x0 = cell_lo(j > 0 ? j - 1 : 0, g.nx, g.W);
    r.rh = min(cell_lo(min(i + 2, g.ny), g.ny, g.H) - r.y0, g.R3);
    r.rw = min(cell_lo(min(j + 2, g.nx), g.nx, g.W) - r.x0, g.R3);
    return r;
}

// a pixel's scaled guide values: fl(scale_g * I_g), the features a centre averages
__device__ __forceinline__ void slic_features(const float* guide, const float* sc, int G, int64_t pix, float* v) {
#pragma unroll
    for (int q = 0; q < SLIC_MAXG; ++q) v[q] = q < G ? __fmul_rn(sc[q], guide[pix * G + q]) : 0.f;
}

// The winner among the centres of the 3 x 3 cells around the pixel's home cell (hi, hj), in ascending centre index; cells outside
// the grid are left out.  A smaller distance wins, a tie stays with the lower index, a NaN distance loses to every number, and
// when all are NaN the home cell's centre wins with distance NaN.  Centre (ci, cj) lies at cen + ((ci - oi) * pitch + cj - oj) * 8.
struct SlicWin { int k; float d; };
__device__ __forceinline__ SlicWin slic_nearest(const float* v, int G, int y, int x, int hi, int hj, const SlicGrid& g, float w,
                                                const float* cen, int oi, int oj, int pitch) {
    SlicWin best{hi * g.nx + hj, __builtin_nanf("")};
    const float fy = (float)y, fx = (float)x;
    for (int ci = hi - 1; ci <= hi + 1; ++ci) {
        if (ci < 0 || ci >= g.ny) continue;
        for (int cj = hj - 1; cj <= hj + 1; ++cj) {
            if (cj < 0 || cj >= g.nx) continue;
            const float* c = cen + ((ci - oi) * pitch + cj - oj) * SLIC_CW;
            float d = 0.f;
#pragma unroll
            for (int q = 0; q < SLIC_MAXG; ++q)
                if (q < G) {
                    const float t = v[q] - c[q];
                    d = fmaf(t, t, d);
                }
            const float dy = fy - c[G], dx = fx - c[G + 1];
            const float s = fmaf(dx, dx, __fmul_rn(dy, dy));
            d = fmaf(w, s, d);
            if (!__builtin_isnan(d) && (__builtin_isnan(best.d) || d < best.d)) best = SlicWin{ci * g.nx + cj, d};
        }
    }
    return best;
}

__global__ __launch_bounds__(256) void slic_init_kernel(hsimae_slic_params p, SlicGrid g) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= g.K) return;
    const int i = k / g.nx, j = k - i * g.nx;
    const int y = (int)((int64_t)(2 * i + 1) * g.H / (2 * g.ny)), x = (int)((int64_t)(2 * j + 1) * g.W / (2 * g.nx));
    float v[SLIC_MAXG], sc[SLIC_MAXG];
    for (int q = 0; q < SLIC_MAXG; ++q) sc[q] = q < p.G ? p.guide_scale[q] : 0.f;
    slic_features(p.guide, sc, p.G, (int64_t)y * g.W + x, v);
    float* c = p.centres + (int64_t)k * SLIC_CW;
    for (int q = 0; q < SLIC_CW; ++q) c[q] = q < p.G ? v[q] : q == p.G ? (float)y : q == p.G + 1 ? (float)x : 0.f;
}

template <bool FINAL>
__global__ __launch_bounds__(256) void slic_round_kernel(hsimae_slic_params p, SlicGrid g, const float* cin, float* cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* part = reinterpret_cast<double*>(smem);                          // [SLIC_MAXR][8]: a scene row's sums
    int* rcnt = reinterpret_cast<int*>(part + SLIC_MAXR * 8);                // [SLIC_MAXR]: its member count
    float* cen = reinterpret_cast<float*>(rcnt + SLIC_MAXR);                 // [5 x 5][8]: the old centres around k
    unsigned char* mine = reinterpret_cast<unsigned char*>(cen + 25 * SLIC_CW);      // [rh rw]: 1 where k won the pixel
    const int tid = threadIdx.x, G = p.G;
    float sc[SLIC_MAXG];
#pragma unroll
    for (int q = 0; q < SLIC_MAXG; ++q) sc[q] = q < G ? p.guide_scale[q] : 0.f;

    for (int k = blockIdx.x; k < g.K; k += gridDim.x) {                      // workgroup-uniform
        const int i = k / g.nx, j = k - i * g.nx;
        const Region r = region_of(i, j, g);
        if (tid < 25 * SLIC_CW) {
            const int cell = tid >> 3, ci = i - 2 + cell / 5, cj = j - 2 + cell % 5;
            cen[tid] = ci >= 0 && ci < g.ny && cj >= 0 && cj < g.nx ? cin[((int64_t)ci * g.nx + cj) * SLIC_CW + (tid & 7)] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < r.rh * r.rw; e += 256) {
            const int ry = e / r.rw, y = r.y0 + ry, x = r.x0 + e - ry * r.rw;
            const int64_t pix = (int64_t)y * g.W + x;                        // H W < 2^31
            float v[SLIC_MAXG];
            slic_features(p.guide, sc, G, pix, v);
            const SlicWin win = slic_nearest(v, G, y, x, home_cell(y, g.ny, g.H), home_cell(x, g.nx, g.W), g, p.w, cen, i - 2, j - 2, 5);
            mine[e] = win.k == k;
            if (FINAL && win.k == k) {
                p.labels[pix] = k;
                if (p.dist) p.dist[pix] = win.d;
            }
        }
        __syncthreads();
        if (tid < r.rh) {                                                    // one ascending-x chain per scene row
            double a0 = 0, a1 = 0, a2 = 0, a3 = 0, ay = 0, ax = 0;
            int n = 0;
            const int y = r.y0 + tid;
            for (int rx = 0; rx < r.rw; ++rx) {
                if (!mine[tid * r.rw + rx]) continue;
                ++n;
                if (FINAL) continue;
                float v[SLIC_MAXG];
                slic_features(p.guide, sc, G, (int64_t)y * g.W + r.x0 + rx, v);
                a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
                ay += (double)y; ax += (double)(r.x0 + rx);
            }
            double* o = part + tid * 8;
            o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = ay; o[5] = ax;
            rcnt[tid] = n;
        }
        __syncthreads();
        if (tid < SLIC_CW) {                                                 // the row partials in ascending y, one lane per slot
            const int slot = tid < G ? tid : tid == G ? 4 : 5;
            double s = 0;
            int n = 0;
            for (int ry = 0; ry < r.rh; ++ry) { s += part[ry * 8 + slot]; n += rcnt[ry]; }
            const float old = cen[12 * SLIC_CW + tid];                       // centre k itself
            if (FINAL) {
                if (cout) cout[(int64_t)k * SLIC_CW + tid] = old;            // the result ends in the first buffer
                if (tid == 0 && p.counts) p.counts[k] = n;
            } else {
                cout[(int64_t)k * SLIC_CW + tid] = n > 0 && tid < G + 2 ? (float)(s / (double)n) : old;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void segment_vote_kernel(hsimae_segment_vote_params p, SlicGrid g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* part = reinterpret_cast<double*>(smem);                          // [SLIC_MAXR][8]
    int* rcnt = reinterpret_cast<int*>(part + SLIC_MAXR * SLIC_SLAB);        // [SLIC_MAXR]
    float* vec = reinterpret_cast<float*>(rcnt + SLIC_MAXR);                 // [C]: the segment's vector
    float* res = vec + p.C;                                                  // label (as bits), its value, the runner-up
    int* rowi = reinterpret_cast<int*>(res + 4);                             // [rh rw]: -1 not in k, -2 in k without a row, else the row
    const int tid = threadIdx.x, C = p.C, first = p.first;

    for (int k = blockIdx.x; k < g.K; k += gridDim.x) {                      // workgroup-uniform
        const int i = k / g.nx, j = k - i * g.nx;
        const Region r = region_of(i, j, g);
        const int np = r.rh * r.rw;
        for (int e = tid; e < np; e += 256) {
            const int ry = e / r.rw;
            const int64_t pix = (int64_t)(r.y0 + ry) * g.W + r.x0 + e - ry * r.rw;
            int row = -1;
            if (p.labels[pix] == k) {
                row = p.row_of ? p.row_of[pix] : (int)pix;
                if (row < 0 || row >= p.n) row = -2;                         // never a read past probs' n rows
            }
            rowi[e] = row;
        }
        __syncthreads();
        if (tid < r.rh) {
            int n = 0;
            for (int rx = 0; rx < r.rw; ++rx) n += rowi[tid * r.rw + rx] >= 0;
            rcnt[tid] = n;
        }
        __syncthreads();
        int cnt = 0;
        for (int ry = 0; ry < r.rh; ++ry) cnt += rcnt[ry];
        if (tid == 0 && p.seg_count) p.seg_count[k] = cnt;
        if (cnt == 0) { __syncthreads(); continue; }                         // no classified pixel: nothing else is written

        if (p.mode == 0) {
            for (int c0 = first; c0 < C; c0 += SLIC_SLAB) {
                const int nc = C - c0 < SLIC_SLAB ? C - c0 : SLIC_SLAB;
                if (tid < r.rh) {                                            // one ascending-x chain per scene row and class
                    double acc[SLIC_SLAB];
#pragma unroll
                    for (int q = 0; q < SLIC_SLAB; ++q) acc[q] = 0;
                    for (int rx = 0; rx < r.rw; ++rx) {
                        const int row = rowi[tid * r.rw + rx];
                        if (row < 0) continue;
                        const float* pr = p.probs + (int64_t)row * p.ldp + c0;
#pragma unroll
                        for (int q = 0; q < SLIC_SLAB; ++q)
                            if (q < nc) acc[q] += (double)pr[q];
                    }
#pragma unroll
                    for (int q = 0; q < SLIC_SLAB; ++q) part[tid * SLIC_SLAB + q] = acc[q];
                }
                __syncthreads();
                if (tid < nc) {                                              // the row partials in ascending y
                    double s = 0;
                    for (int ry = 0; ry < r.rh; ++ry) s += part[ry * SLIC_SLAB + tid];
                    vec[c0 + tid] = (float)(s / (double)cnt);
                }
                __syncthreads();
            }
        } else {
            for (int e = tid; e < np; e += 256) {                            // a classified member's own argmax, first on ties
                const int row = rowi[e];
                if (row < 0) continue;
                const float* pr = p.probs + (int64_t)row * p.ldp;
                float key = -__builtin_inff();
                int best = 0x7fffffff;
                for (int c = first; c < C; ++c) arg_better(key, best, pr[c], c);
                rowi[e] = best;                                              // >= first >= 0: still "classified"
            }
            __syncthreads();
            for (int c = first + tid; c < C; c += 256) {
                int m = 0;
                for (int e = 0; e < np; ++e) m += rowi[e] == c;
                vec[c] = (float)((double)m / (double)cnt);
            }
            __syncthreads();
        }

        if (tid < 64) {                                                      // wave 0: the argmax of the vector and its runner-up
            float key = -__builtin_inff();
            int best = 0x7fffffff;
            for (int c = first + tid; c < C; c += 64) arg_better(key, best, vec[c], c);
            wave_argmax(key, best);
            const float second = row_runner_up(vec, 1.f, first, C, tid, best);
            if (tid == 0) { res[0] = __builtin_bit_cast(float, best); res[1] = key; res[2] = second; }
        }
        __syncthreads();
        const int best = __builtin_bit_cast(int, res[0]);
        const float key = res[1], second = res[2];
        for (int e = tid; e < np; e += 256) {
            const int row = rowi[e];
            if (row >= 0 || (row == -2 && p.fill)) {
                const int ry = e / r.rw;
                write_maps(p.label_map, p.conf_map, p.margin_map, (int64_t)(r.y0 + ry) * g.W + r.x0 + e - ry * r.rw, best, key, second,
                           C - first == 1);
            }
        }
        if (p.out_probs)
            for (int c = tid; c < C; c += 256) p.out_probs[(int64_t)k * p.ldo + c] = c < first ? 0.f : vec[c];
        __syncthreads();
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return a && b && x < y + nb && y < x + na;
}

}  // namespace

int hs_slic(const hsimae_slic_params& p, hipStream_t s) {
    if (p.H <= 0 || p.W <= 0 || (int64_t)p.H * p.W >= (int64_t)1 << 31 || p.G < 1 || p.G > SLIC_MAXG || p.size < SLIC_MINS ||
        p.size > SLIC_MAXS || p.rounds < 0 || (p.init != 0 && p.init != 1) || !(p.w >= 0.f) || __builtin_isinf(p.w)) return HS_EDIMS;
    if (!p.guide || !p.guide_scale || !p.centres || !p.labels || (p.rounds > 0 && !p.centres_tmp)) return HS_ENULL;
    if (misaligned(p.guide, 3) || misaligned(p.guide_scale, 3) || misaligned(p.centres, 3) || misaligned(p.centres_tmp, 3) ||
        misaligned(p.counts, 3) || misaligned(p.labels, 3) || misaligned(p.dist, 3)) return HS_EALIGN;
    const SlicGrid g = slic_grid(p.H, p.W, p.size);
    const size_t hw = (size_t)p.H * p.W, cb = (size_t)g.K * SLIC_CW * 4;
    const void* outs[5] = {p.centres, p.centres_tmp, p.counts, p.labels, p.dist};
    const size_t nout[5] = {cb, cb, (size_t)g.K * 4, hw * 4, hw * 4};
    for (int a = 0; a < 5; ++a) {                                            // no output over an input or over another output
        if (overlap(outs[a], nout[a], p.guide, hw * p.G * 4) || overlap(outs[a], nout[a], p.guide_scale, (size_t)p.G * 4)) return HS_EDIMS;
        for (int b = a + 1; b < 5; ++b)
            if (overlap(outs[a], nout[a], outs[b], nout[b])) return HS_EDIMS;
    }
    if (p.init) hipLaunchKernelGGL(slic_init_kernel, dim3((g.K + 255) / 256), dim3(256), 0, s, p, g);
    const int region = 3 * p.size;
    const size_t lds = SLIC_MAXR * 8 * sizeof(double) + SLIC_MAXR * 4 + 25 * SLIC_CW * 4 + (size_t)((region * region + 15) & ~15);
    const unsigned grid = g.K < SLIC_GRID ? g.K : SLIC_GRID;
    float* buf[2] = {p.centres, p.centres_tmp};
    for (int t = 0; t < p.rounds; ++t)
        hipLaunchKernelGGL(slic_round_kernel<false>, dim3(grid), dim3(256), lds, s, p, g, (const float*)buf[t & 1], buf[(t + 1) & 1]);
    hipLaunchKernelGGL(slic_round_kernel<true>, dim3(grid), dim3(256), lds, s, p, g, (const float*)buf[p.rounds & 1],
                       (p.rounds & 1) ? p.centres : (float*)nullptr);
    return (int)hipGetLastError();
}

int hs_segment_vote(const hsimae_segment_vote_params& p, hipStream_t s) {
    if (p.H <= 0 || p.W <= 0 || (int64_t)p.H * p.W >= (int64_t)1 << 31 || p.n < 0 || p.C < 2 || p.first < 0 || p.first >= p.C ||
        p.ldp < p.C || (p.out_probs && p.ldo < p.C) || p.size < SLIC_MINS || p.size > SLIC_MAXS || (p.mode != 0 && p.mode != 1) ||
        (p.fill != 0 && p.fill != 1)) return HS_EDIMS;
    if (p.C > SLIC_MAXC) return HS_EUNSUPPORTED;
    if (!p.probs || !p.labels || !p.label_map) return HS_ENULL;
    if (misaligned(p.probs, 3) || misaligned(p.row_of, 3) || misaligned(p.labels, 3) || misaligned(p.out_probs, 3) ||
        misaligned(p.seg_count, 3) || misaligned(p.conf_map, 3) || misaligned(p.margin_map, 3) || misaligned(p.label_map, 7))
        return HS_EALIGN;
    const SlicGrid g = slic_grid(p.H, p.W, p.size);
    const size_t hw = (size_t)p.H * p.W, np = p.n > 0 ? ((size_t)(p.n - 1) * p.ldp + p.C) * 4 : 0;
    const void* outs[5] = {p.out_probs, p.seg_count, p.label_map, p.conf_map, p.margin_map};
    const size_t nout[5] = {((size_t)(g.K - 1) * p.ldo + p.C) * 4, (size_t)g.K * 4, hw * 8, hw * 4, hw * 4};
    for (int a = 0; a < 5; ++a) {
        if (overlap(outs[a], nout[a], p.probs, np) || overlap(outs[a], nout[a], p.labels, hw * 4) ||
            overlap(outs[a], nout[a], p.row_of, hw * 4)) return HS_EDIMS;
        for (int b = a + 1; b < 5; ++b)
            if (overlap(outs[a], nout[a], outs[b], nout[b])) return HS_EDIMS;
    }
    const int region = 3 * p.size;
    const size_t lds = SLIC_MAXR * SLIC_SLAB * sizeof(double) + SLIC_MAXR * 4 + ((size_t)p.C + 4) * 4 + (size_t)region * region * 4;
    hipLaunchKernelGGL(segment_vote_kernel, dim3(g.K < SLIC_GRID ? g.K : SLIC_GRID), dim3(256), lds, s, p, g);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(slic)
