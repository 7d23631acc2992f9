// Edge-preserving smoothing of a scene's class-probability maps before the argmax (hsimae_prob_filter, include/hsimae_hip.h):
// the joint bilateral filter of Kang, Li and Benediktsson (EPF, IEEE TGRS 2014) with a guide image taken from the scene, over
// all class planes in one launch, and from the filtered probabilities the products of hsimae_class_prob: label, confidence,
// margin and (optionally) the probabilities themselves.
//
//   prob_filter_kernel   one workgroup per 16 x 16 tile of output pixels, one lane per pixel, a 2-D grid of tiles.  The tile and
//                        its halo, S x S pixels with S = 16 + 2 radius <= 32, are staged in LDS once: the row of `probs` behind
//                        every pixel (-1: outside the scene or without a row) and its guide values.  The probabilities follow in
//                        slabs of at most 16 classes as class-major planes [class][halo pixel]; a lane keeps the slab's 16
//                        accumulators and the weight sum in registers and forms each tap's weight once per slab (once per tap
//                        when C - first <= 16).  The sequence of every sum is the contract tests/smooth_ref.py restates.
//
// LDS banks.  ds_read_b32 serves a wave in two groups of 32 lanes, bank = word address mod 32.  A pixel-major slab
// [halo pixel][16 classes] would put the 32 lanes of a group 16 words apart: two banks, a 16-way conflict on the read that the
// tap loop issues 16 times per tap.  With class-major planes the 16 lanes of one tile row read 16 neighbouring words, and the
// two tile rows of a group lie k SP words apart (SP = the row stride of a plane).  They share no bank exactly when
// k SP = 16 (mod 32), so the lane -> pixel map pairs the tile rows y and y + k in one group, with k chosen per radius:
// S = 18, 22, 26, 30 (radius odd): k = 8;  S = 20, 28: k = 4;  S = 24: k = 2;  S = 32 (radius 8): SP = 34 and k = 8.  A tap
// moves both rows by the same offset, so this holds at every tap.  (The slab's staging stores do conflict: consecutive lanes
// write `plane` words apart so that their global reads are 64 contiguous bytes of one row.  There are 16 S^2 / 64 of them per
// slab against 16 (2 radius + 1)^2 x 4 reads.)
//
// LDS: (1 + G + 16) planes of SP x S words: 35 KB at the default radius 3 with one guide channel and 41 KB with four (three to
// four workgroups per CU), 78 to 91 KB at radius 8 (two, one).  No atomics, a pixel is written by one lane: two runs are bit-identical.
// A latency- and LDS-bound kernel: a 610 x 340 scene with 16 classes at radius 3 is 858 workgroups, about 0.4 GFLOP on 14 MB,
// and what a lane waits for is its 18 LDS reads per tap.  No roofline applies and none is claimed.
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int SMOOTH_MAXC = 1024;
constexpr int SMOOTH_MAXR = 8;
constexpr int SMOOTH_MAXG = 4;
constexpr int SMOOTH_SLAB = 16;         // classes per slab: the accumulators a lane holds
constexpr int SMOOTH_TILE = 16;
constexpr int SMOOTH_MAXTILES = 65535;  // per grid dimension

// row stride of a plane and log2 of the tile-row pairing k (see "LDS banks" above)
struct SmoothLayout { int SP, kshift; };
inline SmoothLayout smooth_layout(int radius) {
    const int S = SMOOTH_TILE + 2 * radius, SP = S == 32 ? 34 : S;
    for (int ks = 3; ks >= 1; --ks)
        if (((SP << ks) & 31) == 16) return {SP, ks};
    return {SP, 0};
}

__global__ __launch_bounds__(256) void prob_filter_kernel(hsimae_prob_filter_params p, int SP, int kshift) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int r = p.radius, S = SMOOTH_TILE + 2 * r, plane = SP * S, G = p.G, C = p.C, first = p.first;
    const bool ranged = p.a_r != 0.f;
    int* rows = reinterpret_cast<int*>(smem);                       // [plane]
    float* gd = reinterpret_cast<float*>(smem) + plane;             // [G][plane], absent without the range term
    float* slab = gd + (ranged ? G : 0) * plane;                    // [<= 16][plane]
    const int tid = threadIdx.x, ty0 = blockIdx.y * SMOOTH_TILE, tx0 = blockIdx.x * SMOOTH_TILE;

    // the halo's rows and guide values: 8 halo rows of up to 32 pixels per pass
    for (int hy = tid >> 5; hy < S; hy += 8) {
        const int hx = tid & 31, gy = ty0 - r + hy, gx = tx0 - r + hx;
        if (hx >= S) continue;
        int row = -1, pix = 0;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
            pix = gy * p.W + gx;                                    // H W < 2^31
            row = p.row_of ? p.row_of[pix] : pix;
            if (row >= p.n) row = -1;                               // never a read past probs' n rows
        }
        rows[hy * SP + hx] = row;
        if (ranged && row >= 0)
            for (int g = 0; g < G; ++g) gd[g * plane + hy * SP + hx] = p.guide[(int64_t)pix * G + g];
    }
    __syncthreads();

    // lane -> pixel: 16 lanes along x; the tile rows y and y + (1 << kshift) share a group of 32 lanes
    const int x = tid & 15, q = tid >> 4, t = q >> 1, lowmask = (1 << kshift) - 1;
    const int y = ((t >> kshift) << (kshift + 1)) | ((q & 1) << kshift) | (t & lowmask);
    const int gy = ty0 + y, gx = tx0 + x, centre = (y + r) * SP + x + r;
    const int myrow = gy < p.H && gx < p.W ? rows[centre] : -1;
    const bool active = myrow >= 0;
    float gi[SMOOTH_MAXG] = {0.f, 0.f, 0.f, 0.f}, sc[SMOOTH_MAXG] = {0.f, 0.f, 0.f, 0.f};
    if (ranged && active) {
#pragma unroll
        for (int g = 0; g < SMOOTH_MAXG; ++g)
            if (g < G) { gi[g] = gd[g * plane + centre]; sc[g] = p.guide_scale[g]; }
    }
    float* out = p.out_probs && active ? p.out_probs + (int64_t)myrow * p.ldo : nullptr;
    if (out) for (int c = 0; c < first; ++c) out[c] = 0.f;

    float key = -__builtin_inff(), second = -__builtin_inff();
    int best = 0x7fffffff;
    for (int c0 = first; c0 < C; c0 += SMOOTH_SLAB) {                                               // workgroup-uniform
        const int nc = C - c0 < SMOOTH_SLAB ? C - c0 : SMOOTH_SLAB;
        if (c0 != first) __syncthreads();                           // every lane is done with the slab before
        for (int hy = 0; hy < S; ++hy)
            for (int e = tid; e < S * SMOOTH_SLAB; e += 256) {      // 16 lanes read 64 contiguous bytes of one row
                const int hx = e >> 4, k = e & 15, row = rows[hy * SP + hx];
                if (k < nc && row >= 0) slab[k * plane + hy * SP + hx] = p.probs[(int64_t)row * p.ldp + c0 + k];
            }
        __syncthreads();
        if (!active) continue;
        float acc[SMOOTH_SLAB], wsum = 0.f;
#pragma unroll
        for (int k = 0; k < SMOOTH_SLAB; ++k) acc[k] = 0.f;
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) {
                const int h = centre + dy * SP + dx;
                if (rows[h] < 0) continue;                          // outside the scene or without a row: never read
                float arg = p.a_s * (float)(dy * dy + dx * dx);
                if (ranged) {
                    float d2 = 0.f;
#pragma unroll
                    for (int g = 0; g < SMOOTH_MAXG; ++g)
                        if (g < G) {
                            const float d = (gd[g * plane + h] - gi[g]) * sc[g];
                            d2 = fmaf(d, d, d2);
                        }
                    arg = fmaf(p.a_r, d2, arg);
                }
                const float w = __builtin_amdgcn_exp2f(-arg);       // exactly 1 at the centre
                wsum += w;
#pragma unroll
                for (int k = 0; k < SMOOTH_SLAB; ++k)
                    if (k < nc) acc[k] = fmaf(w, slab[k * plane + h], acc[k]);
            }
        const float inv = 1.f / wsum;                               // wsum >= 1: the centre tap
#pragma unroll
        for (int k = 0; k < SMOOTH_SLAB; ++k)
            if (k < nc) {                                           // ascending c: first of a tie stays
                const float v = acc[k] * inv;
                if (out) out[c0 + k] = v;
                const int was = best;
                const float old = key;
                arg_better(key, best, v, c0 + k);
                if (best == was) second = fmaxf(second, v);
                else if (was != 0x7fffffff) second = fmaxf(second, old);
            }
    }
    if (active) write_maps(p.label_map, p.conf_map, p.margin_map, (int64_t)gy * p.W + gx, best, key, second, C - first == 1);
}

}  // namespace

int hs_prob_filter(const hsimae_prob_filter_params& p, hipStream_t s) {
    if (p.H <= 0 || p.W <= 0 || p.n < 0 || p.C < 2 || p.first < 0 || p.first >= p.C || p.ldp < p.C || (p.out_probs && p.ldo < p.C) ||
        p.G < 1 || p.G > SMOOTH_MAXG || p.radius < 1 || p.radius > SMOOTH_MAXR || (int64_t)p.H * p.W >= (int64_t)1 << 31 ||
        !(p.a_s >= 0.f) || !(p.a_r >= 0.f) || __builtin_isinf(p.a_s) || __builtin_isinf(p.a_r)) return HS_EDIMS;
    const int tx = (p.W + SMOOTH_TILE - 1) / SMOOTH_TILE, ty = (p.H + SMOOTH_TILE - 1) / SMOOTH_TILE;
    if (p.C > SMOOTH_MAXC || tx > SMOOTH_MAXTILES || ty > SMOOTH_MAXTILES) return HS_EUNSUPPORTED;
    const bool ranged = p.a_r != 0.f;
    if (!p.probs || !p.label_map || (ranged && (!p.guide || !p.guide_scale))) return HS_ENULL;
    if (misaligned(p.probs, 3) || misaligned(p.row_of, 3) || misaligned(p.guide, 3) || misaligned(p.guide_scale, 3) ||
        misaligned(p.out_probs, 3) || misaligned(p.conf_map, 3) || misaligned(p.margin_map, 3) || misaligned(p.label_map, 7))
        return HS_EALIGN;
    if (p.out_probs && p.n > 0) {                                   // a tap reads its neighbours' rows: in place would be wrong
        const uintptr_t a = reinterpret_cast<uintptr_t>(p.probs), b = reinterpret_cast<uintptr_t>(p.out_probs);
        const uintptr_t na = ((uintptr_t)(p.n - 1) * p.ldp + p.C) * 4, nb = ((uintptr_t)(p.n - 1) * p.ldo + p.C) * 4;
        if (a < b + nb && b < a + na) return HS_EDIMS;
    }
    if (p.n == 0) return HS_OK;                                     // no pixel has a row: nothing is written
    const SmoothLayout L = smooth_layout(p.radius);
    const int S = SMOOTH_TILE + 2 * p.radius, K = p.C - p.first;
    const size_t lds = (size_t)L.SP * S * (1 + (ranged ? p.G : 0) + (K < SMOOTH_SLAB ? K : SMOOTH_SLAB)) * 4;
    // common.h's hs_launch_lds opts a kernel in to the size of its FIRST launch; this kernel's size changes with the radius,
    // the guide and the class count of every call, so it is opted in once to the largest of them (radius 8, G = 4: 91 KB)
    static bool max_lds_set = false;
    if (!max_lds_set) {
        const SmoothLayout M = smooth_layout(SMOOTH_MAXR);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prob_filter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  M.SP * (SMOOTH_TILE + 2 * SMOOTH_MAXR) * (1 + SMOOTH_MAXG + SMOOTH_SLAB) * 4);
        max_lds_set = true;
    }
    hipLaunchKernelGGL(prob_filter_kernel, dim3(tx, ty), dim3(256), lds, s, p, L.SP, L.kshift);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(smooth)
