// What the optimizer units (clip.hip, lamb.hip, ema.hip) share, each piece once: the group table and its staging into LDS, Adam's
// moments and AdamW's element, the fixed-order workgroup sum, and the launchers' checks and grids.  The grouped step, LAMB with
// every trust ratio 1 and hsimae_adamw_step_ctl are one arithmetic because they call the same functions here.
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

struct GroupTable { hsimae_adamw_group e[HSIMAE_ADAMW_MAX_GROUPS]; };            // by value in the launch: 512 bytes of kernarg
static_assert(sizeof(GroupTable) == 512, "the table travels as a kernel argument");

__device__ __forceinline__ double sq64(float x) { return (double)x * (double)x; }

// the table into LDS once per workgroup (64 lanes, one entry each); an element's id indexes it
__device__ __forceinline__ void stage_table(float2* tab, const GroupTable& table, int ngroups) {
    if (threadIdx.x < HSIMAE_ADAMW_MAX_GROUPS) {
        const int k = threadIdx.x < (unsigned)ngroups ? (int)threadIdx.x : 0;   // entries behind ngroups are never used
        tab[threadIdx.x] = make_float2(table.e[k].lr, table.e[k].weight_decay);
    }
    __syncthreads();
}

// Adam's two moments of the gradient scaled by coef (one fp32 multiply), in place
__device__ __forceinline__ void adam_moments(float g, float& m, float& v, float b1, float b2, float coef) {
    const float gc = g * coef;
    m = m + (gc - m) * (1.f - b1);                                               // lerp, as torch does it
    v = v * b2 + gc * gc * (1.f - b2);
}

// one element of torch.optim.AdamW with that element's own lr and weight decay (wd == 0 is "no decay": the multiply is left out)
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float lr, float wd, float b1, float b2, float eps,
                                          float inv_bc1, float inv_sqrt_bc2, float coef) {
    float x = p, mn = m, vn = v;
    if (wd != 0.f) x *= 1.f - lr * wd;
    adam_moments(g, mn, vn, b1, b2, coef);
    const float denom = sqrtf(vn) * inv_sqrt_bc2 + eps;
    p = x - lr * inv_bc1 * (mn / denom);
    m = mn; v = vn;
}

// floats in front of the first 16-byte boundary (0 .. 3); the caller clamps it to its length
__device__ __forceinline__ unsigned head_floats(const float* p) { return ((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2; }

// K sums over a workgroup of 256 in a fixed order, one per argument a (a thread's four accumulators, double[4]): per thread the four
// added pairwise, per wave the xor shuffle tree, the four waves in order.  Thread 0 writes out[0 .. K).
template <class... A>
__device__ __forceinline__ void block_sum(double* out, const A&... a) {
    constexpr int K = sizeof...(A);
    __shared__ double wsum[K][4];
    double s[K] = {((a[0] + a[1]) + (a[2] + a[3]))...};
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = tree_sum(s[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) wsum[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = ((wsum[k][0] + wsum[k][1]) + wsum[k][2]) + wsum[k][3];
    }
}

// ------------------------------------------------------------------ host side (misaligned(): row_wave.h)
// one id for all elements (no id array) must be a table index, or 2: frozen in any table
inline bool bad_group_uniform(const void* group, int group_uniform, int ngroups) {
    return !group && group_uniform != 2 && (group_uniform < 0 || group_uniform >= ngroups);
}

// table[0 .. ngroups) padded to the full kernel argument; HS_EDIMS for a negative or NaN value (entry 2 is never read: ignored)
inline int fill_group_table(GroupTable& t, const hsimae_adamw_group* table, int ngroups) {
    for (int k = 0; k < HSIMAE_ADAMW_MAX_GROUPS; ++k) {
        t.e[k] = k < ngroups ? table[k] : hsimae_adamw_group{0.f, 0.f};
        if (k != 2 && !(t.e[k].lr >= 0.f && t.e[k].weight_decay >= 0.f)) return HS_EDIMS;
    }
    return HS_OK;
}

// torch.optim.AdamW's bias corrections at `step`, formed in fp64
inline void bias_corrections(float b1, float b2, int step, float& inv_bc1, float& inv_sqrt_bc2) {
    const double bc1 = 1.0 - pow((double)b1, step), bc2 = 1.0 - pow((double)b2, step);
    inv_bc1 = (float)(1.0 / bc1);
    inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
}

// The streaming kernels' shape: a 16-byte body where every array of `arrays` is 16-byte aligned (and `ids`, a byte per element, 4-byte
// aligned), one element per thread behind it (everything otherwise).  Sets n4, the float4s of the body; returns the grid that covers
// body and tail, at most `cap` workgroups of 256 that stride over the rest.
inline int body_and_grid(std::initializer_list<const void*> arrays, const void* ids, int64_t n, int cap, int64_t& n4) {
    bool vec = !misaligned(ids, 3);
    for (const void* a : arrays) vec = vec && !misaligned(a, 15);
    n4 = vec ? n / 4 : 0;
    const int64_t work = vec ? n4 + 3 : n;
    return (int)std::min<int64_t>((work + 255) / 256, cap);
}
