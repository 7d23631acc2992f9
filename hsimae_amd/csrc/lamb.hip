// LAMB (You et al. 2020; apex FusedLAMB, timm Lamb): Adam's update, scaled PER PARAMETER TENSOR by |w| / |update|, on the flat
// parameter buffer.  Three launches on one stream, no atomics, every addition in a fixed order: two runs are bit-identical.
//
//   lamb_moments_kernel  one workgroup of 256 per CHUNK: at most HSIMAE_LAMB_CHUNK consecutive floats of ONE tensor.  The workgroup
//                        finds its tensor by binary search on hsimae_lamb_tensor.chunk0 (uniform), reads p, g, m, v, writes m', v'
//                        in place and partials[2 chunk] = sum p^2, partials[2 chunk + 1] = sum u^2 in fp64 (block_sum, optim.h).
//                        16-byte accesses over the aligned body of the chunk, the <= 3 elements before and behind it one per thread.
//   lamb_ratio_kernel    one wave per tensor: lane l adds the tensor's chunk partials l, l + 64, ... in order, then the same tree;
//                        lane 0 writes ratios[T] = (float)sqrt(sum p^2 / sum u^2) in fp64 (1 where the tensor is not adapted).
//   lamb_apply_kernel    the first kernel's grid: RECOMPUTES u from p, m', v' through the same lamb_u() and writes
//                        p' = p - (lr * r_T) * u.  No n-float scratch for u: 10 array passes either way, and the optimizer's memory
//                        stays AdamW's.
//
// A tensor's group id is the id byte of its FIRST element (FusedAdamW writes ids per whole tensor).  Id 2 and ids >= ngroups are
// frozen: nothing of the tensor is read but that byte, nothing is written, its ratio is 1.  ctl->apply == 0: all three kernels return
// before any read of p, g, m, v and any write.  A chunk whose table entry is inconsistent writes nothing and sets *bad; the three
// kernels apply the same test to an entry, so a tensor is stepped whole (moments, ratio, parameters) or not at all.
#include "optim.h"

namespace {

constexpr int CHUNK = HSIMAE_LAMB_CHUNK;
static_assert(CHUNK == 4096, "a thread of lamb_moments_kernel holds at most four float4 of its chunk");
static_assert(sizeof(hsimae_lamb_tensor) == 24, "hsimae_amd/_lib.py LambTensor mirrors this layout");

// the update direction of one element, from the NEW moments (adam_moments): both kernels call this and nothing else
__device__ __forceinline__ float lamb_u(float p, float mn, float vn, float wd, float eps, float inv_bc1, float inv_sqrt_bc2) {
    float u = (mn * inv_bc1) / (sqrtf(vn) * inv_sqrt_bc2 + eps);
    if (wd != 0.f) u += wd * p;
    return u;
}

struct ChunkOf { int tensor; int64_t start; int len; int id; };                  // len 0: nothing to do (frozen, or a bad entry)

// Which tensor this workgroup's chunk belongs to, where the chunk lies and the tensor's group id.  Every thread runs the same
// search on the same values.  The entry is checked before anything is read through it.
__device__ __forceinline__ ChunkOf find_chunk(const hsimae_lamb_tensor* tensors, int ntensors, int64_t n_total, const uint8_t* group,
                                              int group_uniform, int ngroups, int* bad) {
    const int chunk = (int)blockIdx.x;
    int lo = 0, hi = ntensors - 1;                                               // the last tensor whose chunk0 <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tensors[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const hsimae_lamb_tensor t = tensors[lo];
    ChunkOf c{lo, 0, 0, 2};
    const int64_t local = (int64_t)chunk - t.chunk0, nch = t.n > 0 ? (t.n + CHUNK - 1) / CHUNK : 0;
    // lamb_ratio_kernel's test of the entry, so that a tensor without a ratio is not stepped either: the chunks [chunk0, chunk0 + nch)
    // end where the next tensor's begin (the grid is nchunks)
    const int64_t next = lo + 1 < ntensors ? (int64_t)tensors[lo + 1].chunk0 : (int64_t)gridDim.x;
    if (t.off < 0 || t.n <= 0 || t.n > n_total - t.off || local < 0 || local >= nch || t.chunk0 < 0 || t.chunk0 + nch != next ||
        next > (int64_t)gridDim.x) {
        if (threadIdx.x == 0) *bad = 1;
        return c;
    }
    const unsigned id = group ? group[t.off] : (unsigned)group_uniform;
    if (id == 2u || id >= (unsigned)ngroups) return c;                           // frozen
    c.id = (int)id;
    c.start = t.off + local * CHUNK;
    const int64_t left = t.n - local * CHUNK;
    c.len = left < CHUNK ? (int)left : CHUNK;
    return c;
}

// floats of the chunk in front of its 16-byte body; `vec` says that the four arrays share their alignment (else: the whole chunk)
__device__ __forceinline__ int chunk_head(const float* p, int len, bool vec) { return vec ? min((int)head_floats(p), len) : len; }

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* p, const float* g, float* m, float* v, const uint8_t* group,
                                                           int group_uniform, int64_t n_total, const hsimae_lamb_tensor* tensors,
                                                           int ntensors, int ngroups, GroupTable table, float b1, float b2, float eps,
                                                           int vec, double* partials, int* bad, const hsimae_clip_ctl* ctl) {
    __shared__ float2 tab[HSIMAE_ADAMW_MAX_GROUPS];
    if (ctl->apply == 0) return;                                                 // uniform: a skipped step reads and writes nothing
    const float coef = ctl->coef, inv_bc1 = ctl->inv_bc1, inv_sqrt_bc2 = ctl->inv_sqrt_bc2;
    stage_table(tab, table, ngroups);
    const ChunkOf c = find_chunk(tensors, ntensors, n_total, group, group_uniform, ngroups, bad);
    if (c.len == 0) return;                                                      // uniform
    const float wd = tab[c.id].y;
    p += c.start; g += c.start; m += c.start; v += c.start;
    const int head = chunk_head(p, c.len, vec != 0), n4 = (c.len - head) >> 2, tail0 = head + 4 * n4;
    double sp[4] = {0.0, 0.0, 0.0, 0.0}, su[4] = {0.0, 0.0, 0.0, 0.0};
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    float4* m4 = reinterpret_cast<float4*>(m + head);
    float4* v4 = reinterpret_cast<float4*>(v + head);
    float4 P[4], G[4], M[4], V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                                // up to sixteen 16-byte loads in flight
        const int i = threadIdx.x + 256 * k;
        if (i < n4) { P[k] = p4[i]; G[k] = g4[i]; M[k] = m4[i]; V[k] = v4[i]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (i >= n4) continue;
        const float* pp = &P[k].x; const float* gg = &G[k].x;
        float* mm = &M[k].x; float* vv = &V[k].x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            adam_moments(gg[e], mm[e], vv[e], b1, b2, coef);
            const float u = lamb_u(pp[e], mm[e], vv[e], wd, eps, inv_bc1, inv_sqrt_bc2);
            sp[e] += sq64(pp[e]);
            su[e] += sq64(u);
        }
        m4[i] = M[k]; v4[i] = V[k];
    }
    for (int t = threadIdx.x; t < head + (c.len - tail0); t += 256) {            // <= 6 elements when vec, the whole chunk otherwise
        const int e = t < head ? t : tail0 + (t - head);
        float mn = m[e], vn = v[e];
        const float pe = p[e];
        adam_moments(g[e], mn, vn, b1, b2, coef);
        const float u = lamb_u(pe, mn, vn, wd, eps, inv_bc1, inv_sqrt_bc2);
        sp[0] += sq64(pe);
        su[0] += sq64(u);
        m[e] = mn; v[e] = vn;
    }
    block_sum(partials + 2 * (int64_t)blockIdx.x, sp, su);
}

__global__ __launch_bounds__(256) void lamb_ratio_kernel(const uint8_t* group, int group_uniform, int64_t n_total,
                                                         const hsimae_lamb_tensor* tensors, int ntensors, int nchunks, int ngroups,
                                                         GroupTable table, float trust_clip, int always_adapt, const double* partials,
                                                         float* ratios, int* bad, const hsimae_clip_ctl* ctl) {
    __shared__ float2 tab[HSIMAE_ADAMW_MAX_GROUPS];
    if (ctl->apply == 0) return;                                                 // ratios keep the last applied step's values
    stage_table(tab, table, ngroups);
    const int T = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (T >= ntensors) return;                                                   // uniform per wave
    const hsimae_lamb_tensor t = tensors[T];
    const int64_t nch = t.n > 0 ? (t.n + CHUNK - 1) / CHUNK : 0;
    const int64_t next = T + 1 < ntensors ? (int64_t)tensors[T + 1].chunk0 : (int64_t)nchunks;
    if (t.off < 0 || t.n < 0 || t.n > n_total - t.off || t.chunk0 < 0 || t.chunk0 + nch != next || next > nchunks) {
        if (lane == 0) *bad = 1;                                                 // the chunks do not tile this tensor: no ratio
        return;
    }
    const unsigned id = (group && t.n > 0) ? group[t.off] : (group ? 2u : (unsigned)group_uniform);
    if (id == 2u || id >= (unsigned)ngroups) {                                   // frozen: its partials were never written
        if (lane == 0) ratios[T] = 1.f;
        return;
    }
    double sp = 0.0, su = 0.0;
    for (int64_t j = lane; j < nch; j += 64) {
        sp += partials[2 * (t.chunk0 + j)];
        su += partials[2 * (t.chunk0 + j) + 1];
    }
    wave_tree<TreeAdd>(sp, su);
    if (lane != 0) return;
    float r = 1.f;
    if ((tab[id].y != 0.f || always_adapt) && sp > 0.0 && su > 0.0) r = (float)sqrt(sp / su);
    if (trust_clip > 0.f) r = fminf(r, trust_clip);
    ratios[T] = r;
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(float* p, const float* m, const float* v, const uint8_t* group,
                                                         int group_uniform, int64_t n_total, const hsimae_lamb_tensor* tensors,
                                                         int ntensors, int ngroups, GroupTable table, float eps, int vec,
                                                         const float* ratios, int* bad, const hsimae_clip_ctl* ctl) {
    __shared__ float2 tab[HSIMAE_ADAMW_MAX_GROUPS];
    if (ctl->apply == 0) return;
    const float inv_bc1 = ctl->inv_bc1, inv_sqrt_bc2 = ctl->inv_sqrt_bc2;
    stage_table(tab, table, ngroups);
    const ChunkOf c = find_chunk(tensors, ntensors, n_total, group, group_uniform, ngroups, bad);
    if (c.len == 0) return;
    const float wd = tab[c.id].y, step = tab[c.id].x * ratios[c.tensor];
    p += c.start; m += c.start; v += c.start;
    const int head = chunk_head(p, c.len, vec != 0), n4 = (c.len - head) >> 2, tail0 = head + 4 * n4;
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const float4* m4 = reinterpret_cast<const float4*>(m + head);
    const float4* v4 = reinterpret_cast<const float4*>(v + head);
    float4 P[4], M[4], V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (i < n4) { P[k] = p4[i]; M[k] = m4[i]; V[k] = v4[i]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (i >= n4) continue;
        float* pp = &P[k].x;
        const float* mm = &M[k].x; const float* vv = &V[k].x;
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = pp[e] - step * lamb_u(pp[e], mm[e], vv[e], wd, eps, inv_bc1, inv_sqrt_bc2);
        p4[i] = P[k];
    }
    for (int t = threadIdx.x; t < head + (c.len - tail0); t += 256) {
        const int e = t < head ? t : tail0 + (t - head);
        const float pe = p[e];
        p[e] = pe - step * lamb_u(pe, m[e], v[e], wd, eps, inv_bc1, inv_sqrt_bc2);
    }
}

}  // namespace

int hs_lamb_step(float* p, const float* g, float* m, float* v, const unsigned char* group, int group_uniform, int64_t n,
                 const hsimae_lamb_tensor* tensors, int ntensors, int nchunks, const hsimae_adamw_group* table, int ngroups, float b1,
                 float b2, float eps, float trust_clip, int always_adapt, double* partials, float* ratios, int* bad,
                 const hsimae_clip_ctl* ctl, hipStream_t s) {
    if (!p || !g || !m || !v || !tensors || !table || !partials || !ratios || !bad || !ctl) return HS_ENULL;
    if (n < 0 || ntensors < 1 || nchunks < 1 || ngroups < 1 || ngroups > HSIMAE_ADAMW_MAX_GROUPS) return HS_EDIMS;
    if (bad_group_uniform(group, group_uniform, ngroups)) return HS_EDIMS;
    GroupTable t;
    if (fill_group_table(t, table, ngroups) != HS_OK) return HS_EDIMS;
    if (misaligned(p, 3) || misaligned(g, 3) || misaligned(m, 3) || misaligned(v, 3) || misaligned(ratios, 3) || misaligned(bad, 3) ||
        misaligned(partials, 7) || misaligned(tensors, 7) || misaligned(ctl, 7))
        return HS_EALIGN;
    if (n == 0) return HS_OK;
    const uintptr_t a = (uintptr_t)p & 15u;                                      // 16-byte accesses where the four arrays agree mod 16
    const int vec = ((uintptr_t)g & 15u) == a && ((uintptr_t)m & 15u) == a && ((uintptr_t)v & 15u) == a;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(nchunks), dim3(256), 0, s, p, g, m, v, group, group_uniform, n, tensors, ntensors,
                       ngroups, t, b1, b2, eps, vec, partials, bad, ctl);
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3((ntensors + 3) / 4), dim3(256), 0, s, group, group_uniform, n, tensors, ntensors, nchunks,
                       ngroups, t, trust_clip, always_adapt ? 1 : 0, partials, ratios, bad, ctl);
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(nchunks), dim3(256), 0, s, p, m, v, group, group_uniform, n, tensors, ntensors, ngroups, t,
                       eps, vec, ratios, bad, ctl);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(lamb)
