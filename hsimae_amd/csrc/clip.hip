// Control over the size of the update without a host wait: the global gradient norm, torch.nn.utils.clip_grad_norm_'s
// coefficient, and the decision to skip a step whose gradient is not finite, all kept in device memory (hsimae_clip_ctl).
//
//   grad_sumsq_kernel   a FIXED grid of CLIP_GRID workgroups walks up to 8 segments {g, group, n} grid-stride: 16-byte loads over
//                       the aligned body of each segment, the <= 3 elements before and after it one per thread of workgroup 0.
//                       An element whose group id is 2 (frozen, or without a gradient this step: it may hold NaN) never enters
//                       the sum.  Squares and sums are fp64 (|g| = 1e30 squares to 1e60); block_sum -> partials[CLIP_GRID].
//                       No atomics: the order of every addition is fixed by the grid, so two runs are bit-identical.
//   clip_finish_kernel  one workgroup: thread t adds partials t, t + 256, ... in order, then the LDS tree of loss_final_kernel;
//                       thread 0 fills the control block.
//   adamw_groups_kernel adamw_one on g * coef with a learning rate and a weight decay PER GROUP ID: up to 64 {lr, weight_decay}
//                       pairs travel in the launch.  With a control block the bias corrections are read from it and nothing is
//                       written when ctl->apply is 0; without one coef = 1.  Any n, group ids per element or one id for all.
//                       hsimae_adamw_step_ctl is this kernel with a two-entry table.
// The table, adamw_one, block_sum and the launchers' shared checks are in optim.h.
#include "optim.h"

namespace {

constexpr int CLIP_GRID = HSIMAE_CLIP_GRID;
static_assert(CLIP_GRID % 256 == 0, "clip_finish_kernel gives every thread the same number of partials");
static_assert(sizeof(hsimae_clip_ctl) == 48, "hsimae_amd/_lib.py ClipCtl mirrors this layout");

struct ClipSegs { hsimae_grad_seg s[HSIMAE_CLIP_MAX_SEGS]; int n; };

// a float4 of gradients with its four group ids: a lane with id 2 is not summed (a select, never a product: NaN * 0 is NaN)
__device__ __forceinline__ void acc4(double (&a)[4], const float4 G, const uchar4 r) {
    a[0] += r.x != 2 ? sq64(G.x) : 0.0;
    a[1] += r.y != 2 ? sq64(G.y) : 0.0;
    a[2] += r.z != 2 ? sq64(G.z) : 0.0;
    a[3] += r.w != 2 ? sq64(G.w) : 0.0;
}

__device__ __forceinline__ uchar4 ids_at(const uint8_t* grp, int64_t i, bool aligned) {
    if (!grp) return make_uchar4(0, 0, 0, 0);
    if (aligned) return reinterpret_cast<const uchar4*>(grp)[i];
    return make_uchar4(grp[4 * i], grp[4 * i + 1], grp[4 * i + 2], grp[4 * i + 3]);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(ClipSegs segs, double* partials) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)CLIP_GRID * 256;
    for (int k = 0; k < segs.n; ++k) {                                          // uniform
        const float* g = segs.s[k].g;
        const uint8_t* grp = segs.s[k].group;
        const int64_t n = segs.s[k].n;
        if (n <= 0) continue;
        const int64_t head = min((int64_t)head_floats(g), n);
        const int64_t n4 = (n - head) >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(g + head);
        const uint8_t* gb = grp ? grp + head : nullptr;
        const bool al = ((uintptr_t)gb & 3u) == 0;
        int64_t i = tid;
        for (; i + 3 * stride < n4; i += 4 * stride) {                          // four loads in flight
            const uchar4 r0 = ids_at(gb, i, al), r1 = ids_at(gb, i + stride, al), r2 = ids_at(gb, i + 2 * stride, al),
                         r3 = ids_at(gb, i + 3 * stride, al);
            const float4 G0 = g4[i], G1 = g4[i + stride], G2 = g4[i + 2 * stride], G3 = g4[i + 3 * stride];
            acc4(a, G0, r0); acc4(a, G1, r1); acc4(a, G2, r2); acc4(a, G3, r3);
        }
        for (; i < n4; i += stride) acc4(a, g4[i], ids_at(gb, i, al));
        const int64_t tail0 = head + 4 * n4, ends = head + (n - tail0);         // <= 6 elements outside the body
        if (tid < ends) {
            const int64_t e = tid < head ? tid : tail0 + (tid - head);
            if (!grp || grp[e] != 2) a[0] += sq64(g[e]);
        }
    }
    block_sum(partials + blockIdx.x, a);
}

__global__ __launch_bounds__(256) void clip_finish_kernel(const double* partials, float max_norm, int skip_nonfinite, int step,
                                                          float beta1, float beta2, hsimae_clip_ctl* ctl) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < CLIP_GRID; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double sumsq = red[0], norm = sqrt(sumsq);
    const int finite = __builtin_isfinite(sumsq) ? 1 : 0;
    const double c = (double)max_norm / (norm + 1e-6);
    const double coef = c > 1.0 ? 1.0 : c;                                      // torch.clamp(max = 1): a NaN stays a NaN
    const int apply = (skip_nonfinite && !finite) ? 0 : 1;
    const int64_t skipped = ctl->skipped + (apply ? 0 : 1);
    const double t = (double)((int64_t)step - skipped);
    ctl->sumsq = sumsq;
    ctl->norm = (float)norm;
    ctl->coef = (float)coef;
    ctl->finite = finite;
    ctl->apply = apply;
    ctl->skipped = skipped;
    ctl->inv_bc1 = (float)(1.0 / (1.0 - pow((double)beta1, t)));
    ctl->inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, t)));
    if (finite) ctl->norm_max = fmaxf(ctl->norm_max, (float)norm);
}

// The grouped step.  An element's id indexes the table staged into LDS.
// Id 2 and every id >= ngroups are frozen: never read, never written, so the table is never indexed past ngroups.
// ctl != NULL: coef, apply and the bias corrections come from the control block; NULL: coef = 1 and the launcher's corrections.
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* p, const float* g, float* m, float* v, const uint8_t* group,
                                                           int group_uniform, int64_t n, int64_t n4, int ngroups, GroupTable table,
                                                           float b1, float b2, float eps, float inv_bc1, float inv_sqrt_bc2,
                                                           const hsimae_clip_ctl* ctl) {
    __shared__ float2 tab[HSIMAE_ADAMW_MAX_GROUPS];
    float coef = 1.f;
    if (ctl) {                                                                   // uniform
        if (ctl->apply == 0) return;                                            // a skipped step writes nothing
        coef = ctl->coef; inv_bc1 = ctl->inv_bc1; inv_sqrt_bc2 = ctl->inv_sqrt_bc2;
    }
    stage_table(tab, table, ngroups);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const unsigned char gu = (unsigned char)group_uniform;
    const unsigned ng = (unsigned)ngroups;
    for (int64_t i = tid; i < n4; i += stride) {
        const uchar4 gr = group ? reinterpret_cast<const uchar4*>(group)[i] : make_uchar4(gu, gu, gu, gu);
        const unsigned char grp[4] = {gr.x, gr.y, gr.z, gr.w};
        bool live[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) live[e] = grp[e] != 2 && grp[e] < ng;
        if (!(live[0] || live[1] || live[2] || live[3])) continue;
        float4 P = reinterpret_cast<float4*>(p)[i], M = reinterpret_cast<float4*>(m)[i], V = reinterpret_cast<float4*>(v)[i];
        const float4 G = reinterpret_cast<const float4*>(g)[i];
        float* pp = &P.x; float* mm = &M.x; float* vv = &V.x;
        const float* gg = &G.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!live[e]) continue;
            const float2 t = tab[grp[e]];
            adamw_one(pp[e], gg[e], mm[e], vv[e], t.x, t.y, b1, b2, eps, inv_bc1, inv_sqrt_bc2, coef);
        }
        reinterpret_cast<float4*>(p)[i] = P; reinterpret_cast<float4*>(m)[i] = M; reinterpret_cast<float4*>(v)[i] = V;
    }
    for (int64_t e = 4 * n4 + tid; e < n; e += stride) {                        // behind the float4 body (everything when unaligned)
        const unsigned grp = group ? group[e] : gu;
        if (grp == 2 || grp >= ng) continue;
        const float2 t = tab[grp];
        adamw_one(p[e], g[e], m[e], v[e], t.x, t.y, b1, b2, eps, inv_bc1, inv_sqrt_bc2, coef);
    }
}

}  // namespace

int hs_grad_norm(const hsimae_grad_seg* segs, int nseg, float max_norm, int skip_nonfinite, int step, float beta1, float beta2,
                 double* partials, hsimae_clip_ctl* ctl, hipStream_t s) {
    if (nseg < 1 || nseg > HSIMAE_CLIP_MAX_SEGS || step < 1 || !ctl || !partials || !(max_norm > 0.f)) return HS_EDIMS;
    if (!segs) return HS_ENULL;
    ClipSegs a;
    a.n = nseg;
    for (int k = 0; k < nseg; ++k) {
        if (segs[k].n < 0) return HS_EDIMS;
        a.s[k] = segs[k];
    }
    for (int k = 0; k < nseg; ++k) {
        if (segs[k].n > 0 && !segs[k].g) return HS_ENULL;
        if (misaligned(segs[k].g, 3)) return HS_EALIGN;
    }
    if (misaligned(partials, 7) || misaligned(ctl, 7)) return HS_EALIGN;
    for (int k = nseg; k < HSIMAE_CLIP_MAX_SEGS; ++k) a.s[k] = hsimae_grad_seg{nullptr, nullptr, 0};
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(CLIP_GRID), dim3(256), 0, s, a, partials);
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, s, partials, max_norm, skip_nonfinite ? 1 : 0, step, beta1, beta2, ctl);
    return (int)hipGetLastError();
}

int hs_adamw_groups(float* p, const float* g, float* m, float* v, const unsigned char* group, int group_uniform, int64_t n,
                    const hsimae_adamw_group* table, int ngroups, float b1, float b2, float eps, int step, const hsimae_clip_ctl* ctl,
                    hipStream_t s) {
    if (n < 0 || ngroups < 1 || ngroups > HSIMAE_ADAMW_MAX_GROUPS) return HS_EDIMS;
    if (bad_group_uniform(group, group_uniform, ngroups)) return HS_EDIMS;
    if (!ctl && step < 1) return HS_EDIMS;
    if (n == 0) return HS_OK;
    if (!p || !g || !m || !v || !table) return HS_ENULL;
    GroupTable t;
    if (fill_group_table(t, table, ngroups) != HS_OK) return HS_EDIMS;
    if (misaligned(p, 3) || misaligned(g, 3) || misaligned(m, 3) || misaligned(v, 3) || misaligned(ctl, 7)) return HS_EALIGN;
    if (!group && group_uniform == 2) return HS_OK;                              // all frozen: nothing to do
    float inv_bc1 = 0.f, inv_sqrt_bc2 = 0.f;                                     // read from ctl when there is one
    if (!ctl) bias_corrections(b1, b2, step, inv_bc1, inv_sqrt_bc2);
    int64_t n4;
    const int grid = body_and_grid({p, g, m, v}, group, n, 2048, n4);
    hipLaunchKernelGGL(adamw_groups_kernel, dim3(grid), dim3(256), 0, s, p, g, m, v, group, group_uniform, n, n4, ngroups, t, b1, b2,
                       eps, inv_bc1, inv_sqrt_bc2, ctl);
    return (int)hipGetLastError();
}

// hsimae_adamw_step_ctl: the grouped step with the table {(lr, wd), (lr, 0)}
int hs_adamw_ctl(float* p, const float* g, float* m, float* v, const unsigned char* group, int group_uniform, int64_t n, float lr,
                 float b1, float b2, float eps, float wd, const hsimae_clip_ctl* ctl, hipStream_t s) {
    if (n < 0 || (!group && (group_uniform < 0 || group_uniform > 2))) return HS_EDIMS;
    if (n == 0) return HS_OK;
    if (!ctl) return HS_ENULL;
    const hsimae_adamw_group table[2] = {{lr, wd}, {lr, 0.f}};
    return hs_adamw_groups(p, g, m, v, group, group_uniform, n, table, 2, b1, b2, eps, 1, ctl, s);
}

HS_UNIT_VARIANT_BITS(clip)
