// An exponential moving average of the weights that follows the optimizer step's contract: one launch, no host wait, and a
// skipped step changes nothing.
//
//   ema_update_kernel   t = step - ctl->skipped (ctl NULL: step), d = warmup ? min(decay, (1 + t) / (10 + t)) : decay in fp64,
//                       a = (float)(1 - d); per element ema = fmaf(a, p - ema, ema) in fp32, and an element whose p equals its ema
//                       bit for bit keeps its bits (a select: -0.0 - -0.0 is +0.0, and a frozen parameter must stay bit-equal to
//                       its average).  ctl->apply == 0: the kernel returns before it reads either array.
//   ema_swap_kernel     exchanges two arrays as 32-bit words, so NaN payloads travel unchanged.
//
// Both have the streaming shape of body_and_grid (optim.h), with at most HSIMAE_EMA_MAX_GRID workgroups.  Plain vector loads and
// stores; no atomics, no LDS.
#include "optim.h"

namespace {

constexpr int EMA_MAX_GRID = HSIMAE_EMA_MAX_GRID;                                // 256 CUs x 8 workgroups: the streaming-kernel cap

__device__ __forceinline__ float ema_one(float e, float p, float a) {
    const float r = fmaf(a, p - e, e);
    return __float_as_uint(p) == __float_as_uint(e) ? e : r;
}

__global__ __launch_bounds__(256) void ema_update_kernel(float* ema, const float* p, int64_t n, int64_t n4, double decay, int warmup,
                                                         int step, const hsimae_clip_ctl* ctl) {
    int64_t t = step;
    if (ctl) {                                                                   // uniform
        if (ctl->apply == 0) return;                                            // a skipped step moves neither the average nor t
        t -= ctl->skipped;
    }
    double d = decay;
    if (warmup) d = fmin(decay, (1.0 + (double)t) / (10.0 + (double)t));
    const float a = (float)(1.0 - d);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        float4 E = reinterpret_cast<float4*>(ema)[i];
        const float4 P = reinterpret_cast<const float4*>(p)[i];
        E.x = ema_one(E.x, P.x, a); E.y = ema_one(E.y, P.y, a); E.z = ema_one(E.z, P.z, a); E.w = ema_one(E.w, P.w, a);
        reinterpret_cast<float4*>(ema)[i] = E;
    }
    for (int64_t e = 4 * n4 + tid; e < n; e += stride) ema[e] = ema_one(ema[e], p[e], a);
}

__global__ __launch_bounds__(256) void ema_swap_kernel(uint32_t* a, uint32_t* b, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        const uint4 A = reinterpret_cast<uint4*>(a)[i], B = reinterpret_cast<uint4*>(b)[i];
        reinterpret_cast<uint4*>(a)[i] = B;
        reinterpret_cast<uint4*>(b)[i] = A;
    }
    for (int64_t e = 4 * n4 + tid; e < n; e += stride) {
        const uint32_t x = a[e], y = b[e];
        a[e] = y; b[e] = x;
    }
}

}  // namespace

int hs_ema_update(float* ema, const float* params, int64_t n, double decay, int warmup, int step, const hsimae_clip_ctl* ctl,
                  hipStream_t s) {
    if (n < 0 || !(decay >= 0.0 && decay < 1.0) || step < 1) return HS_EDIMS;    // (a NaN decay fails both comparisons)
    if (n == 0) return HS_OK;
    if (!ema || !params) return HS_ENULL;
    if (misaligned(ema, 3) || misaligned(params, 3) || misaligned(ctl, 7)) return HS_EALIGN;
    int64_t n4;
    const int grid = body_and_grid({ema, params}, nullptr, n, EMA_MAX_GRID, n4);
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(256), 0, s, ema, params, n, n4, decay, warmup ? 1 : 0, step, ctl);
    return (int)hipGetLastError();
}

int hs_ema_swap(float* a, float* b, int64_t n, hipStream_t s) {
    if (n < 0) return HS_EDIMS;
    if (n == 0) return HS_OK;
    if (!a || !b) return HS_ENULL;
    if (misaligned(a, 3) || misaligned(b, 3)) return HS_EALIGN;
    const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    if (ua < ub + bytes && ub < ua + bytes) return HS_EDIMS;                     // the ranges overlap
    int64_t n4;
    const int grid = body_and_grid({a, b}, nullptr, n, EMA_MAX_GRID, n4);
    hipLaunchKernelGGL(ema_swap_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<uint32_t*>(a), reinterpret_cast<uint32_t*>(b), n, n4);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(ema)
