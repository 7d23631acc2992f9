// The supervised half of fine-tuning (Model_Finetuning.py:150-178, 206-215, 268-290): cross-entropy with an ignored class on
// the head's logits, the predictions, the confusion counts of (label, prediction) and OA / AA / kappa from them.
//
//   cls_rows_kernel      one wave per row of logits [N][ld] (only columns [0, C) are classes): row maximum, sum of
//                        exp(z - max), loss_i = log(sum) - (z[y] - max) (torch's log_softmax form: no 1e4 - 1e4 cancellation),
//                        pred_i = first + argmax(z[first:C]), the UNSCALED gradient softmax - onehot (exact zeros for ignored
//                        rows and the pad columns [C, ldd)), and per workgroup the fp64 sum of its rows' losses and their
//                        count                                                        -> partials [nb] (nb <= 256)
//   cls_finish_kernel    the partials summed in block order by one wave (a fixed shuffle tree: two runs are bit-identical, no
//                        floating-point atomics), loss = sum / n_valid, and the gradient scaled in place by 1 / n_valid
//   cls_scale_kernel     dst = src * *scale, the scalar read from device memory (the loss's incoming gradient)
//   confusion_kernel     cm[gt][pred] += 1 where gt != 0: a histogram per workgroup in LDS (C <= 64) flushed with 64-bit
//                        integer atomics, whose result does not depend on their order; the map form also writes the masked map
//   scores_kernel        one workgroup, fp64, finetune_train.scores on the counts
//
// Latency kernels: a fine-tuning batch is 32 rows of about 10 classes.  Nothing here waits for the host.
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int CLS_MAXC = 1024;
constexpr int CLS_MAXNB = 256;        // workgroups of the row kernel = partials the finish kernel sums (4 per lane of one wave)
constexpr int CM_LDS_CELLS = 4096;    // confusion counts of one workgroup kept in LDS up to C = 64

struct ClsPartials { double* sum; long long* cnt; };
__host__ __device__ inline ClsPartials cls_carve(void* ws) {
    return ClsPartials{static_cast<double*>(ws), reinterpret_cast<long long*>(static_cast<double*>(ws) + CLS_MAXNB)};
}

// (arg_better, the argmax rule of the predictions: common.h; the row's statistics, its argmax and the xor tree: row_wave.h)
__global__ __launch_bounds__(256) void cls_rows_kernel(hsimae_cls_params p, ClsPartials part) {
    __shared__ double wsum[4];
    __shared__ long long wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = p.C;
    const float LN2 = 0.6931471805599453f;
    double lsum = 0.0;
    long long cnt = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.N; r += (int64_t)gridDim.x * 4) {       // wave-uniform
        const float* z = p.logits + r * p.ld;
        const int64_t y = p.targets[r];
        const bool in_range = y >= 0 && y < C;
        const bool valid = y != p.ignore_index && in_range;
        if (y != p.ignore_index && !in_range && lane == 0 && p.bad) *p.bad = 1;
        if (p.pred) {
            float bv = -__builtin_inff();
            int bi = 0x7fffffff;
            for (int c = p.first + lane; c < C; c += 64) arg_better(bv, bi, z[c], c);              // ascending: first of a tie stays
            wave_argmax(bv, bi);
            if (lane == 0) p.pred[r] = bi;
        }
        if (!valid) {                                     // ignored: no loss, an exactly zero gradient row
            if (p.dlogits) for (int c = lane; c < p.ldd; c += 64) p.dlogits[r * p.ldd + c] = 0.f;
            continue;
        }
        float m, sum;
        row_softmax_stats(z, 0, C, lane, m, sum);
        const float loss = __builtin_amdgcn_logf(sum) * LN2 - (z[y] - m);
        lsum += (double)loss;
        ++cnt;
        if (p.dlogits) {
            const float rs = 1.f / sum;
            float* d = p.dlogits + r * p.ldd;
            for (int c = lane; c < p.ldd; c += 64) {
                float g = 0.f;
                if (c < C) g = row_exp(z[c], m) * rs - (c == y ? 1.f : 0.f);
                d[c] = g;
            }
        }
    }
    if (lane == 0) { wsum[wave] = lsum; wcnt[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part.sum[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];                          // waves in order
        part.cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
}

// every workgroup sums the nb partials the same way (lane l: partials l, l + 64, l + 128, l + 192, then the xor tree)
__global__ __launch_bounds__(256) void cls_finish_kernel(ClsPartials part, int nb, float* loss, int64_t* n_valid, float* dlogits, int64_t total) {
    __shared__ float inv_s;
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        double s = 0.0;
        long long n = 0;
        for (int b = lane; b < nb; b += 64) { s += part.sum[b]; n += part.cnt[b]; }
        wave_tree<TreeAdd>(s, n);
        if (lane == 0) {
            inv_s = n > 0 ? 1.f / (float)n : 0.f;
            if (blockIdx.x == 0) {
                *loss = (float)(s / (double)n);           // n = 0: 0 / 0 = NaN, torch's mean over no rows
                if (n_valid) *n_valid = n;
            }
        }
    }
    __syncthreads();
    const float inv = inv_s;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) dlogits[e] *= inv;
}

__global__ __launch_bounds__(256) void cls_scale_kernel(const float* __restrict__ src, const float* __restrict__ scale, float* __restrict__ dst, int64_t n) {
    const float a = *scale;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) dst[e] = src[e] * a;
}

__global__ __launch_bounds__(256) void confusion_kernel(const int64_t* __restrict__ gt, const int64_t* __restrict__ mask, const int64_t* pred,
                                                        int64_t* masked, int64_t n, int C, unsigned long long* cm, int32_t* bad) {
    __shared__ unsigned int hist[CM_LDS_CELLS];
    const bool lds = C * C <= CM_LDS_CELLS;               // uniform
    if (lds) {
        for (int e = threadIdx.x; e < C * C; e += 256) hist[e] = 0u;
        __syncthreads();
    }
    // a workgroup takes at most 2^24 elements (the host sizes the grid so), so a 32-bit LDS cell cannot wrap
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int64_t pr = pred[i];
        if (mask) {
            if (mask[i] == 0) pr = 0;
            masked[i] = pr;
        }
        const int64_t g = gt[i];
        if (g == 0) continue;
        if (g < 0 || g >= C || pr < 0 || pr >= C) { *bad = 1; continue; }
        const int cell = (int)g * C + (int)pr;
        if (lds) atomicAdd(&hist[cell], 1u);
        else atomicAdd(&cm[cell], 1ull);
    }
    if (lds) {
        __syncthreads();
        for (int e = threadIdx.x; e < C * C; e += 256)
            if (hist[e]) atomicAdd(&cm[e], (unsigned long long)hist[e]);
    }
}

// finetune_train.scores on the counts: labels 1 .. C - 1 (the function's classes 0 .. C - 2), a prediction of 0 its own column.
// The sums of counts are integers (exact); every quotient is the one fp64 division the host function does.
__global__ __launch_bounds__(256) void scores_kernel(const int64_t* __restrict__ cm, int C, double* __restrict__ out) {
    __shared__ long long rn[256], rt[256], rp[256];
    __shared__ double rec[CLS_MAXC];
    __shared__ unsigned char pres[CLS_MAXC];
    const int t = threadIdx.x;
    long long n = 0, tr = 0, pp = 0;
    for (int k = 1 + t; k < C; k += 256) {
        long long row = 0, col = 0;
        for (int j = 0; j < C; ++j) row += cm[(int64_t)k * C + j];
        for (int g = 1; g < C; ++g) col += cm[(int64_t)g * C + k];
        const long long dg = cm[(int64_t)k * C + k];
        n += row; tr += dg; pp += row * col;
        pres[k] = row > 0;
        rec[k] = row > 0 ? (double)dg / (double)row : 0.0;
    }
    rn[t] = n; rt[t] = tr; rp[t] = pp;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { rn[t] += rn[t + h]; rt[t] += rt[t + h]; rp[t] += rp[t + h]; }
        __syncthreads();
    }
    for (int k = 1 + t; k < C; k += 256) { out[3 + k - 1] = rec[k]; out[3 + (C - 1) + k - 1] = pres[k] ? 1.0 : 0.0; }
    if (t == 0) {
        const double nn = (double)rn[0];
        const double oa = (double)rt[0] / nn;
        double sum = 0.0;
        int np = 0;
        for (int k = 1; k < C; ++k) if (pres[k]) { sum += rec[k]; ++np; }                          // classes in order
        const double pe = (double)rp[0] / (nn * nn);
        out[0] = oa;
        out[1] = sum / (double)np;
        out[2] = pe < 1.0 ? (oa - pe) / (1.0 - pe) : 0.0;
    }
}

int confusion_check(const int64_t* gt, const int64_t* pred, int64_t n, int C, const int64_t* cm, const int32_t* bad) {
    if (n < 0 || C < 2) return HS_EDIMS;
    if (C > CLS_MAXC) return HS_EUNSUPPORTED;
    if (!cm || !bad || (n > 0 && (!gt || !pred))) return HS_ENULL;
    if (misaligned(gt, 7) || misaligned(pred, 7) || misaligned(cm, 7) || misaligned(bad, 3)) return HS_EALIGN;
    return HS_OK;
}

int confusion_launch(const int64_t* gt, const int64_t* mask, const int64_t* pred, int64_t* masked, int64_t n, int C, int64_t* cm,
                     int32_t* bad, hipStream_t s) {
    if (n == 0) return HS_OK;
    int64_t nb = (n + 1023) / 1024;                       // about 4 elements per thread
    const int64_t least = (n + (1 << 24) - 1) >> 24;      // <= 2^24 elements per workgroup (32-bit LDS cells)
    nb = nb > 256 ? 256 : nb;
    nb = nb < least ? least : nb;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)nb), dim3(256), 0, s, gt, mask, pred, masked, n, C,
                       reinterpret_cast<unsigned long long*>(cm), bad);
    return (int)hipGetLastError();
}

}  // namespace

int64_t hs_cls_workspace_bytes(int N) {
    if (N < 0) return HS_EDIMS;
    return (int64_t)CLS_MAXNB * 16;                       // the partials: independent of N (the row kernel's grid is capped)
}

int hs_cls_loss(const hsimae_cls_params& p, hipStream_t s) {
    if (p.N < 0 || p.C < 2 || p.ld < p.C || p.first < 0 || p.first >= p.C || (p.dlogits && p.ldd < p.C)) return HS_EDIMS;
    if (p.C > CLS_MAXC) return HS_EUNSUPPORTED;
    if (!p.loss || !p.workspace || (p.N > 0 && (!p.logits || !p.targets))) return HS_ENULL;
    if (misaligned(p.logits, 3) || misaligned(p.loss, 3) || misaligned(p.dlogits, 3) || misaligned(p.bad, 3) ||
        misaligned(p.targets, 7) || misaligned(p.n_valid, 7) || misaligned(p.pred, 7) || misaligned(p.workspace, 7)) return HS_EALIGN;
    const ClsPartials part = cls_carve(p.workspace);
    int nb = 0;
    if (p.N > 0) {
        nb = (int)rows_grid(p.N, CLS_MAXNB);
        hipLaunchKernelGGL(cls_rows_kernel, dim3(nb), dim3(256), 0, s, p, part);
    }
    const int64_t total = p.dlogits ? (int64_t)p.N * p.ldd : 0;
    int64_t fb = (total + 1023) / 1024;
    fb = fb < 1 ? 1 : fb > 1024 ? 1024 : fb;
    hipLaunchKernelGGL(cls_finish_kernel, dim3((unsigned)fb), dim3(256), 0, s, part, nb, p.loss, p.n_valid, p.dlogits, total);
    return (int)hipGetLastError();
}

int hs_cls_grad_scale(const float* src, const float* scale, float* dst, int64_t n, hipStream_t s) {
    if (n < 0) return HS_EDIMS;
    if (n == 0) return HS_OK;
    if (!src || !scale || !dst) return HS_ENULL;
    if (misaligned(src, 3) || misaligned(scale, 3) || misaligned(dst, 3)) return HS_EALIGN;
    int64_t nb = (n + 1023) / 1024;
    nb = nb > 1024 ? 1024 : nb;
    hipLaunchKernelGGL(cls_scale_kernel, dim3((unsigned)nb), dim3(256), 0, s, src, scale, dst, n);
    return (int)hipGetLastError();
}

int hs_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int C, int64_t* cm, int32_t* bad, hipStream_t s) {
    const int rc = confusion_check(gt, pred, n, C, cm, bad);
    if (rc) return rc;
    return confusion_launch(gt, nullptr, pred, nullptr, n, C, cm, bad, s);
}

int hs_confusion_map(const int64_t* gt_map, const int64_t* mask_map, const int64_t* pred_map, int64_t* masked, int64_t n, int C,
                     int64_t* cm, int32_t* bad, hipStream_t s) {
    const int rc = confusion_check(gt_map, pred_map, n, C, cm, bad);
    if (rc) return rc;
    if (n > 0 && !masked) return HS_ENULL;
    if (misaligned(mask_map, 7) || misaligned(masked, 7)) return HS_EALIGN;
    return confusion_launch(gt_map, mask_map ? mask_map : gt_map, pred_map, masked, n, C, cm, bad, s);
}

int hs_scores(const int64_t* cm, int C, double* out, hipStream_t s) {
    if (C < 2) return HS_EDIMS;
    if (C > CLS_MAXC) return HS_EUNSUPPORTED;
    if (!cm || !out) return HS_ENULL;
    if (misaligned(cm, 7) || misaligned(out, 7)) return HS_EALIGN;
    hipLaunchKernelGGL(scores_kernel, dim3(1), dim3(256), 0, s, cm, C, out);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(cls)
