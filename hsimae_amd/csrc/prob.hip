// The products of a scene's classification beyond the label (hsimae_class_prob, include/hsimae_hip.h): the class
// probabilities of every pixel averaged over the views (flips) it was looked at in, the label they give, the winning
// probability and the top-1 / top-2 margin.
//
//   class_prob_kernel    one wave per row of logits [N][ld], one launch per view of a chunk: the softmax over the columns
//                        [first, C) in row_softmax_stats' sequence (row_wave.h: row maximum, exp2((z - m) log2 e), a lane-strided
//                        sum and the xor tree), e * (1 / s) stored (view 0) or added (later views) into the caller's acc [N][lda]; the
//                        last view's wave scales its row by fl(1 / n_views) and writes the label, the confidence and the
//                        margin at the row's pixel and the mean probabilities in chunk order.
//
// A row is touched by one wave only and the views follow each other in stream order: no atomics, two runs are bit-identical.
// A latency kernel like its neighbour in cls.hip: 8192 rows of 10 - 20 classes per chunk.
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int PROB_MAXC = 1024;
constexpr int PROB_MAXV = 8;
constexpr int PROB_MAXNB = 2048;      // workgroups of 4 waves: one row per wave up to 8192 rows, a stride loop beyond

__global__ __launch_bounds__(256) void class_prob_kernel(hsimae_class_prob_params p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = p.C, first = p.first;
    const bool start = p.view == 0, last = p.view == p.n_views - 1, single = p.n_views == 1;
    const float inv_v = 1.f / (float)p.n_views;
    const int64_t HW = (int64_t)p.H * p.W;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.N; r += (int64_t)gridDim.x * 4) {       // wave-uniform
        const float* z = p.logits + r * p.ld;
        float* a = p.acc + r * p.lda;
        float m, sum;
        row_softmax_stats(z, first, C, lane, m, sum);
        const float rs = 1.f / sum;
        // the label's key is the logit with one view (hsimae_class_argmax's label, bit for bit) and the mean with more;
        // `val` carries the mean of the candidate along
        float key = -__builtin_inff(), val = 0.f;
        int best = 0x7fffffff;
        if (start) for (int c = lane; c < first; c += 64) a[c] = 0.f;
        if (last && p.probs) for (int c = lane; c < first; c += 64) p.probs[r * p.ldp + c] = 0.f;
        for (int c = first + lane; c < C; c += 64) {                                               // ascending: first of a tie stays
            const float pc = row_exp(z[c], m) * rs;
            const float t = start ? pc : a[c] + pc;       // view 0 never reads acc
            a[c] = t;
            if (last) {
                const float mean = t * inv_v;
                if (p.probs) p.probs[r * p.ldp + c] = mean;
                const int was = best;
                arg_better(key, best, single ? z[c] : mean, c);
                if (best != was) val = mean;
            }
        }
        if (!last) continue;
        const ArgVal top = wave_argmax(key, best, val);
        // the runner-up among the other classes: this lane re-reads the sums it stored itself
        const float second = row_runner_up(a, inv_v, first, C, lane, top.idx);
        const int64_t pix = row_pixel(p.pixels, p.p0, r, HW);
        if (lane == 0) write_maps(p.label_map, p.conf_map, p.margin_map, pix, top.idx, top.val, second, C - first == 1);
    }
}

}  // namespace

int hs_class_prob(const hsimae_class_prob_params& p, hipStream_t s) {
    if (p.N < 0 || p.C < 2 || p.first < 0 || p.first >= p.C || p.n_views < 1 || p.n_views > PROB_MAXV || p.view < 0 ||
        p.view >= p.n_views || p.ld < p.C || p.lda < p.C || (p.probs && p.ldp < p.C) || p.H <= 0 || p.W <= 0) return HS_EDIMS;
    if (p.C > PROB_MAXC) return HS_EUNSUPPORTED;
    if (p.N > 0 && (!p.logits || !p.acc || !p.label_map)) return HS_ENULL;
    if (misaligned(p.logits, 3) || misaligned(p.acc, 3) || misaligned(p.conf_map, 3) || misaligned(p.margin_map, 3) ||
        misaligned(p.probs, 3) || misaligned(p.pixels, 7) || misaligned(p.label_map, 7)) return HS_EALIGN;
    if (p.N == 0) return HS_OK;
    hipLaunchKernelGGL(class_prob_kernel, dim3(rows_grid(p.N, PROB_MAXNB)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(prob)
