// Masked reconstruction of a whole scene (hsimae_recon_accumulate / hsimae_recon_finish, include/hsimae_hip.h): the way back from
// the 9 x 9 windows hsimae_forward reconstructs (pred_img / mask_img, [n][C][9][9]) to the scene [H][W][C], and the per-pixel
// error maps and the sums behind PSNR / SAM.
//
//   recon_accumulate_kernel   a gather: one lane per scene voxel (r, c, b), band-fastest, so sum / cnt are read and written in
//                             whole contiguous runs.  The lane walks the windows of the chunk that hold its pixel un-reflected
//                             (at most 9 per axis: the centres are distinct integers within 4 of the pixel) in ascending window
//                             index and adds the predictions whose mask is set.  A voxel has one owner: no atomics.
//   recon_finish_kernel       one wave per pixel, the bands lane-strided, fp64 sums through the xor tree (tree_sum, row_wave.h);
//                             a workgroup's four waves leave one partial of each of the four statistics.
//   recon_stats_kernel        one workgroup, one wave per statistic: the partials lane-strided in ascending order, then the xor tree.
//
// pred_img is band-major (81 floats between the bands of a pixel), so a wave's loads there touch one cache line per lane.  Staging
// every window row through LDS (read pixel-fastest, handed to the owners band-fastest) was built and measured: 136 us per chunk against
// 132 us, no gain, so these reads are not what bounds the kernel and the plain form stays (profiles/EXPERIMENTS.md).
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

constexpr int RECON_ACC_MAXNB = 1 << 16;      // workgroups of the accumulate launch at most (16 M lanes): a block-stride loop beyond

// first index in list[0, n) whose value is >= v (n when none): lower bound of an ascending list; stays inside [0, n] whatever it holds
__device__ __forceinline__ int first_at_least(const int32_t* list, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void recon_accumulate_kernel(hsimae_recon_accumulate_params p) {
    const int C = p.C;
    const int64_t WC = (int64_t)p.W * C;
    const int64_t segs = (WC + 255) / 256, nblk = (int64_t)p.H * segs;
    const int64_t w_end = p.w0 + p.n;
    const int ir_lo = (int)(p.w0 / p.ncols), ir_hi = (int)((w_end - 1) / p.ncols);      // window rows the chunk touches
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int r = (int)(blk / segs);                                               // block-uniform
        const int64_t e = (blk - (int64_t)r * segs) * 256 + threadIdx.x;
        int ira = first_at_least(p.rows, p.nrows, r - 4);
        if (ira < ir_lo) ira = ir_lo;
        if (ira > ir_hi || ira >= p.nrows || p.rows[ira] > r + 4) continue;             // no window row of this chunk holds row r
        if (e >= WC) continue;
        const int c = (int)(e / C), b = (int)(e - (int64_t)c * C);
        const int ica = first_at_least(p.cols, p.ncols, c - 4);
        const int64_t vox = (int64_t)r * WC + e;
        float s = 0.f;
        int k = 0;
        bool touched = false;
        for (int ir = ira; ir <= ir_hi && ir < p.nrows && ir < ira + 9; ++ir) {         // ascending window index: rows outer
            const int i = r - p.rows[ir] + 4;
            if (i < 0 || i > 8) continue;
            for (int ic = ica; ic < p.ncols && ic < ica + 9; ++ic) {
                const int j = c - p.cols[ic] + 4;
                if (j < 0 || j > 8) continue;
                const int64_t w = (int64_t)ir * p.ncols + ic;
                if (w < p.w0 || w >= w_end) continue;
                const int64_t at = (((w - p.w0) * C + b) * 9 + i) * 9 + j;
                if (p.mask_img[at] != 0.f) {                                            // a select: pred under mask 0 is never read
                    if (!touched) { s = p.sum[vox]; k = p.cnt[vox]; touched = true; }
                    s += p.pred_img[at];
                    k += 1;
                }
            }
        }
        if (touched) { p.sum[vox] = s; p.cnt[vox] = k; }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void recon_finish_kernel(hsimae_recon_finish_params p) {
    __shared__ double part[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = p.C;
    const int64_t HW = (int64_t)p.H * p.W;
    const T* scene = reinterpret_cast<const T*>(p.scene);
    double st_se = 0., st_m = 0., st_sam = 0., st_n = 0.;      // this wave's pixels, in ascending pixel order (the same in every lane)
    for (int64_t px = (int64_t)blockIdx.x * 4 + wave; px < HW; px += (int64_t)gridDim.x * 4) {      // wave-uniform
        const int64_t base = px * C;
        double se = 0., rr = 0., xx = 0.;
        int m = 0;
        for (int b = lane; b < C; b += 64) {
            const float x = (float)scene[base + b];
            const int k = p.cnt[base + b];
            const float r = k > 0 ? p.sum[base + b] / (float)k : x;
            if (p.recon) p.recon[base + b] = r;
            if (k > 0) {
                const double d = (double)r - (double)x;
                se = fma(d, d, se);
                rr = fma((double)r, (double)r, rr);
                xx = fma((double)x, (double)x, xx);
                m += 1;
            }
        }
        se = tree_sum(se); rr = tree_sum(rr); xx = tree_sum(xx);
        m = tree_sum(m);
        double rmse = 0., sam = 0.;
        if (m > 0) {
            rmse = sqrt(se / (double)m);
            const double nr = sqrt(rr), nx = sqrt(xx);
            if (nr == 0. && nx == 0.) {
                sam = 0.;
            } else if (nr == 0. || nx == 0.) {
                sam = 1.5707963267948966;
            } else {                                          // (a NaN norm takes this path and stays NaN)
                double dm = 0., dp = 0.;
                for (int b = lane; b < C; b += 64) {
                    const int k = p.cnt[base + b];
                    if (k > 0) {
                        const double u = (double)(p.sum[base + b] / (float)k) / nr, v = (double)(float)scene[base + b] / nx;
                        dm = fma(u - v, u - v, dm);
                        dp = fma(u + v, u + v, dp);
                    }
                }
                dm = tree_sum(dm); dp = tree_sum(dp);
                sam = 2. * atan2(sqrt(dm), sqrt(dp));
            }
            st_se += se; st_m += (double)m; st_sam += sam; st_n += 1.;
        }
        if (lane == 0) {
            if (p.cover) p.cover[px] = m;
            if (p.rmse) p.rmse[px] = (float)rmse;
            if (p.sam) p.sam[px] = (float)sam;
        }
    }
    if (lane == 0) { part[wave][0] = st_se; part[wave][1] = st_m; part[wave][2] = st_sam; part[wave][3] = st_n; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        p.partials[(int64_t)blockIdx.x * 4 + j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
    }
}

// wave j owns statistic j: lane l adds the workgroups' partials l, l + 64, .. in order, then the xor tree (a serial walk over the
// 1024 partials took 110 us: longer than the accumulate launch of a chunk)
__global__ __launch_bounds__(256) void recon_stats_kernel(const double* partials, int nblocks, double* stats) {
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    double t = 0.;
    for (int i = lane; i < nblocks; i += 64) t += partials[(int64_t)i * 4 + j];
    t = tree_sum(t);
    if (lane == 0) stats[j] = t;
}

}  // namespace

int hs_recon_accumulate(const hsimae_recon_accumulate_params& p, hipStream_t s) {
    if (p.n < 0 || p.H <= 0 || p.W <= 0 || p.C <= 0 || p.nrows <= 0 || p.ncols <= 0 || p.w0 < 0) return HS_EDIMS;
    // strictly ascending centres inside the scene are at most as many as the axis is long: what the host can see of the lists
    if (p.nrows > p.H || p.ncols > p.W) return HS_EDIMS;
    if (p.w0 + p.n > (int64_t)p.nrows * p.ncols) return HS_EDIMS;
    if (p.n > 0 && (!p.pred_img || !p.mask_img || !p.rows || !p.cols || !p.sum || !p.cnt)) return HS_ENULL;
    if (misaligned(p.pred_img, 3) || misaligned(p.mask_img, 3) || misaligned(p.rows, 3) || misaligned(p.cols, 3) ||
        misaligned(p.sum, 3) || misaligned(p.cnt, 3)) return HS_EALIGN;
    if (p.n == 0) return HS_OK;
    const int64_t nblk = (int64_t)p.H * (((int64_t)p.W * p.C + 255) / 256);
    hipLaunchKernelGGL(recon_accumulate_kernel, dim3((unsigned)(nblk < RECON_ACC_MAXNB ? nblk : RECON_ACC_MAXNB)), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

int hs_recon_finish(const hsimae_recon_finish_params& p, hipStream_t s) {
    if (p.H <= 0 || p.W <= 0 || p.C <= 0) return HS_EDIMS;
    if (!p.scene || !p.sum || !p.cnt || !p.partials || !p.stats) return HS_ENULL;
    if (misaligned(p.scene, p.scene_f64 ? 7 : 3) || misaligned(p.sum, 3) || misaligned(p.cnt, 3) || misaligned(p.recon, 3) ||
        misaligned(p.cover, 3) || misaligned(p.rmse, 3) || misaligned(p.sam, 3) || misaligned(p.partials, 7) ||
        misaligned(p.stats, 7)) return HS_EALIGN;
    const int grid = (int)rows_grid((int64_t)p.H * p.W, HSIMAE_RECON_GRID);
    if (p.scene_f64) hipLaunchKernelGGL(recon_finish_kernel<double>, dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(recon_finish_kernel<float>, dim3(grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL(recon_stats_kernel, dim3(1), dim3(256), 0, s, p.partials, grid, p.stats);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(recon)
