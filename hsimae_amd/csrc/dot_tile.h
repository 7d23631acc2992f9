// The exact-fp32 64 x 64 dot-product tile shared by knn.hip (knn_topk_kernel), kmeans.hip (kmeans_assign_kernel) and probe.hip (the
// forward and the gradient partials), and the wave-per-row normalisation the first two apply (row_normalize_kernel, the cosine
// centroids of kmeans_finish_kernel).
//
//   A workgroup of 256 threads (4 waves) holds 64 rows of A and 64 rows of B.  K-slabs of 32 columns of both operands are staged
//   in LDS (fetch_slab / put_slab), every wave forms one 32 x 32 block of dot products on v_mfma_f32_32x32x2_f32: a k-ordered fmaf
//   chain from +0 (k = 0, 1, .., D - 1 for every output, wherever its row sits in the tile), one rounding per product-and-add.
//   dot_tile() walks the slabs of one tile and prefetches the first slab of the next; hand_over() writes the wave's block into the
//   64 x 64 block P that lies over the slabs.  Rows beyond the matrices and columns beyond D are zero-filled in the slabs.
#pragma once
#include "common.h"
#include "row_wave.h"

constexpr int TQ = 64, TB = 64, KS = 32;
constexpr int SLD = KS + 1;           // LDS row stride of a slab: lane (i, h) reads [i][2 t + h], 33 i + h spreads over the banks
constexpr int PLD = TB + 1;           // row stride of the handed-over block
static_assert(TQ == TB && 2 * TQ * SLD >= TQ * PLD, "P fits over the slabs");

typedef __attribute__((ext_vector_type(16))) float f32x16;

// does candidate s go in front of entry e?  (strictly: an equal one stays behind; a NaN goes in front of nothing)
__device__ __forceinline__ bool beats(float s, float e) { return !__builtin_isnan(s) && (__builtin_isnan(e) || s > e); }

// one 64-row x 32-column slab of a [rows][ld] matrix: this thread's two 16-byte pieces, zero beyond `rows` and beyond D (fetch),
// and their place in LDS (put).  The two halves are apart so that the global loads of the next slab fly during the MFMAs of this one.
struct SlabRegs { f32x4 v[2]; };
__device__ __forceinline__ SlabRegs fetch_slab(const float* src, int64_t row0, int64_t rows, int ld, int k0, int D) {
    const int c4 = threadIdx.x & 7;
    SlabRegs s;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = (threadIdx.x >> 3) + 32 * h;
        s.v[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row0 + r < rows && k0 + 4 * c4 < D) s.v[h] = *reinterpret_cast<const f32x4*>(src + (row0 + r) * ld + k0 + 4 * c4);    // D % 4 == 0
    }
    return s;
}
__device__ __forceinline__ void put_slab(float (*dst)[SLD], const SlabRegs& s) {
    const int c4 = threadIdx.x & 7;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = (threadIdx.x >> 3) + 32 * h;
        dst[r][4 * c4 + 0] = s.v[h][0]; dst[r][4 * c4 + 1] = s.v[h][1]; dst[r][4 * c4 + 2] = s.v[h][2]; dst[r][4 * c4 + 3] = s.v[h][3];
    }
}

// The dot products of the A rows a0 .. a0 + 63 with the B rows b0 .. b0 + 63: this wave's 32 x 32 block (A rows qi + .., B rows
// bj + ..).  On entry ra / rb hold the tile's first slabs; on exit those of the tile (a0, b0 + 64) when B has such rows.
// dot_tile_staged: A holds only DA <= D of the chain's D columns, and stage(slab, k0) turns every fetched A slab (zero from column DA
// on) into the operand before it reaches LDS (probe.hip standardises feature rows there); the caller stages the first slab itself.
struct StageAsIs { __device__ __forceinline__ void operator()(SlabRegs&, int) const {} };
template <class Stage>
__device__ __forceinline__ f32x16 dot_tile_staged(float (*As)[SLD], float (*Bs)[SLD], SlabRegs& ra, SlabRegs& rb, const float* A,
                                                  int64_t a0, int64_t arows, int lda, int DA, const float* B, int64_t b0, int64_t brows,
                                                  int ldb, int D, const Stage& stage) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = (wave & 1) * 32, bj = (wave >> 1) * 32;                 // this wave's 32 x 32 block of the tile
    const int li = lane & 31, lh = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < D; k0 += KS) {
        __syncthreads();                                           // the slab's readers (and P's, a tile earlier) are done
        put_slab(As, ra);
        put_slab(Bs, rb);
        __syncthreads();
        // the next slab of this tile, or the first of the next tile (it arrives during the tile's epilogue); none after the last
        const bool more = k0 + KS < D;
        if (more || b0 + TB < brows) {
            ra = fetch_slab(A, a0, arows, lda, more ? k0 + KS : 0, DA);
            stage(ra, more ? k0 + KS : 0);
            rb = fetch_slab(B, more ? b0 : b0 + TB, brows, ldb, more ? k0 + KS : 0, D);
        }
#pragma unroll
        for (int t = 0; t < KS / 2; ++t)                           // lane half h carries k0 + 2 t + h: ascending k
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[qi + li][2 * t + lh], Bs[bj + li][2 * t + lh], acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ f32x16 dot_tile(float (*As)[SLD], float (*Bs)[SLD], SlabRegs& ra, SlabRegs& rb, const float* A, int64_t a0,
                                           int64_t arows, int lda, const float* B, int64_t b0, int64_t brows, int ldb, int D) {
    return dot_tile_staged(As, Bs, ra, rb, A, a0, arows, lda, D, B, b0, brows, ldb, D, StageAsIs{});
}

// the wave's block into P [A row][B row]; barriers on both sides: every wave has read its last slab, and P is whole afterwards
__device__ __forceinline__ void hand_over(float (*P)[PLD], const f32x16& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = (wave & 1) * 32, bj = (wave >> 1) * 32;                 // this wave's 32 x 32 block of the tile
    const int li = lane & 31, lh = lane >> 5;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) P[qi + (i & 3) + 8 * (i >> 2) + 4 * lh][bj + li] = acc[i];
    __syncthreads();
}

// F.normalize's rule for one row held by one wave: ss = lane-strided fmaf(x, x, ss) over the columns l, l + 64, .., the xor tree
// over the 64 lanes, n = sqrtf(ss) -> 1 / fmaxf(n, 1e-12f) (a zero row gives zeros).  `n` receives the norm.
__device__ __forceinline__ float row_inv_norm(const float* x, int D, int lane, float& n) {
    float ss = 0.f;
    for (int c = lane; c < D; c += 64) ss = fmaf(x[c], x[c], ss);
    n = sqrtf(tree_sum(ss));
    return 1.f / fmaxf(n, 1e-12f);
}
