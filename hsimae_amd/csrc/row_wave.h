// What the wave-per-row kernels of the whole-scene family share (cls.hip, prob.hip, knn.hip, kmeans.hip, recon.hip, scene.hip and the
// optimizers' fixed-order sums), each piece once: the 64-lane xor tree, a row's softmax statistics, the argmax of a row held
// lane-strided by one wave, its runner-up, the pixel a row belongs to and the label / confidence / margin maps written there.
// Every sequence here is a bit-exactness contract: the fp64 restatements under tests/*_ref.py state the order of each sum, and
// hsimae_class_prob with one view must give hsimae_class_argmax's label bit for bit.
#pragma once
#include "common.h"

constexpr float HS_LOG2E = 1.4426950408889634f;

// The xor tree, the butterfly over the 64 lanes of a wave: at step s = FIRST, 2 FIRST, .., 32 every lane combines its values with
// those of lane ^ s (Op::f(mine.., theirs..) updates `mine` in place), so after the last step every lane holds the same result,
// formed in the same order.  Several values travel together where the rule needs them (an argmax and its index).  FIRST = 16 merges
// only the four 16-lane rows.  (__shfl_xor serves every type here; the DPP reductions of common.h are for float.)
template <class Op, int FIRST = 1, class... T>
__device__ __forceinline__ void wave_tree(T&... v) {
    for (int s = FIRST; s < 64; s <<= 1) Op::f(v..., __shfl_xor(v, s)...);
}
struct TreeAdd {                                                                 // one sum, or two side by side
    template <class T> static __device__ __forceinline__ void f(T& a, T b) { a += b; }
    template <class T, class U> static __device__ __forceinline__ void f(T& a, U& b, T a2, U b2) { a += a2; b += b2; }
};
struct TreeMax { static __device__ __forceinline__ void f(float& a, float b) { a = fmaxf(a, b); } };
template <class T> __device__ __forceinline__ T tree_sum(T v) { wave_tree<TreeAdd>(v); return v; }      // float, double, int, long long
__device__ __forceinline__ float tree_max(float v) { wave_tree<TreeMax>(v); return v; }

// A row of logits or scores is held by one wave, lane l the columns l, l + 64, ..   exp(z - m), as every softmax here forms it:
__device__ __forceinline__ float row_exp(float z, float m) { return __builtin_amdgcn_exp2f((z - m) * HS_LOG2E); }

// m = the maximum of z[first, C), sum = the sum of exp(z - m) over them: lane-strided and ascending, then the tree
__device__ __forceinline__ void row_softmax_stats(const float* z, int first, int C, int lane, float& m, float& sum) {
    m = -__builtin_inff();
    for (int c = first + lane; c < C; c += 64) m = fmaxf(m, z[c]);
    m = tree_max(m);
    sum = 0.f;
    for (int c = first + lane; c < C; c += 64) sum += row_exp(z[c], m);
    sum = tree_sum(sum);
}

// arg_better (common.h) as the tree's rule; in the second form a payload w follows the winner
struct TreeArg {
    static __device__ __forceinline__ void f(float& v, int& i, float v2, int i2) { arg_better(v, i, v2, i2); }
    static __device__ __forceinline__ void f(float& v, int& i, float& w, float v2, int i2, float w2) {
        const int was = i;
        arg_better(v, i, v2, i2);
        if (i != was) w = w2;
    }
};
// the lanes' candidates (each the best of its own columns, scanned ascending from key = -inf, idx = 0x7fffffff) into the row's
// argmax, in every lane.  The form with a payload takes and returns values: handed the caller's variables by reference, hipcc 7.2
// keeps six more VGPRs live in class_prob_kernel.
__device__ __forceinline__ void wave_argmax(float& key, int& idx) { wave_tree<TreeArg>(key, idx); }
struct ArgVal { float key; int idx; float val; };
__device__ __forceinline__ ArgVal wave_argmax(float key, int idx, float val) { wave_tree<TreeArg>(key, idx, val); return ArgVal{key, idx, val}; }

// the largest of v[c] * scale over the columns [first, C) other than `best` (-inf when there is none); a lane reads its own columns
__device__ __forceinline__ float row_runner_up(const float* v, float scale, int first, int C, int lane, int best) {
    float second = -__builtin_inff();
    for (int c = first + lane; c < C; c += 64)
        if (c != best) second = fmaxf(second, v[c] * scale);
    return tree_max(second);
}

// the pixel of row r of a chunk (pixels[r], or p0 + r), -1 when it lies outside the scene: such a row writes no map
__device__ __forceinline__ int64_t row_pixel(const int64_t* pixels, int64_t p0, int64_t r, int64_t HW) {
    const int64_t pix = pixels ? pixels[r] : p0 + r;
    return pix >= 0 && pix < HW ? pix : -1;
}

// label, winning value and top-1 / top-2 margin (the winning value itself when there is one class) at pixel pix >= 0; one lane calls it
__device__ __forceinline__ void write_maps(int64_t* label_map, float* conf_map, float* margin_map, int64_t pix, int label, float top,
                                           float second, bool one_class) {
    if (pix < 0) return;
    label_map[pix] = label;
    if (conf_map) conf_map[pix] = top;
    if (margin_map) margin_map[pix] = one_class ? top : top - second;
}

// ------------------------------------------------------------------ host side
inline bool misaligned(const void* q, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

// workgroups of 256 threads for one wave per row: ceil(n_rows / 4), at most max_wg (the kernels stride over the rest)
inline unsigned rows_grid(int64_t n_rows, int max_wg) {
    const int64_t quads = (n_rows + 3) / 4;
    return (unsigned)(quads < max_wg ? quads : max_wg);
}
