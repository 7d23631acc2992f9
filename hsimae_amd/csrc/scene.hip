// Whole-scene inference (Model_Finetuning.py:243-300 `test_model`): the padded 9 x 9 window of every pixel cut from the
// HBM-resident scene, and the per-pixel label from the head's logits, written in place into a device-resident [H*W] map.
//
// The reference builds every window on the host (Utils/Preprocessing.py:208-213: np.pad 'symmetric' + splitHSI, 81 copies
// of each pixel) and uploads them.  Here one launch writes a chunk's windows straight into the encoder's input: a pure
// gather, HBM-bound (at C = 32 about 10 KB written per window against ~170 MFLOP of encoder work per Base window), so it
// reads whole pixels (C contiguous values; the 9 pixels of a window row are one contiguous 9*C run away from the border)
// with 16-byte loads and stores where the layout allows, as cube_gather_kernel does.  The conversion fp64 -> fp32 is the
// round-to-nearest-even v_cvt_f32_f64, what torch.tensor(x, dtype=torch.float32) does: bit-exact windows.
#include "common.h"
#include "kernels.h"
#include "row_wave.h"

namespace {

// numpy's 'symmetric' pad index: valid for any n >= 1 and any offset (also pads wider than the scene)
__device__ __forceinline__ int sym_index(int q, int n) {
    int m = q % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// Where window k of a launch comes from: its pixel (-1: outside the scene, a zero window) and its flip bits.  The two entry points
// differ in this and in what else window_pixel writes; scene, H, W, C, out and the strides have the same names in both parameter
// blocks.  hsimae_scene_windows: pixel k of the chunk, no flip, nothing else written
__device__ __forceinline__ int64_t window_pixel(const SceneParams& p, int k) { return row_pixel(p.pixels, p.p0, k, (int64_t)p.H * p.W); }
__device__ __forceinline__ int window_flip(const SceneParams&, int) { return 0; }
// hsimae_scene_batch (Model_Finetuning.py:28-63 `HSIdataset`): sample k is entry items[k] of a dataset's tables: its pixel (pixels[item],
// or the item itself), its label (written here), and the batch's own flip bits.  An item or a pixel out of range: zero window,
// y = -1, *bad = 1.
__device__ __forceinline__ int64_t window_pixel(const hsimae_scene_batch_params& p, int k) {
    const int64_t item = p.items[k];                      // every thread the same address: block-uniform
    const int64_t pix = item >= 0 && item < p.n_items ? row_pixel(p.pixels, 0, item, (int64_t)p.H * p.W) : -1;
    if (threadIdx.x == 32) {
        if (p.y) p.y[k] = pix >= 0 ? p.labels[item] : -1;
        if (pix < 0) *p.bad = 1;                          // every writer stores the same value
    }
    return pix;
}
__device__ __forceinline__ int window_flip(const hsimae_scene_batch_params& p, int k) { return p.flips ? p.flips[k] : 0; }

// entry t < 18 of the window's offset table around pixel (r, c): the element offsets of its 9 source rows (t < 9), then of its 9
// source columns.  A flip only reverses the table of its axis (bit 1: rows, bit 0: columns), so the copy below is the unflipped one.
__device__ __forceinline__ int64_t window_offset(int t, int r, int c, int flip, int H, int W, int C) {
    if (t < 9) return (int64_t)sym_index(r - 4 + ((flip & 2) ? 8 - t : t), H) * W * C;
    return (int64_t)sym_index(c - 4 + ((flip & 1) ? 17 - t : t - 9), W) * C;
}

// the 81 pixels of window k by a workgroup of 256: whole pixels of C contiguous values, zeros when !ok (block-uniform).
// VEC: C % 4 == 0, sb == 1, the other strides and both buffers 16-byte aligned (launch_cut below).
template <typename T, bool VEC, class P>
__device__ __forceinline__ void copy_window(const P& p, const int64_t* off, bool ok, int k) {
    const T* src = reinterpret_cast<const T*>(p.scene);
    float* dst = p.out + (int64_t)k * p.sn;
    const int C = p.C;
    if (VEC) {
        const int C4 = C >> 2;
        for (int e = threadIdx.x; e < 81 * C4; e += 256) {
            const int px = e / C4, b4 = e - px * C4;
            const int i = px / 9, j = px - i * 9;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                const T* s = src + off[i] + off[9 + j] + 4 * b4;
                if (sizeof(T) == 4) {
                    o = *reinterpret_cast<const float4*>(s);
                } else {
                    const double2 a = reinterpret_cast<const double2*>(s)[0], b = reinterpret_cast<const double2*>(s)[1];
                    o = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
                }
            }
            *reinterpret_cast<float4*>(dst + (int64_t)i * p.sh + (int64_t)j * p.sw + 4 * b4) = o;
        }
    } else {
        for (int e = threadIdx.x; e < 81 * C; e += 256) {
            const int px = e / C, b = e - px * C;
            const int i = px / 9, j = px - i * 9;
            const float v = ok ? (float)src[off[i] + off[9 + j] + b] : 0.f;
            dst[(int64_t)b * p.sb + (int64_t)i * p.sh + (int64_t)j * p.sw] = v;
        }
    }
}

// one workgroup per window; P = the entry point's parameter block
template <typename T, bool VEC, class P>
__global__ __launch_bounds__(256) void scene_cut_kernel(P p) {
    __shared__ int64_t off[18];
    const int k = blockIdx.x;
    const int64_t pix = window_pixel(p, k);
    const bool ok = pix >= 0;                             // block-uniform
    if (ok && threadIdx.x < 18) {
        const int r = (int)(pix / p.W), c = (int)(pix - (int64_t)r * p.W);
        off[threadIdx.x] = window_offset(threadIdx.x, r, c, window_flip(p, k), p.H, p.W, p.C);
    }
    __syncthreads();
    copy_window<T, VEC>(p, off, ok, k);
}

// one thread per pixel: a row of at most 256 logits, scanned in order (ties keep the lower index, the first NaN wins)
__global__ __launch_bounds__(256) void class_argmax_kernel(SceneParams p, const float* logits, int ld, int num_class, int first,
                                                           int64_t* map) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= p.N) return;
    const int64_t pix = row_pixel(p.pixels, p.p0, k, (int64_t)p.H * p.W);
    if (pix < 0) return;
    const float* row = logits + (int64_t)k * ld;
    float best = row[first];
    int arg = first;
    for (int c = first + 1; c < num_class && !__builtin_isnan(best); ++c) {
        const float v = row[c];
        if (v > best || __builtin_isnan(v)) { best = v; arg = c; }
    }
    map[pix] = arg;
}

template <class P>
int launch_cut(const P& p, hipStream_t s) {
    if (p.N <= 0) return HS_OK;
    if (p.H <= 0 || p.W <= 0 || p.C <= 0) return HS_EDIMS;
    const bool f64 = p.scene_f64 != 0;
    const bool vec = (p.C & 3) == 0 && p.sb == 1 && (p.sw & 3) == 0 && (p.sh & 3) == 0 && (p.sn & 3) == 0 && !misaligned(p.out, 15) &&
                     !misaligned(p.scene, f64 ? 31 : 15);
    if (f64 && vec) hipLaunchKernelGGL((scene_cut_kernel<double, true, P>), dim3(p.N), dim3(256), 0, s, p);
    else if (f64) hipLaunchKernelGGL((scene_cut_kernel<double, false, P>), dim3(p.N), dim3(256), 0, s, p);
    else if (vec) hipLaunchKernelGGL((scene_cut_kernel<float, true, P>), dim3(p.N), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((scene_cut_kernel<float, false, P>), dim3(p.N), dim3(256), 0, s, p);
    return (int)hipGetLastError();
}

}  // namespace

int hs_scene_windows(const SceneParams& p, hipStream_t s) { return launch_cut(p, s); }

int hs_class_argmax(const SceneParams& p, const float* logits, int ld, int num_class, int first, int64_t* map, hipStream_t s) {
    if (p.N <= 0) return HS_OK;
    hipLaunchKernelGGL(class_argmax_kernel, dim3((p.N + 255) / 256), dim3(256), 0, s, p, logits, ld, num_class, first, map);
    return (int)hipGetLastError();
}

int hs_scene_batch(const hsimae_scene_batch_params& p, hipStream_t s) { return launch_cut(p, s); }

HS_UNIT_VARIANT_BITS(scene)
