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

namespace {

// numpy's 'symmetric' pad index: valid for any n >= 1 and any offset (also pads wider than the scene)
__device__ __forceinline__ int sym_index(int q, int n) {
    int m = q % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

__device__ __forceinline__ int64_t chunk_pixel(const SceneParams& p, int k) {
    return p.pixels ? p.pixels[k] : p.p0 + k;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void scene_window_kernel(SceneParams p) {
    __shared__ int64_t row_off[9], col_off[9];            // element offsets of the window's 9 source rows / columns
    const int k = blockIdx.x;
    const int64_t pix = chunk_pixel(p, k);
    const bool ok = pix >= 0 && pix < (int64_t)p.H * p.W;   // block-uniform
    const int C = p.C;
    if (ok && threadIdx.x < 18) {
        const int r = (int)(pix / p.W), c = (int)(pix - (int64_t)r * p.W), t = threadIdx.x;
        if (t < 9) row_off[t] = (int64_t)sym_index(r - 4 + t, p.H) * p.W * C;
        else col_off[t - 9] = (int64_t)sym_index(c - 13 + t, p.W) * C;
    }
    __syncthreads();
    const T* src = reinterpret_cast<const T*>(p.scene);
    float* dst = p.out + (int64_t)k * p.sn;
    if (VEC) {                                            // C % 4 == 0, sb == 1, the other strides and `out` 16-byte aligned
        const int C4 = C >> 2;
        for (int e = threadIdx.x; e < 81 * C4; e += 256) {
            const int px = e / C4, b4 = e - px * C4;
            const int i = px / 9, j = px - i * 9;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                const T* s = src + row_off[i] + col_off[j] + 4 * b4;
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
            const float v = ok ? (float)src[row_off[i] + col_off[j] + b] : 0.f;
            dst[(int64_t)b * p.sb + (int64_t)i * p.sh + (int64_t)j * p.sw] = v;
        }
    }
}

// one thread per pixel: a row of at most 256 logits, scanned in order (ties keep the lower index, the first NaN wins)
__global__ __launch_bounds__(256) void class_argmax_kernel(SceneParams p, const float* logits, int ld, int num_class, int first,
                                                           int64_t* map) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= p.N) return;
    const int64_t pix = chunk_pixel(p, k);
    if (pix < 0 || pix >= (int64_t)p.H * p.W) return;
    const float* row = logits + (int64_t)k * ld;
    float best = row[first];
    int arg = first;
    for (int c = first + 1; c < num_class && !__builtin_isnan(best); ++c) {
        const float v = row[c];
        if (v > best || __builtin_isnan(v)) { best = v; arg = c; }
    }
    map[pix] = arg;
}

template <typename T>
void launch_windows(const SceneParams& p, bool vec, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((scene_window_kernel<T, true>), dim3(p.N), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((scene_window_kernel<T, false>), dim3(p.N), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------ fine-tuning batches (Model_Finetuning.py:28-63 `HSIdataset`)
// Sample k of a batch is entry items[k] of a dataset's tables: its pixel (pixels[item], or the item itself), its label, and the
// batch's own flip bits.  The same gather as above; a flip only reverses the 9-entry offset table of its axis, so the copy loop
// is the unflipped one.  An item or a pixel out of range reads nothing: zero window, y = -1, *bad = 1.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void scene_batch_kernel(hsimae_scene_batch_params p) {
    __shared__ int64_t row_off[9], col_off[9];
    const int k = blockIdx.x;
    const int64_t item = p.items[k];                      // every thread the same address: block-uniform
    int64_t pix = -1;
    if (item >= 0 && item < p.n_items) pix = p.pixels ? p.pixels[item] : item;
    const bool ok = pix >= 0 && pix < (int64_t)p.H * p.W;
    const int C = p.C;
    if (ok && threadIdx.x < 18) {
        const int r = (int)(pix / p.W), c = (int)(pix - (int64_t)r * p.W), t = threadIdx.x;
        const int f = p.flips ? p.flips[k] : 0;
        if (t < 9) row_off[t] = (int64_t)sym_index(r - 4 + ((f & 2) ? 8 - t : t), p.H) * p.W * C;
        else col_off[t - 9] = (int64_t)sym_index(c - 4 + ((f & 1) ? 17 - t : t - 9), p.W) * C;
    }
    if (threadIdx.x == 32) {
        if (p.y) p.y[k] = ok ? p.labels[item] : -1;
        if (!ok) *p.bad = 1;                              // every writer stores the same value
    }
    __syncthreads();
    const T* src = reinterpret_cast<const T*>(p.scene);
    float* dst = p.out + (int64_t)k * p.sn;
    if (VEC) {                                            // C % 4 == 0, sb == 1, the other strides and `out` 16-byte aligned
        const int C4 = C >> 2;
        for (int e = threadIdx.x; e < 81 * C4; e += 256) {
            const int px = e / C4, b4 = e - px * C4;
            const int i = px / 9, j = px - i * 9;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                const T* s = src + row_off[i] + col_off[j] + 4 * b4;
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
            const float v = ok ? (float)src[row_off[i] + col_off[j] + b] : 0.f;
            dst[(int64_t)b * p.sb + (int64_t)i * p.sh + (int64_t)j * p.sw] = v;
        }
    }
}

template <typename T>
void launch_batch(const hsimae_scene_batch_params& p, bool vec, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((scene_batch_kernel<T, true>), dim3(p.N), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((scene_batch_kernel<T, false>), dim3(p.N), dim3(256), 0, s, p);
}

}  // namespace

int hs_scene_windows(const SceneParams& p, hipStream_t s) {
    if (p.N <= 0) return HS_OK;
    if (p.H <= 0 || p.W <= 0 || p.C <= 0) return HS_EDIMS;
    const bool vec = (p.C & 3) == 0 && p.sb == 1 && (p.sw & 3) == 0 && (p.sh & 3) == 0 && (p.sn & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(p.scene) & (p.scene_f64 ? 31 : 15)) == 0;
    if (p.scene_f64) launch_windows<double>(p, vec, s);
    else launch_windows<float>(p, vec, s);
    return (int)hipGetLastError();
}

int hs_class_argmax(const SceneParams& p, const float* logits, int ld, int num_class, int first, int64_t* map, hipStream_t s) {
    if (p.N <= 0) return HS_OK;
    hipLaunchKernelGGL(class_argmax_kernel, dim3((p.N + 255) / 256), dim3(256), 0, s, p, logits, ld, num_class, first, map);
    return (int)hipGetLastError();
}

int hs_scene_batch(const hsimae_scene_batch_params& p, hipStream_t s) {
    if (p.N <= 0) return HS_OK;
    if (p.H <= 0 || p.W <= 0 || p.C <= 0) return HS_EDIMS;
    const bool vec = (p.C & 3) == 0 && p.sb == 1 && (p.sw & 3) == 0 && (p.sh & 3) == 0 && (p.sn & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(p.out) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(p.scene) & (p.scene_f64 ? 31 : 15)) == 0;
    if (p.scene_f64) launch_batch<double>(p, vec, s);
    else launch_batch<float>(p, vec, s);
    return (int)hipGetLastError();
}

HS_UNIT_VARIANT_BITS(scene)
