/* libhsimae_hip.so — C ABI of the MI355X (gfx950) kernels behind the HSIMAE pretraining path.
 *
 * The reference (Ryan21wy/HSIMAE) has no native code: its "operator API" for this path is the
 * `HSIMAE` nn.Module (Models.py:309-634) whose forward dispatches ~700 ATen kernels and whose
 * backward is autograd.  A reference-side integration binds the entry points below with ctypes
 *  in place of those ATen calls.  Every entry point names the reference
 * lines it replaces.
 *
 * Contract
 *  - every pointer is device memory owned by the caller (PyTorch tensors); the library never
 *    allocates, frees or retains device memory;
 *  - process-wide state is limited to (a) per DEVICE, created on first use and kept for the life of the process:
 *    one non-blocking side stream that runs the spectral axis stack next to the spatial one, plus a small pool of
 *    timing-disabled events (fork / join, one per gradient range handed to the bucket callback) — the whole-pass
 *    entry points look them up by the device that is current when they are called, so the caller must make the
 *    device of its pointers current (HSIMAE_TWO_STREAMS=0 keeps everything on the caller's stream); (b) the cached
 *    values of the HSIMAE_* environment switches (kernel-generation A/B switches for tests, read once);
 *  - all work is enqueued on the caller's `stream` (hipStream_t passed as void*) or on the side stream, which is
 *    forked from and joined back into it with events inside the same call: no implicit sync, nothing outlives the
 *    caller's stream order;
 *  - return 0 on success; <0 argument errors (HSIMAE_E*); >0 a hipError_t from the launch.
 *    Nothing throws or exits across the boundary.  hsimae_strerror() names a code.
 *  - bf16 buffers are raw 16-bit words (`hs_bf16`); activation buffers that feed a GEMM as its
 *    K operand are zero-padded to a multiple of 32 columns by the kernel that produces them.
 */
#ifndef HSIMAE_HIP_H
#define HSIMAE_HIP_H
#include <stdint.h>

#ifdef __HIPCC__
typedef __bf16 hs_bf16;
#else
typedef uint16_t hs_bf16;
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)

#define HSIMAE_OK 0
#define HSIMAE_EDIMS (-1)        /* bad dimensions / strides */
#define HSIMAE_EUNSUPPORTED (-2) /* configuration outside what the kernels are built for */
#define HSIMAE_EALIGN (-3)       /* misaligned pointer */
#define HSIMAE_ENULL (-4)        /* required pointer is NULL */
#define HSIMAE_ENOFORWARD (-5)   /* a backward entry point was given a workspace that no forward entry point of this process has
                                    filled: the backward follows the schedule its forward recorded (which intermediates exist,
                                    q|k|v saved or recomputed, ...) and never re-derives it from the environment */

/* ABI version of this header; hsimae_version() returns the value the loaded library was built with, and a binder must
 * refuse a library that answers differently (hsimae_amd/_lib.py does).  104 (round 5): HSIMAE_ENOFORWARD, schedule recorded
 * by the forward; 103 -> 104 also covers round 4's incompatible change of the weight-gradient parameter block (t[8] -> t[16]), which had
 * shipped without a bump.  105 (round 6): hsimae_build_info; hsimae_attn_params lost the fused-projection fields
 * (proj_w .. rowscale) with the whole-sample d = 128 attention kernels they drove (superseded by the fused attention half).
 * 106: hsimae_scene_params, hsimae_scene_windows, hsimae_class_argmax (whole-scene inference).
 * 107: hsimae_attn_block_weights, hsimae_attn_block_fwd / _bwd (the fused attention halves, per kernel); hsimae_attn_fwd / _bwd
 * refuse invalid mode, len_l, Ts, kv_off, ld and lddo values they used to launch with.
 * 108: hsimae_gwpca_params, hsimae_gwpca_workspace_bytes, hsimae_gwpca_fit, hsimae_gwpca_apply (group-wise PCA of a raw scene). */
#define HSIMAE_VERSION 108
int hsimae_version(void);
/* What the loaded library was built from (round 6).  `variant_bits` has one bit per compile-time switch that makes a kernel
 * compute WRONG results on purpose (timing ablations: HS_ABL_*, HS_EXP_*, HS_EXPERIMENT_*) or adds instrumentation
 * (HS_PHASE_TIMING), OR-ed over every translation unit of the library; hsimae_variant_name(bit) names bit 0..31 (NULL: unused).
 * A binder must refuse a library with any bit set unless the caller asked for a variant (hsimae_amd/_lib.py:
 * HSIMAE_ALLOW_VARIANT=1).  `kernel_source_hash` = the first 64 bits of hsimae_amd.build.kernel_source_hash() at build time,
 * `flags_hash` = the same of the hipcc flag list (0: built by hand, outside hsimae_amd/build.py); `default_flags` = 1 when that
 * list is build.py's own, i.e. no tuning knob (-DHS_*) was overridden either. */
typedef struct {
    int32_t abi_version; uint32_t variant_bits; uint64_t kernel_source_hash; uint64_t flags_hash; int32_t default_flags; int32_t reserved;
} hsimae_build_info_t;
int hsimae_build_info(hsimae_build_info_t* out);
const char* hsimae_variant_name(int bit);
const char* hsimae_strerror(int code);
/* 1 if the library runs the two axis stacks of the encoder on two streams on the CURRENT device (the side stream is created
 * on first use; HSIMAE_TWO_STREAMS=0 or a failed hipStreamCreate give 0).  The order in which hsimae_backward reports gradient
 * ranges depends on it, so data-parallel callers check that every rank answers the same (hsimae_amd/model.py
 * enable_data_parallel) before they issue collectives in callback order. */
int hsimae_two_streams_active(void);

/* ------------------------------------------------------------------ model geometry */
/* Mirrors the HSIMAE constructor arguments that shape the tensors (Models.py:312-332) for the
 * supported family: img_size 9, patch_size 3, b_patch_size 8, in_chans 1, qkv bias on; embed_dim / dec_dim multiples
 * of 8 up to 512 with head dim 8 or 16 (widths that are not multiples of 32 run zero-padded to the next one). */
typedef struct {
    int32_t bands;          /* B, multiple of 8; T = B/8 */
    int32_t embed_dim;      /* D */
    int32_t depth;          /* total encoder depth */
    int32_t s_depth;        /* depth of each axis stack (blocks_1 / blocks_2) */
    int32_t num_heads;
    int32_t dec_dim;        /* Dd */
    int32_t dec_depth;
    int32_t dec_heads;
    int32_t hidden;         /* SwiGLU hidden of the encoder blocks (Models.py:225) */
    int32_t dec_hidden;
    int32_t norm_pix_loss;
    int32_t precision;      /* HSIMAE_PREC_BF16 (0) or HSIMAE_PREC_FP8: operand type of the encoder linears (see below) */
} hsimae_config;
/* Operand type the encoder blocks' stand-alone linears actually run in for this configuration: HSIMAE_PREC_FP8 only when
   cfg->precision is FP8 AND the width is one where the MX GEMMs are used (embed_dim >= 512, or HSIMAE_FP8_UNFUSED=1 in the
   environment); otherwise HSIMAE_PREC_BF16 — precision = FP8 at embed_dim 128 / 256 computes exactly what BF16 computes.
   < 0: invalid configuration.  (bench.py prices its roofline against the peak of THIS type.) */
int hsimae_effective_precision(const hsimae_config* cfg);
/* precision: BF16 = bf16 MFMA operands everywhere.  FP8 = the encoder blocks' linears (q|k|v, proj, w1|w3, w2 and their
 * data gradients) run on the MX block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) with OCP e4m3 operands: weights are
 * quantised at pack time, activations as they are staged, both with one e8m0 scale per 32 consecutive K elements (MX),
 * fp32 accumulate; weight gradients, attention, LayerNorm, the decoder and the loss stay as in BF16.  fp32 masters and the
 * state_dict are untouched. */
enum { HSIMAE_PREC_BF16 = 0, HSIMAE_PREC_FP8 = 1 };

/* Flat fp32 parameter buffer: parameters in `named_parameters()` registration order
 * (Models.py:342-424), each contiguous, no padding.  Returns the number of parameter tensors;
 * offsets[i]/sizes[i] (in floats) are filled when non-NULL. Total floats = offsets[n-1]+sizes[n-1]. */
int hsimae_param_layout(const hsimae_config* cfg, int64_t* offsets, int64_t* sizes, int max_entries);

/* bf16 packed weight images (MFMA B-fragment order; W and W^T of every linear). */
int64_t hsimae_wpk_elems(const hsimae_config* cfg);
/* Host-side descriptor table for hsimae_pack_params: fill `table_host` (size from
 * hsimae_pack_table_bytes) for the given device pointers; the caller uploads it to the device. */
int64_t hsimae_pack_table_bytes(const hsimae_config* cfg);
int hsimae_build_pack_table(const hsimae_config* cfg, const float* params_dev, hs_bf16* wpk_dev, void* table_host);
/* fp32 master weights -> packed bf16 images; run after every optimizer step. */
int hsimae_pack_params(const hsimae_config* cfg, const void* table_dev, void* stream);

/* ------------------------------------------------------------------ whole-pass entry points */
/* Replaces HSIMAE.forward (Models.py:627-634): forward_encoder 537-571, forward_decoder 573-601,
 * forward_loss 603-616, recons 618-625; and, for hsimae_backward, the autograd backward of all
 * of it (Model_Pretraining.py:101). */
typedef struct {
    const float* x;               /* [N,1,B,9,9] fp32 cube, arbitrary strides (elements) */
    int64_t sn, sb, sh, sw;
    int32_t N, len_t, len_l;      /* grid drawn on the host (Models.py:484-493) */
    const float* noise1;          /* [N,T]  (Models.py:506) */
    const float* noise2;          /* [N,9]  (Models.py:513) */
    const float* params;          /* flat fp32 parameters */
    const hs_bf16* wpk;           /* packed images */
    void* workspace;              /* hsimae_workspace_bytes() bytes, 256-B aligned.  When embed_dim or dec_dim is not a multiple
                                     of 32, rows are stored at the width rounded up to 32 and the columns past the true
                                     width must be zeros: zero-fill the workspace once before its first use with a given
                                     (N, len_t * len_l) — the kernels never write anything but zeros there. */
    int64_t workspace_bytes;
    float grad_scale;             /* folded into dLoss/dpred (1/world_size for data parallel) */
    int32_t want_recons;          /* write pred_img / mask_img */
    /* outputs */
    float* loss;                  /* [1] */
    float* pred_img;              /* [N,1,B,9,9] contiguous */
    float* mask_img;              /* [N,1,B,9,9] contiguous */
    float* mask;                  /* [N,T*9] 0 keep / 1 remove */
    int32_t* ids_keep;            /* [N,K] ascending */
    int32_t* ids_restore;         /* [N,T*9] */
    float* latent;                /* optional [N*K, D] fp32 copy of the encoder output (may be NULL) */
    float* pred;                  /* optional [N*T*9, 72] fp32 copy of decoder_pred output (may be NULL) */
    /* optional stochastic depth of the encoder blocks (DropPath, Models.py:235-263, 304-305; fine-tuning only):
       per-ROW factors (0 or 1/keep_prob, equal within a sequence) for the attention branch and the MLP branch of
       every encoder block, [n_enc_blocks][2][N*K] fp32 in execution order blocks_1[0..], blocks_2[0..], blocks[0..];
       x += scale * branch(x).  NULL = no DropPath.  Must be the same array in forward and backward. */
    const float* drop_scale;
    /* optional (hsimae_backward / hsimae_encode_backward with a bucket callback): the stream the callback's consumer
       launches its collectives from.  Before each callback the library makes this stream wait (event) for the kernels that
       complete the reported range — including the ones on the side stream — so the ranges of the two axis stacks are
       reported block by block instead of after the join.  NULL: ranges are reported once they are complete on `stream`. */
    void* bucket_stream;
    /* optional deterministic gradient reduction (hsimae_backward / _encode_backward / _decode_backward): an int64 buffer
       with one element per element of `grads` (contents irrelevant on entry).  Weight-gradient partial sums are then
       accumulated in 64-bit fixed point with integer atomics (order-independent) and converted to fp32 at the end, so two
       runs on the same inputs produce bit-identical gradients.  NULL: fp32 atomics (faster; last-bit run-to-run noise). */
    int64_t* det_acc;
} hsimae_io;

int64_t hsimae_workspace_bytes(const hsimae_config* cfg, int32_t N, int32_t len_t, int32_t len_l);
int hsimae_forward(const hsimae_config* cfg, const hsimae_io* io, void* stream);

/* Called on the host thread right after the kernels that complete the gradients of
 * grads[off, off+len) have been enqueued (reverse registration order, so buckets are contiguous
 * suffixes of the flat buffer).  Used to start the RCCL all-reduce of that bucket on a side stream. */
typedef void (*hsimae_bucket_cb)(int32_t stage, int64_t off, int64_t len, void* user);
/* grads: flat fp32 buffer, same layout as params, zeroed by the caller (weight grads are
 * accumulated with atomics). */
int hsimae_backward(const hsimae_config* cfg, const hsimae_io* io, float* grads, hsimae_bucket_cb cb, void* user,
                    void* stream);

/* ------------------------------------------------------------------ per-kernel entry points */
/* Structured random masking, closed form of Models.py:495-535 (bit-exact given the noise). */
typedef struct {
    const float* noise1; const float* noise2; int32_t N, T, L, len_t, len_l;
    int32_t* ids_keep; int32_t* ids_restore; float* mask;
} hsimae_mask_params;
int hsimae_mask_from_noise(const hsimae_mask_params* p, void* stream);

/* Kept-token patch rows of the cube as a bf16 GEMM operand [N*K, 96] (Conv3d k=s=(8,3,3) == GEMM
 * with K=72, Models.py:147-158; selection Models.py:527-528 fused in). */
typedef struct {
    const float* x; int64_t sn, sb, sh, sw; int32_t N, T, K; const int32_t* ids_keep;
    hs_bf16* out; int32_t* pos_ids;
} hsimae_patch_params;
int hsimae_patch_gather(const hsimae_patch_params* p, void* stream);

/* Row-panel MFMA GEMM out = epi(pro(A) * W^T) — every nn.Linear of Attention/SwiGLU/Block
 * (Models.py:180-184, 226-228, 402, 420) with LayerNorm (Models.py:288, 299, 399, 419) fused
 * as prologue and bias / residual / SiLU-gate (Models.py:232, 304-305) as epilogue. */
enum { HSIMAE_A_BF16 = 0, HSIMAE_A_F32 = 1, HSIMAE_A_F32_LN = 2 };
enum { HSIMAE_E_BF16 = 0, HSIMAE_E_F32 = 1, HSIMAE_E_RES_F32 = 2, HSIMAE_E_POS_F32 = 3, HSIMAE_E_SWIGLU = 4,
       HSIMAE_E_SWIGLU_BWD = 5,
       /* E_LN_BWD: the product is dL/d(LayerNorm output); the epilogue applies the LayerNorm backward (autograd of
          Models.py:304 `x + attn(norm1(x))` w.r.t. x) in place of a separate pass: out = res + LNbwd(acc; lnx, gamma)
          (+ out when `accumulate`; out may be res), dgamma / dbeta accumulated with atomics, or committed in 64-bit fixed
          point when det_acc is set.  Needs N == n_valid, N = 128, 256 or 512 (bf16) or 256 / 512 (fp8).  u_out (a bf16 copy
          of out, ld = ldu) is written at N = 256 / 512 only; at N = 128 a non-NULL u_out is refused (HSIMAE_EUNSUPPORTED). */
       HSIMAE_E_LN_BWD = 6 };
/* Columns [n_valid, N) of the output (N a multiple of 16, n_valid <= N): E_F32 / E_RES_F32 / E_POS_F32 leave them untouched
   (n_valid must be a multiple of 8); E_BF16 and E_SWIGLU (out and both halves of h13) write them as exact zeros;
   E_SWIGLU_BWD and E_LN_BWD use all N columns.  Nothing past N in a row, nor past M rows, is written.  M = 0 is a no-op. */
typedef struct {
    const void* A; int32_t lda;
    int32_t M, N, K;
    int32_t n_valid;
    const hs_bf16* W; const hs_bf16* W2;
    const float* bias; const float* bias2;
    const float* gamma; const float* beta;
    float* stats;
    hs_bf16* u_out; int32_t ldu;
    void* out; int32_t ldo;
    const float* res; const float* res2; int32_t ldr;
    const float* pos; const int32_t* ids; int32_t ldpos;
    hs_bf16* h13; int32_t ldh; int32_t hoff;
    const float* lnx; float* dgamma; float* dbeta; int32_t accumulate;    /* E_LN_BWD only (lnx: the LayerNorm's input, ld = ldr) */
    /* optional per-row factors [M] (DropPath): a_rowscale multiplies the rows of an A_F32 operand as it is staged;
       out_rowscale multiplies (product + bias) before the residual is added in E_RES_F32.  NULL = 1. */
    const float* a_rowscale; const float* out_rowscale;
    /* prec = HSIMAE_PREC_FP8: the MX block-scaled e4m3 form of the same product (fp32 accumulate, same epilogues except
       E_POS_F32, and E_LN_BWD at N = 256 / 512 only).  A is quantised on the fly; W8 / S8 (and W8b / S8b for the second matrix of E_SWIGLU) are the
       e4m3 image and its e8m0 scale image of the weight as produced by hsimae_pack_matrix with desc.fp8 = 1
       (K padded to a multiple of 128).  W / W2 are ignored.  prec = 0: bf16, the fields below are ignored. */
    int32_t prec;
    const uint8_t* W8; const uint8_t* S8; const uint8_t* W8b; const uint8_t* S8b;
    /* A_F32_LN: number of leading columns the LayerNorm runs over when the rows are stored wider than the model width
       (K = storage width, a multiple of 32; the columns past ln_width are not read, they stage and u_out-store as zeros); 0 = K.
       Must be a multiple of 8 and <= K (HSIMAE_EDIMS otherwise). */
    int32_t ln_width;
    const float* det_base; int64_t* det_acc;      /* E_LN_BWD: deterministic dgamma / dbeta commits, as in hsimae_lnbwd_params */
} hsimae_gemm_params;
int hsimae_gemm(const hsimae_gemm_params* p, int32_t a_kind, int32_t epilogue, void* stream);
/* The same kernel with the row-panel height (bm: 64 or 128) and the depth of an A chunk (kc: 128 or 256; ignored by the
 * LayerNorm prologue, which stages all of K, by fp8, which stages 512, and by E_LN_BWD, which ignores both) forced instead of
 * chosen by shape; 0 = the shape rule.  Measurement hook (scripts/gemm_sweep.py): every tiling runs the same k-steps in the
 * same order into the same accumulators, so results are bit-identical for every tiling (tests/test_gpu_gemm.py). */
int hsimae_gemm_tiled(const hsimae_gemm_params* p, int32_t a_kind, int32_t epilogue, int32_t bm, int32_t kc, void* stream);

/* One fp32 matrix -> packed image (placement n_off/k_off lets q|k|v or w1|w3 share an image). */
typedef struct {
    const float* src; int32_t rows, cols;
    int32_t transpose;
    int32_t n_off, k_off;
    int32_t KS;
    hs_bf16* dst;
    /* fp8 = 1: quantise to the MX e4m3 image instead (hsimae_gemm_params.prec): KS = 128-deep k-steps of the image
       (K padded to a multiple of 128), dst = the e4m3 image (bytes), scales = its e8m0 image, one dword per (n-tile,
       512-deep chunk, lane).  k_off and the source's K extent must be multiples of 32 (a scale block never straddles
       two sources).  Both images must be zero-filled once before the first pack. */
    int32_t fp8;
    uint8_t* scales;
} hsimae_pack_desc;
int hsimae_pack_matrix(const hsimae_pack_desc* desc_dev, int32_t ndesc, int32_t max_elems, void* stream);

/* MLP half of an encoder Block in one kernel each way (Models.py:305 `x + mlp(norm2(x))`, SwiGLU :231-232):
 * forward  x2 = x1 + rowscale * (b2 + (silu(u2 W1^T + b1) * (u2 W3^T + b3)) W2^T) (+ res2), u2 = LN2(x1); backward recomputes
 * u2 / h1 / h3 and writes dx1 (fp32) plus the bf16 operands of the block's weight gradients: u2, dh1|dh3 [M, 2 hp], g [M, hp]
 * (columns [hidden, hp) are zeros), dY and dx1 copies; LayerNorm-2 parameter grads are accumulated onto g_n2w / g_n2b.
 * Accepted (d, hp), hp = hidden rounded up to 32: (128, 352) Base, (256, 704) Large, (64, 192) the decoder width, i.e. hidden in
 * (hp - 32, hp]; anything else is HSIMAE_EUNSUPPORTED.  w1b / w3b are read below `hidden` only.
 * Weight images as produced by hsimae_pack_params (w13T = W1^T | W3^T along K, W3^T at k = hp).  rowscale / rs_mlp / rs_attn:
 * DropPath row factors (NULL = 1): dyb = bf16(rs_mlp dY), dx1b = bf16(rs_attn dx1), dx1 itself carries neither.
 * Optional outputs of the backward, each NULL or passed as a whole: {u2, dyb}, {dh13, g}, dx1b; dx1 does not depend on them.
 * Returns: M <= 0: HSIMAE_OK, nothing touched.  HSIMAE_ENULL: x1 / x2 / w (forward), x1 / dy / dx1 / w / g_n2w / g_n2b
 * (backward) NULL, or one of {u2, dyb} / {dh13, g} without the other.  HSIMAE_EDIMS: 0 < plane_rows < M. */
typedef struct {
    const float* n2w; const float* n2b; const float* w1b; const float* w3b; const float* w2b;
    const hs_bf16* w1; const hs_bf16* w3; const hs_bf16* w2; const hs_bf16* w2T; const hs_bf16* w13T;
    int32_t hidden;
} hsimae_mlp_weights;
int hsimae_enc_mlp_fwd(const float* x1, const float* res2, float* x2, int32_t M, int32_t d, const hsimae_mlp_weights* w,
                       const float* rowscale, void* stream);
/* plane_rows = 0: dh13 [M][2 * hp], g [M][hp] row-major (hp = hidden rounded up to 32).  plane_rows = R >= M: 64-column planes
 * (see hsimae_wgrad_task): g = [P][R][64], dh13 = dh1 [P][R][64] followed by dh3 [P][R][64], P = ceil(hp / 64); rows past M
 * and the columns past hp of the last plane are not written. */
int hsimae_enc_mlp_bwd(const float* x1, const float* dy, float* dx1, hs_bf16* u2, hs_bf16* dh13, hs_bf16* g, hs_bf16* dyb,
                       hs_bf16* dx1b, int32_t M, int32_t d, const hsimae_mlp_weights* w, float* g_n2w, float* g_n2b,
                       const float* rs_mlp, const float* rs_attn, int32_t plane_rows, void* stream);

/* Masked multi-head attention over one sample's tokens (Models.py:192-215) and its backward.
 * Rows are sample-major: token t of sample s is row s * Ts + t, rows [0, nsamples * Ts).  Token i attends to token j when both
 * are in the same class: mode 0 one class, mode 1 class = i / len_l, mode 2 class = i % len_l (len_l >= 1; Ts need not be a
 * multiple of it).  Head h owns columns [h hd, (h + 1) hd) of q, k, v, o; q at column 0 of a qkv row, k at kv_off, v at 2 kv_off.
 * Scores are q k^T / sqrt(hd).  hd = 16 serves Ts <= 112, hd = 8 Ts <= 224 (else HSIMAE_EUNSUPPORTED).
 * forward : o [rows][ldo], columns [0, d) (nothing past d is written); lse [rows][heads] when non-NULL: the logsumexp of the
 *           row's scores in LOG2 units, log2 sum_j 2^(s_ij log2 e) (what the backward takes back).
 * backward: from dout = dL/do [rows][lddo] and the forward's lse (and o) -> dqkv [rows][ld]: dq, dk, dv in columns [0, d),
 *           [kv_off, kv_off + d), [2 kv_off, 2 kv_off + d); the columns between them and past 2 kv_off + d are not written
 *           (they keep what the caller put there).  dqkv may not alias qkv or dout.
 * Refused: d != heads * hd, ld % 8, ldo % 4, ld < 2 kv_off + d, ldo < d, Ts < 1, len_l < 1 in mode 1 / 2, kv_off not 0 and
 * (< d or not a multiple of 8), backward: lddo < d or lddo % 8 (HSIMAE_EDIMS); mode not 0 / 1 / 2 (HSIMAE_EUNSUPPORTED);
 * qkv / o NULL, backward: dout / dqkv NULL (HSIMAE_ENULL), lse NULL (HSIMAE_EUNSUPPORTED).  nsamples <= 0 is a no-op. */
typedef struct {
    const hs_bf16* qkv; int32_t ld;
    int32_t d, heads, hd;
    int32_t Ts;
    int32_t nsamples;
    int32_t mode, len_l;
    hs_bf16* o; int32_t ldo;
    float* lse;
    const hs_bf16* dout; int32_t lddo;
    hs_bf16* dqkv;
    /* column offset of k (and 2x: of v) inside a qkv / dqkv row when rows are stored wider than d (storage width); 0 = d */
    int32_t kv_off;
} hsimae_attn_params;
int hsimae_attn_fwd(const hsimae_attn_params* p, void* stream);
int hsimae_attn_bwd(const hsimae_attn_params* p, void* stream);

/* The attention half of an encoder Block (Models.py:304 `x + drop_path(attn(norm1(x)))`, Attention.forward :192-219) in one
   persistent kernel each way, as hsimae_forward / hsimae_backward run it at d = 128 with 8 heads (blk128_*) and d = 256 with 16
   heads (blk256_*) — exposed per kernel for the parity tests.  Any other (d, heads) is HSIMAE_EUNSUPPORTED.  Rows are unpadded
   and sample-major (row s * Ts + t), 1 <= Ts <= 32; mode / len_l as in hsimae_attn_params; at d = 256 nsamples * Ts * 3 d
   must stay below 2^31.  Every row pointer must be 16-byte aligned (HSIMAE_EALIGN).  Nothing outside rows [0, nsamples * Ts)
   nor past the columns named below is written.
   Weights: fp32 n1w / n1b (LayerNorm-1), bqkv = bq | bk | bv [3 d], pb [d]; bf16 images as hsimae_pack_matrix makes them:
   qkv = Wq | Wk | Wv [3 d][d], p = Wp [d][d], qkvT = (Wq | Wk | Wv)^T [d][3 d], pT = Wp^T [d][d] (KS = K / 32). */
typedef struct {
    const float *n1w, *n1b, *bqkv, *pb;
    const hs_bf16 *qkv, *p, *qkvT, *pT;
} hsimae_attn_block_weights;
/* forward: x [rows][d] fp32 -> u = LN1(x) bf16 [rows][d]; q|k|v bf16 [rows][3 d] (q | k | v, bias added; NULL: not written,
   d = 128 only — the backward then recomputes them from u); o bf16 [rows][d] (the attention output); lse fp32 [rows][heads]
   (log2-domain logsumexp, as in hsimae_attn_params); x1 = x + rowscale * (o Wp^T + pb) fp32 [rows][d].  rowscale [rows]:
   optional DropPath factors, NULL = 1. */
int hsimae_attn_block_fwd(const hsimae_attn_block_weights* w, const float* x, hs_bf16* u, hs_bf16* qkv, hs_bf16* o, float* lse,
                          float* x1, const float* rowscale, int32_t d, int32_t heads, int32_t Ts, int32_t nsamples, int32_t mode,
                          int32_t len_l, void* stream);
/* backward: dO = dx1b Wp (bf16, formed inside), the attention backward, du = dq|dk|dv Wqkv and the LayerNorm-1 backward.
   Inputs: the forward's q|k|v, u, o, lse and x; dx1b = bf16 of dL/d(attn branch output) with the DropPath factor folded in;
   dx1 = dL/dx1 fp32 (the residual path).  qkv NULL: recompute q|k|v from u (d = 128 only; HSIMAE_EUNSUPPORTED at d = 256).
   Outputs: dqkv bf16 [rows][3 d] = dq | dk | dv (whole rows); dx fp32 [rows][d] = dx1 + LN1-backward(du) (+ what dx held when
   `accumulate`); dgamma / dbeta [d] fp32: the LayerNorm-1 parameter gradients ADDED to what they hold (float
   atomics).  det_acc: optional int64 scratch [2 d] (contents irrelevant); when given, dbeta must be dgamma + d (HSIMAE_EDIMS
   otherwise), the sums are committed in 64-bit fixed point (bit-reproducible) and the call converts them itself: dgamma /
   dbeta come back final.  Same refusals as the forward. */
int hsimae_attn_block_bwd(const hsimae_attn_block_weights* w, const hs_bf16* qkv, const hs_bf16* u, const hs_bf16* o, const float* lse,
                          const hs_bf16* dx1b, const float* dx1, const float* x, hs_bf16* dqkv, float* dx, float* dgamma, float* dbeta,
                          int64_t* det_acc, int32_t accumulate, int32_t d, int32_t heads, int32_t Ts, int32_t nsamples, int32_t mode,
                          int32_t len_l, void* stream);

/* One fused decoder Block (Models.py:303-306 at width 64, 8 heads of 8, SwiGLU hidden 164..192 — hp = 192, the image height
   the kernels are compiled for; any other hidden width returns HSIMAE_EUNSUPPORTED; sequences of 16..112 tokens),
   as hsimae_forward / hsimae_backward run it for every decoder block — exposed per kernel for the parity tests and the bench's
   kernel replays.  Weights: fp32 vectors, packed bf16 images (hsimae_pack_matrix: qkv = q | k | v fused [192][64], p [64][64],
   w1 / w3 [hp][64], w2 [64][hp], w2T [hp][64] = W2 transposed, hp = hidden rounded up to 32) and the fp32 row-major masters of
   q, k, v, proj, w1, w3 (the backward stages those in LDS itself).  bqkv = bq | bk | bv.
   forward : x [nsamples * Ts][64] fp32 -> x1 = x + proj(attention(LN1 x)), x2 = x1 + mlp(LN2 x1); keeps o (attention output,
             bf16 [rows][64]) and lse (log2-domain logsumexp, [rows][8]) for the backward.  split != 0: the attention half with
             q / k / v in registers + the row-panel MLP kernel (two launches, the default schedule); 0: one kernel.
   backward: from dy = dL/dx2 -> dx = dL/dx (dx1_tmp: scratch [rows][64] fp32, dL/dx1) and the block's 18 parameter gradients,
             ACCUMULATED into the given tensors.  slab: NULL = float atomics; else >= hsimae_dec_block_slab_floats() floats of
             scratch: per-workgroup partials + one fixed-order reduce launch (bit-reproducible). */
typedef struct {
    const float *n1w, *n1b, *bqkv, *pb, *n2w, *n2b, *w1b, *w3b, *w2b;
    const hs_bf16 *qkv, *p, *w1, *w3, *w2, *w2T;
    const float *qf, *kf, *vf, *pf, *w1f, *w3f;
    int32_t hidden;
} hsimae_dec_block_weights;
typedef struct {
    float *n1w, *n1b, *qw, *qb, *kw, *kb, *vw, *vb, *pw, *pb, *n2w, *n2b, *w1w, *w1b, *w2w, *w2b, *w3w, *w3b;
} hsimae_dec_block_grads;
int hsimae_dec_block_fwd(const hsimae_dec_block_weights* w, const float* x, float* x1, float* x2, hs_bf16* o, float* lse,
                         int32_t nsamples, int32_t Ts, int32_t split, void* stream);
#define HSIMAE_DEC_BLOCK_SLAB_FLOATS (256ll * (104 * 512 + 2112))   /* workgroups x (in-register dW values x threads + bias / LayerNorm sums) */
int64_t hsimae_dec_block_slab_floats(void);     /* = HSIMAE_DEC_BLOCK_SLAB_FLOATS of the library that is loaded: size of `slab` above */
/* Bytes of weight-gradient slab that hsimae_workspace_bytes() reserves for the caller's stream (side_stream = 0) or for the
   side stream of the forked spectral stack (1; 0 bytes = that stream commits with float atomics).  Whenever a stream can run
   a 256 x 256-tile weight-gradient launch (an encoder OR — caller's stream, layer-at-a-time decoder — a decoder of storage
   width >= 256) the answer is >= 64 MiB = 256 workgroups x 256 KB, what such a launch may write (csrc/plan.h slab_bytes). */
int64_t hsimae_wgrad_slab_bytes(const hsimae_config* cfg, int32_t side_stream);
int hsimae_dec_block_bwd(const hsimae_dec_block_weights* w, const hsimae_dec_block_grads* g, const float* x, const float* x1,
                         const float* dy, float* dx1_tmp, float* dx, const hs_bf16* o, const float* lse, int32_t nsamples,
                         int32_t Ts, float* slab, void* stream);

/* Weight / bias gradients of up to 16 linears in one launch (autograd of F.linear).  msplit = number of row slices the
   128 x 128 dW tiles are split into (partial sums meet in dW through atomics).  When every task of a launch has N >= 256 and
   K >= 256 and bf16 operands, the launch runs on 256 x 256 tiles, one workgroup per CU, and sizes its own row split (msplit is
   then only validated); the result is the same sum. */
typedef struct {
    const void* dO; int32_t dO_f32; int32_t ldo;
    const hs_bf16* A; int32_t lda;
    int32_t N, K;
    float* dW; int32_t ldw;
    float* db;
    const float* dO_rowscale;     /* optional per-row factor [M] on an fp32 dO (DropPath), applied in fp32 before the bf16 rounding;
                                     NULL = 1.  With a bf16 dO (dO_f32 == 0) it must be NULL: HSIMAE_EUNSUPPORTED, nothing is launched
                                     (fold the factor into the bf16 copy instead, as hsimae_backward does) */
    /* Operand layout (round 5).  0 = row-major [M][ldo] / [M][lda].  R > 0 = 64-column PLANES of R >= M rows each: the operand
       is [ldo / 64][R][64] (lda likewise), i.e. column c of row r lives at (c / 64) * R * 64 + r * 64 + c % 64 and ldo / lda is
       the padded width, a multiple of 64.  A producer that emits its operand 64 columns at a time (hsimae_enc_mlp_bwd: one
       hidden chunk per step) then writes row-contiguous blocks instead of 128-byte pieces at the row pitch — 5.2 against
       4.1 TB/s for the same bytes (scripts/micro/hbm_stride.hip) — and a dW tile's operand slice is two sequential streams.
       R > M (hsimae_backward uses M + 48) keeps the planes from starting a large power of two apart.  Planar operands need
       bf16, M % 32 == 0 and the LDS-DMA kernel (any launch with bf16 operands below 4 GB); else HSIMAE_EDIMS / _EUNSUPPORTED. */
    int32_t dO_plane_rows, A_plane_rows;
} hsimae_wgrad_task;
typedef struct {
    hsimae_wgrad_task t[16]; int32_t ntasks; int32_t M; int32_t msplit;      /* (16 since round 4: the 2 x 7 linears of a pair of axis-stack blocks) */
    const float* det_base; int64_t* det_acc;      /* deterministic dW / db commits, as in hsimae_lnbwd_params; NULL = fp32 atomics */
    /* optional scratch of >= 64 MiB (256 workgroups x 256 x 256 floats), private to the calling stream: a launch on 256 x 256
       tiles then writes every workgroup's partial dW tile there as coalesced rows and a second launch sums the row slices in
       a fixed order and adds them into dW — no float atomics on dW (they are ~6x slower per byte than stores, and with every
       workgroup committing at once were 26 % of the launch at d = 256), bit-reproducible.  NULL = atomics. */
    float* slab;
} hsimae_wgrad_params;
int hsimae_wgrad(const hsimae_wgrad_params* p, void* stream);
/* The row split (msplit) hsimae_backward uses for a launch of `tiles` 128x128 dW tiles over M rows: one resident
   wave of workgroups, whole groups of 8 (row slice ms runs on XCD ms % 8). */
int32_t hsimae_wgrad_msplit(int32_t tiles, int64_t M);

/* LayerNorm backward (autograd of Models.py:288/299/399/419), residual grad fused. */
typedef struct {
    const float* du; const float* x; const float* stats; const float* gamma; const float* dres;
    float* dx; int32_t accumulate; float* dgamma; float* dbeta; int32_t M, d;
    int32_t ld;                   /* row stride of du / x / dres / dx in floats (storage width); 0 = d */
    /* deterministic commits (hsimae_io.det_acc): dgamma / dbeta point into the flat gradient buffer starting at det_base and
       the sums go to det_acc[ptr - det_base] in 64-bit fixed point instead; both NULL = fp32 atomics */
    const float* det_base; int64_t* det_acc;
} hsimae_lnbwd_params;
int hsimae_ln_bwd(const hsimae_lnbwd_params* p, void* stream);
/* Plain LayerNorm forward, fp32 in/out (Models.py:570 when a caller wants the fp32 latent). */
int hsimae_ln_fwd(const float* x, const float* gamma, const float* beta, float* out, int32_t M, int32_t d, void* stream);

/* Decoder sequence assembly: mean-token fill + unshuffle + pos (Models.py:583-592) and backward. */
typedef struct {
    const float* y; int32_t N, K, TL, Dd; const int32_t* ids_restore; const float* pos;
    float* yfull; const float* dyfull; hs_bf16* dy;
    int32_t ld;                   /* row stride of y / yfull / dyfull / dy (storage width); 0 = Dd */
} hsimae_assemble_params;
int hsimae_assemble_fwd(const hsimae_assemble_params* p, void* stream);
int hsimae_assemble_bwd(const hsimae_assemble_params* p, void* stream);

/* patchify + norm_pix target + masked MSE + dLoss/dpred + recons images (Models.py:603-625). */
typedef struct {
    const float* x; int64_t sn, sb, sh, sw; int32_t N, T; const float* pred; const float* mask;
    int32_t norm_pix; float inv_scale;
    float* partial; float* loss; float sum_mask;
    hs_bf16* dpred; float* pred_img; float* mask_img;
} hsimae_loss_params;
int hsimae_loss_partials(int32_t N, int32_t T);   /* floats needed in `partial` */
int hsimae_loss(const hsimae_loss_params* p, void* stream);

/* ------------------------------------------------------------------ next row N1: optimizer step */
/* AdamW over the flat parameter / gradient buffers in ONE launch, torch.optim.AdamW semantics
 * (Model_Pretraining.py:80-86,102: betas (.9,.95), decay only on names without 'bias'/'norm').
 * group[i] per element: 0 = decayed, 1 = not decayed, 2 = frozen / unused (left untouched). `step` is 1-based. */
int hsimae_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* ------------------------------------------------------------------ next row N3: fine-tuning (DualViT) */
/* Encoder only, through `norm` (DualViT / HSIViT `forward_encoder`, Models.py:869-894, 1119-1146): same io as
 * hsimae_forward; io->latent [N, len_t*len_l, embed_dim] is required, loss / pred / recons outputs are not touched.
 * For the unmasked encoder pass len_t = T, len_l = 9 and increasing noise (ids_keep = identity). */
int hsimae_encode(const hsimae_config* cfg, const hsimae_io* io, void* stream);
/* Backward of hsimae_encode (fine-tuning, Model_Finetuning.py:156 `loss.backward()` through the classification
 * branch): dlatent [N*K, D] fp32 is dL/d(latent); the activations hsimae_encode left in io->workspace are consumed.
 * Accumulates into `grads` like hsimae_backward (the decoder's entries are not touched), same bucket callback. */
int hsimae_encode_backward(const hsimae_config* cfg, const hsimae_io* io, const float* dlatent, float* grads,
                           hsimae_bucket_cb cb, void* user, void* stream);
/* 'AGG' pooling of the classification head (Models.py:962-970): [N, T*L, D] -> [N, T*D], mean over the L tokens of
 * each spectral group; the Linear that follows is hsimae_gemm(A_F32, E_F32). */
int hsimae_agg_pool(const float* latent, float* pooled, int32_t N, int32_t T, int32_t L, int32_t D, void* stream);
/* Backward of that head (Models.py:962-970) from g = dL/d(class_pred) [N][C], fp32: gw [C][T*D] = g^T pooled, gb [C] = column
   sums of g, dlatent [N][T][L][D] = (g W)[n][t*D + c] / L for every l (W [C][T*D] = cls_head.weight).  One launch; results are
   ASSIGNED.  C <= 256. */
int hsimae_head_bwd(const float* g, const float* pooled, const float* w, float* gw, float* gb, float* dlatent, int32_t N, int32_t C,
                    int32_t T, int32_t L, int32_t D, void* stream);
/* Stand-alone decoder (HSIMAE / DualViT `forward_decoder`, Models.py:573-601 / 923-945), inference: latent [N*K, D] fp32
 * (the output of `norm`) -> pred [N*T*9, 72] fp32.  io supplies N, len_t, len_l (K = len_t*len_l), ids_restore, params,
 * wpk and the workspace, as for hsimae_forward. */
int hsimae_decode(const hsimae_config* cfg, const hsimae_io* io, const float* latent, float* pred, void* stream);
/* Backward of hsimae_decode (autograd of Models.py:573-601 for callers that compose forward_encoder / forward_decoder /
 * forward_loss themselves, e.g. Models.py:975-993): dpred [N*T*9, 72] fp32 is dL/d(pred); the activations hsimae_decode
 * left in io->workspace are consumed.  Writes dlatent [N*K, D] fp32 (dL/d(latent), the input of hsimae_decode) and
 * accumulates the decoder's parameter gradients into `grads` (flat layout; encoder entries are not touched). */
int hsimae_decode_backward(const hsimae_config* cfg, const hsimae_io* io, const float* dpred, float* dlatent, float* grads,
                           hsimae_bucket_cb cb, void* user, void* stream);

/* ------------------------------------------------------------------ next row N2: input pipeline */
/* One batch of training cubes assembled on the device from HBM-resident scenes (Model_Pretraining.py:40-51
 * `HSIdataset4PT.__getitem__`): window [h:h+9, w:w+9, :] of scene `num`, (x - min) / (max - min) in the scenes'
 * dtype, optional flips along w (bit 0, np.flip(data, 1)) and h (bit 1, np.flip(data, 0)), written as
 * out[n, 0, b, i, j] through the given element strides (band-fastest: sb = 1, sw = bands, sh = 9 * bands).
 * scenes: all scenes concatenated, each [h][w][bands] row-major; scene_off[s] element offset, scene_w[s] = w.
 * cut: the reference's int16 table, rows (c, h, w, scene, max, min) (Utils/Preprocessing.py:69-117); like the
 * reference, `c` is ignored and all bands are taken.  Bit-exact with the numpy arithmetic for fp32 / fp64 scenes. */
typedef struct {
    const void* scenes; int32_t scene_f64; const int64_t* scene_off; const int32_t* scene_w; int32_t bands;
    const int16_t* cut; const int64_t* index; const uint8_t* flips; int32_t N;
    float* out; int64_t sn, sb, sh, sw;
} hsimae_cube_params;
int hsimae_cube_gather(const hsimae_cube_params* p, void* stream);

/* ------------------------------------------------------------------ whole-scene inference (Model_Finetuning.py:243-300) */
/* A chunk of pixels of one scene [H][W][C] (row-major, fp32 or fp64, the `HSI_data` of Utils/Preprocessing.py:189-213 after
 * GWPCA / norm).  Pixel k of the chunk is `pixels[k]` when `pixels` (int64, device) is given, else `p0 + k`; a pixel index is
 * the row-major r * W + c.  Indices outside [0, H*W) are the caller's error: such a window is written as zeros and such a
 * label is not written.
 * hsimae_scene_windows: out[k, 0, b, i, j] = (float) scene[sym(r - 4 + i, H)][sym(c - 4 + j, W)][b] through the element strides
 *   sn, sb, sh, sw (band-fastest, the view the reference's HSIdataset yields: sb = 1, sw = C, sh = 9 * C), sym = numpy's
 *   'symmetric' pad of 4 (m = p mod 2H; m < H ? m : 2H - 1 - m, valid for any H >= 1).  fp64 -> fp32 rounds to nearest even
 *   (torch.tensor(x, dtype=float32)): bit-exact with the reference's windows (:209-213 + Model_Finetuning.py:49-50).
 * hsimae_class_argmax: map[pixel_k] = first + argmax(logits[k, first:num_class]) as int64, logits rows `ld` floats apart;
 *   ties go to the lowest index and NaN counts as the maximum (torch.argmax).  `scene` and `out` are not used.
 *   1 <= num_class - first, num_class <= 256. */
typedef struct {
    const void* scene; int32_t scene_f64; int32_t H, W, C;
    int64_t p0; const int64_t* pixels; int32_t N;
    float* out; int64_t sn, sb, sh, sw;
} hsimae_scene_params;
int hsimae_scene_windows(const hsimae_scene_params* p, void* stream);
int hsimae_class_argmax(const hsimae_scene_params* p, const float* logits, int32_t ld, int32_t num_class, int32_t first, int64_t* map,
                        void* stream);

/* ------------------------------------------------------------------ fine-tuning batches from the scene (Model_Finetuning.py:28-63)
 * ADDED under HSIMAE_VERSION 108 like the classification entry points below: nothing that 108 already had changes.
 * One launch assembles a batch of the fine-tuning `HSIdataset` from the HBM-resident scene [H][W][C] (fp32 or fp64, as in
 * hsimae_scene_params) instead of from host-built `data_cubes`: windows, flips and labels.
 *   items   int64 [N], device: sample k is entry items[k] of the dataset's tables (a batch may repeat an entry);
 *   n_items the tables' length;
 *   pixels  int64 [n_items] or NULL: the entry's pixel r * W + c.  NULL: entry i is pixel i, and n_items = H * W;
 *   labels  int64 [n_items] or NULL;
 *   flips   uint8 [N] or NULL (no flips): bit 0 = np.flip(data, 1), along w; bit 1 = np.flip(data, 0), along h;
 *   out     out[k, 0, b, i, j] = (float) scene[sym(r - 4 + i', H)][sym(c - 4 + j', W)][b] through the element strides sn, sb, sh,
 *           sw, with i' = bit 1 ? 8 - i : i, j' = bit 0 ? 8 - j : j, and sym and the fp64 -> fp32 rounding of
 *           hsimae_scene_windows: bit-exact with the reference's items.  An unpadded 9 x 9 tile with origin (r0, c0)
 *           (`data_cubes_2`, the unlabeled set) is the window of pixel (r0 + 4, c0 + 4);
 *   y       int64 [N] = labels[items[k]]; required exactly when `labels` is given;
 *   bad     int32 flag, required: an item outside [0, n_items) or a pixel outside [0, H * W) reads nothing, gets a window of
 *           zeros and y = -1, and sets *bad = 1.  The call never clears the flag.
 * One workgroup per sample, no host wait; two runs are bit-identical.
 * Refusals: params or bad NULL, `labels` without `y` or `y` without `labels`, and with N > 0 scene, items or out NULL ->
 * HSIMAE_ENULL; H, W or C <= 0, N < 0, n_items < 0 -> HSIMAE_EDIMS; a pointer not aligned to its element -> HSIMAE_EALIGN.
 * N = 0 -> HSIMAE_OK, nothing written. */
typedef struct {
    const void* scene; int32_t scene_f64; int32_t H, W, C;
    const int64_t* items; int32_t N;
    int64_t n_items; const int64_t* pixels; const int64_t* labels; const uint8_t* flips;
    float* out; int64_t sn, sb, sh, sw;
    int64_t* y; int32_t* bad;
} hsimae_scene_batch_params;
int hsimae_scene_batch(const hsimae_scene_batch_params* p, void* stream);

/* ------------------------------------------------------------------ group-wise PCA of a raw scene (Utils/GroupWisePCA.py) */
/* `applyGWPCA` on the device: x = (X - min X) / (max X - min X) over the whole scene [H][W][C] (row-major, fp32 or fp64; an
 * fp32 scene is widened to fp64 exactly, where the reference would stay in fp32), the band axis halved `group / 2` times
 * (`split_data`: c -> c / 2, c - c / 2; 103 bands -> 25, 26, 26, 26), and per group, with n = H * W and k = nc / group: mean,
 * covariance with divisor n - 1, eigenpairs in descending order, negative eigenvalues clipped to 0, every retained
 * eigenvector signed so that its entry of largest magnitude (the first one on a tie) is positive, y = (x - mean) . v_j, with
 * `whiten` times 1 / max(sqrt(lambda_j), 2^-52).  out[H][W][nc]: group g's k components at columns g k .. g k + k - 1.
 * Arithmetic is fp64 throughout.  Stated deviations from the reference: (1) the covariance is accumulated centred, in a second
 * pass after the mean, not as X^T X - n mean mean^T (that subtraction costs the reference 3 digits on data in [0, 1]);
 * (2) this is the exact PCA, what scikit-learn >= 1.5 computes for any scene (`covariance_eigh` when n >= 10 w, LAPACK `full`
 * otherwise); the 1.3 the reference pins sends a large scene through its randomized solver, an approximation of the same PCA.
 * The eigen-solve is a cyclic Jacobi iteration on the device (to off-diagonal norm <= 2^-52 trace, at most 30 sweeps), so
 * the fit never waits for the host.  Every reduction is combined in a fixed order: two runs are bit-identical.
 *
 * The model block is device memory of the caller: minmax[2] = (min, max); mean[C] of the normalised bands; lambda[C], ALL
 * eigenvalues of each group in descending order at the group's band offsets; proj[C][k], row b = band b's coefficients of its
 * group's k components, whitening folded in; group_off[5], the groups' band offsets, entries past `group` = C.
 * The fit routine writes the block, the apply routine reads it; the apply routine may be given another scene with the same C, so that one fit
 * transforms many scenes.  The workspace query returns the bytes the fit needs for these dimensions
 * (or a negative code); its contents are scratch.  `out` is fp64 (out_f64 != 0) or fp32 rounded to nearest even.
 *
 * Refusals: H, W, C or nc <= 0, H * W < 2, nc not a multiple of group, nc / group larger than the narrowest group or than
 * H * W -> HSIMAE_EDIMS; group not 1, 2 or 4, a group wider than 128 bands -> HSIMAE_EUNSUPPORTED; params, scene, a model
 * pointer, workspace or out NULL -> HSIMAE_ENULL; scene or a model pointer not aligned to its element, workspace or out not
 * 16-byte aligned -> HSIMAE_EALIGN.  max X == min X and non-finite values cannot be seen without a host wait: as in the
 * reference the output is then NaN (all of it), and the kernels still terminate (sweep cap). */
typedef struct {
    const void* scene; int32_t scene_f64; int32_t H, W, C;
    int32_t nc, group, whiten;
    double* minmax; double* mean; double* lambda; double* proj; int32_t* group_off;
} hsimae_gwpca_params;
int64_t hsimae_gwpca_workspace_bytes(const hsimae_gwpca_params* p);
int hsimae_gwpca_fit(const hsimae_gwpca_params* p, void* workspace, void* stream);
int hsimae_gwpca_apply(const hsimae_gwpca_params* p, void* out, int32_t out_f64, void* stream);

/* ------------------------------------------------------------------ classification loss, predictions and scores
 * (Model_Finetuning.py:150-178, 206-215, 268-290).  These entry points were ADDED under HSIMAE_VERSION 108: no struct or
 * function that 108 already had changes, so a caller written against 108 is unaffected, and a binder that wants them looks
 * the symbols up.
 *
 * hsimae_cls_loss: torch.nn.functional.cross_entropy(logits, targets, reduction="mean", ignore_index=ignore_index).
 *   logits fp32 [N][ld], of which only columns [0, C) are classes (the head's output is padded to 16 columns: the pad is never
 *   read); targets int64 [N].  A row is valid when its target is not ignore_index and lies in [0, C); a target that is neither
 *   sets *bad = 1 (never cleared here) and the row counts as ignored.  Written, each optional except `loss`:
 *     loss     fp32 scalar: sum over valid rows of (log sum_c exp(z_c - max z) - (z_y - max z)) / n_valid; NaN when n_valid = 0
 *              (also for N = 0), as torch;
 *     n_valid  int64 scalar;
 *     dlogits  fp32 [N][ldd]: (softmax(z_i) - onehot(y_i)) / n_valid in a valid row; exact zeros in an ignored row and in the
 *              columns [C, ldd);
 *     pred     int64 [N]: first + argmax(z_i[first:C]), for every row; ties go to the lowest index and NaN counts as the
 *              maximum (torch.argmax, hsimae_class_argmax);
 *     bad      int32 flag, see above.
 *   The row maximum is subtracted before the exponentials.  Two launches on `stream`, no host wait; the losses of the rows are
 *   summed in fp64 in a fixed order (no floating-point atomics): two runs are bit-identical.  `logits` is only read.
 *   workspace: hsimae_cls_workspace_bytes(N) bytes of scratch, 8-byte aligned.
 *   Refusals: params NULL -> HSIMAE_ENULL; N < 0, C < 2, ld < C, first outside [0, C), dlogits given with ldd < C -> HSIMAE_EDIMS;
 *   C > 1024 -> HSIMAE_EUNSUPPORTED; loss or workspace NULL, logits or targets NULL with N > 0 -> HSIMAE_ENULL; a pointer not
 *   aligned to its element (workspace: 8 bytes) -> HSIMAE_EALIGN.  hsimae_cls_workspace_bytes: N < 0 -> HSIMAE_EDIMS.
 * hsimae_cls_grad_scale: dst[i] = src[i] * *scale for i < n, `scale` an fp32 scalar in DEVICE memory (the gradient that
 *   arrives at the loss): the chain rule without a host read.  n < 0 -> HSIMAE_EDIMS, a NULL pointer with n > 0 -> HSIMAE_ENULL.
 * hsimae_confusion: cm[gt_i * C + pred_i] += 1 for every i < n with gt_i != 0; gt, pred int64 [n], cm int64 [C][C] that the
 *   caller zeroes once: counts accumulate over calls.  A gt_i or pred_i outside [0, C) (with gt_i != 0) sets *bad = 1 and is
 *   skipped.  Integer atomics: the result does not depend on their order.
 * hsimae_confusion_map: the same over a label map and a prediction map (hsimae_class_argmax's) of n pixels, with
 *   masked[i] = mask_map[i] != 0 ? pred_map[i] : 0 written first and counted in place of pred_map[i] (Model_Finetuning.py:285);
 *   mask_map NULL = gt_map.  `masked` may be pred_map itself.
 *   Refusals of both: n < 0, C < 2 -> HSIMAE_EDIMS; C > 1024 -> HSIMAE_EUNSUPPORTED; cm or bad NULL, and with n > 0 gt, pred or
 *   masked NULL -> HSIMAE_ENULL; a misaligned pointer -> HSIMAE_EALIGN.  n = 0 -> HSIMAE_OK, nothing written.
 * hsimae_scores: out fp64 [3 + 2 (C - 1)] = OA, AA, kappa, recall of label 1 .. C - 1, then 1.0 / 0.0 for "label k occurs in
 *   gt"; from cm as (Model_Finetuning.py:171-178) computes them from gt and pred: over the rows 1 .. C - 1 (gt != 0), n their
 *   total, OA = trace / n, recall_k = cm[k][k] / rowsum_k (0 when the label does not occur), AA the mean recall of the labels
 *   that occur, pe = sum_k rowsum_k colsum_k / n^2 over k >= 1 (a prediction of 0 is a miss with a column of its own),
 *   kappa = (OA - pe) / (1 - pe), 0 when pe = 1.  n = 0 gives NaN, as the host arithmetic does.  One workgroup, fp64; the
 *   count sums are integer and exact below 2^53.
 *   Refusals: C < 2 -> HSIMAE_EDIMS; C > 1024 -> HSIMAE_EUNSUPPORTED; cm or out NULL -> HSIMAE_ENULL; misaligned -> HSIMAE_EALIGN. */
typedef struct {
    const float* logits; int32_t ld;
    const int64_t* targets; int32_t N, C;
    int64_t ignore_index; int32_t first;
    float* loss; int64_t* n_valid; float* dlogits; int32_t ldd; int64_t* pred; int32_t* bad;
    void* workspace;
} hsimae_cls_params;
int64_t hsimae_cls_workspace_bytes(int32_t N);
int hsimae_cls_loss(const hsimae_cls_params* p, void* stream);
int hsimae_cls_grad_scale(const float* src, const float* scale, float* dst, int64_t n, void* stream);
int hsimae_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int32_t C, int64_t* cm, int32_t* bad, void* stream);
int hsimae_confusion_map(const int64_t* gt_map, const int64_t* mask_map, const int64_t* pred_map, int64_t* masked, int64_t n, int32_t C,
                         int64_t* cm, int32_t* bad, void* stream);
int hsimae_scores(const int64_t* cm, int32_t C, double* out, void* stream);

/* ------------------------------------------------------------------ scene products: probabilities, flip views, confidence
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes; hsimae_class_argmax is as it
 * was.  What hsimae_class_argmax throws away: the class probabilities of a chunk of pixels, averaged over the views (flips of
 * the window, hsimae_scene_batch's) the caller ran the model on, and per pixel the label, its probability and the top-1 / top-2
 * margin.  ONE CALL PER VIEW of a chunk, on one stream, view = 0 .. n_views - 1 in order; `logits` may be another buffer in
 * every call, everything else stays.
 *   logits   fp32 [N][ld] of this view; only the columns [first, C) are ever read (neither the classes below `first` nor
 *            the pad [C, ld));
 *   p_c      = softmax(logits[k, first:C])_c for first <= c < C and exactly 0 for c < first: the row maximum m over
 *            [first, C), e_c = exp2((z_c - m) log2 e), s = their sum (per lane in ascending order, then a fixed shuffle tree),
 *            p_c = e_c * (1 / s).  A NaN logit in [first, C) makes every p_c of the row with c >= first NaN;
 *   acc      fp32 [N][lda], required, the caller's scratch for this chunk: acc[k, c] = p_c at view 0 (acc is NOT read: what
 *            it held before cannot leak), acc[k, c] += p_c at a later view, for c < C; columns [C, lda) are never touched;
 *   at view n_views - 1, with mean_c = acc[k, c] * fl(1 / n_views) (exact for 1, 2, 4 and 8 views):
 *   probs    fp32 [N][ldp] or NULL: probs[k, c] = mean_c for c < C, rows in chunk order; columns [C, ldp) are never touched;
 *   label_map int64 [H * W], required: at the row's pixel (`pixels[k]`, or `p0 + k` when `pixels` is NULL: the meaning of
 *            hsimae_scene_params) the label: with n_views = 1, first + argmax(logits[k, first:C]), bit-identical to
 *            hsimae_class_argmax; with more views first + argmax_c mean_c.  Ties go to the lowest index and NaN counts as
 *            the maximum (torch.argmax);
 *   conf_map fp32 [H * W] or NULL: mean_label;
 *   margin_map fp32 [H * W] or NULL: mean_label - max of mean_c over c != label, c >= first; mean_label itself when
 *            C - first = 1.  Not clamped: with one view, two logits one ulp apart may give a margin of -1 ulp.
 *   A pixel index outside [0, H * W) writes none of the three maps (its `acc` and `probs` rows are written: they are in chunk
 *   order).  A pixel that occurs twice in `pixels` is written once per occurrence: which one stays is unspecified unless
 *   their logits are the same.
 * One wave per row, one launch, no host wait, no atomics: two runs are bit-identical.
 * Refusals: params NULL -> HSIMAE_ENULL; N < 0, C < 2, first outside [0, C), n_views outside [1, 8], view outside
 * [0, n_views), ld or lda < C, probs given with ldp < C, H or W <= 0 -> HSIMAE_EDIMS; C > 1024 -> HSIMAE_EUNSUPPORTED; with
 * N > 0 logits, acc or label_map NULL -> HSIMAE_ENULL; a pointer not aligned to its element -> HSIMAE_EALIGN.
 * N = 0 -> HSIMAE_OK, nothing written. */
typedef struct {
    const float* logits; int32_t ld;
    int32_t N, C, first;
    int32_t view, n_views;
    float* acc; int32_t lda;
    int32_t H, W; int64_t p0; const int64_t* pixels;
    int64_t* label_map; float* conf_map; float* margin_map;
    float* probs; int32_t ldp;
} hsimae_class_prob_params;
int hsimae_class_prob(const hsimae_class_prob_params* p, void* stream);

/* ------------------------------------------------------------------ edge-preserving smoothing of the probability maps (csrc/smooth.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  The joint bilateral filter
 * of Kang, Li and Benediktsson (EPF, IEEE TGRS 2014) over all class planes of a scene in one launch, and from the filtered
 * probabilities the products of hsimae_class_prob.
 *   probs    fp32 [n][ldp], the probabilities of n pixels (hsimae_class_prob's, hsimae_knn_vote's, a softmax); only the columns
 *            [first, C) of rows that a pixel points to are ever read;
 *   row_of   int32 [H * W] or NULL: row_of[pix] = the row of `probs` that belongs to pixel pix, negative (or >= n) = the pixel
 *            has no row.  NULL: row = pixel (pixels n .. H W - 1 have none);
 *   guide    fp32 [H * W][G], 1 <= G <= 4, and guide_scale, G fp32 factors IN DEVICE MEMORY (1 / (max - min) per channel);
 *            both may be NULL with a_r = 0 and are then never read.  The guide is read only at pixels that have a row;
 *   a_s, a_r fp32 of log2 e / (2 sigma_s^2) and log2 e / (2 sigma_r^2); a_r = 0 switches the range term off.
 * Per output pixel i that has a row, in this order (every operation fp32):
 *   for dy = -radius .. radius, for dx = -radius .. radius, j = i + (dy, dx); a tap outside the scene or without a row is
 *   skipped (never read, no reflection);
 *     d2 = 0; for g = 0 .. G - 1: d = fl(fl(I_j,g - I_i,g) * scale_g), d2 = fmaf(d, d, d2)            (a_r != 0 only)
 *     arg = fl(a_s * (dy^2 + dx^2)); arg = fmaf(a_r, d2, arg) (a_r != 0 only); w = exp2(-arg) (v_exp_f32); the centre has w = 1
 *     wsum = fl(wsum + w); acc_c = fmaf(w, p_j,c, acc_c) for first <= c < C
 *   out_c = fl(acc_c * fl(1 / wsum)) for first <= c < C, exactly 0 for c < first.
 *   out_probs fp32 [n][ldo] or NULL: out_c for c < C at the pixel's row (the input's row order); columns [C, ldo) and rows
 *            that no pixel points to are never touched.  Must not overlap `probs`;
 *   label_map int64 [H * W], required: argmax of out over [first, C), ties to the lowest index, NaN counts as the maximum;
 *   conf_map fp32 [H * W] or NULL: out[label];  margin_map fp32 [H * W] or NULL: out[label] - the largest other out_c,
 *            c >= first (out[label] itself when C - first = 1).
 * A pixel without a row writes nothing: the caller initialises the maps.  Two pixels must not share a row.
 * One workgroup per 16 x 16 tile, no host wait, no atomics: two runs are bit-identical.
 * Refusals: params NULL -> HSIMAE_ENULL; H or W <= 0, H W >= 2^31, n < 0, C < 2, first outside [0, C), ldp < C, out_probs given
 * with ldo < C, G outside [1, 4], radius outside [1, 8], a_s or a_r negative, NaN or infinite, out_probs overlapping probs ->
 * HSIMAE_EDIMS; C > 1024, or more than 65535 tiles along H or W -> HSIMAE_EUNSUPPORTED; probs or label_map NULL, or guide or
 * guide_scale NULL with a_r != 0 -> HSIMAE_ENULL; a pointer not aligned to its element -> HSIMAE_EALIGN.
 * n = 0 -> HSIMAE_OK, nothing written. */
typedef struct {
    const float* probs; int32_t ldp;
    int32_t n, C, first;
    int32_t H, W;
    const int32_t* row_of;
    const float* guide; int32_t G;
    const float* guide_scale;
    int32_t radius;
    float a_s, a_r;
    float* out_probs; int32_t ldo;
    int64_t* label_map; float* conf_map; float* margin_map;
} hsimae_prob_filter_params;
int hsimae_prob_filter(const hsimae_prob_filter_params* p, void* stream);

/* ------------------------------------------------------------------ superpixels and object-level class maps (csrc/slic.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  SLIC (Achanta et al., TPAMI
 * 2012) in gSLIC's gather form (Ren and Reid 2011) over a guide image, and the vote of every superpixel over the class
 * probabilities of its pixels.
 *
 * hsimae_slic.  guide fp32 [H * W][G], 1 <= G <= 4, and guide_scale, G fp32 factors IN DEVICE MEMORY (hsimae_prob_filter's pair).
 *   Grid: ny = ceil(H / size), nx = ceil(W / size), K = ny nx centres, centre k = i nx + j; the home cell of pixel (y, x) is
 *   (y ny / H, x nx / W) in integer arithmetic.  A centre is 8 floats: G features, y, x, pad (the pad keeps what it held).
 *   init = 1: centre (i, j) is placed at pixel y = (2 i + 1) H / (2 ny), x = (2 j + 1) W / (2 nx) (integer division) with that
 *   pixel's features fl(scale_g I_g) and pad 0; no gradient perturbation.  init = 0: `centres` is read as given.
 *   Distance of pixel p = (y, x) to a centre c, every operation fp32, in this order:
 *     d = 0; for g = 0 .. G - 1: t = fl(fl(scale_g I_g(p)) - c_g), d = fmaf(t, t, d);
 *     dy = fl(y - c_y), dx = fl(x - c_x), s = fmaf(dx, dx, fl(dy dy)), d = fmaf(w, s, d)        w = fp32(compactness^2 / size^2).
 *   Assign: a pixel compares the centres of the 3 x 3 cells around its home cell in ascending k, cells outside the grid left
 *   out; the smallest d wins, a tie stays with the lower k, a NaN d loses to every number, and if all are NaN the home cell's
 *   centre wins (with distance NaN).
 *   Update: a centre becomes the mean (G features fl(scale_g I_g), y, x) of the pixels assigned to it: fp64 sums, one ascending-x
 *   chain per scene row, then the row partials in ascending y; one fp64 division, one rounding to fp32.  A centre with no pixel
 *   keeps its bits.
 *   `rounds` times assign + update (one launch each, reading one centre buffer and writing the other), then one final assign:
 *   labels int32 [H * W] = k, dist fp32 [H * W] or NULL = the winning d, counts int32 [K] or NULL = the pixels that carry label k.
 *   The centres end in `centres` whatever the parity of `rounds`; centres_tmp is scratch of the same size (may be NULL with rounds = 0).
 *   Connectivity is not enforced.  Every label of a pixel is one of the 3 x 3 cells around its home cell.
 *   No atomics, no host wait: two runs are bit-identical.
 *   Refusals: params NULL -> HSIMAE_ENULL; H or W <= 0, H W >= 2^31, G outside [1, 4], size outside [2, 32], rounds < 0, init not
 *   0 or 1, w negative, NaN or infinite, an output overlapping an input or another output -> HSIMAE_EDIMS; guide, guide_scale,
 *   centres or labels NULL, centres_tmp NULL with rounds > 0 -> HSIMAE_ENULL; a pointer not aligned to its element -> HSIMAE_EALIGN.
 *
 * hsimae_segment_vote.  labels int32 [H * W]: hsimae_slic's map for the same H, W and size (the vote relies on its locality: a
 *   pixel whose label is not one of the 3 x 3 cells around its home cell belongs to no segment here).  probs fp32 [n][ldp],
 *   row_of int32 [H * W] or NULL, first, C: as in hsimae_prob_filter; a pixel that has a row is "classified".
 *   Per segment k with at least one classified pixel (cnt of them), v_c for first <= c < C:
 *     mode 0: v_c = fp32(sum / cnt), the fp64 sum of probs[row, c] over its classified pixels in hsimae_slic's order (one
 *             ascending-x chain per scene row, then the rows in ascending y), one fp64 division;
 *     mode 1: v_c = fp32(m_c / cnt) in fp64, m_c = the classified pixels whose own argmax over [first, C) is c (ties to the
 *             lowest index, NaN counts as the maximum).
 *   label = argmax_c v_c (ties to the lowest index, NaN counts as the maximum), conf = v_label, margin = v_label - the largest
 *   other v_c (v_label itself when C - first = 1): written to label_map int64 [H * W] (required), conf_map, margin_map fp32
 *   [H * W] (or NULL) at the segment's classified pixels, and with fill = 1 at its other pixels too.
 *   out_probs fp32 [K][ldo] or NULL: v_c for c < C (0 below `first`) in row k; seg_count int32 [K] or NULL: cnt.
 *   A segment without a classified pixel writes only its seg_count (0): its pixels keep what the maps held, its out_probs row too.
 *   One workgroup per segment, no atomics, no host wait: two runs are bit-identical.
 *   Refusals: params NULL -> HSIMAE_ENULL; H or W <= 0, H W >= 2^31, n < 0, C < 2, first outside [0, C), ldp < C, out_probs given
 *   with ldo < C, size outside [2, 32], mode or fill not 0 or 1, an output overlapping an input or another output ->
 *   HSIMAE_EDIMS; C > 1024 -> HSIMAE_EUNSUPPORTED; probs, labels or label_map NULL -> HSIMAE_ENULL; a pointer not aligned to its
 *   element -> HSIMAE_EALIGN. */
typedef struct {
    const float* guide;
    const float* guide_scale;
    int32_t G, H, W, size;
    float w;
    int32_t init, rounds;
    float* centres;
    float* centres_tmp;
    int32_t* counts;
    int32_t* labels;
    float* dist;
} hsimae_slic_params;
int hsimae_slic(const hsimae_slic_params* p, void* stream);

typedef struct {
    const float* probs; int32_t ldp;
    int32_t n, C, first;
    const int32_t* row_of;
    const int32_t* labels;
    int32_t H, W, size, mode, fill;
    float* out_probs; int32_t ldo;
    int32_t* seg_count;
    int64_t* label_map; float* conf_map; float* margin_map;
} hsimae_segment_vote_params;
int hsimae_segment_vote(const hsimae_segment_vote_params* p, void* stream);

/* ------------------------------------------------------------------ k-NN evaluation of frozen features (csrc/knn.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  The weighted k-NN classifier a
 * pretrained encoder is judged by without fine-tuning (Wu et al. 2018; DINO's knn_classifier): L2-normalised features, the k
 * most similar rows of a labelled bank, a vote weighted by exp(similarity / T).  Three launches, no host wait, no atomics: two
 * runs are bit-identical.  Common refusals: params NULL -> HSIMAE_ENULL; a negative count, or a leading dimension below the
 * width -> HSIMAE_EDIMS; with work to do, a required pointer NULL -> HSIMAE_ENULL; a pointer not aligned to its element ->
 * HSIMAE_EALIGN; N or Q = 0 -> HSIMAE_OK and no launch (the dimension checks come first).
 *
 * hsimae_row_normalize: out[r, c] = x[r, c] / max(||x[r]||_2, 1e-12) (torch.nn.functional.normalize: a zero row gives zeros)
 *   for x fp32 [N][ld], out fp32 [N][ldo], columns c < D; `norms` fp32 [N] or NULL receives ||x[r]||_2.  out == x is allowed.
 *   One wave per row, in this order: lane l forms ss = fmaf(x_c, x_c, ss) over c = l, l + 64, .. from 0; the 64 sums are added by
 *   the xor tree (partner lane ^ 1, ^ 2, .. ^ 32); n = sqrtf(ss); r = 1 / fmaxf(n, 1e-12f) (IEEE division); out_c = x_c * r.
 *   A row whose sum of squares overflows fp32 (||x|| above 1.8e19) comes out as zeros.  D = 0 -> HSIMAE_OK, no launch.
 *
 * hsimae_knn_topk: for every row of q fp32 [Q][ldq] the k largest dot products with the rows of bank fp32 [M][ldb] over D
 *   columns: idx int32 [Q][k] and sim fp32 [Q][k], descending by similarity, equal similarities by ascending bank index, a NaN
 *   similarity below every number (NaNs among themselves by ascending index).  Every dot product is an exact-fp32 fmaf chain
 *   from +0 over the columns 0, 1, .., D - 1 in this order (v_mfma_f32_32x32x2_f32), one rounding per product, the same for
 *   every bank row: duplicated bank rows give bit-equal similarities.  q and bank are read as given (normalise them first for
 *   cosine similarity).  Rows must be 16-byte aligned: the two base pointers, and ldq % 4 = ldb % 4 = 0, else HSIMAE_EALIGN.
 *   D <= 0, D % 4 != 0, k < 1 or k > M -> HSIMAE_EDIMS; k > 64, M > 2^20 or D > 4096 -> HSIMAE_EUNSUPPORTED.
 *   The [Q][M] matrix is never written to memory: a workgroup keeps the lists of 64 query rows in LDS while it walks the bank.
 *
 * hsimae_knn_vote: idx / sim [Q][k] as hsimae_knn_topk wrote them (sim[r][0] is the row's largest), bank_labels int64 [M],
 *   classes [first, C) (class 0 is "unlabelled" with first = 1, as in hsimae_class_prob).  Per row, with neighbour j in lane j:
 *     w_j     = exp2(((sim_j - sim_0) * inv_temperature) * log2 e)     (inv_temperature: the host's fp64 1 / T rounded once;
 *               the shift by sim_0 cancels in p and keeps T = 0.01 inside fp32)
 *     score_c = the w_j with bank_labels[idx_j] = c added in rank order j = 0 .. k - 1 from 0
 *     total   = sum of score_c: lane l adds its classes first + l, first + l + 64, .. in order, then the xor tree
 *     p_c     = score_c * (1 / total), exactly 0 for c < first
 *   probs fp32 [Q][ldp] or NULL: p_c for c < C in row order (columns [C, ldp) untouched); at the row's pixel (`pixels[r]`, or
 *   p0 + r when `pixels` is NULL; nothing is written for a pixel outside [0, H * W)): label_map int64 = argmax_c p_c (ties to
 *   the lower class), conf_map fp32 or NULL = p_label, margin_map fp32 or NULL = p_label - the largest other p_c (p_label
 *   itself when C - first = 1).  A neighbour index outside [0, M) or a bank label outside [first, C) sets *bad (int32, required)
 *   to 1 and gives the row label 0, confidence 0, margin 0 and probabilities 0.
 *   M < 1, k < 1, C < 2, first outside [0, C), probs given with ldp < C, H or W <= 0, inv_temperature not a positive finite
 *   number -> HSIMAE_EDIMS; k > 64 or C > 1024 -> HSIMAE_EUNSUPPORTED. */
typedef struct {
    const float* x; int32_t ld;
    int32_t N, D;
    float* out; int32_t ldo;
    float* norms;
} hsimae_row_normalize_params;
int hsimae_row_normalize(const hsimae_row_normalize_params* p, void* stream);

typedef struct {
    const float* q; int32_t ldq;
    const float* bank; int32_t ldb;
    int32_t Q, M, D, k;
    int32_t* idx; float* sim;
} hsimae_knn_topk_params;
int hsimae_knn_topk(const hsimae_knn_topk_params* p, void* stream);

typedef struct {
    const int32_t* idx; const float* sim;
    int32_t Q, k, M;
    const int64_t* bank_labels;
    int32_t C, first;
    float inv_temperature;
    int32_t H, W; int64_t p0; const int64_t* pixels;
    int64_t* label_map; float* conf_map; float* margin_map;
    float* probs; int32_t ldp;
    int32_t* bad;
} hsimae_knn_vote_params;
int hsimae_knn_vote(const hsimae_knn_vote_params* p, void* stream);

/* ------------------------------------------------------------------ k-means on frozen features (csrc/kmeans.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  Lloyd's algorithm over the
 * rows x fp32 [N][ldx] and K centroids c fp32 [K][ldc] of D columns: one round is hsimae_kmeans_assign, then hsimae_kmeans_update.
 * No atomics, no host wait: two runs are bit-identical, and a round at a fixed point changes nothing, bit for bit.
 * One formulation serves both metrics: score(i, k) = x_i . c_k - bias_k, the label is the argmax.  Euclidean: bias_k =
 * 1/2 ||c_k||^2 (argmax score = argmin ||x_i - c_k||^2).  Cosine (spherical k-means): unit rows, unit centroids, bias NULL = 0.
 * Limits of both: D > 0, D % 4 = 0, 1 <= K, first >= 0, leading dimensions >= D, else HSIMAE_EDIMS; K > 1024 or D > 4096 ->
 * HSIMAE_EUNSUPPORTED; params NULL, or with N > 0 a required pointer NULL -> HSIMAE_ENULL; x or c not 16-byte aligned, ldx % 4 or
 * ldc % 4 != 0, another pointer not aligned to its element -> HSIMAE_EALIGN; N = 0 -> HSIMAE_OK, nothing written (the dimension
 * checks come first).  A refusal writes nothing.
 *
 * hsimae_kmeans_assign: for every row i, dot_ik as hsimae_knn_topk forms it (the exact-fp32 fmaf chain from +0 over the columns
 *   0 .. D - 1, the same for every centroid), score_ik = dot_ik - bias_k in fp32 (one rounding; bias NULL: the dot product
 *   itself).  The best centroid: a strictly larger score wins, equal scores stay with the lower index, a NaN score beats nothing
 *   (among NaNs only: the lowest index).  At the row's pixel (`pixels[i]`, or p0 + i when `pixels` is NULL; nothing is written
 *   for a pixel outside [0, H * W), as hsimae_knn_vote): labels int64 = first + best index; score fp32 or NULL = the best
 *   score; margin fp32 or NULL = best - second best score (the best score itself when K = 1; a NaN second when every other
 *   score is NaN).  changed int32 [HSIMAE_KMEANS_GRID] or NULL: before a label is overwritten it is compared with the value
 *   there; entry g receives the number of rows of workgroup g whose label changed (0 for workgroups that do not exist), so the
 *   sum of all entries is the number of changed labels.  H or W <= 0 -> HSIMAE_EDIMS.
 *
 * hsimae_kmeans_update: from x, labels int64 [N] in row order (cluster k = labels[i] - first) and the centroids c the labels were
 *   assigned against (read, then overwritten), two launches:
 *     counts int64 [K]  = members of cluster k
 *     sums fp64 [K][D]  = the member rows added in ascending row order from 0, one fp64 chain per element (no grid dependence)
 *     c[k]              = fp32(sums[k] / counts[k]) (fp64 division, one rounding); with normalize != 0 that mean is then
 *                         normalised in fp32 by hsimae_row_normalize's rule and order, in place
 *     bias fp32 [K] or NULL: bias_k = fp32(1/2 sum_d c_kd^2), the sum in fp64 over the stored fp32 centroid: lane l of one wave
 *                         takes d = l, l + 64, .. in order with fma, then the xor tree (partner lane ^ 1, ^ 2, .. ^ 32)
 *     an empty cluster keeps c[k] and bias_k bit for bit (sums[k] = 0, counts[k] = 0)
 *     state fp64 [HSIMAE_KMEANS_STATE]:
 *       [0] inertia    = sum_i ||x_i - c_old[labels[i]]||^2 in fp64: per (cluster, 64-column slab) lane l adds fma(d, d, .)
 *                        over the members in ascending row order for column 64 slab + l, the xor tree adds the lanes; then lane l
 *                        of one wave takes the (cluster, slab) partials l, l + 64, .. in order, and the xor tree
 *       [1] changed    = the sum of `changed` int32 [HSIMAE_KMEANS_GRID] as hsimae_kmeans_assign wrote it (NULL: 0)
 *       [2] iterations = its previous value + 1 if changed > 0 (the caller zeroes state once before the first round)
 *       [3] empty      = clusters without a member
 *       [4] bad        = labels outside [first, first + K): such a row belongs to no cluster and is counted here
 *       [5 .. 7]       = 0
 *     scratch fp64 [K * ceil(D / 64) + 1], required.  sums, counts, c, state required.
 *   Seeding is one update over the K seed rows with labels first .. first + K - 1 and changed NULL. */
#define HSIMAE_KMEANS_GRID 2048      /* workgroups of hsimae_kmeans_assign at most (a stride loop beyond); ints in `changed` */
#define HSIMAE_KMEANS_STATE 8        /* doubles in `state` */
typedef struct {
    const float* x; int32_t ldx;
    const float* c; int32_t ldc;
    const float* bias;
    int32_t N, K, D, first;
    int32_t H, W; int64_t p0; const int64_t* pixels;
    int64_t* labels; float* score; float* margin;
    int32_t* changed;
} hsimae_kmeans_assign_params;
int hsimae_kmeans_assign(const hsimae_kmeans_assign_params* p, void* stream);

typedef struct {
    const float* x; int32_t ldx;
    const int64_t* labels;
    int32_t N, K, D, first, normalize;
    float* c; int32_t ldc;
    float* bias;
    int64_t* counts; double* sums;
    const int32_t* changed;
    double* scratch; double* state;
} hsimae_kmeans_update_params;
int hsimae_kmeans_update(const hsimae_kmeans_update_params* p, void* stream);

/* ------------------------------------------------------------------ linear probe on frozen features (csrc/probe.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  Multinomial logistic
 * regression over the real classes [first, C) (class 0 is "unlabelled" with first = 1, as in hsimae_class_prob) on fp32 feature
 * rows x [n][ldx] of D columns, standardised per column (MAE's probe: BatchNorm1d(affine=False, eps) ahead of the linear layer),
 * the bias carried as column D whose feature is the constant 1, trained by full-batch AdamW with decoupled decay (none on the
 * bias column).  Kp = D + 4 is the operand width (column D = 1, columns D + 1 .. Kp - 1 = 0).  The weights w, and Adam's moments
 * m and v, are fp32 [64][Kp]; the caller zeroes all three once; the rows below `first` and from C on, and the columns behind D,
 * are never written and stay 0.  No atomics, no cooperative launch, no grid-wide barrier, no flag, no host wait: every output
 * element is one chain in a fixed order that does not depend on the grid, so two runs are bit-identical.
 * Limits of all four: n >= 0, D > 0, D % 4 = 0, 2 <= C, 0 <= first < C, a leading dimension below its width, Kp != D + 4 ->
 * HSIMAE_EDIMS; C > 64, D > 4096 or n > 2^20 -> HSIMAE_EUNSUPPORTED; params NULL, or with n > 0 a required pointer NULL ->
 * HSIMAE_ENULL; a matrix not 16-byte aligned or with a leading dimension that is no multiple of 4, another pointer not aligned
 * to its element -> HSIMAE_EALIGN; n = 0 -> HSIMAE_OK and no launch (the dimension checks come first).  A refusal writes nothing.
 *
 * hsimae_probe_prepare (two launches): a bank row i is valid when labels[i] (int64 [n]) lies in [first, C); any other row is
 *   counted in `bad` and is inert: it enters no statistic, its rows of xs and xt are 0 (column D too), so it adds exact zeros to
 *   every later sum.  nv = the number of valid rows.  Per column d, one thread, fp64, the valid rows in ascending order from 0:
 *     sum_d = x_0d + x_1d + ..;  mu = sum_d / nv;  ss_d = fma(x_id - mu, x_id - mu, ss_d);  var = ss_d / nv (population variance)
 *     mean[d] = fp32(mu);  rstd[d] = fp32(1 / sqrt(var + (double)eps))            (nv = 0: mean 0, rstd 0)
 *   xs fp32 [n][Kp]: xs[i][d] = fl(fl(x[i][d] - mean[d]) * rstd[d]), xs[i][D] = 1, 0 behind; xt fp32 [Kp][ldn] its transpose with
 *   zeros in the columns n .. roundup(n, 4) - 1 (ldn >= roundup(n, 4); columns behind that are neither written nor read).
 *   state fp64 [HSIMAE_PROBE_STATE] = {0, 0, 0, bad, nv, 0, 0, 0}.  eps must be a positive finite number, else HSIMAE_EDIMS.
 *
 * hsimae_probe_step: iteration `step` = 1, 2, .. (an ARGUMENT: the host counts, and AdamW's bias corrections 1 / (1 - b1^step) and
 *   1 / sqrt(1 - b2^step) are formed on the host in fp64 and rounded once, as hsimae_adamw_step forms them), four launches:
 *   forward   one workgroup per 64 rows: z_ic = the exact-fp32 fmaf chain from +0 over k = 0 .. Kp - 1 of xs[i][k] w[c][k]
 *             (hsimae_knn_topk's dot tile); per row, one wave: m = max of z over [first, C), e_c = exp2((z_c - m) log2 e), sum =
 *             the e_c added by the xor tree over the lanes (lane = c - first), p_c = e_c * (1 / sum);
 *             g_ic = (p_ic - [c = labels[i]]) * fp32(1 / nv), written transposed into gt fp32 [64][ldn]: 0 for c < first, c >= C,
 *             an invalid row and the columns n .. roundup(n, 4) - 1.  The row's loss = log(sum) - (z_iy - m) in fp64; a wave adds
 *             its 16 rows in ascending order, the four waves are added in order: loss_part fp64 [ceil(n / 64)].
 *   gradient  the rows are cut into S = ceil(n / HSIMAE_PROBE_SEG) segments; workgroup (64 columns of Kp, segment s):
 *             dW_s[c][k] = the fmaf chain from +0 over the segment's rows i ascending of gt[c][i] xt[k][i] -> scratch fp32 [S][64][Kp].
 *   update    per element (c, k), first <= c < C, k <= D: dW = scratch[0][c][k] + scratch[1][c][k] + .. in ascending s (fp32, from
 *             the first term); torch.optim.AdamW's element with lr, weight_decay (0 for k = D), b1, b2, eps, in hsimae_adamw_step's
 *             operation order; per workgroup of 256 elements the fp64 sum of dW^2 (the optimizers' fixed-order block sum).
 *   finish    one wave: lane l adds loss_part[l], [l + 64], .. in order, then the xor tree; the same for the dW^2 partials:
 *             state = {loss / nv (the mean cross-entropy BEFORE this update), step, ||dW||^2, bad, nv, 0, 0, 0} (bad and nv kept);
 *             loss_hist[step - 1] = fp32 of that loss when loss_hist is not NULL.
 *   norm_part fp64 [ceil(64 Kp / 256)].  step < 1, or lr, weight_decay, eps negative or NaN, b1 or b2 outside [0, 1) -> HSIMAE_EDIMS.
 *
 * hsimae_probe_logits: z fp32 [n][ldz] = the forward tile alone for any rows x [n][ldx]: every row is standardised while it is
 *   staged (fl(fl(x - mean) * rstd), column D = 1) and meets w in the same chain, so the logits of the bank equal the forward's
 *   bit for bit.  Columns c < first receive 0 (never -inf), columns C .. ldz - 1 are untouched.  ldz < C -> HSIMAE_EDIMS.
 *
 * hsimae_probe_fold: the head in the model's terms, for rows of raw features: weight fp32 [C][ldw], weight[c][d] = fl(w[c][d] *
 *   rstd[d]); bias fp32 [C], bias[c] = fp32(w[c][D] - sum_d w[c][d] mean[d] rstd[d]), the products and the sum in fp64 over
 *   ascending d from 0 (one thread).  Rows below `first` are 0.  ldw < D -> HSIMAE_EDIMS. */
#define HSIMAE_PROBE_SEG 256         /* bank rows behind one gradient partial: a constant, so no sum depends on the grid */
#define HSIMAE_PROBE_STATE 8         /* doubles in `state` */
#define HSIMAE_PROBE_ROWS 64         /* rows of w, m, v and gt: C at most */
typedef struct {
    const float* x; int32_t ldx;
    const int64_t* labels;
    int32_t n, D, C, first;
    float eps;
    float* mean; float* rstd;
    float* xs; int32_t Kp;
    float* xt; int32_t ldn;
    double* state;
} hsimae_probe_prepare_params;
int hsimae_probe_prepare(const hsimae_probe_prepare_params* p, void* stream);

typedef struct {
    const float* xs; const float* xt; int32_t Kp, ldn;
    const int64_t* labels;
    int32_t n, D, C, first;
    float* w; float* m; float* v;
    float* gt; float* scratch;
    double* loss_part; double* norm_part;
    float lr, weight_decay, b1, b2, eps;
    int32_t step;
    double* state; float* loss_hist;
} hsimae_probe_step_params;
int hsimae_probe_step(const hsimae_probe_step_params* p, void* stream);

typedef struct {
    const float* x; int32_t ldx;
    const float* mean; const float* rstd;
    const float* w; int32_t Kp;
    int32_t n, D, C, first;
    float* z; int32_t ldz;
} hsimae_probe_logits_params;
int hsimae_probe_logits(const hsimae_probe_logits_params* p, void* stream);

typedef struct {
    const float* w; int32_t Kp;
    const float* mean; const float* rstd;
    int32_t D, C, first;
    float* weight; int32_t ldw;
    float* bias;
} hsimae_probe_fold_params;
int hsimae_probe_fold(const hsimae_probe_fold_params* p, void* stream);

/* ------------------------------------------------------------------ RBF support-vector classifier (csrc/svm.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  C-SVC in libsvm's dual form
 * with the kernel K_ts = exp(-gamma ||x_t - x_s||^2), one-vs-one over the class pairs (a, b), a < b, in the order (0, 1), (0, 2),
 * .., (1, 2), ..: rows of class a carry y = +1, rows of class b y = -1; minimise 1/2 a'Qa - e'a, Q_ts = y_t y_s K_ts, 0 <= a <= C,
 * y'a = 0.  The bank rows are sorted by class, so every class is one contiguous row range.  Four entry points: the kernel matrices,
 * the solver (one launch for any number of problems), the compact model, the prediction.  No atomics, no grid-wide barrier,
 * nothing waits for the host: two runs are bit-identical.  Common refusals: params NULL, or with work to do a required pointer
 * NULL -> HSIMAE_ENULL; a negative count or a leading dimension below its width -> HSIMAE_EDIMS; a matrix not 16-byte aligned or
 * with a leading dimension that is no multiple of 4, another pointer not aligned to its element -> HSIMAE_EALIGN.  A refusal
 * writes nothing.
 *
 * hsimae_svm_gram: x fp32 [M][ldx], D columns (D > 0, D % 4 = 0, else HSIMAE_EDIMS; D > 4096, M > HSIMAE_SVM_MAX_ROWS or n_gamma >
 *   HSIMAE_SVM_MAX_GAMMAS -> HSIMAE_EUNSUPPORTED; n_gamma < 1, a gamma that is not a positive finite number -> HSIMAE_EDIMS) ->
 *   K fp32 [n_gamma][M][ldk] and sumsq fp32 [M] (required).  In this order:
 *     dot_ts  = hsimae_knn_topk's exact-fp32 fmaf chain from +0 over the columns 0 .. D - 1
 *     n_t     = dot_tt: THE SAME chain (the diagonal of the row's own tile), not the lane-strided sum of hsimae_row_normalize, so
 *               that two equal rows have n_t = n_s = dot_ts bit for bit and d2 = 0 exactly -> sumsq
 *     d2_ts   = fmaf(-2, dot_ts, fl(n_t + n_s)), a negative value replaced by 0 (a NaN stays)
 *     g2      = fl(gamma * fl32(log2 e))
 *     K_ts    = exp2(fl(-g2 * d2_ts))   (v_exp_f32);   K_tt = 1 is written as a constant, for a NaN row too
 *   Only the tiles on and above the diagonal are computed; a tile writes K_ts and K_st from the same value: K is symmetric bit
 *   for bit.  A NaN row makes its row and its column NaN (the diagonal element excepted) and nothing else.  M = 0 -> HSIMAE_OK.
 *
 * hsimae_svm_solve: `table` holds n_problems rows of the struct hsimae_svm_problem below, in device memory, all fields 8 bytes.  Problem r: kernel
 *   matrix k_index (< n_k) of K fp32 [n_k][M][ldk], box constant C, the rows a0 .. a0 + na - 1 (y = +1) then b0 .. b0 + nb - 1
 *   (y = -1), n = na + nb local variables t = 0 .. n - 1 in that order.  One workgroup of 256 threads per problem runs libsvm's SMO
 *   with second-order working-set selection (Fan, Chen and Lin 2005, WSS 2), no shrinking, no cache: alpha and the gradient G are
 *   fp64 in LDS for the whole solve (16 n bytes + 128 bytes of reduction scratch: n <= HSIMAE_SVM_MAX_ROWS = 8192 is 128 KiB of the
 *   160 KiB a gfx950 workgroup may hold); the kernel rows K_i and K_j are read from memory in every iteration.  Per iteration:
 *     1. i = argmax over I_up = {y_t = +1, alpha_t < C} u {y_t = -1, alpha_t > 0} of -y_t G_t = G_max; m2 = max over I_low =
 *        {y_t = +1, alpha_t > 0} u {y_t = -1, alpha_t < C} of y_t G_t (a maximum of -0 is +0: m2 + 0);  gap = G_max + m2.  gap < eps, or no i -> converged.
 *        Otherwise `max_iter` iterations done in this call -> stop, not converged.
 *     2. j = argmax over t in I_low with b = G_max + y_t G_t > 0 of (b * b) / a, a = 2 - 2 K_it (fp64 of the fp32 K), a <= 0
 *        replaced by 1e-12.  No j -> converged.
 *     3. libsvm's Solver::Solve two-variable update with its clipping to the box, Q_ij = y_i y_j K_ij, Q_ii = Q_jj = 1.
 *     4. G_t = G_t + (Q_ti * d_i + Q_tj * d_j) for every t, d = the change of alpha_i, alpha_j.
 *   Every argmax: the larger value wins, of equals the lower t, a NaN never wins: per thread over t = tid, tid + 256, .., then the
 *   xor tree over the 64 lanes (partner lane ^ 1, .. ^ 32) and the four waves in ascending order, all by that one rule, which is
 *   associative: the result is that of a serial scan.  Every fp64 operation is a single correctly rounded IEEE operation (no fused
 *   multiply-add, contraction off); no floating-point sum is reduced across threads.
 *   rho as libsvm's calculate_rho, one thread over t ascending: the mean of y_t G_t over the free variables (0 < alpha_t < C), else
 *   the midpoint of max{y_t G_t: at the bound on the I_up-only side} and min{.. on the I_low-only side}.
 *   Outputs of problem r: alpha fp64 [n] at alpha + out_offset, G fp64 [n] at grad + out_offset, state fp64 [HSIMAE_SVM_STATE] at
 *   state + 8 r = {iterations, converged, gap, n_sv (alpha_t > 0), n_bounded (alpha_t >= C), rho, 0, 0}.  converged: 1 yes, 0 no
 *   (max_iter), -1 the table row is refused (k_index outside [0, n_k), a negative field, a range beyond M, n > M, out_offset + n >
 *   alpha_len, C not a positive finite number): nothing but the state is written; -2 na = 0 or nb = 0: alpha = 0, G = -1, rho = 0; -3 an alpha or a G that is not finite when the
 *   problem stopped (a NaN or an infinity in K: no NaN ever wins an argmax, so the solve ends early and says so here).
 *   resume = 0: start from alpha = 0, G = -1.  resume != 0: start from alpha and grad as they are and add to state[0]; `max_iter`
 *   counts the iterations of THIS call, so r iterations in one call equal r calls of one iteration bit for bit.
 *   n_problems = 0 -> HSIMAE_OK; M < 1, M > HSIMAE_SVM_MAX_ROWS -> HSIMAE_EDIMS / HSIMAE_EUNSUPPORTED; max_iter < 0, eps not a
 *   positive finite number, alpha_len < 0 -> HSIMAE_EDIMS.
 *
 * hsimae_svm_pack: the n_class (n_class - 1) / 2 problems table[first_problem ..] of ONE model (pair order as above, class c =
 *   rows a0 / b0 of its pairs) into libsvm's compact form, one workgroup per class:
 *     sv_index int32 [M]: the bank rows with alpha > 0 in any of their pairs, ascending (so grouped by class); sv_start int32
 *     [n_class + 1]: where each class starts in that list, sv_start[n_class] = S;  coef fp32 [n_class - 1][ldc]: for support row s
 *     of class c, coef[j][s] = fp32(y alpha) of c's pair with class j (j < c) or j + 1 (j >= c), y = +1 when c is the lower class;
 *     rho fp32 [P] = fp32(state rho);  sv fp32 [S][ldsv] and sv_sumsq fp32 [S]: the support rows of x and their sumsq gathered.
 *   Entries behind S are not written.  A refused or out-of-range table row makes S = 0.  2 <= n_class <= HSIMAE_SVM_MAX_CLASSES.
 *
 * hsimae_svm_predict: for the rows q fp32 [Q][ldq], a workgroup owns 64 rows and walks the S = sv_start[n_class] (at most S_max)
 *   support rows in tiles of 64 in ascending order.  Per tile: qn = sum of squares of the query row (hsimae_row_normalize's
 *   lane-strided chain and xor tree: NOT the dot tile's chain, so a query equal to a support row gives a K next to 1, not exactly
 *   1 as in hsimae_svm_gram), the dot tile, d2 / g2 / exp2 as hsimae_svm_gram (no constant on a diagonal), then for every
 *   pair p = (a, b): dec_p = fmaf(coef, K, dec_p) over the tile's support rows of class a (coef[b - 1]) then of class b (coef[a])
 *   in ascending order, from +0 (LDS, [pair][row]; thread = (row, pairs p with p % 4 = wave)).  After the last tile, per row:
 *   d_p = dec_p - rho_p (fp32); d_p > 0 votes for a, else for b; label = first + the class with most votes, ties to the lower
 *   class; share_c = fp32(votes_c) / fp32(P).  At the row's pixel (`pixels[r]`, or p0 + r; nothing is written for a pixel outside
 *   [0, H * W)): label_map int64, conf_map fp32 or NULL = the winner's share, margin_map fp32 or NULL = that minus the largest
 *   other share.  probs fp32 [Q][ldp] or NULL: 0 below `first`, share_c at first + c (ldp >= first + n_class).  These are SHARES OF
 *   THE PAIRWISE CONTESTS, not Platt probabilities.  decision fp32 [Q][ldd] or NULL: d_p.  outside int32 [HSIMAE_SVM_GRID] or
 *   NULL: entry g = the rows of workgroup g whose pixel lay outside (0 for workgroups that do not exist).
 *   LDS: 16.9 KiB of slabs, norms and class starts + 256 P bytes of decision sums: n_class <= HSIMAE_SVM_MAX_CLASSES = 32 (P = 496: 140.5 KiB). */
#define HSIMAE_SVM_MAX_ROWS 8192     /* rows of a Gram matrix, variables of one problem */
#define HSIMAE_SVM_MAX_GAMMAS 16
#define HSIMAE_SVM_MAX_CLASSES 32    /* real classes of hsimae_svm_pack / hsimae_svm_predict */
#define HSIMAE_SVM_STATE 8           /* doubles per problem in `state` */
#define HSIMAE_SVM_GRID 2048         /* workgroups of hsimae_svm_predict at most (a stride loop beyond); ints in `outside` */
typedef struct {
    const float* x; int32_t ldx;
    int32_t M, D, n_gamma;
    float gamma[HSIMAE_SVM_MAX_GAMMAS];
    float* K; int32_t ldk;
    float* sumsq;
} hsimae_svm_gram_params;
int hsimae_svm_gram(const hsimae_svm_gram_params* p, void* stream);

typedef struct {
    int64_t k_index; double C;
    int64_t a0, na, b0, nb, out_offset, reserved;
} hsimae_svm_problem;

typedef struct {
    const float* K; int32_t ldk;
    int32_t M, n_k;
    const hsimae_svm_problem* table; int32_t n_problems;
    int32_t resume, max_iter;
    double eps;
    double* alpha; double* grad; int64_t alpha_len;
    double* state;
} hsimae_svm_solve_params;
int hsimae_svm_solve(const hsimae_svm_solve_params* p, void* stream);

typedef struct {
    const hsimae_svm_problem* table; int32_t first_problem, n_class;
    const double* alpha; int64_t alpha_len; const double* state;
    const float* x; int32_t ldx;
    int32_t M, D;
    const float* sumsq;
    int32_t* sv_index; int32_t* sv_start;
    float* coef; int32_t ldc;
    float* rho;
    float* sv; int32_t ldsv;
    float* sv_sumsq;
} hsimae_svm_pack_params;
int hsimae_svm_pack(const hsimae_svm_pack_params* p, void* stream);

typedef struct {
    const float* q; int32_t ldq;
    int32_t Q, D;
    const float* sv; int32_t ldsv;
    const float* sv_sumsq; const int32_t* sv_start; int32_t S_max;
    const float* coef; int32_t ldc;
    const float* rho;
    int32_t n_class, first;
    float gamma;
    int32_t H, W; int64_t p0; const int64_t* pixels;
    int64_t* label_map; float* conf_map; float* margin_map;
    float* probs; int32_t ldp;
    float* decision; int32_t ldd;
    int32_t* outside;
} hsimae_svm_predict_params;
int hsimae_svm_predict(const hsimae_svm_predict_params* p, void* stream);

/* ------------------------------------------------------------------ masked reconstruction of a whole scene (csrc/recon.hip)
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.  The way back from the
 * windows hsimae_forward reconstructs to the scene they were cut from, and the error maps and sums behind PSNR and the spectral
 * angle (SAM).  No atomics, no host wait: two runs are bit-identical; chunks and passes are ordered by the stream.
 *
 * Window grid: 9 x 9 windows (hsimae_scene_batch's) centred on the scene pixels (rows[ir], cols[ic]); window w = ir * ncols + ic.
 * Only a window's un-reflected positions map back to the scene: position (i, j) of window (ir, ic) is pixel
 * (rows[ir] - 4 + i, cols[ic] - 4 + j) when that lies inside the scene, and is ignored when the symmetric pad filled it.
 *
 * hsimae_recon_accumulate: one call per forward chunk.  pred_img / mask_img fp32 [n][C][9][9], contiguous as hsimae_forward
 *   writes them, hold the windows w0 .. w0 + n - 1; rows int32 [nrows] and cols int32 [ncols] are DEVICE memory, strictly
 *   ascending, inside the scene; sum fp32 [H][W][C] and cnt int32 [H][W][C] are zeroed once by the caller.  For every voxel
 *   (r, c, b) and every window of the chunk with |rows[ir] - r| <= 4 and |cols[ic] - c| <= 4, in ascending w:
 *     if mask_img[w - w0][b][r - rows[ir] + 4][c - cols[ic] + 4] != 0:  sum += pred_img[the same],  cnt += 1
 *   in fp32, starting from what sum held.  A select, not a product: a pred_img value under mask 0 is never read into the
 *   result.  A gather with one lane per voxel; a voxel no window of the chunk reconstructs is not written.
 *   Refusals: params NULL -> HSIMAE_ENULL; n < 0, w0 < 0, H, W, C, nrows or ncols <= 0, nrows > H or ncols > W (all the host can
 *   see of a list that is not strictly ascending inside the scene), w0 + n > nrows * ncols -> HSIMAE_EDIMS; with n > 0 a NULL
 *   pointer -> HSIMAE_ENULL; a pointer not aligned to its element -> HSIMAE_EALIGN.  n = 0 -> HSIMAE_OK, nothing written.
 *   List values the host cannot see are never trusted for an address: a centre further than 4 from the voxel is skipped.
 *
 * hsimae_recon_finish: two launches.  Per pixel, with x_b = the scene value as fp32 (fp64 -> fp32 rounds to nearest even, as the
 *   windows), S = {b : cnt_b > 0}, m = |S|, r_b = sum_b / (float)cnt_b (IEEE fp32 division) on S and x_b elsewhere; each output
 *   optional except stats:
 *     recon fp32 [H][W][C] = r;      cover int32 [H][W] = m;
 *     rmse  fp32 [H][W] = (float)sqrt(se / m), se = sum over S of (r - x)^2;
 *     sam   fp32 [H][W] = (float)(2 atan2(sqrt(sum_S (r/nr - x/nx)^2), sqrt(sum_S (r/nr + x/nx)^2))), nr = sqrt(sum_S r^2),
 *           nx = sqrt(sum_S x^2): the well-conditioned form of the angle, not acos of a ratio.  nr = nx = 0 -> 0; one of them
 *           0 -> pi / 2.  m = 0 -> rmse = sam = 0.
 *   All sums are fp64: lane l of the pixel's wave takes the bands l, l + 64, .. in order with fma, the 64 sums are added by the
 *   xor tree (partner lane ^ 1, ^ 2, .. ^ 32).
 *     stats fp64 [4] = sum of se, sum of m, sum of the fp64 sam, and the count, over the pixels with m > 0.  Wave v of workgroup
 *           g takes the pixels 4 g + v, 4 g + v + 4 G, .. (G = min(ceil(H W / 4), HSIMAE_RECON_GRID) workgroups) in order, the
 *           workgroup adds its waves 0 .. 3 into partials [G][4], and one workgroup adds those: per statistic, lane l of one
 *           wave takes g = l, l + 64, .. in order, then the xor tree.
 *     partials fp64, 4 * HSIMAE_RECON_GRID doubles of scratch, required.
 *   A NaN that was accumulated shows in that pixel's outputs and in stats.
 *   Refusals: params NULL -> HSIMAE_ENULL; H, W or C <= 0 -> HSIMAE_EDIMS; scene, sum, cnt, partials or stats NULL ->
 *   HSIMAE_ENULL; a pointer not aligned to its element -> HSIMAE_EALIGN. */
#define HSIMAE_RECON_GRID 1024       /* workgroups of the finish's first launch at most; partials holds 4 doubles for each */
typedef struct {
    const float* pred_img; const float* mask_img;
    int32_t n; int64_t w0;
    const int32_t* rows; int32_t nrows;
    const int32_t* cols; int32_t ncols;
    int32_t H, W, C;
    float* sum; int32_t* cnt;
} hsimae_recon_accumulate_params;
int hsimae_recon_accumulate(const hsimae_recon_accumulate_params* p, void* stream);

typedef struct {
    const void* scene; int32_t scene_f64; int32_t H, W, C;
    const float* sum; const int32_t* cnt;
    float* recon; int32_t* cover; float* rmse; float* sam;
    double* partials; double* stats;
} hsimae_recon_finish_params;
int hsimae_recon_finish(const hsimae_recon_finish_params* p, void* stream);

/* ------------------------------------------------------------------ gradient norm, clipping and the non-finite step skip
 * (what torch.nn.utils.clip_grad_norm_ and an `isfinite(...).item()` test do on the host, kept in device memory: no host wait).
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes; hsimae_adamw_step is as it was.
 *
 * hsimae_grad_norm: the 2-norm over up to HSIMAE_CLIP_MAX_SEGS segments of fp32 gradients.  A segment without `group` counts
 *   every element; with it (one id per element, hsimae_adamw_step's) an element whose id is 2 is left out of the sum, whatever
 *   it holds.  `n` need not be a multiple of 4 and `g` need only be 4-byte aligned.  Two launches on `stream`: a fixed grid of
 *   HSIMAE_CLIP_GRID workgroups forms squares and sums in fp64 and writes one fp64 partial per workgroup (`partials`:
 *   HSIMAE_CLIP_GRID doubles, 8-byte aligned, scratch); one workgroup then adds them in a fixed order and fills `ctl`.  No
 *   atomics: two runs on the same input agree bit for bit.  Written to ctl:
 *     sumsq, norm = (float)sqrt(sumsq), finite = sumsq is finite;
 *     coef    = (float)min(1, max_norm / (norm + 1e-6)) evaluated in fp64 (clip_grad_norm_'s formula; 1.0f for max_norm = +inf
 *               and a finite norm; with a norm that is not finite, what IEEE arithmetic gives: 0 for +inf, NaN for NaN);
 *     apply   = !(skip_nonfinite && !finite);   skipped += !apply (the caller zeroes it once);
 *     inv_bc1, inv_sqrt_bc2 = 1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t) for t = step - skipped, fp64 rounded to fp32;
 *     norm_max = max(norm_max, norm) when finite (the caller zeroes it when it has read it).
 *   Refusals, before any launch: nseg outside 1 .. 8, a segment with n < 0, step < 1, ctl or partials NULL, max_norm not > 0
 *   (NaN included; +inf is allowed and means report only) -> HSIMAE_EDIMS; segs NULL, g NULL with n > 0 -> HSIMAE_ENULL; g not
 *   4-byte, partials or ctl not 8-byte aligned -> HSIMAE_EALIGN.
 * hsimae_adamw_step_ctl: hsimae_adamw_step's update, element for element, on g * ctl->coef (one fp32 multiply; `g` itself is
 *   not modified) with the bias corrections read from ctl; when ctl->apply is 0 nothing is written.  group NULL: every element
 *   has the id `group_uniform`.  Any n >= 0.  One launch, no host wait.
 *   Refusals: n < 0, group NULL with group_uniform outside 0 .. 2 -> HSIMAE_EDIMS; a NULL array or ctl with n > 0 -> HSIMAE_ENULL;
 *   an array not 4-byte or ctl not 8-byte aligned -> HSIMAE_EALIGN. */
#define HSIMAE_CLIP_GRID 1024        /* workgroups of the norm's first launch = doubles the caller provides in `partials` */
#define HSIMAE_CLIP_MAX_SEGS 8
typedef struct { const float* g; const uint8_t* group; int64_t n; } hsimae_grad_seg;
typedef struct hsimae_clip_ctl {     /* written by hsimae_grad_norm, read by hsimae_adamw_step_ctl; 48 bytes */
    double sumsq;
    float norm;
    float coef;
    int32_t finite;
    int32_t apply;
    int64_t skipped;
    float inv_bc1, inv_sqrt_bc2;
    float norm_max;
} hsimae_clip_ctl;
int hsimae_grad_norm(const hsimae_grad_seg* segs, int32_t nseg, float max_norm, int32_t skip_nonfinite, int32_t step, float beta1,
                     float beta2, double* partials, hsimae_clip_ctl* ctl, void* stream);
int hsimae_adamw_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group,
                          int32_t group_uniform, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                          const hsimae_clip_ctl* ctl, void* stream);

/* ------------------------------------------------------------------ AdamW with a learning rate and a weight decay per group id
 * (what torch.optim.AdamW does with one param_group per layer: layer-wise learning-rate decay, a head stepped faster than the
 * encoder, frozen layers), still ONE launch over the flat buffer and no host wait.
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes; hsimae_adamw_step is as it
 * was, and hsimae_adamw_step_ctl is this entry point with the two-entry table {(lr, weight_decay), (lr, 0)}.
 *
 * hsimae_adamw_step_groups: an element's id (one byte per element in `group`; group NULL: every element has `group_uniform`)
 *   indexes `table` directly, and the element is stepped with table[id].lr and table[id].weight_decay by hsimae_adamw_step's
 *   arithmetic; the decay multiply is applied when weight_decay != 0.  Id 2 keeps its meaning: frozen or absent, never read,
 *   never written, left out of hsimae_grad_norm; table[2] is ignored.  An id >= ngroups found in device memory is treated as
 *   frozen too: the table is never indexed past ngroups.  `table` is HOST memory and is copied into the launch (512 bytes of
 *   kernel argument, staged into LDS once per workgroup): the caller need not keep it alive.
 *   ctl != NULL: the gradient is multiplied by ctl->coef, the bias corrections are read from ctl and nothing is written when
 *   ctl->apply is 0, exactly as hsimae_adamw_step_ctl does; `step` is ignored.  ctl == NULL: coef = 1 and the bias corrections
 *   are formed on the host from `step` (fp64 pow, rounded to fp32), as hsimae_adamw_step forms them.
 *   Any n >= 0 and any 4-byte alignment (16-byte loads when all four arrays are 16-byte and `group` 4-byte aligned).
 *   Refusals, before any launch: n < 0, ngroups outside 1 .. HSIMAE_ADAMW_MAX_GROUPS, group NULL with group_uniform neither 2
 *   nor inside 0 .. ngroups - 1, ctl NULL with step < 1, an lr or weight_decay (other than table[2]'s) that is negative or NaN
 *   -> HSIMAE_EDIMS; a NULL array or table with n > 0 -> HSIMAE_ENULL; an array not 4-byte or ctl not 8-byte aligned ->
 *   HSIMAE_EALIGN.  n == 0, or a uniform id of 2: HSIMAE_OK and no launch. */
#define HSIMAE_ADAMW_MAX_GROUPS 64
typedef struct { float lr; float weight_decay; } hsimae_adamw_group;
int hsimae_adamw_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group,
                             int32_t group_uniform, int64_t n, const hsimae_adamw_group* table /* host */, int32_t ngroups,
                             float beta1, float beta2, float eps, int32_t step, const hsimae_clip_ctl* ctl /* device, may be NULL */,
                             void* stream);

/* ------------------------------------------------------------------ LAMB: Adam's update scaled per parameter tensor by |w| / |update|
 * (You et al., "Large Batch Optimization for Deep Learning", 2020; the optimizer of apex FusedLAMB and timm Lamb), on the flat buffer
 * hsimae_adamw_step_groups steps, with its id byte per element, its {lr, weight_decay} table and hsimae_grad_norm's control block.
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.
 *
 * hsimae_lamb_step: for every tensor T of `tensors` (device memory: `off` and `n` in floats into the four arrays, `chunk0` the
 *   prefix sum of ceil(n / HSIMAE_LAMB_CHUNK) over the tensors in front of it; `nchunks` the total), with k the id byte of the
 *   tensor's FIRST element (group NULL: `group_uniform`), in fp32 unless stated:
 *     gc = g * ctl->coef;   m' = m + (gc - m) (1 - beta1);   v' = v beta2 + gc gc (1 - beta2)          (hsimae_adamw_step's forms)
 *     u  = (m' ctl->inv_bc1) / (sqrtf(v') ctl->inv_sqrt_bc2 + eps)   [+ table[k].weight_decay p   when that is != 0]
 *     r  = (float)sqrt(sum_T p^2 / sum_T u^2), sums and root in fp64, when (weight_decay != 0 or always_adapt) and both sums are > 0,
 *          otherwise 1;   r = min(r, trust_clip) when trust_clip > 0
 *     p' = p - (table[k].lr r) u
 *   With every r = 1 this is AdamW's step.  ratios[T] = r.  k == 2 or k >= ngroups: the tensor is frozen; nothing of it is read but
 *   that byte, nothing is written (its gradient may hold NaN) and ratios[T] = 1.  `grads` is never written.
 *   Three launches on `stream`, no atomics, every sum in a fixed order: two runs agree bit for bit.  `partials` (2 nchunks doubles)
 *   is scratch.  `ctl` is required; when ctl->apply is 0 nothing is read from the arrays and nothing is written, `ratios` keeps the
 *   values of the last applied step.  A chunk whose table entry is inconsistent (off < 0, off + n > n_total, the chunk outside
 *   [chunk0, chunk0 + ceil(n / HSIMAE_LAMB_CHUNK)), chunk0 not the prefix sum) writes nothing and sets *bad = 1; `bad` is never
 *   cleared here.  `table` is HOST memory, copied into the launch.
 *   Refusals, before any launch: a NULL among params, grads, the moments, tensors, table, partials, ratios, bad, ctl ->
 *   HSIMAE_ENULL; n < 0, ntensors < 1, nchunks < 1, ngroups outside 1 .. HSIMAE_ADAMW_MAX_GROUPS, group NULL with group_uniform
 *   neither 2 nor inside 0 .. ngroups - 1, an lr or weight_decay (other than table[2]'s) negative or NaN -> HSIMAE_EDIMS; an array,
 *   ratios or bad not 4-byte, partials, tensors or ctl not 8-byte aligned -> HSIMAE_EALIGN.  n == 0: HSIMAE_OK and no launch. */
#define HSIMAE_LAMB_CHUNK 4096
typedef struct { int64_t off; int64_t n; int32_t chunk0; int32_t reserved; } hsimae_lamb_tensor;   /* device table, 24 bytes */
int hsimae_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group,
                     int32_t group_uniform, int64_t n, const hsimae_lamb_tensor* tensors /* device */, int32_t ntensors,
                     int32_t nchunks, const hsimae_adamw_group* table /* host */, int32_t ngroups, float beta1, float beta2, float eps,
                     float trust_clip /* <= 0: none */, int32_t always_adapt, double* partials /* device, 2 * nchunks */,
                     float* ratios /* device, ntensors */, int32_t* bad /* device */, const hsimae_clip_ctl* ctl /* device, required */,
                     void* stream);

/* ------------------------------------------------------------------ an exponential moving average (EMA) of the weights, kept next
 * to them in device memory (timm's ModelEma, TensorFlow's ExponentialMovingAverage), and the exchange of weights and averages for
 * an evaluation.  What eager torch does with one foreach op over every parameter tensor and a host-side `if` on whether the step
 * was skipped is one launch that reads hsimae_grad_norm's control block: no host wait.
 * ADDED under HSIMAE_VERSION 108 like the entry points above: nothing that 108 already had changes.
 *
 * hsimae_ema_update: with t = step - (ctl ? ctl->skipped : 0), the number of applied optimizer steps including this one (the count
 *   ctl's bias corrections use), evaluated in fp64:
 *     d = warmup ? min(decay, (1 + t) / (10 + t)) : decay;     a = (float)(1 - d)
 *   and then per element, in fp32, exactly this sequence:
 *     s = p - ema (one rounding);   ema' = fmaf(a, s, ema) (one rounding)
 *   An element whose p equals its ema bit for bit keeps its bits (a select, not arithmetic: -0.0 stays -0.0, a NaN keeps its
 *   payload), so a parameter that is never stepped stays bit-equal to its average for good.  There is no group array: the average
 *   covers every element.  `params` is never written.  ctl != NULL and ctl->apply == 0: nothing is read from the arrays and nothing
 *   is written; a skipped step moves neither the average nor its warm-up count.
 *   Any n >= 0 and any 4-byte alignment: 16-byte loads and stores where both arrays are 16-byte aligned, one element per thread
 *   behind that body (all of them otherwise); at most HSIMAE_EMA_MAX_GRID workgroups of 256 threads, which stride over the rest.
 *   One launch on `stream`, no atomics, no LDS.  The average is fp32, as timm's is: at decay = 0.9999 an increment a (p - ema)
 *   smaller than half an ulp of ema is lost.
 *   Refusals, before any launch: n < 0, decay NaN or outside [0, 1), step < 1 -> HSIMAE_EDIMS; a NULL array with n > 0 ->
 *   HSIMAE_ENULL; an array not 4-byte or ctl not 8-byte aligned -> HSIMAE_EALIGN.  n == 0: HSIMAE_OK and no launch.
 * hsimae_ema_swap: exchanges a[0 .. n) and b[0 .. n) as 32-bit words (NaN payloads included); the same freedom of size and
 *   alignment, one launch.  Refusals: n < 0, or the two ranges overlap -> HSIMAE_EDIMS; a NULL array with n > 0 -> HSIMAE_ENULL;
 *   an array not 4-byte aligned -> HSIMAE_EALIGN.  n == 0: HSIMAE_OK and no launch. */
#define HSIMAE_EMA_MAX_GRID 2048
int hsimae_ema_update(float* ema, const float* params, int64_t n, double decay, int32_t warmup, int32_t step,
                      const hsimae_clip_ctl* ctl /* device, may be NULL */, void* stream);
int hsimae_ema_swap(float* a, float* b, int64_t n, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
