// Internal launcher interface between the kernel translation units and the C ABI (api.hip).
// Parameter blocks are the public C structs of include/hsimae_hip.h.
#pragma once
#include "common.h"
#include "../../include/hsimae_hip.h"

enum AKind { A_BF16 = HSIMAE_A_BF16, A_F32 = HSIMAE_A_F32, A_F32_LN = HSIMAE_A_F32_LN };
enum Epi { E_BF16 = HSIMAE_E_BF16, E_F32 = HSIMAE_E_F32, E_RES_F32 = HSIMAE_E_RES_F32,
           E_POS_F32 = HSIMAE_E_POS_F32, E_SWIGLU = HSIMAE_E_SWIGLU, E_SWIGLU_BWD = HSIMAE_E_SWIGLU_BWD,
           E_LN_BWD = HSIMAE_E_LN_BWD };

typedef hsimae_gemm_params GemmParams;
typedef hsimae_pack_desc PackDesc;
typedef hsimae_attn_params AttnParams;
typedef hsimae_wgrad_task WgradTask;
typedef hsimae_wgrad_params WgradParams;
typedef hsimae_lnbwd_params LnBwdParams;
typedef hsimae_mask_params MaskParams;
typedef hsimae_patch_params PatchParams;
typedef hsimae_assemble_params AssembleParams;
typedef hsimae_loss_params LossParams;
typedef hsimae_cube_params CubeParams;
typedef hsimae_scene_params SceneParams;

int hs_gemm(const GemmParams& p, int akind, int epi, hipStream_t s);
int hs_gemm_tiled(const GemmParams& p, int akind, int epi, int bm, int kc, hipStream_t s);   // tile sweep hook
int hs_pack(const PackDesc* descs_dev, int ndesc, int max_elems, hipStream_t s);
int hs_attn_fwd(const AttnParams& p, hipStream_t s);
int hs_attn_bwd(const AttnParams& p, hipStream_t s);
int hs_wgrad(const WgradParams& p, hipStream_t s);
int hs_ln_bwd(const LnBwdParams& p, hipStream_t s);
int hs_ln_fwd(const float* x, const float* gamma, const float* beta, float* out, int M, int d, hipStream_t s, int ldx = 0, int ldo = 0);
int hs_mask(const MaskParams& p, hipStream_t s);
int hs_patch_gather(const PatchParams& p, hipStream_t s);
int hs_assemble_fwd(const AssembleParams& p, hipStream_t s);
int hs_assemble_bwd(const AssembleParams& p, hipStream_t s);
int hs_loss(const LossParams& p, hipStream_t s);
int hs_loss_partials(int N, int T);
int hs_cube_gather(const CubeParams& p, hipStream_t s);
int hs_scene_windows(const SceneParams& p, hipStream_t s);
int hs_class_argmax(const SceneParams& p, const float* logits, int ld, int num_class, int first, int64_t* map, hipStream_t s);
int hs_scene_batch(const hsimae_scene_batch_params& p, hipStream_t s);
int64_t hs_gwpca_workspace_bytes(const hsimae_gwpca_params& p);
int hs_gwpca_fit(const hsimae_gwpca_params& p, void* workspace, hipStream_t s);
int hs_gwpca_apply(const hsimae_gwpca_params& p, void* out, int out_f64, hipStream_t s);
int64_t hs_cls_workspace_bytes(int N);
int hs_cls_loss(const hsimae_cls_params& p, hipStream_t s);
int hs_cls_grad_scale(const float* src, const float* scale, float* dst, int64_t n, hipStream_t s);
int hs_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int C, int64_t* cm, int32_t* bad, hipStream_t s);
int hs_confusion_map(const int64_t* gt_map, const int64_t* mask_map, const int64_t* pred_map, int64_t* masked, int64_t n, int C,
                     int64_t* cm, int32_t* bad, hipStream_t s);
int hs_scores(const int64_t* cm, int C, double* out, hipStream_t s);
int hs_class_prob(const hsimae_class_prob_params& p, hipStream_t s);
int hs_prob_filter(const hsimae_prob_filter_params& p, hipStream_t s);
int hs_slic(const hsimae_slic_params& p, hipStream_t s);
int hs_segment_vote(const hsimae_segment_vote_params& p, hipStream_t s);
int hs_row_normalize(const hsimae_row_normalize_params& p, hipStream_t s);
int hs_knn_topk(const hsimae_knn_topk_params& p, hipStream_t s);
int hs_knn_vote(const hsimae_knn_vote_params& p, hipStream_t s);
int hs_kmeans_assign(const hsimae_kmeans_assign_params& p, hipStream_t s);
int hs_kmeans_update(const hsimae_kmeans_update_params& p, hipStream_t s);
int hs_probe_prepare(const hsimae_probe_prepare_params& p, hipStream_t s);
int hs_probe_step(const hsimae_probe_step_params& p, hipStream_t s);
int hs_probe_logits(const hsimae_probe_logits_params& p, hipStream_t s);
int hs_probe_fold(const hsimae_probe_fold_params& p, hipStream_t s);
int hs_svm_gram(const hsimae_svm_gram_params& p, hipStream_t s);
int hs_svm_solve(const hsimae_svm_solve_params& p, hipStream_t s);
int hs_svm_pack(const hsimae_svm_pack_params& p, hipStream_t s);
int hs_svm_predict(const hsimae_svm_predict_params& p, hipStream_t s);
int hs_recon_accumulate(const hsimae_recon_accumulate_params& p, hipStream_t s);
int hs_recon_finish(const hsimae_recon_finish_params& p, hipStream_t s);
int hs_agg_pool(const float* latent, float* pooled, int N, int T, int L, int D, hipStream_t s);
int hs_head_bwd(const float* g, const float* pooled, const float* w, float* gw, float* gb, float* dlat, int N, int C, int T, int L,
                int D, hipStream_t s);
int hs_rows_to_bf16(const float* src, hs_bf16* dst, int64_t rows, int d, const float* rowscale, hipStream_t s);
int hs_rows_pad_bf16(const float* src, hs_bf16* dst, int64_t rows, int cols, int ldd, hipStream_t s);
int hs_det_convert(const int64_t* acc, float* g, int64_t n, hipStream_t s);
int hs_add2(const float* a, const float* b, float* out, int64_t n, hipStream_t s);

// ------------------------------------------------------------------ one transformer Block's parameters
// What every block launcher below takes: api.hip fills one per block of a pass (resolve()) and one from each weights struct of
// the C ABI.  A member its source does not have stays NULL; each unit copies the subset its kernels read (DecW, EncMlpW, Blk*Args).
struct BlockW {
    const float *n1w, *n1b, *bqkv, *pb, *n2w, *n2b, *w1b, *w3b, *w2b;
    const bf16_t *qkv, *p, *w1, *w3, *w2, *qkvT, *pT, *w13T, *w2T;
    const float *qf, *kf, *vf, *pf, *w1f, *w3f;    // fp32 row-major weights [out][in] (the fused decoder backward stages them in LDS as bf16)
    int h;                                         // hidden width of the MLP
};

// ------------------------------------------------------------------ fused_dec.hip (decoder Block, one workgroup per sample)
// The 18 gradient pointers are the C ABI's struct itself (hsimae_dec_block_bwd's caller hands one over as it is): a member added to
// hsimae_dec_block_grads reaches hs_dec_block_bwd, which must then commit it (the assert below stops the build until someone looks).
struct DecBlockGrads : hsimae_dec_block_grads {
    HsDet det;                    // deterministic commits (common.h); {nullptr, nullptr} = fp32 atomics
};
static_assert(sizeof(hsimae_dec_block_grads) == 18 * sizeof(float*), "hsimae_dec_block_grads changed: fused_dec.hip commits exactly 18 gradients");
int hs_dec_block_fwd(const float* x, float* x1, float* x2, hs_bf16* o, float* lse, int nsamples, int Ts, const BlockW& w, hipStream_t s);
int hs_dec_attn_fwd(const float* x, float* x1, hs_bf16* o, float* lse, int nsamples, int Ts, const BlockW& w, hipStream_t s);
// slab: NULL = the block's gradients are committed with float atomics; else >= kDecSlabFloats floats of scratch
// (plan.h slab_bytes(); C ABI: hsimae_dec_block_slab_floats()): per-workgroup partials, summed into the gradients by one
// reduce launch per block.  256 workgroups x (104 in-register dW values x 512 threads + 2112 bias / LayerNorm sums).
constexpr long long kDecSlabFloats = HSIMAE_DEC_BLOCK_SLAB_FLOATS;
struct DecBlockBwd {
    const float *x, *x1, *dy; float *dx1_tmp, *dx; const hs_bf16* o; const float* lse;
    int nsamples, Ts; float* slab = nullptr;
    bool defer_reduce = false;    // slab given: leave its partials for the caller's hs_dec_dw_reduce
};
int hs_dec_block_bwd(const BlockW& w, const DecBlockGrads& g, const DecBlockBwd& p, hipStream_t s);
// The reduce launch of up to hsplan::kDecReduceBlocks blocks whose hs_dec_block_bwd ran with defer_reduce, each into its own slab,
// at the same nsamples: g[i] / slabs[i] of block i.  A block's sums are what its own reduce launch gives, bit for bit.
int hs_dec_dw_reduce(const DecBlockGrads* g, float* const* slabs, int nblocks, int nsamples, int h, hipStream_t s);

// ------------------------------------------------------------------ attn.hip / attn_wide.hip (attention half of an encoder Block)
// blk128_* at D = 128 (8 heads of 16), blk256_* at D = 256 (16 heads of 16), <= 32 tokens: LN1 + q|k|v + attention + projection +
// residual forward; dO + attention backward + du + LayerNorm-1 backward.  Members as in hsimae_attn_block_fwd / _bwd.
struct AttnBlockFwd {
    const float* x; hs_bf16 *u, *qkv, *o; float *lse, *x1; const float* rowscale = nullptr;      // qkv NULL (D = 128): not saved; rowscale NULL: 1
    int Ts, nsamples, mode, len_l;
};
struct AttnBlockBwd {
    const hs_bf16 *qkv, *u, *o; const float* lse; const hs_bf16* dx1b; const float *dx1, *x;      // qkv NULL (D = 128): recomputed from u
    hs_bf16* dqkv; float *dx, *dgamma, *dbeta; HsDet det{nullptr, nullptr};
    int Ts, nsamples, mode, len_l, accumulate;
};
int hs_attn_block_fwd(const BlockW& w, const AttnBlockFwd& p, hipStream_t s);
int hs_attn_block_bwd(const BlockW& w, const AttnBlockBwd& p, hipStream_t s);
int hs_attn_block256_fwd(const BlockW& w, const AttnBlockFwd& p, hipStream_t s);
int hs_attn_block256_bwd(const BlockW& w, const AttnBlockBwd& p, hipStream_t s);      // (reads neither u nor o)

// ------------------------------------------------------------------ fused_enc.hip (MLP half of a Block, D = 128 / 256 / 64)
int hs_enc_mlp_fwd(const float* x1, const float* res2, float* x2, int M, int d, const BlockW& w, hipStream_t s,
                   const float* rowscale = nullptr);
struct EncMlpBwd {
    const float *x1, *dy; float* dx1; hs_bf16 *u2, *dh13, *g, *dyb, *dx1b; float *g_n2w, *g_n2b;
    const float *rs_mlp = nullptr, *rs_attn = nullptr; HsDet det{nullptr, nullptr}; int M, d, plane_rows = 0;      // the optional ones: NULL / 0 = none
};
int hs_enc_mlp_bwd(const BlockW& w, const EncMlpBwd& p, hipStream_t s);

int hs_adamw(float* p, const float* g, float* m, float* v, const unsigned char* group, int64_t n, float lr, float b1, float b2,
             float eps, float wd, int step, hipStream_t s);
// clip.hip: the gradient norm / clip coefficient / skip decision in device memory, and the AdamW step that reads them
int hs_grad_norm(const hsimae_grad_seg* segs, int nseg, float max_norm, int skip_nonfinite, int step, float beta1, float beta2,
                 double* partials, hsimae_clip_ctl* ctl, hipStream_t s);
int hs_adamw_ctl(float* p, const float* g, float* m, float* v, const unsigned char* group, int group_uniform, int64_t n, float lr,
                 float b1, float b2, float eps, float wd, const hsimae_clip_ctl* ctl, hipStream_t s);
int hs_adamw_groups(float* p, const float* g, float* m, float* v, const unsigned char* group, int group_uniform, int64_t n,
                    const hsimae_adamw_group* table, int ngroups, float b1, float b2, float eps, int step, const hsimae_clip_ctl* ctl,
                    hipStream_t s);
// lamb.hip: LAMB's per-tensor trust ratios and step over the flat buffer (moments + partial sums, ratios, apply)
int hs_lamb_step(float* p, const float* g, float* m, float* v, const unsigned char* group, int group_uniform, int64_t n,
                 const hsimae_lamb_tensor* tensors, int ntensors, int nchunks, const hsimae_adamw_group* table, int ngroups, float b1,
                 float b2, float eps, float trust_clip, int always_adapt, double* partials, float* ratios, int* bad,
                 const hsimae_clip_ctl* ctl, hipStream_t s);
// ema.hip: the moving average of the weights behind the step (skipped with it), and the exchange of weights and averages
int hs_ema_update(float* ema, const float* params, int64_t n, double decay, int warmup, int step, const hsimae_clip_ctl* ctl,
                  hipStream_t s);
int hs_ema_swap(float* a, float* b, int64_t n, hipStream_t s);
