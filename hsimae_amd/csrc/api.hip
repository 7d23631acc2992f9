// C ABI of libhsimae_hip.so (include/hsimae_hip.h): geometry/layout helpers, per-kernel entry points and
// the whole-pass forward / backward schedules of the HSIMAE pretraining path.
#include "common.h"
#include "kernels.h"
#include "plan.h"
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <unordered_map>
#include <initializer_list>

using namespace hsplan;

namespace {

#define CK(expr) do { int _e = (expr); if (_e) return _e; } while (0)
#define CK0(expr) do { int _e0 = (expr); if (_e0) return _e0; } while (0)

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
struct BlkP : BlockW {   // resolved pointers of one block of a pass: what the launchers take (kernels.h) + the fp8 images
    struct I8 { const uint8_t* w; const uint8_t* s; } qkv8, p8, w1_8, w3_8, w2_8, qkvT8, pT8, w13T8, w2T8;     // MX e4m3 images (BlockPlan::gemm_fp8)
};

BlkP resolve(const BlkOff& o, const BlkW& w, const float* P, const hs_bf16* wpk, const WLayout& WL, int h) {
    const float* fbase = reinterpret_cast<const float*>(wpk + WL.bf16_elems);
    BlkP b;
    b.h = h;
    b.n1w = P + o.n1w; b.n1b = P + o.n1b; b.bqkv = fbase + w.bqkv; b.pb = P + o.pb; b.n2w = P + o.n2w; b.n2b = P + o.n2b;
    b.w1b = P + o.w1b; b.w3b = P + o.w3b; b.w2b = P + o.w2b;
    b.qkv = wpk + w.qkv; b.p = wpk + w.p; b.w1 = wpk + w.w1; b.w3 = wpk + w.w3; b.w2 = wpk + w.w2;
    b.qkvT = wpk + w.qkvT; b.pT = wpk + w.pT; b.w13T = wpk + w.w13T; b.w2T = wpk + w.w2T;
    b.qf = P + o.qw; b.kf = P + o.kw; b.vf = P + o.vw; b.pf = P + o.pw; b.w1f = P + o.w1w; b.w3f = P + o.w3w;
    const uint8_t* base8 = reinterpret_cast<const uint8_t*>(fbase + WL.f32_elems);
    auto i8 = [&](const Img8& im) { BlkP::I8 r; r.w = base8 + im.w; r.s = base8 + im.s; return r; };
    b.qkv8 = i8(w.qkv8); b.p8 = i8(w.p8); b.w1_8 = i8(w.w1_8); b.w3_8 = i8(w.w3_8); b.w2_8 = i8(w.w2_8);
    b.qkvT8 = i8(w.qkvT8); b.pT8 = i8(w.pT8); b.w13T8 = i8(w.w13T8); b.w2T8 = i8(w.w2T8);
    return b;
}
// The schedule word of a pass (plan.h SC_*): read from the environment by its forward entry point, once, and recorded for the
// workspace arena it fills; the backward entry points look the record up (HSIMAE_ENOFORWARD if there is none).
uint32_t sched_from_env() {
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    auto one = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
    uint32_t b = 0;
    if (!off("HSIMAE_FUSED_DEC")) b |= SC_FUSED_DEC;
    if (!off("HSIMAE_DEC_SPLIT")) b |= SC_DEC_SPLIT;
    if (one("HSIMAE_FP8_UNFUSED")) b |= SC_FP8_UNFUSED;
    if (!off("HSIMAE_FUSED_MLP")) b |= SC_FUSED_MLP;
    if (!off("HSIMAE_FUSED_ATTN_BLOCK")) b |= SC_ATTN_BLOCK;
    if (!off("HSIMAE_FUSED_ATTN_BLOCK256")) b |= SC_ATTN_BLOCK256;
    if (!off("HSIMAE_FUSED_ATTN_BLOCK_BWD")) b |= SC_ATTN_BLOCK_BWD;
    if (!off("HSIMAE_FUSED_PROJ_BWD")) b |= SC_PROJ_BWD;
    if (!off("HSIMAE_FUSED_LNBWD")) b |= SC_LNBWD;
    if (!off("HSIMAE_FUSED_LNBWD_512")) b |= SC_LNBWD_512;
    if (!off("HSIMAE_ATTN_BWD_RECOMPUTE")) b |= SC_RECOMPUTE;
    if (!off("HSIMAE_WGRAD_SLAB")) b |= SC_WGRAD_SLAB;
    if (!off("HSIMAE_DEC_SLAB")) b |= SC_DEC_SLAB;
    if (!off("HSIMAE_WGRAD_PLANAR")) b |= SC_PLANAR;
    if (!off("HSIMAE_FUSED_ATTN_BLOCK256_BWD")) b |= SC_ATTN_BLOCK256_BWD;
    if (!off("HSIMAE_WGRAD_PAIR")) b |= SC_WGRAD_PAIR;
    if (!off("HSIMAE_DEC_REDUCE_ONCE")) b |= SC_DEC_REDUCE_ONCE;
    return b;
}
struct SchedRec { uint32_t enc = 0, dec = 0; bool has_enc = false, has_dec = false; uint64_t gen = 0; int64_t bytes = 0; };
std::mutex g_sched_mu;
std::unordered_map<const void*, SchedRec> g_sched;          // keyed by the workspace arena the forward filled
uint64_t g_sched_gen = 0;
// bytes: the carve of the pass (Ws::bytes).  An allocator hands the address of a freed arena out again, often to a pass of another
// shape: a record only speaks for a backward whose carve is the one the forward filled.
void record_sched(const void* ws, int64_t bytes, bool enc, bool dec, uint32_t bits) {
    std::lock_guard<std::mutex> lk(g_sched_mu);
    // A process that keeps handing new arena addresses (caching allocator churn): drop the OLDEST half — never the entry being
    // recorded, and not the recent ones, whose backward may still be pending (clearing the whole map made a live
    // arena's backward fail with HSIMAE_ENOFORWARD)
    if (g_sched.size() > 4096 && g_sched.find(ws) == g_sched.end()) {
        std::vector<uint64_t> gens;
        gens.reserve(g_sched.size());
        for (auto& kv : g_sched) gens.push_back(kv.second.gen);
        std::nth_element(gens.begin(), gens.begin() + gens.size() / 2, gens.end());
        const uint64_t cut = gens[gens.size() / 2];
        for (auto it = g_sched.begin(); it != g_sched.end();) it = it->second.gen < cut ? g_sched.erase(it) : std::next(it);
    }
    SchedRec& r = g_sched[ws];
    r.gen = ++g_sched_gen;
    if (r.bytes != bytes) { r.has_enc = r.has_dec = false; r.bytes = bytes; }
    if (enc) {
        r.enc = bits; r.has_enc = true;
        // an encoder-only forward re-fills the arena: a decoder record of an EARLIER pass no longer describes what is in it
        if (!dec) r.has_dec = false;
    }
    if (dec) { r.dec = bits; r.has_dec = true; }
}
int lookup_sched(const void* ws, int64_t bytes, bool need_enc, bool need_dec, uint32_t& enc, uint32_t& dec) {
    std::lock_guard<std::mutex> lk(g_sched_mu);
    auto it = g_sched.find(ws);
    if (it == g_sched.end() || it->second.bytes != bytes || (need_enc && !it->second.has_enc) || (need_dec && !it->second.has_dec))
        return HSIMAE_ENOFORWARD;
    enc = it->second.enc; dec = it->second.dec;
    return HSIMAE_OK;
}

// The two axis stacks (blocks_1 / blocks_2, Models.py:556-560) are independent until x1 + x2: the spectral
// stack runs on a side stream so two kernels are resident at once (a single 864-workgroup launch leaves a
// ~45 % tail on 256 CUs).  The stream and its two events are created once per process; HSIMAE_TWO_STREAMS=0
// keeps everything on the caller's stream.
struct Side {
    hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; bool ok = false, init = false;
    std::vector<hipEvent_t> pool; size_t next = 0;        // events handed to the bucket stream, one per reported range
};
// One Side per device, looked up by the device that is current at the call (include/hsimae_hip.h, Contract): a model
// on cuda:1 gets a side stream on cuda:1.  One host thread per device is assumed (fork / join events are shared).
Side& side() {
    static Side sides[32];
    static Side none;
    static std::mutex mu;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return none;
    std::lock_guard<std::mutex> lk(mu);
    Side& x = sides[dev];
    if (!x.init) {
        x.init = true;
        const char* e = getenv("HSIMAE_TWO_STREAMS");
        if (!(e && e[0] == '0'))
            x.ok = hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) == hipSuccess &&
                   hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess &&
                   hipEventCreateWithFlags(&x.join, hipEventDisableTiming) == hipSuccess;
    }
    return x;
}
// next event of the per-device pool (grown on demand, reused round-robin: a wait captures the record that precedes it)
hipEvent_t pool_event(Side& sd) {
    if (sd.pool.size() < 96) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) { sd.pool.push_back(e); return e; }
    }
    if (sd.pool.empty()) return nullptr;
    return sd.pool[sd.next++ % sd.pool.size()];
}

// Reports gradient ranges to the caller's bucket callback.  With io->bucket_stream the consumer's launch stream is
// made to wait for the stream the range's kernels were enqueued on (so side-stream ranges can be reported at once);
// without it a range may only be reported once it is complete on the caller's stream.
struct Emitter {
    hsimae_bucket_cb cb; void* user; hipStream_t bucket; int stage;
    float* grads; const int64_t* det_acc;              // deterministic mode: the range's fixed-point sums become fp32 first
    int operator()(int64_t off, int64_t end, hipStream_t done_on) {
        if (det_acc) CK0(hs_det_convert(det_acc + off, grads + off, end - off, done_on));
        if (cb) {
            if (bucket) {
                hipEvent_t e = pool_event(side());
                if (!e) return (int)hipErrorOutOfMemory;
                CK0((int)hipEventRecord(e, done_on));
                CK0((int)hipStreamWaitEvent(bucket, e, 0));
            }
            cb(stage, off, end - off, user);
        }
        ++stage;
        return HSIMAE_OK;
    }
};

// The C ABI's per-kernel weight structs as a BlockW: what a struct does not have stays NULL
BlockW block_w(const hsimae_mlp_weights& w) {
    BlockW b{};
    b.n2w = w.n2w; b.n2b = w.n2b; b.w1b = w.w1b; b.w3b = w.w3b; b.w2b = w.w2b;
    b.w1 = w.w1; b.w3 = w.w3; b.w2 = w.w2; b.w2T = w.w2T; b.w13T = w.w13T; b.h = w.hidden;
    return b;
}
BlockW block_w(const hsimae_attn_block_weights& w) {
    BlockW b{};
    b.n1w = w.n1w; b.n1b = w.n1b; b.bqkv = w.bqkv; b.pb = w.pb; b.qkv = w.qkv; b.p = w.p; b.qkvT = w.qkvT; b.pT = w.pT;
    return b;
}
BlockW block_w(const hsimae_dec_block_weights& w) {
    BlockW b{};
    b.n1w = w.n1w; b.n1b = w.n1b; b.bqkv = w.bqkv; b.pb = w.pb; b.n2w = w.n2w; b.n2b = w.n2b;
    b.w1b = w.w1b; b.w3b = w.w3b; b.w2b = w.w2b;
    b.qkv = w.qkv; b.p = w.p; b.w1 = w.w1; b.w3 = w.w3; b.w2 = w.w2; b.w2T = w.w2T;
    b.qf = w.qf; b.kf = w.kf; b.vf = w.vf; b.pf = w.pf; b.w1f = w.w1f; b.w3f = w.w3f; b.h = w.hidden;
    return b;
}

// The 18 gradients of one block inside the flat gradient buffer, as the fused decoder backward commits them
DecBlockGrads dec_grads(float* grads, const BlkOff& o, HsDet det) {
    DecBlockGrads g;
    g.n1w = grads + o.n1w; g.n1b = grads + o.n1b; g.qw = grads + o.qw; g.qb = grads + o.qb;
    g.kw = grads + o.kw; g.kb = grads + o.kb; g.vw = grads + o.vw; g.vb = grads + o.vb;
    g.pw = grads + o.pw; g.pb = grads + o.pb; g.n2w = grads + o.n2w; g.n2b = grads + o.n2b;
    g.w1w = grads + o.w1w; g.w1b = grads + o.w1b; g.w2w = grads + o.w2w; g.w2b = grads + o.w2b;
    g.w3w = grads + o.w3w; g.w3b = grads + o.w3b;
    g.det = det;
    return g;
}

GemmParams gp() { GemmParams p; std::memset(&p, 0, sizeof(p)); return p; }

// Weight and bias gradient of one linear outside the blocks: dW [N][K] at grads + dW, db [N] at grads + db, from dO [M][ldo] and A [M][lda].
// tiles: the tile count the row split is sized for (each call site's own: decoder_pred has always passed 1, whatever the decoder width)
int wgrad_one(const void* dO, bool dO_f32, int ldo, const hs_bf16* A, int lda, int N, int K, int64_t M, int tiles, float* grads,
              int64_t dW, int64_t db, int64_t* det_acc, hipStream_t s) {
    WgradParams wg; std::memset(&wg, 0, sizeof(wg));
    WgradTask& t = wg.t[0]; t.dO = dO; t.dO_f32 = dO_f32; t.ldo = ldo; t.A = A; t.lda = lda; t.N = N; t.K = K;
    t.dW = grads + dW; t.ldw = K; t.db = grads + db;
    wg.det_base = grads; wg.det_acc = det_acc;
    wg.ntasks = 1; wg.M = (int)M; wg.msplit = wgrad_msplit(tiles, M);
    return hs_wgrad(wg, s);
}

// One transformer Block forward (Models.py:303-306): 5 launches.
// rs_a / rs_m: optional per-row DropPath factors of the attention / MLP branch (Models.py:304-305), NULL = none.
int block_fwd(const BlkP& P, const BlockPlan& pl, const float* x_in, const BlkBuf& b, int mode, int len_l, const float* res2,
              hipStream_t s, const float* rs_a = nullptr, const float* rs_m = nullptr) {
    GemmParams p = gp();
    const int d = pl.d, dp = pl.dp, heads = pl.heads, h = pl.h, hp = pl.hp, Ts = pl.Ts, nsamples = pl.nsamples;
    const int64_t M = pl.M;
    auto w8 = [&](GemmParams& q, const BlkP::I8& a) { if (pl.gemm_fp8) { q.prec = HSIMAE_PREC_FP8; q.W8 = a.w; q.S8 = a.s; } };
    if (pl.attn_fwd != ATTN_FWD_LAYERED) {
        AttnBlockFwd f;
        f.x = x_in; f.u = b.u; f.qkv = b.qkv; f.o = b.o; f.lse = b.lse; f.x1 = b.x1; f.rowscale = rs_a;
        f.Ts = Ts; f.nsamples = nsamples; f.mode = mode; f.len_l = len_l;
        if (pl.attn_fwd == ATTN_FWD_BLK128) {
            // LN1 + q|k|v + attention + projection + residual in one persistent kernel (attn.hip blk128_fwd_kernel)
            if (!pl.save_qkv) f.qkv = nullptr;
            CK(hs_attn_block_fwd(P, f, s));
        } else {
            // the same half at D = 256 (attn_wide.hip blk256_fwd_kernel: 16 waves = 16 heads, weights streamed from L2)
            CK(hs_attn_block256_fwd(P, f, s));
        }
    } else {
    p.A = x_in; p.lda = dp; p.M = (int)M; p.N = 3 * dp; p.K = dp; p.n_valid = 3 * dp; p.W = P.qkv; p.bias = P.bqkv;
    p.gamma = P.n1w; p.beta = P.n1b; p.u_out = b.u; p.ldu = dp; p.out = b.qkv; p.ldo = 3 * dp; p.ln_width = d;
    w8(p, P.qkv8);
    CK(hs_gemm(p, A_F32_LN, E_BF16, s));
    AttnParams a; std::memset(&a, 0, sizeof(a));
    a.qkv = b.qkv; a.ld = 3 * dp; a.d = d; a.heads = heads; a.hd = d / heads; a.Ts = Ts; a.nsamples = nsamples;
    a.mode = mode; a.len_l = len_l; a.o = b.o; a.ldo = dp; a.lse = b.lse; a.kv_off = dp;
    CK(hs_attn_fwd(a, s));
    p = gp();
    p.A = b.o; p.lda = dp; p.M = (int)M; p.N = dp; p.K = dp; p.n_valid = d; p.W = P.p; p.bias = P.pb;
    p.res = x_in; p.ldr = dp; p.out = b.x1; p.ldo = dp; p.out_rowscale = rs_a;
    w8(p, P.p8);
    CK(hs_gemm(p, A_BF16, E_RES_F32, s));
    }
    if (pl.mlp_fused) return hs_enc_mlp_fwd(b.x1, res2, b.x2, (int)M, d, P, s, rs_m);
    p = gp();
    p.A = b.x1; p.lda = dp; p.M = (int)M; p.N = hp; p.K = dp; p.n_valid = h; p.W = P.w1; p.W2 = P.w3; p.bias = P.w1b;
    p.bias2 = P.w3b; p.gamma = P.n2w; p.beta = P.n2b; p.u_out = b.u2; p.ldu = dp; p.out = b.g; p.ldo = hp;
    p.h13 = b.h13; p.ldh = 2 * hp; p.hoff = hp; p.ln_width = d;
    if (pl.gemm_fp8) { w8(p, P.w1_8); p.W8b = P.w3_8.w; p.S8b = P.w3_8.s; }
    CK(hs_gemm(p, A_F32_LN, E_SWIGLU, s));
    p = gp();
    p.A = b.g; p.lda = hp; p.M = (int)M; p.N = dp; p.K = hp; p.n_valid = d; p.W = P.w2; p.bias = P.w2b;
    p.res = b.x1; p.res2 = res2; p.ldr = dp; p.out = b.x2; p.ldo = dp; p.out_rowscale = rs_m;
    w8(p, P.w2_8);
    return hs_gemm(p, A_BF16, E_RES_F32, s);
}

// The weight-gradient launch of up to two consecutive blocks of a stack (BlockPlan::wgrad_pair), and of decoder_embed with the first
// fusion pair: block_bwd deposits its 7 tasks here instead of launching, the stack's loop launches when the second block has
// deposited or the stack ends, and reports the ranges the launch completed, in the order they were noted (back to front).  Every
// task shares M.  The operands that are per-stream scratch alternate between two sets (plan.h Ws::scb), so the stream's order alone
// keeps them alive until the launch.
struct WgPair {
    WgradParams g; int nblk = 0, nrange = 0; int64_t off[3], end[3];
    WgPair() { std::memset(&g, 0, sizeof(g)); }
    void note(int64_t o, int64_t e) { off[nrange] = o; end[nrange] = e; ++nrange; }
};
// launch what is pending on `s` and report its ranges (emit NULL: the caller reports them later)
int wgpair_flush(WgPair& pr, int concurrent, hipStream_t s, Emitter* emit) {
    if (pr.g.ntasks) {
        pr.g.msplit = wgrad_msplit(wg_tiles(pr.g, 128), pr.g.M, concurrent);
        CK(hs_wgrad(pr.g, s));
    }
    if (emit)
        for (int i = 0; i < pr.nrange; ++i) CK((*emit)(pr.off[i], pr.end[i], s));
    pr = WgPair();
    return HSIMAE_OK;
}
// block [off, end) of a stack has run its block_bwd on `s`: launch and report now, or with the next block (pairing, not the last)
int wgpair_block_done(WgPair& pr, bool pairing, bool last, int64_t off, int64_t end, int concurrent, hipStream_t s, Emitter* emit) {
    pr.note(off, end);
    ++pr.nblk;
    if (pairing && pr.nblk < 2 && !last) return HSIMAE_OK;
    return wgpair_flush(pr, concurrent, s, emit);
}

// One Block backward: data grads (7 launches) + all weight/bias grads of the block (1 launch; pend: deposited there, see WgPair).
int block_bwd(const BlkP& P, const BlockPlan& pl, const BlkOff& o, float* grads, const float* x_in, const BlkBuf& b, int mode,
              int len_l, float* G0, const Scr& w, float* dx_out, int accumulate, hipStream_t s, int concurrent = 1,
              const float* rs_a = nullptr, const float* rs_m = nullptr, int64_t* det_acc = nullptr, WgradParams* pend = nullptr) {
    float* G1 = w.G1;
    if (pend && !pl.wgrad_pair) return HSIMAE_EUNSUPPORTED;
    GemmParams p = gp();
    const int d = pl.d, dp = pl.dp, heads = pl.heads, h = pl.h, hp = pl.hp, Ts = pl.Ts, nsamples = pl.nsamples;
    const int64_t M = pl.M;
    LnBwdParams l; std::memset(&l, 0, sizeof(l));
    l.M = (int)M; l.d = d; l.ld = dp; l.det_base = grads; l.det_acc = det_acc;
    const HsDet det{grads, reinterpret_cast<long long*>(det_acc)};
    auto w8 = [&](GemmParams& q, const BlkP::I8& a) { if (pl.gemm_fp8) { q.prec = HSIMAE_PREC_FP8; q.W8 = a.w; q.S8 = a.s; } };
    bool g1b_done = false;
    // g / dh1 / dh3 as 64-column planes (include/hsimae_hip.h, hsimae_wgrad_task) of prow rows (plan.h: the arena reserves kPlanePadRows)
    const int hp64 = rup(hp, 64), prow = pl.plane_rows;
    if (pl.mlp_fused) {
        // recompute u2 / h1 / h3 / g inside the tile; emits dx1 and the wgrad operands u2, dh1|dh3, g, bf16 dY and dx1
        EncMlpBwd m;
        m.x1 = b.x1; m.dy = G0; m.dx1 = G1; m.u2 = b.u2; m.dh13 = w.dh13; m.g = b.g; m.dyb = w.g0b; m.dx1b = w.g1b;
        m.g_n2w = grads + o.n2w; m.g_n2b = grads + o.n2b; m.rs_mlp = rs_m; m.rs_attn = rs_a; m.det = det;
        m.M = (int)M; m.d = d; m.plane_rows = prow;
        CK(hs_enc_mlp_bwd(P, m, s));
    } else {
        p.A = G0; p.lda = dp; p.M = (int)M; p.N = hp; p.K = dp; p.n_valid = hp; p.W = P.w2T; p.out = w.dh13; p.ldo = 2 * hp;
        p.h13 = b.h13; p.ldh = 2 * hp; p.hoff = hp; p.a_rowscale = rs_m;        // DropPath: the branch saw rs_m * dY
        w8(p, P.w2T8);
        CK(hs_gemm(p, A_F32, E_SWIGLU_BWD, s));
        p = gp();
        p.A = w.dh13; p.lda = 2 * hp; p.M = (int)M; p.N = dp; p.K = 2 * hp; p.n_valid = d; p.W = P.w13T;
        w8(p, P.w13T8);
        if (pl.ln2_bwd == LN_GEMM_EPILOGUE) { // LayerNorm-2 backward as the epilogue of the k-outer GEMM (the whole row is on chip)
            p.out = G1; p.ldo = dp; p.res = G0; p.ldr = dp; p.lnx = b.x1; p.gamma = P.n2w; p.accumulate = 0;
            p.dgamma = grads + o.n2w; p.dbeta = grads + o.n2b; p.det_base = grads; p.det_acc = det_acc;
            if (!rs_a) { p.u_out = w.g1b; p.ldu = dp; g1b_done = true; }      // bf16 copy of dx1 from the epilogue (no DropPath factor to fold in)
            CK(hs_gemm(p, A_BF16, E_LN_BWD, s));
        } else {
            p.out = w.du; p.ldo = dp;
            CK(hs_gemm(p, A_BF16, E_F32, s));
            l.du = w.du; l.x = b.x1; l.gamma = P.n2w; l.dres = G0; l.dx = G1; l.accumulate = 0;
            l.dgamma = grads + o.n2w; l.dbeta = grads + o.n2b;
            CK(hs_ln_bwd(l, s));
        }
        // bf16 copies of dY / dx1 (with the DropPath factors folded in) so that the weight gradients below take the
        // LDS-DMA kernel: 666 -> ~300 us per block at D = 256
        CK(hs_rows_to_bf16(G0, w.g0b, M, dp, rs_m, s));
        if (!g1b_done) CK(hs_rows_to_bf16(G1, w.g1b, M, dp, rs_a, s));
    }
    // All weight / bias gradients of the block: 7 tasks for the batched weight-gradient kernel (every operand is a bf16 buffer on the
    // fused path, so no launch below reads G0 / G1, which the LayerNorm-1 backward overwrites with dx when the caller runs in place).
    // (Round 4 measured the same work as two launches, each right behind the kernel that produced its operands: + 0.3 ms per step,
    //  removed in round 5.)
    auto run_wgrad = [&]() -> int {
        WgradParams own; std::memset(&own, 0, sizeof(own));
        WgradParams& g = pend ? *pend : own;
        if (g.ntasks + 7 > 16) return HSIMAE_EDIMS;
        auto task = [&](int, const void* dO, int ldo, const hs_bf16* A, int lda, int N, int K, int64_t dW, int64_t db) {
            WgradTask& t = g.t[g.ntasks++];
            t.dO = dO; t.dO_f32 = 0; t.ldo = ldo; t.A = A; t.lda = lda; t.N = N; t.K = K; t.dW = grads + dW; t.ldw = K;
            t.db = grads + db; t.dO_rowscale = nullptr;
        };
        task(0, w.dqkv, 3 * dp, b.u, dp, d, d, o.qw, o.qb);
        task(1, w.dqkv + dp, 3 * dp, b.u, dp, d, d, o.kw, o.kb);
        task(2, w.dqkv + 2 * dp, 3 * dp, b.u, dp, d, d, o.vw, o.vb);
        task(3, w.g1b, dp, b.o, dp, d, d, o.pw, o.pb);              // all-bf16 operands: wgrad takes its LDS-DMA path
        if (pl.planar) {
            task(4, w.dh13, hp64, b.u2, dp, h, d, o.w1w, o.w1b); g.t[g.ntasks - 1].dO_plane_rows = prow;
            task(5, w.dh13 + (int64_t)hp64 * prow, hp64, b.u2, dp, h, d, o.w3w, o.w3b); g.t[g.ntasks - 1].dO_plane_rows = prow;
        } else {
            task(4, w.dh13, 2 * hp, b.u2, dp, h, d, o.w1w, o.w1b);
            task(5, w.dh13 + hp, 2 * hp, b.u2, dp, h, d, o.w3w, o.w3b);
        }
#ifdef HS_ABL_DW2           /* timing ablation (variant builds only, see fused_enc.hip): the W2 task leaves the launch on the fused path */
        if (!pl.mlp_fused)
#endif
        { task(6, w.g0b, dp, b.g, pl.planar ? hp64 : hp, d, h, o.w2w, o.w2b); g.t[g.ntasks - 1].A_plane_rows = prow; }
        g.M = (int)M; g.det_base = grads; g.det_acc = det_acc;
        if (pend) return HSIMAE_OK;                              // (128-tiles: no slab)
        g.slab = pl.wgrad_slab ? w.slab : nullptr;               // this stream's slab (NULL: float atomics on dW also in the 256 x 256-tile launches)
        g.msplit = wgrad_msplit(wg_tiles(g, 128), M, concurrent);
        return hs_wgrad(g, s);
    };
    AttnParams a; std::memset(&a, 0, sizeof(a));
    a.qkv = b.qkv; a.ld = 3 * dp; a.d = d; a.heads = heads; a.hd = d / heads; a.Ts = Ts; a.nsamples = nsamples;
    a.mode = mode; a.len_l = len_l; a.o = b.o; a.ldo = dp; a.lse = b.lse; a.dout = w.dob; a.lddo = dp; a.dqkv = w.dqkv; a.kv_off = dp;
    // dO, the attention backward, du and the LayerNorm-1 backward as ONE persistent launch: round 5 at D = 256 (Large; attn_wide.hip
    // blk256_bwd_kernel, from the saved q|k|v), round 4 at d = 128 (attn.hip blk128_bwd_kernel; q|k|v recomputed from u when the
    // forward did not save them)
    if (pl.attn_bwd != ATTN_BWD_LAYERED) {
        AttnBlockBwd r;
        r.qkv = b.qkv; r.u = b.u; r.o = b.o; r.lse = b.lse; r.dx1b = w.g1b; r.dx1 = G1; r.x = x_in; r.dqkv = w.dqkv; r.dx = dx_out;
        r.dgamma = grads + o.n1w; r.dbeta = grads + o.n1b; r.det = det;
        r.Ts = Ts; r.nsamples = nsamples; r.mode = mode; r.len_l = len_l; r.accumulate = accumulate;
        if (pl.attn_bwd == ATTN_BWD_BLK256) {
            CK(hs_attn_block256_bwd(P, r, s));
        } else {
            if (!pl.save_qkv) r.qkv = nullptr;
            CK(hs_attn_block_bwd(P, r, s));
        }
        return run_wgrad();
    }
    p = gp();
    p.A = w.g1b; p.lda = dp; p.M = (int)M; p.N = dp; p.K = dp; p.n_valid = dp;  // (the bf16 copy carries the DropPath factor)
    p.W = P.pT; p.out = w.dob; p.ldo = dp;
    w8(p, P.pT8);
    CK(hs_gemm(p, A_BF16, E_BF16, s));
    CK(hs_attn_bwd(a, s));
    CK(run_wgrad());
    // du = dqkv * Wqkv and the LayerNorm-1 backward: one kernel where the GEMM has the LN backward as its epilogue (du never goes
    // to HBM), two otherwise
    const bool ln_fused = pl.ln1_bwd == LN_GEMM_EPILOGUE;
    p = gp();
    p.A = w.dqkv; p.lda = 3 * dp; p.M = (int)M; p.N = dp; p.K = 3 * dp; p.n_valid = d; p.W = P.qkvT;
    if (ln_fused) {
        p.out = dx_out; p.ldo = d; p.res = G1; p.ldr = d; p.lnx = x_in; p.gamma = P.n1w; p.accumulate = accumulate;
        p.dgamma = grads + o.n1w; p.dbeta = grads + o.n1b; p.det_base = grads; p.det_acc = det_acc;
        if (d != 128) w8(p, P.qkvT8);
        CK(hs_gemm(p, A_BF16, E_LN_BWD, s));       // d = 128: row-panel kernel with the LN backward as its epilogue; d = 256 / 512: k-outer
    } else {
        p.out = w.du; p.ldo = dp;
        w8(p, P.qkvT8);
        CK(hs_gemm(p, A_BF16, E_F32, s));
        l.du = w.du; l.x = x_in; l.gamma = P.n1w; l.dres = G1; l.dx = dx_out; l.accumulate = accumulate;
        l.dgamma = grads + o.n1w; l.dbeta = grads + o.n1b;
        CK(hs_ln_bwd(l, s));
    }
    return HSIMAE_OK;
}

struct Ctx {
    Geo g; PLayout L; WLayout W; Ws w;
    int N, K, len_t, len_l;
    int64_t Me, Md;
};

int make_ctx(const hsimae_config* cfg, const hsimae_io* io, Ctx& c, bool need_ws) {
    CK(make_geo(cfg, c.g));
    if (!io) return HSIMAE_ENULL;
    c.N = io->N; c.len_t = io->len_t; c.len_l = io->len_l;
    if (c.N <= 0 || c.len_t < 1 || c.len_t > c.g.T || c.len_l < 1 || c.len_l > 9) return HSIMAE_EDIMS;
    c.K = c.len_t * c.len_l;
    c.Me = (int64_t)c.N * c.K; c.Md = (int64_t)c.N * c.g.TL;
    if (c.Md * 96 >= (1ll << 31) || c.Me * 3 * c.g.Dp >= (1ll << 31)) return HSIMAE_EUNSUPPORTED;   // 32-bit row math in kernels
    make_playout(c.g, c.L);
    make_wlayout(c.g, c.W);
    if (need_ws) {
        if (!io->workspace || !io->params || !io->wpk) return HSIMAE_ENULL;
        if (reinterpret_cast<uintptr_t>(io->workspace) % 256) return HSIMAE_EALIGN;
        carve(c.g, c.N, c.K, reinterpret_cast<char*>(io->workspace), c.w);
        if (c.w.bytes > io->workspace_bytes) return HSIMAE_EDIMS;
    }
    return HSIMAE_OK;
}

// The plans of a pass (plan.h), each filled once per stack per pass from the pass's schedule word
BlockPlan enc_plan(const Ctx& c, uint32_t sc) {
    return plan_block(c.g.D, c.g.H, c.g.h, c.K, c.N, c.Me, enc_linears_fp8(c.g.prec, c.g.D, sc), sc);
}
BlockPlan dec_block_plan(const Ctx& c, uint32_t sc) {           // the decoder run layer at a time
    return plan_block(c.g.Dd, c.g.Hd, c.g.hdec, c.g.TL, c.N, c.Md, false, sc);
}

// The decoder after decoder_embed (Models.py:582-600), shared by hsimae_forward and hsimae_decode: sequence assembly from w.y,
// the blocks, decoder_norm + decoder_pred into pred [Md][72]
int decoder_stack_fwd(const Ctx& c, const hsimae_io* io, uint32_t sc, float* pred, hipStream_t s) {
    const Geo& g = c.g; const Ws& w = c.w; const float* P = io->params;
    AssembleParams as; std::memset(&as, 0, sizeof(as));
    as.y = w.y; as.N = c.N; as.K = c.K; as.TL = g.TL; as.Dd = g.Dd; as.ld = g.Ddp; as.ids_restore = io->ids_restore; as.pos = P + c.L.dpos;
    as.yfull = w.yfull;
    CK(hs_assemble_fwd(as, s));
    const DecPlan dec = plan_dec(c.g.Dd, c.g.Hd, c.g.hdec, c.g.TL, sc);
    const BlockPlan lay = dec_block_plan(c, sc);
    const float* z = w.yfull;
    for (int i = 0; i < g.ddepth; ++i) {
        const BlkP bp = resolve(c.L.bd[i], c.W.bd[i], P, io->wpk, c.W, g.hdec);
        const BlkBuf& b = w.bd[i];
        if (!dec.fused) {
            CK(block_fwd(bp, lay, z, b, 0, 9, nullptr, s));
        } else if (dec.split) {
            CK(hs_dec_attn_fwd(z, b.x1, b.o, b.lse, c.N, g.TL, bp, s));
            CK(hs_enc_mlp_fwd(b.x1, nullptr, b.x2, (int)c.Md, g.Dd, bp, s));
        } else {
            CK(hs_dec_block_fwd(z, b.x1, b.x2, b.o, b.lse, c.N, g.TL, bp, s));
        }
        z = b.x2;
    }
    GemmParams p = gp();
    p.A = z; p.lda = g.Ddp; p.M = (int)c.Md; p.N = 80; p.K = g.Ddp; p.n_valid = 72; p.W = io->wpk + c.W.dp; p.bias = P + c.L.dpb;
    p.gamma = P + c.L.dnw; p.beta = P + c.L.dnb; p.u_out = w.zn; p.ldu = g.Ddp; p.out = pred; p.ldo = 72; p.ln_width = g.Dd;
    return hs_gemm(p, A_F32_LN, E_F32, s);
}

}  // namespace

// ====================================================================== C ABI
extern "C" unsigned hs_variant_bits_gemm();
extern "C" unsigned hs_variant_bits_attn();
extern "C" unsigned hs_variant_bits_attn_wide();
extern "C" unsigned hs_variant_bits_wgrad();
extern "C" unsigned hs_variant_bits_elem();
extern "C" unsigned hs_variant_bits_pack();
extern "C" unsigned hs_variant_bits_fused_dec();
extern "C" unsigned hs_variant_bits_fused_enc();
extern "C" unsigned hs_variant_bits_loader();
extern "C" unsigned hs_variant_bits_scene();
extern "C" unsigned hs_variant_bits_gwpca();
extern "C" unsigned hs_variant_bits_cls();
extern "C" unsigned hs_variant_bits_clip();
extern "C" unsigned hs_variant_bits_lamb();
extern "C" unsigned hs_variant_bits_ema();
extern "C" unsigned hs_variant_bits_prob();
extern "C" unsigned hs_variant_bits_knn();
extern "C" unsigned hs_variant_bits_kmeans();
extern "C" unsigned hs_variant_bits_recon();
extern "C" unsigned hs_variant_bits_probe();
extern "C" unsigned hs_variant_bits_smooth();
extern "C" unsigned hs_variant_bits_slic();
extern "C" unsigned hs_variant_bits_svm();
#ifndef HS_KERNEL_SOURCE_HASH
#define HS_KERNEL_SOURCE_HASH 0ULL
#endif
#ifndef HS_BUILD_FLAGS_HASH
#define HS_BUILD_FLAGS_HASH 0ULL
#endif
#ifndef HS_BUILD_DEFAULT_FLAGS
#define HS_BUILD_DEFAULT_FLAGS 0
#endif

extern "C" {

int hsimae_version(void) { return HSIMAE_VERSION; }

int hsimae_build_info(hsimae_build_info_t* out) {
    if (!out) return HSIMAE_ENULL;
    out->abi_version = HSIMAE_VERSION;
    out->variant_bits = hs_variant_bits() | hs_variant_bits_gemm() | hs_variant_bits_attn() | hs_variant_bits_attn_wide() | hs_variant_bits_wgrad() | hs_variant_bits_elem() | hs_variant_bits_pack() | hs_variant_bits_fused_dec() | hs_variant_bits_fused_enc() | hs_variant_bits_loader() | hs_variant_bits_scene() | hs_variant_bits_gwpca() | hs_variant_bits_cls() | hs_variant_bits_clip() | hs_variant_bits_lamb() | hs_variant_bits_ema() | hs_variant_bits_prob() | hs_variant_bits_knn() | hs_variant_bits_kmeans() | hs_variant_bits_recon() | hs_variant_bits_probe() | hs_variant_bits_smooth() | hs_variant_bits_slic() | hs_variant_bits_svm();
    out->kernel_source_hash = HS_KERNEL_SOURCE_HASH;
    out->flags_hash = HS_BUILD_FLAGS_HASH;
    out->default_flags = HS_BUILD_DEFAULT_FLAGS;
    out->reserved = 0;
    return HSIMAE_OK;
}
const char* hsimae_variant_name(int bit) {
    switch (bit) {
#define HS_X(b, name) case b: return #name;
        HS_VARIANT_TABLE(HS_X)
#undef HS_X
        default: return nullptr;
    }
}

int hsimae_two_streams_active(void) { return side().ok ? 1 : 0; }
int hsimae_effective_precision(const hsimae_config* cfg) {
    if (!cfg) return HSIMAE_ENULL;
    Geo g; CK(make_geo(cfg, g));
    return enc_linears_fp8(g.prec, g.D, sched_from_env()) ? HSIMAE_PREC_FP8 : HSIMAE_PREC_BF16;
}

const char* hsimae_strerror(int code) {
    switch (code) {
        case HSIMAE_OK: return "ok";
        case HSIMAE_EDIMS: return "bad dimensions or strides";
        case HSIMAE_EUNSUPPORTED: return "configuration not supported by the gfx950 kernels";
        case HSIMAE_EALIGN: return "misaligned pointer";
        case HSIMAE_ENULL: return "required pointer is NULL";
        case HSIMAE_ENOFORWARD: return "no forward pass of this process has filled this workspace (the backward follows the forward's recorded schedule)";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int hsimae_param_layout(const hsimae_config* cfg, int64_t* offsets, int64_t* sizes, int max_entries) {
    return param_layout(cfg, offsets, sizes, max_entries);
}

int64_t hsimae_wpk_elems(const hsimae_config* cfg) { return wpk_elems(cfg); }

int64_t hsimae_pack_table_bytes(const hsimae_config* cfg) { return pack_table_bytes(cfg); }

int hsimae_build_pack_table(const hsimae_config* cfg, const float* params_dev, hs_bf16* wpk_dev, void* table_host) {
    return build_pack_table(cfg, params_dev, wpk_dev, table_host);
}

int hsimae_pack_params(const hsimae_config* cfg, const void* table_dev, void* stream) {
    Geo g; CK(make_geo(cfg, g));
    if (!table_dev) return HSIMAE_ENULL;
    const int n = (int)(hsimae_pack_table_bytes(cfg) / (int64_t)sizeof(PackDesc));
    const int maxe = std::max({g.D * g.D, g.h * g.D, g.Dd * g.Dd, g.hdec * g.Dd, g.D * g.Dd, g.D * 72});
    return hs_pack(reinterpret_cast<const PackDesc*>(table_dev), n, maxe, S(stream));
}

int64_t hsimae_workspace_bytes(const hsimae_config* cfg, int32_t N, int32_t len_t, int32_t len_l) {
    return workspace_bytes(cfg, N, len_t, len_l);
}

// DropPath factors of encoder block `e` (execution order blocks_1, blocks_2, blocks): {attention, MLP} row vectors
struct DropRs { const float* a; const float* m; };
static DropRs drop_rs(const hsimae_io* io, int e, int64_t Me) {
    if (!io->drop_scale) return DropRs{nullptr, nullptr};
    const float* base = io->drop_scale + (int64_t)e * 2 * Me;
    return DropRs{base, base + Me};
}

static int forward_impl(const hsimae_config* cfg, const hsimae_io* io, void* stream, bool encoder_only) {
    Ctx c; CK(make_ctx(cfg, io, c, true));
    if (!io->x || !io->noise1 || !io->noise2 || !io->mask || !io->ids_keep || !io->ids_restore) return HSIMAE_ENULL;
    if (encoder_only ? !io->latent : !io->loss) return HSIMAE_ENULL;
    if (!encoder_only && io->want_recons && (!io->pred_img || !io->mask_img)) return HSIMAE_ENULL;
    hipStream_t s = S(stream);
    const Geo& g = c.g; const float* P = io->params; const Ws& w = c.w;
    const uint32_t sc = sched_from_env();             // the pass's schedule: read here, recorded for the backward (plan.h SC_*)
    record_sched(io->workspace, c.w.bytes, true, !encoder_only, sc);
    const BlockPlan enc = enc_plan(c, sc);

    MaskParams m; m.noise1 = io->noise1; m.noise2 = io->noise2; m.N = c.N; m.T = g.T; m.L = 9; m.len_t = c.len_t;
    m.len_l = c.len_l; m.ids_keep = io->ids_keep; m.ids_restore = io->ids_restore; m.mask = io->mask;
    CK(hs_mask(m, s));
    PatchParams pp; pp.x = io->x; pp.sn = io->sn; pp.sb = io->sb; pp.sh = io->sh; pp.sw = io->sw; pp.N = c.N; pp.T = g.T;
    pp.K = c.K; pp.ids_keep = io->ids_keep; pp.out = w.a_pe; pp.pos_ids = nullptr;
    CK(hs_patch_gather(pp, s));
    GemmParams p = gp();
    p.A = w.a_pe; p.lda = 96; p.M = (int)c.Me; p.N = g.Dp; p.K = 96; p.n_valid = g.D; p.W = io->wpk + c.W.pe; p.bias = P + c.L.peb;
    p.pos = P + c.L.pos; p.ids = io->ids_keep; p.ldpos = g.D; p.out = w.x0; p.ldo = g.Dp;
    CK(hs_gemm(p, A_BF16, E_POS_F32, s));

    const float* x = w.x0;
    if (g.has_axis) {
        Side& sd = side();
        const bool forked = sd.ok && g.sdepth > 1;
        if (forked) {
            CK((int)hipEventRecord(sd.fork, s));
            CK((int)hipStreamWaitEvent(sd.s, sd.fork, 0));
        }
        const float* xa = w.x0;
        const float* xb = w.x0;
        for (int i = 0; i < g.sdepth; ++i) {
            // spatial stack: attend within one kept band group (Models.py:553,556)
            BlkP b1 = resolve(c.L.b1[i], c.W.b1[i], P, io->wpk, c.W, g.h);
            const DropRs r1 = drop_rs(io, i, c.Me), r2d = drop_rs(io, g.sdepth + i, c.Me);
            CK(block_fwd(b1, enc, xa, w.b1[i], 1, c.len_l, nullptr, s, r1.a, r1.m));
            xa = w.b1[i].x2;
            // spectral stack: attend within one kept position (Models.py:554,559)
            BlkP b2 = resolve(c.L.b2[i], c.W.b2[i], P, io->wpk, c.W, g.h);
            const bool last = (i == g.sdepth - 1);
            const float* r2 = last ? xa : nullptr;                      // x1 + x2 fused into the last epilogue (Models.py:564)
            if (last && forked) {                                       // needs the spatial stack's result: rejoin first
                CK((int)hipEventRecord(sd.join, sd.s));
                CK((int)hipStreamWaitEvent(s, sd.join, 0));
            }
            CK(block_fwd(b2, enc, xb, w.b2[i], 2, c.len_l, r2, (forked && !last) ? sd.s : s, r2d.a, r2d.m));
            xb = w.b2[i].x2;
        }
        x = xb;
    }
    for (int i = 0; i < g.nfus; ++i) {
        BlkP bp = resolve(c.L.bf[i], c.W.bf[i], P, io->wpk, c.W, g.h);
        const DropRs rf = drop_rs(io, (g.has_axis ? 2 * g.sdepth : 0) + i, c.Me);
        CK(block_fwd(bp, enc, x, w.bf[i], 0, c.len_l, nullptr, s, rf.a, rf.m));
        x = w.bf[i].x2;
    }
    if (encoder_only) {                       // `norm` only (Models.py:570 / 892): the latent the fine-tuning head reads
        CK(hs_ln_fwd(x, P + c.L.nw, P + c.L.nb, io->latent, (int)c.Me, g.D, s, g.Dp, g.D));
        return HSIMAE_OK;
    }
    // norm + decoder_embed (Models.py:570, 579)
    p = gp();
    p.A = x; p.lda = g.Dp; p.M = (int)c.Me; p.N = g.Ddp; p.K = g.Dp; p.n_valid = g.Dd; p.W = io->wpk + c.W.de; p.bias = P + c.L.deb;
    p.gamma = P + c.L.nw; p.beta = P + c.L.nb; p.u_out = w.lat; p.ldu = g.Dp; p.out = w.y; p.ldo = g.Ddp; p.ln_width = g.D;
    CK(hs_gemm(p, A_F32_LN, E_F32, s));
    CK(decoder_stack_fwd(c, io, sc, w.pred, s));
    LossParams lp; std::memset(&lp, 0, sizeof(lp));
    const float sum_mask = (float)((int64_t)c.N * (g.TL - c.K));
    lp.x = io->x; lp.sn = io->sn; lp.sb = io->sb; lp.sh = io->sh; lp.sw = io->sw; lp.N = c.N; lp.T = g.T; lp.pred = w.pred;
    lp.mask = io->mask; lp.norm_pix = g.norm_pix; lp.inv_scale = io->grad_scale / (72.f * sum_mask); lp.partial = w.partial;
    lp.loss = io->loss; lp.sum_mask = sum_mask; lp.dpred = w.dpred;
    lp.pred_img = io->want_recons ? io->pred_img : nullptr; lp.mask_img = io->want_recons ? io->mask_img : nullptr;
    CK(hs_loss(lp, s));
    if (io->pred) CK((int)hipMemcpyAsync(io->pred, w.pred, c.Md * 72 * 4, hipMemcpyDeviceToDevice, s));
    if (io->latent) CK(hs_ln_fwd(x, P + c.L.nw, P + c.L.nb, io->latent, (int)c.Me, g.D, s, g.Dp, g.D));
    return HSIMAE_OK;
}

int hsimae_forward(const hsimae_config* cfg, const hsimae_io* io, void* stream) { return forward_impl(cfg, io, stream, false); }
int hsimae_encode(const hsimae_config* cfg, const hsimae_io* io, void* stream) { return forward_impl(cfg, io, stream, true); }

int hsimae_decode(const hsimae_config* cfg, const hsimae_io* io, const float* latent, float* pred, void* stream) {
    Ctx c; CK(make_ctx(cfg, io, c, true));
    if (!latent || !pred || !io->ids_restore) return HSIMAE_ENULL;
    hipStream_t s = S(stream);
    const Geo& g = c.g; const float* P = io->params; const Ws& w = c.w;
    const uint32_t sc = sched_from_env();
    record_sched(io->workspace, c.w.bytes, false, true, sc);     // (the decoder's part only: an encoder pass in the same arena keeps its own record)
    GemmParams p = gp();                      // decoder_embed (Models.py:579)
    const float* lat_in = latent;
    if (g.Dp != g.D) {      // rows stored wider than the model: stage the caller's [Me][D] latent into a padded buffer (pad columns are zeros)
        CK((int)hipMemcpy2DAsync(w.G2, (size_t)g.Dp * 4, latent, (size_t)g.D * 4, (size_t)g.D * 4, (size_t)c.Me, hipMemcpyDeviceToDevice, s));
        lat_in = w.G2;
    }
    p.A = lat_in; p.lda = g.Dp; p.M = (int)c.Me; p.N = g.Ddp; p.K = g.Dp; p.n_valid = g.Dd; p.W = io->wpk + c.W.de; p.bias = P + c.L.deb;
    p.out = w.y; p.ldo = g.Ddp;
    CK(hs_gemm(p, A_F32, E_F32, s));
    CK(hs_rows_to_bf16(lat_in, w.lat, c.Me, g.Dp, nullptr, s));     // decoder_embed's wgrad operand (hsimae_decode_backward)
    return decoder_stack_fwd(c, io, sc, pred, s);
}

// Backward of the encoder stacks + patch embedding, from d(x of the last encoder block) in w.G0.  Shared by
// hsimae_backward (after the decoder) and hsimae_encode_backward (after `norm`).
// first: what the caller already deposited for the first fusion-block launch (decoder_embed's task and range), else empty.
static int encoder_backward(const Ctx& c, const hsimae_io* io, float* grads, hipStream_t s, Emitter& emit, uint32_t sc, WgPair& first) {
    const Geo& g = c.g; const float* P = io->params; const Ws& w = c.w; const PLayout& L = c.L;
    const BlockPlan enc = enc_plan(c, sc);
    // paired weight-gradient launches: block k of a stack (counted from its last) leaves its operands in scratch set k % 2
    const bool pairing = enc.wgrad_pair;
    float* dx = w.G0;               // d(x0) once the blocks are through
    for (int i = g.nfus - 1, k = 0; i >= 0; --i, ++k) {
        BlkP bp = resolve(L.bf[i], c.W.bf[i], P, io->wpk, c.W, g.h);
        const float* xin = (i > 0) ? w.bf[i - 1].x2 : (g.has_axis ? w.b2[g.sdepth - 1].x2 : w.x0);
        const DropRs rf = drop_rs(io, (g.has_axis ? 2 * g.sdepth : 0) + i, c.Me);
        CK(block_bwd(bp, enc, L.bf[i], grads, xin, w.bf[i], 0, c.len_l, w.G0, (pairing && (k & 1)) ? w.scb : w.sc, w.G0, 0, s, 1, rf.a, rf.m,
                     io->det_acc, pairing ? &first.g : nullptr));
        CK(wgpair_block_done(first, pairing, i == 0, L.bf[i].n1w, L.bf[i].end, 1, s, &emit));
    }
    if (g.has_axis) {
        // d(x1 + x2) in G0 feeds both stacks (Models.py:564) and neither overwrites it: the spatial stack's dX goes to G2, the spectral
        // stack's, which runs on the side stream, to G3; the spatial stack's last step accumulates onto G3 after the join
        Side& sd = side();
        const bool forked = sd.ok && g.sdepth > 1;
        if (forked) {
            CK((int)hipEventRecord(sd.fork, s));
            CK((int)hipStreamWaitEvent(sd.s, sd.fork, 0));
        }
        hipStream_t s2 = forked ? sd.s : s;
        // (pairing on one stream: the spectral stack's pending operands must outlive the spatial block that follows, so it takes the
        //  side stream's sets there too)
        const Scr& scr2 = (forked || pairing) ? w.sc2 : w.sc;
        // with a bucket stream every block's range is reported as soon as its kernels are enqueued (the consumer waits
        // for the right stream through an event); without one the side stream's ranges wait for the join
        const bool per_block = emit.bucket != nullptr || !forked;
        Emitter* em = per_block ? &emit : nullptr;
        const int conc = forked ? 2 : 1, top = g.sdepth - 1;
        WgPair pr1, pr2;
        for (int i = top, k = 0; i >= 0; --i, ++k) {
            const bool alt = pairing && (k & 1);
            BlkP b2 = resolve(L.b2[i], c.W.b2[i], P, io->wpk, c.W, g.h);
            const DropRs r1 = drop_rs(io, i, c.Me), r2d = drop_rs(io, g.sdepth + i, c.Me);
            const float* xin2 = (i > 0) ? w.b2[i - 1].x2 : w.x0;
            CK(block_bwd(b2, enc, L.b2[i], grads, xin2, w.b2[i], 2, c.len_l, i == top ? w.G0 : w.G3, alt ? w.sc2b : scr2, w.G3, 0, s2, conc,
                         r2d.a, r2d.m, io->det_acc, pairing ? &pr2.g : nullptr));
            CK(wgpair_block_done(pr2, pairing, i == 0, L.b2[i].n1w, L.b2[i].end, conc, s2, em));
            if (i == 0 && forked) {                 // the spatial stack's last step accumulates onto the spectral dX
                CK((int)hipEventRecord(sd.join, sd.s));
                CK((int)hipStreamWaitEvent(s, sd.join, 0));
            }
            BlkP b1 = resolve(L.b1[i], c.W.b1[i], P, io->wpk, c.W, g.h);
            const float* xin1 = (i > 0) ? w.b1[i - 1].x2 : w.x0;
            float* out = (i == 0) ? w.G3 : w.G2;
            CK(block_bwd(b1, enc, L.b1[i], grads, xin1, w.b1[i], 1, c.len_l, i == top ? w.G0 : w.G2, alt ? w.scb : w.sc, out, i == 0, s, conc,
                         r1.a, r1.m, io->det_acc, pairing ? &pr1.g : nullptr));
            CK(wgpair_block_done(pr1, pairing, i == 0, L.b1[i].n1w, L.b1[i].end, conc, s, em));
        }
        if (!per_block) {     // back-to-front, all complete on the caller's stream by now
            for (int i = g.sdepth - 1; i >= 0; --i) CK(emit(L.b2[i].n1w, L.b2[i].end, s));
            for (int i = g.sdepth - 1; i >= 0; --i) CK(emit(L.b1[i].n1w, L.b1[i].end, s));
        }
        dx = w.G3;
    }
    if (first.g.ntasks || first.nrange) CK(wgpair_flush(first, 1, s, &emit));      // (no fusion block took the caller's deposit)
    // patch_embed.proj: only the kept tokens carry gradient (Models.py:528); no input gradient
    CK(wgrad_one(dx, true, g.Dp, w.a_pe, 96, g.D, 72, c.Me, (g.D + 127) / 128, grads, L.pew, L.peb, io->det_acc, s));
    CK(emit(0, L.peb + g.D, s));
    return HSIMAE_OK;
}

// Backward of the decoder from dL/dpred (bf16 [Md][96] in w.dpred) down to dL/d(latent) in w.du [Me][D]
// (autograd of Models.py:573-601): decoder_pred / decoder_norm, the decoder blocks, the sequence assembly and
// decoder_embed (its weight gradient included).  Shared by hsimae_backward and hsimae_decode_backward.
// fold: decoder_embed's weight gradient becomes a task of that pending launch (same M as the encoder blocks; both operands are bf16
// and stay untouched to the end of the pass) instead of a launch of its own here.
static int decoder_backward(const Ctx& c, const hsimae_io* io, float* grads, hipStream_t s, Emitter& emit, uint32_t sc, WgPair* fold) {
    const Geo& g = c.g; const float* P = io->params; const Ws& w = c.w; const PLayout& L = c.L;
    const float* zlast = w.bd[g.ddepth - 1].x2;
    GemmParams p = gp();
    p.A = w.dpred; p.lda = 96; p.M = (int)c.Md; p.N = g.Ddp; p.K = 96; p.n_valid = g.Dd; p.W = io->wpk + c.W.dpT; p.out = w.du; p.ldo = g.Ddp;
    CK(hs_gemm(p, A_BF16, E_F32, s));
    CK(wgrad_one(w.dpred, false, 96, w.zn, g.Ddp, 72, g.Dd, c.Md, 1, grads, L.dpw, L.dpb, io->det_acc, s));
    LnBwdParams l; std::memset(&l, 0, sizeof(l));
    l.du = w.du; l.x = zlast; l.gamma = P + L.dnw; l.dres = nullptr; l.dx = w.G0; l.dgamma = grads + L.dnw; l.dbeta = grads + L.dnb;
    l.M = (int)c.Md; l.d = g.Dd; l.ld = g.Ddp; l.det_base = grads; l.det_acc = io->det_acc;
    CK(hs_ln_bwd(l, s));
    CK(emit(L.dnw, L.total, s));

    const DecPlan dec = plan_dec(c.g.Dd, c.g.Hd, c.g.hdec, c.g.TL, sc);
    const BlockPlan lay = dec_block_plan(c, sc);
    // one reduce launch for up to kDecReduceBlocks blocks, each with its own slab; their ranges are reported after it
    const bool once = dec.reduce_once && w.dec_slabs != nullptr;
    DecBlockGrads rg[kDecReduceBlocks]; float* rslab[kDecReduceBlocks]; int rblk[kDecReduceBlocks]; int nr = 0;
    for (int i = g.ddepth - 1; i >= 0; --i) {
        BlkP bp = resolve(L.bd[i], c.W.bd[i], P, io->wpk, c.W, g.hdec);
        const float* xin = (i == 0) ? w.yfull : w.bd[i - 1].x2;
        if (dec.fused && once) {
            DecBlockBwd d;
            d.x = xin; d.x1 = w.bd[i].x1; d.dy = w.G0; d.dx1_tmp = w.G1; d.dx = w.G0; d.o = w.bd[i].o; d.lse = w.bd[i].lse;
            d.nsamples = c.N; d.Ts = g.TL; d.slab = dec_slab(w.slab, w.dec_slabs, nr); d.defer_reduce = true;
            rg[nr] = dec_grads(grads, L.bd[i], HsDet{grads, reinterpret_cast<long long*>(io->det_acc)});
            rslab[nr] = d.slab; rblk[nr] = i;
            CK(hs_dec_block_bwd(bp, rg[nr], d, s));
            if (++nr == kDecReduceBlocks || i == 0) {
                CK(hs_dec_dw_reduce(rg, rslab, nr, c.N, g.hdec, s));
                for (int k = 0; k < nr; ++k) CK(emit(L.bd[rblk[k]].n1w, L.bd[rblk[k]].end, s));
                nr = 0;
            }
            continue;
        }
        if (dec.fused) {
            // MLP half then attention half, both persistent with the block's weight gradients held in registers
            // (measured equal to "row-tile kernel + wgrad operands through HBM" at d = 64, with 0.7 GB less traffic)
            // slab NULL: commit the in-register weight gradients with float atomics (rounds 1-2) instead of slab + reduce
            DecBlockBwd d;
            d.x = xin; d.x1 = w.bd[i].x1; d.dy = w.G0; d.dx1_tmp = w.G1; d.dx = w.G0; d.o = w.bd[i].o; d.lse = w.bd[i].lse;
            d.nsamples = c.N; d.Ts = g.TL; d.slab = dec.slab ? w.slab : nullptr;
            CK(hs_dec_block_bwd(bp, dec_grads(grads, L.bd[i], HsDet{grads, reinterpret_cast<long long*>(io->det_acc)}), d, s));
        } else {
            CK(block_bwd(bp, lay, L.bd[i], grads, xin, w.bd[i], 0, 9, w.G0, w.sc, w.G0, 0, s, 1, nullptr, nullptr, io->det_acc));
        }
        CK(emit(L.bd[i].n1w, L.bd[i].end, s));
    }
    // sequence assembly + decoder_embed
    AssembleParams as; std::memset(&as, 0, sizeof(as));
    as.N = c.N; as.K = c.K; as.TL = g.TL; as.Dd = g.Dd; as.ld = g.Ddp; as.ids_restore = io->ids_restore; as.dyfull = w.G0; as.dy = w.dyb;
    CK(hs_assemble_bwd(as, s));
    p = gp();
    p.A = w.dyb; p.lda = g.Ddp; p.M = (int)c.Me; p.N = g.Dp; p.K = g.Ddp; p.n_valid = g.D; p.W = io->wpk + c.W.deT; p.out = w.du; p.ldo = g.Dp;
    CK(hs_gemm(p, A_BF16, E_F32, s));
    if (fold) {
        WgradParams& q = fold->g;
        WgradTask& t = q.t[q.ntasks++];
        t.dO = w.dyb; t.dO_f32 = 0; t.ldo = g.Ddp; t.A = w.lat; t.lda = g.Dp; t.N = g.Dd; t.K = g.D;
        t.dW = grads + L.dew; t.ldw = g.D; t.db = grads + L.deb; t.dO_rowscale = nullptr;
        q.M = (int)c.Me; q.det_base = grads; q.det_acc = io->det_acc;
        return HSIMAE_OK;
    }
    return wgrad_one(w.dyb, false, g.Ddp, w.lat, g.Dp, g.Dd, g.D, c.Me, ((g.Dd + 127) / 128) * ((g.D + 127) / 128), grads, L.dew, L.deb,
                     io->det_acc, s);
}

// Backward of `norm` (Models.py:570 / 892): du [Me][Dp] -> d(x of the last encoder block) in w.G0
static int norm_backward(const Ctx& c, const hsimae_io* io, const float* du, float* grads, hipStream_t s) {
    const Geo& g = c.g; const Ws& w = c.w; const PLayout& L = c.L;
    LnBwdParams l; std::memset(&l, 0, sizeof(l));
    l.du = du; l.x = g.nfus ? w.bf[g.nfus - 1].x2 : (g.has_axis ? w.b2[g.sdepth - 1].x2 : w.x0);
    l.gamma = io->params + L.nw; l.dres = nullptr; l.dx = w.G0; l.dgamma = grads + L.nw; l.dbeta = grads + L.nb;
    l.M = (int)c.Me; l.d = g.D; l.ld = g.Dp; l.det_base = grads; l.det_acc = io->det_acc;
    return hs_ln_bwd(l, s);
}

// What the backward entry points share: the context, the schedule that the forward recorded for this arena (never the environment's
// word now), the zeroed fixed-point shadow sums of deterministic mode and the range reporter.  stacks: which of the forward's records
// the pass needs; have_args: the entry point's own required pointers are all there.
enum Stacks { ENCODER = 1, DECODER = 2 };
struct BwdPass { Ctx c; uint32_t sc_enc = 0, sc_dec = 0; hipStream_t s = nullptr; Emitter emit{}; };
static int begin_backward(BwdPass& b, const hsimae_config* cfg, const hsimae_io* io, int stacks, bool have_args, float* grads,
                          hsimae_bucket_cb cb, void* user, void* stream) {
    CK(make_ctx(cfg, io, b.c, true));
    if (!grads || !have_args || ((stacks & DECODER) && !io->ids_restore)) return HSIMAE_ENULL;
    CK(lookup_sched(io->workspace, b.c.w.bytes, (stacks & ENCODER) != 0, (stacks & DECODER) != 0, b.sc_enc, b.sc_dec));
    b.s = S(stream);
    if (io->det_acc) CK((int)hipMemsetAsync(io->det_acc, 0, (size_t)b.c.L.total * 8, b.s));
    b.emit = Emitter{cb, user, cb ? S(io->bucket_stream) : nullptr, 0, grads, io->det_acc};
    return HSIMAE_OK;
}

int hsimae_backward(const hsimae_config* cfg, const hsimae_io* io, float* grads, hsimae_bucket_cb cb, void* user,
                    void* stream) {
    BwdPass b; CK(begin_backward(b, cfg, io, ENCODER | DECODER, true, grads, cb, user, stream));
    const Ctx& c = b.c; const Geo& g = c.g; const PLayout& L = c.L;
    // where the fusion blocks pair their weight-gradient launches, the first of them takes decoder_embed's along
    WgPair first;
    const bool fold = g.nfus > 0 && enc_plan(c, b.sc_enc).wgrad_pair;
    CK(decoder_backward(c, io, grads, b.s, b.emit, b.sc_dec, fold ? &first : nullptr));
    CK(norm_backward(c, io, c.w.du, grads, b.s));
    if (fold) first.note(L.nw, L.deb + g.Dd);         // reported after that launch, still ahead of the fusion blocks' ranges
    else CK(b.emit(L.nw, L.deb + g.Dd, b.s));
    return encoder_backward(c, io, grads, b.s, b.emit, b.sc_enc, first);
}

int hsimae_decode_backward(const hsimae_config* cfg, const hsimae_io* io, const float* dpred, float* dlatent, float* grads,
                           hsimae_bucket_cb cb, void* user, void* stream) {
    BwdPass b; CK(begin_backward(b, cfg, io, DECODER, dpred && dlatent, grads, cb, user, stream));
    const Ctx& c = b.c; const Geo& g = c.g; const Ws& w = c.w; const PLayout& L = c.L; hipStream_t s = b.s;
    CK(hs_rows_pad_bf16(dpred, w.dpred, c.Md, 72, 96, s));
    CK(decoder_backward(c, io, grads, s, b.emit, b.sc_dec, nullptr));
    CK(b.emit(L.dew, L.deb + g.Dd, s));
    return (int)hipMemcpy2DAsync(dlatent, (size_t)g.D * 4, w.du, (size_t)g.Dp * 4, (size_t)g.D * 4, (size_t)c.Me, hipMemcpyDeviceToDevice, s);
}

int hsimae_encode_backward(const hsimae_config* cfg, const hsimae_io* io, const float* dlatent, float* grads,
                           hsimae_bucket_cb cb, void* user, void* stream) {
    BwdPass b; CK(begin_backward(b, cfg, io, ENCODER, dlatent != nullptr, grads, cb, user, stream));
    const Ctx& c = b.c; const Geo& g = c.g; const Ws& w = c.w; const PLayout& L = c.L; hipStream_t s = b.s;
    const float* dlat = dlatent;
    if (g.Dp != g.D) {          // rows stored wider than the model: the caller's [Me][D] gradient into a padded buffer
        CK((int)hipMemcpy2DAsync(w.du, (size_t)g.Dp * 4, dlatent, (size_t)g.D * 4, (size_t)g.D * 4, (size_t)c.Me, hipMemcpyDeviceToDevice, s));
        dlat = w.du;
    }
    CK(norm_backward(c, io, dlat, grads, s));
    CK(b.emit(L.nw, L.nb + g.D, s));
    WgPair first;
    return encoder_backward(c, io, grads, s, b.emit, b.sc_enc, first);
}

// ---------------------------------------------------------------------- per-kernel entry points
int hsimae_mask_from_noise(const hsimae_mask_params* p, void* stream) { return p ? hs_mask(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_patch_gather(const hsimae_patch_params* p, void* stream) { return p ? hs_patch_gather(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_gemm(const hsimae_gemm_params* p, int32_t a_kind, int32_t epilogue, void* stream) {
    return p ? hs_gemm(*p, a_kind, epilogue, S(stream)) : HSIMAE_ENULL;
}
int hsimae_gemm_tiled(const hsimae_gemm_params* p, int32_t a_kind, int32_t epilogue, int32_t bm, int32_t kc, void* stream) {
    return p ? hs_gemm_tiled(*p, a_kind, epilogue, bm, kc, S(stream)) : HSIMAE_ENULL;
}
int hsimae_pack_matrix(const hsimae_pack_desc* d, int32_t n, int32_t max_elems, void* stream) {
    return d ? hs_pack(d, n, max_elems, S(stream)) : HSIMAE_ENULL;
}
int hsimae_enc_mlp_fwd(const float* x1, const float* res2, float* x2, int32_t M, int32_t d, const hsimae_mlp_weights* w,
                       const float* rowscale, void* stream) {
    if (M <= 0) return HSIMAE_OK;
    if (!x1 || !x2 || !w) return HSIMAE_ENULL;
    if (!mlp_fusable(d, w->hidden)) return HSIMAE_EUNSUPPORTED;
    return hs_enc_mlp_fwd(x1, res2, x2, M, d, block_w(*w), S(stream), rowscale);
}
int hsimae_enc_mlp_bwd(const float* x1, const float* dy, float* dx1, hs_bf16* u2, hs_bf16* dh13, hs_bf16* g, hs_bf16* dyb,
                       hs_bf16* dx1b, int32_t M, int32_t d, const hsimae_mlp_weights* w, float* g_n2w, float* g_n2b,
                       const float* rs_mlp, const float* rs_attn, int32_t plane_rows, void* stream) {
    if (plane_rows && plane_rows < M) return HSIMAE_EDIMS;
    if (M <= 0) return HSIMAE_OK;
    if (!x1 || !dy || !dx1 || !w || !g_n2w || !g_n2b) return HSIMAE_ENULL;
    // operand outputs are optional as groups: {u2, dyb} and {dh13, g} (NULL = not written: the data path alone), dx1b on its own
    if ((!u2) != (!dyb) || (!dh13) != (!g)) return HSIMAE_ENULL;
    if (!mlp_fusable(d, w->hidden)) return HSIMAE_EUNSUPPORTED;
    EncMlpBwd m;
    m.x1 = x1; m.dy = dy; m.dx1 = dx1; m.u2 = u2; m.dh13 = dh13; m.g = g; m.dyb = dyb; m.dx1b = dx1b; m.g_n2w = g_n2w; m.g_n2b = g_n2b;
    m.rs_mlp = rs_mlp; m.rs_attn = rs_attn; m.det = HsDet{nullptr, nullptr}; m.M = M; m.d = d; m.plane_rows = plane_rows;
    return hs_enc_mlp_bwd(block_w(*w), m, S(stream));
}
int hsimae_dec_block_fwd(const hsimae_dec_block_weights* w, const float* x, float* x1, float* x2, hs_bf16* o, float* lse,
                         int32_t nsamples, int32_t Ts, int32_t split, void* stream) {
    if (nsamples <= 0) return HSIMAE_OK;
    if (!w || !x || !x1 || !x2 || !o || !lse) return HSIMAE_ENULL;
    if (!dec_fusable(kDecD, kDecHeads, w->hidden, Ts)) return HSIMAE_EUNSUPPORTED;
    const BlockW d = block_w(*w);
    if (split) {
        CK(hs_dec_attn_fwd(x, x1, o, lse, nsamples, Ts, d, S(stream)));
        return hs_enc_mlp_fwd(x1, nullptr, x2, nsamples * Ts, kDecD, d, S(stream));      // (d.w13T is NULL: forward only)
    }
    return hs_dec_block_fwd(x, x1, x2, o, lse, nsamples, Ts, d, S(stream));
}
int64_t hsimae_dec_block_slab_floats(void) { return kDecSlabFloats; }
int64_t hsimae_wgrad_slab_bytes(const hsimae_config* cfg, int32_t side_stream) { return wgrad_slab_bytes(cfg, side_stream); }
int hsimae_dec_block_bwd(const hsimae_dec_block_weights* w, const hsimae_dec_block_grads* g, const float* x, const float* x1,
                         const float* dy, float* dx1_tmp, float* dx, const hs_bf16* o, const float* lse, int32_t nsamples,
                         int32_t Ts, float* slab, void* stream) {
    if (nsamples <= 0) return HSIMAE_OK;
    if (!w || !g || !x || !x1 || !dy || !dx1_tmp || !dx || !o || !lse) return HSIMAE_ENULL;
    if (!dec_fusable(kDecD, kDecHeads, w->hidden, Ts)) return HSIMAE_EUNSUPPORTED;
    DecBlockBwd d;
    d.x = x; d.x1 = x1; d.dy = dy; d.dx1_tmp = dx1_tmp; d.dx = dx; d.o = o; d.lse = lse; d.nsamples = nsamples; d.Ts = Ts; d.slab = slab;
    // (DecBlockGrads is the ABI's gradient struct + the deterministic-commit pair: none through this entry point)
    return hs_dec_block_bwd(block_w(*w), DecBlockGrads{*g, HsDet{nullptr, nullptr}}, d, S(stream));
}
int hsimae_attn_fwd(const hsimae_attn_params* p, void* stream) { return p ? hs_attn_fwd(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_attn_bwd(const hsimae_attn_params* p, void* stream) { return p ? hs_attn_bwd(*p, S(stream)) : HSIMAE_ENULL; }
// The fused attention halves (attn.hip blk128_*, attn_wide.hip blk256_*), the kernels block_fwd / block_bwd launch at d = 128 / 256.
static int attn_block_check(const hsimae_attn_block_weights* w, int d, int heads, int Ts, int nsamples, int mode, int len_l,
                            std::initializer_list<const void*> rows) {
    if (!w || !w->n1w || !w->n1b || !w->bqkv || !w->pb || !w->qkv || !w->p || !w->qkvT || !w->pT) return HSIMAE_ENULL;
    if (!((d == kAttn128D && heads == kAttn128Heads) || (d == kAttn256D && heads == kAttn256Heads))) return HSIMAE_EUNSUPPORTED;
    if (mode < 0 || mode > 2) return HSIMAE_EUNSUPPORTED;
    if (Ts < 1 || (mode != 0 && len_l < 1)) return HSIMAE_EDIMS;
    if (Ts > kAttnMaxTs) return HSIMAE_EUNSUPPORTED;
    if (d == kAttn256D && !attn256_fusable(d, heads, Ts, nsamples)) return HSIMAE_EUNSUPPORTED;     // 32-bit offsets
    for (const void* r : rows) {
        if (!r) return HSIMAE_ENULL;
        if (reinterpret_cast<uintptr_t>(r) & 15) return HSIMAE_EALIGN;
    }
    return HSIMAE_OK;
}
int hsimae_attn_block_fwd(const hsimae_attn_block_weights* w, const float* x, hs_bf16* u, hs_bf16* qkv, hs_bf16* o, float* lse,
                          float* x1, const float* rowscale, int32_t d, int32_t heads, int32_t Ts, int32_t nsamples, int32_t mode,
                          int32_t len_l, void* stream) {
    if (nsamples < 0) return HSIMAE_EDIMS;
    if (nsamples == 0) return HSIMAE_OK;
    CK(attn_block_check(w, d, heads, Ts, nsamples, mode, len_l, {x, u, o, lse, x1}));
    if (qkv && (reinterpret_cast<uintptr_t>(qkv) & 15)) return HSIMAE_EALIGN;
    AttnBlockFwd f;
    f.x = x; f.u = u; f.qkv = qkv; f.o = o; f.lse = lse; f.x1 = x1; f.rowscale = rowscale;
    f.Ts = Ts; f.nsamples = nsamples; f.mode = mode; f.len_l = len_l;
    if (d == 128) return hs_attn_block_fwd(block_w(*w), f, S(stream));
    if (!qkv) return HSIMAE_EUNSUPPORTED;                // blk256_fwd always saves q|k|v (its backward reads them)
    return hs_attn_block256_fwd(block_w(*w), f, S(stream));
}
int hsimae_attn_block_bwd(const hsimae_attn_block_weights* w, const hs_bf16* qkv, const hs_bf16* u, const hs_bf16* o, const float* lse,
                          const hs_bf16* dx1b, const float* dx1, const float* x, hs_bf16* dqkv, float* dx, float* dgamma, float* dbeta,
                          int64_t* det_acc, int32_t accumulate, int32_t d, int32_t heads, int32_t Ts, int32_t nsamples, int32_t mode,
                          int32_t len_l, void* stream) {
    if (nsamples < 0) return HSIMAE_EDIMS;
    if (nsamples == 0) return HSIMAE_OK;
    CK(attn_block_check(w, d, heads, Ts, nsamples, mode, len_l, {u, o, lse, dx1b, dx1, x, dqkv, dx}));
    if (!dgamma || !dbeta) return HSIMAE_ENULL;
    if (qkv && (reinterpret_cast<uintptr_t>(qkv) & 15)) return HSIMAE_EALIGN;
    if (!qkv && d != 128) return HSIMAE_EUNSUPPORTED;    // recomputing q|k|v from u: blk128_bwd_kernel<RC> only
    if (det_acc && dbeta != dgamma + d) return HSIMAE_EDIMS;
    hipStream_t s = S(stream);
    // deterministic: the kernel commits dgamma | dbeta into det_acc[0, 2 d) (offsets from dgamma), converted and added below
    if (det_acc) CK((int)hipMemsetAsync(det_acc, 0, sizeof(int64_t) * 2 * d, s));
    AttnBlockBwd r;
    r.qkv = qkv; r.u = u; r.o = o; r.lse = lse; r.dx1b = dx1b; r.dx1 = dx1; r.x = x; r.dqkv = dqkv; r.dx = dx;
    r.dgamma = dgamma; r.dbeta = dbeta; r.det = HsDet{dgamma, reinterpret_cast<long long*>(det_acc)};
    r.Ts = Ts; r.nsamples = nsamples; r.mode = mode; r.len_l = len_l; r.accumulate = accumulate;
    CK(d == 128 ? hs_attn_block_bwd(block_w(*w), r, s) : hs_attn_block256_bwd(block_w(*w), r, s));
    return det_acc ? hs_det_convert(det_acc, dgamma, 2 * d, s) : HSIMAE_OK;
}
int hsimae_wgrad(const hsimae_wgrad_params* p, void* stream) { return p ? hs_wgrad(*p, S(stream)) : HSIMAE_ENULL; }
int32_t hsimae_wgrad_msplit(int32_t tiles, int64_t M) { return wgrad_msplit(tiles, M); }
int hsimae_agg_pool(const float* latent, float* pooled, int32_t N, int32_t T, int32_t L, int32_t D, void* stream) {
    if (N <= 0) return HSIMAE_OK;
    if (!latent || !pooled) return HSIMAE_ENULL;
    return hs_agg_pool(latent, pooled, N, T, L, D, S(stream));
}
int hsimae_head_bwd(const float* g, const float* pooled, const float* w, float* gw, float* gb, float* dlatent, int32_t N, int32_t C,
                    int32_t T, int32_t L, int32_t D, void* stream) {
    if (N <= 0) return HSIMAE_OK;
    if (!g || !pooled || !w || !gw || !gb || !dlatent) return HSIMAE_ENULL;
    return hs_head_bwd(g, pooled, w, gw, gb, dlatent, N, C, T, L, D, S(stream));
}
int hsimae_cube_gather(const hsimae_cube_params* p, void* stream) {
    if (!p) return HSIMAE_ENULL;
    if (p->N <= 0) return HSIMAE_OK;
    if (!p->scenes || !p->scene_off || !p->scene_w || !p->cut || !p->index || !p->out) return HSIMAE_ENULL;
    return hs_cube_gather(*p, S(stream));
}
int hsimae_scene_windows(const hsimae_scene_params* p, void* stream) {
    if (!p) return HSIMAE_ENULL;
    if (p->N < 0 || p->H <= 0 || p->W <= 0 || p->C <= 0) return HSIMAE_EDIMS;
    if (p->N == 0) return HSIMAE_OK;
    if (!p->scene || !p->out) return HSIMAE_ENULL;
    if (!p->pixels && (p->p0 < 0 || p->p0 + p->N > (int64_t)p->H * p->W)) return HSIMAE_EDIMS;
    return hs_scene_windows(*p, S(stream));
}
int hsimae_class_argmax(const hsimae_scene_params* p, const float* logits, int32_t ld, int32_t num_class, int32_t first, int64_t* map,
                        void* stream) {
    if (!p) return HSIMAE_ENULL;
    if (p->N < 0 || p->H <= 0 || p->W <= 0 || first < 0 || first >= num_class || num_class > 256 || ld < num_class) return HSIMAE_EDIMS;
    if (p->N == 0) return HSIMAE_OK;
    if (!logits || !map) return HSIMAE_ENULL;
    if (!p->pixels && (p->p0 < 0 || p->p0 + p->N > (int64_t)p->H * p->W)) return HSIMAE_EDIMS;
    return hs_class_argmax(*p, logits, ld, num_class, first, map, S(stream));
}
int hsimae_scene_batch(const hsimae_scene_batch_params* p, void* stream) {
    if (!p || !p->bad) return HSIMAE_ENULL;
    if (p->N < 0 || p->n_items < 0 || p->H <= 0 || p->W <= 0 || p->C <= 0) return HSIMAE_EDIMS;
    if (!p->labels != !p->y) return HSIMAE_ENULL;
    const auto misaligned = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (misaligned(p->scene, p->scene_f64 ? 8 : 4) || misaligned(p->items, 8) || misaligned(p->pixels, 8) || misaligned(p->labels, 8) ||
        misaligned(p->out, 4) || misaligned(p->y, 8) || misaligned(p->bad, 4))
        return HSIMAE_EALIGN;
    if (p->N == 0) return HSIMAE_OK;
    if (!p->scene || !p->items || !p->out) return HSIMAE_ENULL;
    return hs_scene_batch(*p, S(stream));
}
int64_t hsimae_gwpca_workspace_bytes(const hsimae_gwpca_params* p) { return p ? hs_gwpca_workspace_bytes(*p) : (int64_t)HSIMAE_ENULL; }
int hsimae_gwpca_fit(const hsimae_gwpca_params* p, void* workspace, void* stream) {
    return p ? hs_gwpca_fit(*p, workspace, S(stream)) : HSIMAE_ENULL;
}
int hsimae_gwpca_apply(const hsimae_gwpca_params* p, void* out, int32_t out_f64, void* stream) {
    return p ? hs_gwpca_apply(*p, out, out_f64, S(stream)) : HSIMAE_ENULL;
}
int64_t hsimae_cls_workspace_bytes(int32_t N) { return hs_cls_workspace_bytes(N); }
int hsimae_cls_loss(const hsimae_cls_params* p, void* stream) { return p ? hs_cls_loss(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_cls_grad_scale(const float* src, const float* scale, float* dst, int64_t n, void* stream) {
    return hs_cls_grad_scale(src, scale, dst, n, S(stream));
}
int hsimae_confusion(const int64_t* gt, const int64_t* pred, int64_t n, int32_t C, int64_t* cm, int32_t* bad, void* stream) {
    return hs_confusion(gt, pred, n, C, cm, bad, S(stream));
}
int hsimae_confusion_map(const int64_t* gt_map, const int64_t* mask_map, const int64_t* pred_map, int64_t* masked, int64_t n, int32_t C,
                         int64_t* cm, int32_t* bad, void* stream) {
    return hs_confusion_map(gt_map, mask_map, pred_map, masked, n, C, cm, bad, S(stream));
}
int hsimae_scores(const int64_t* cm, int32_t C, double* out, void* stream) { return hs_scores(cm, C, out, S(stream)); }
int hsimae_class_prob(const hsimae_class_prob_params* p, void* stream) { return p ? hs_class_prob(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_prob_filter(const hsimae_prob_filter_params* p, void* stream) { return p ? hs_prob_filter(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_slic(const hsimae_slic_params* p, void* stream) { return p ? hs_slic(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_segment_vote(const hsimae_segment_vote_params* p, void* stream) { return p ? hs_segment_vote(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_row_normalize(const hsimae_row_normalize_params* p, void* stream) { return p ? hs_row_normalize(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_knn_topk(const hsimae_knn_topk_params* p, void* stream) { return p ? hs_knn_topk(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_knn_vote(const hsimae_knn_vote_params* p, void* stream) { return p ? hs_knn_vote(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_kmeans_assign(const hsimae_kmeans_assign_params* p, void* stream) { return p ? hs_kmeans_assign(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_kmeans_update(const hsimae_kmeans_update_params* p, void* stream) { return p ? hs_kmeans_update(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_probe_prepare(const hsimae_probe_prepare_params* p, void* stream) { return p ? hs_probe_prepare(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_probe_step(const hsimae_probe_step_params* p, void* stream) { return p ? hs_probe_step(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_probe_logits(const hsimae_probe_logits_params* p, void* stream) { return p ? hs_probe_logits(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_probe_fold(const hsimae_probe_fold_params* p, void* stream) { return p ? hs_probe_fold(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_svm_gram(const hsimae_svm_gram_params* p, void* stream) { return p ? hs_svm_gram(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_svm_solve(const hsimae_svm_solve_params* p, void* stream) { return p ? hs_svm_solve(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_svm_pack(const hsimae_svm_pack_params* p, void* stream) { return p ? hs_svm_pack(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_svm_predict(const hsimae_svm_predict_params* p, void* stream) { return p ? hs_svm_predict(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_recon_accumulate(const hsimae_recon_accumulate_params* p, void* stream) { return p ? hs_recon_accumulate(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_recon_finish(const hsimae_recon_finish_params* p, void* stream) { return p ? hs_recon_finish(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_ln_bwd(const hsimae_lnbwd_params* p, void* stream) { return p ? hs_ln_bwd(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_ln_fwd(const float* x, const float* gamma, const float* beta, float* out, int32_t M, int32_t d, void* stream) {
    return (x && gamma && beta && out) ? hs_ln_fwd(x, gamma, beta, out, M, d, S(stream)) : HSIMAE_ENULL;
}
int hsimae_assemble_fwd(const hsimae_assemble_params* p, void* stream) { return p ? hs_assemble_fwd(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_assemble_bwd(const hsimae_assemble_params* p, void* stream) { return p ? hs_assemble_bwd(*p, S(stream)) : HSIMAE_ENULL; }
int hsimae_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !group) return HSIMAE_ENULL;
    return hs_adamw(params, grads, exp_avg, exp_avg_sq, group, n, lr, beta1, beta2, eps, weight_decay, step, S(stream));
}
int hsimae_grad_norm(const hsimae_grad_seg* segs, int32_t nseg, float max_norm, int32_t skip_nonfinite, int32_t step, float beta1,
                     float beta2, double* partials, hsimae_clip_ctl* ctl, void* stream) {
    return hs_grad_norm(segs, nseg, max_norm, skip_nonfinite, step, beta1, beta2, partials, ctl, S(stream));
}
int hsimae_adamw_step_ctl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group,
                          int32_t group_uniform, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                          const hsimae_clip_ctl* ctl, void* stream) {
    return hs_adamw_ctl(params, grads, exp_avg, exp_avg_sq, group, group_uniform, n, lr, beta1, beta2, eps, weight_decay, ctl, S(stream));
}
int hsimae_adamw_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group,
                             int32_t group_uniform, int64_t n, const hsimae_adamw_group* table, int32_t ngroups, float beta1,
                             float beta2, float eps, int32_t step, const hsimae_clip_ctl* ctl, void* stream) {
    return hs_adamw_groups(params, grads, exp_avg, exp_avg_sq, group, group_uniform, n, table, ngroups, beta1, beta2, eps, step, ctl,
                           S(stream));
}
int hsimae_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* group,
                     int32_t group_uniform, int64_t n, const hsimae_lamb_tensor* tensors, int32_t ntensors, int32_t nchunks,
                     const hsimae_adamw_group* table, int32_t ngroups, float beta1, float beta2, float eps, float trust_clip,
                     int32_t always_adapt, double* partials, float* ratios, int32_t* bad, const hsimae_clip_ctl* ctl, void* stream) {
    return hs_lamb_step(params, grads, exp_avg, exp_avg_sq, group, group_uniform, n, tensors, ntensors, nchunks, table, ngroups, beta1,
                        beta2, eps, trust_clip, always_adapt, partials, ratios, bad, ctl, S(stream));
}
int hsimae_ema_update(float* ema, const float* params, int64_t n, double decay, int32_t warmup, int32_t step,
                      const hsimae_clip_ctl* ctl, void* stream) {
    return hs_ema_update(ema, params, n, decay, warmup, step, ctl, S(stream));
}
int hsimae_ema_swap(float* a, float* b, int64_t n, void* stream) { return hs_ema_swap(a, b, n, S(stream)); }
int hsimae_loss_partials(int32_t N, int32_t T) { return hs_loss_partials(N, T); }
int hsimae_loss(const hsimae_loss_params* p, void* stream) { return p ? hs_loss(*p, S(stream)) : HSIMAE_ENULL; }

}  // extern "C"
