// Host-side planning of the HSIMAE kernel library: model geometry, the flat parameter layout, the packed-weight layout and
// its descriptor table, the workspace carve, the schedule of a pass and the launch rules of the GEMM and weight-gradient kernels
// (plan_gemm, plan_wgrad).  Pure C++ (no HIP): api.hip, gemm.hip and wgrad.hip include it for the real library;
// csrc/plan_host.cpp builds the same code with g++ -fsanitize=address,undefined into libhsimae_plan_asan.so, which the CPU tests
// drive through the same C entry points (tests/test_plan_asan_cpu.py), and csrc/plan_sched_main.cpp into a stand-alone program
// that prints the planners' decisions (tests/test_sched_plan_cpu.py, tests/test_launch_plan_cpu.py).
#pragma once
#include "../../include/hsimae_hip.h"
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace hsplan {

typedef hsimae_pack_desc PackDesc;
constexpr int LOSS_ROWS_PER_WG = 32;       // rows per workgroup of the row-form loss kernel (elem.hip)
inline int loss_partials(int N, int T) {
    const int64_t M = (int64_t)N * T * 9;
    return (int)std::max<int64_t>((M + LOSS_ROWS_PER_WG - 1) / LOSS_ROWS_PER_WG, N);     // either kernel form of hs_loss
}

inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------ parameter layout (flat fp32, registration order)
struct BlkOff { int64_t n1w, n1b, qw, qb, kw, kb, vw, vb, pw, pb, n2w, n2b, w1w, w1b, w2w, w2b, w3w, w3b, end; };

struct Geo {
    int B, T, TL, D, H, hd, h, hp, Dd, Hd, hdd, hdec, hpd, depth, sdepth, nfus, ddepth, norm_pix, prec;
    // Storage widths: every activation row, packed image and GEMM K extent uses the width rounded up to 32 (one MFMA
    // k-step); the columns past the true width are exact zeros everywhere (zero weight rows / columns, LayerNorm and
    // attention confined to the true width, a zero-filled arena), so widths like 144 / 72 (Model_Finetuning.py:66-67) or
    // 64 / 48 (Model_Pretraining.py:57-58) run on the same kernels.  Dp == D for the multiples of 32.
    int Dp, Ddp;
    bool has_axis, has_fus;
};

inline int make_geo(const hsimae_config* c, Geo& g) {
    if (!c) return HSIMAE_ENULL;
    if (c->bands <= 0 || c->bands % 8) return HSIMAE_EDIMS;
    g.B = c->bands; g.T = c->bands / 8; g.TL = g.T * 9;
    g.D = c->embed_dim; g.H = c->num_heads; g.Dd = c->dec_dim; g.Hd = c->dec_heads;
    if (g.D <= 0 || g.Dd <= 0 || g.H <= 0 || g.Hd <= 0 || g.D % g.H || g.Dd % g.Hd) return HSIMAE_EDIMS;
    g.hd = g.D / g.H; g.hdd = g.Dd / g.Hd;
    g.h = c->hidden; g.hdec = c->dec_hidden; g.hp = rup(g.h, 32); g.hpd = rup(g.hdec, 32);
    g.depth = c->depth; g.sdepth = c->s_depth; g.ddepth = c->dec_depth;
    g.has_axis = g.sdepth > 0;
    g.has_fus = g.sdepth < 12;                     // Models.py:385 (hard-coded 12)
    g.nfus = g.has_fus ? std::max(0, g.depth - g.sdepth) : 0;
    g.norm_pix = c->norm_pix_loss;
    g.prec = c->precision;
    if (g.prec != HSIMAE_PREC_BF16 && g.prec != HSIMAE_PREC_FP8) return HSIMAE_EUNSUPPORTED;
    if (g.D % 8 || g.Dd % 8 || g.D > 512 || g.Dd > 512) return HSIMAE_EUNSUPPORTED;
    g.Dp = rup(g.D, 32); g.Ddp = rup(g.Dd, 32);
    if ((g.hd != 8 && g.hd != 16) || (g.hdd != 8 && g.hdd != 16)) return HSIMAE_EUNSUPPORTED;
    if (g.h <= 0 || g.hdec <= 0 || g.h % 4 || g.hdec % 4 || g.T > 64 || g.ddepth < 1) return HSIMAE_EUNSUPPORTED;
    return HSIMAE_OK;
}

struct PLayout {
    int64_t pos, mask_token, dpos, pew, peb, nw, nb, dew, deb, dnw, dnb, dpw, dpb, total;
    std::vector<BlkOff> b1, b2, bf, bd;
    std::vector<int64_t> offs, sizes;
};

inline void make_playout(const Geo& g, PLayout& L) {
    int64_t cur = 0;
    auto add = [&](int64_t n) { int64_t o = cur; L.offs.push_back(o); L.sizes.push_back(n); cur += n; return o; };
    auto blk = [&](int d, int h) {
        BlkOff b;
        b.n1w = add(d); b.n1b = add(d);
        b.qw = add((int64_t)d * d); b.qb = add(d);
        b.kw = add((int64_t)d * d); b.kb = add(d);
        b.vw = add((int64_t)d * d); b.vb = add(d);
        b.pw = add((int64_t)d * d); b.pb = add(d);
        b.n2w = add(d); b.n2b = add(d);
        b.w1w = add((int64_t)h * d); b.w1b = add(h);
        b.w2w = add((int64_t)d * h); b.w2b = add(d);
        b.w3w = add((int64_t)h * d); b.w3b = add(h);
        b.end = cur;
        return b;
    };
    L.pos = add((int64_t)g.TL * g.D);
    L.mask_token = add(g.Dd);
    L.dpos = add((int64_t)g.TL * g.Dd);
    L.pew = add((int64_t)g.D * 72);
    L.peb = add(g.D);
    if (g.has_axis) {
        for (int i = 0; i < g.sdepth; ++i) L.b1.push_back(blk(g.D, g.h));
        for (int i = 0; i < g.sdepth; ++i) L.b2.push_back(blk(g.D, g.h));
    }
    for (int i = 0; i < g.nfus; ++i) L.bf.push_back(blk(g.D, g.h));
    L.nw = add(g.D); L.nb = add(g.D);
    L.dew = add((int64_t)g.Dd * g.D); L.deb = add(g.Dd);
    for (int i = 0; i < g.ddepth; ++i) L.bd.push_back(blk(g.Dd, g.hdec));
    L.dnw = add(g.Dd); L.dnb = add(g.Dd);
    L.dpw = add((int64_t)72 * g.Dd); L.dpb = add(72);
    L.total = cur;
}

// ------------------------------------------------------------------ packed-weight layout (bf16 images + fp32 bias packs)
struct Img8 { int64_t w, s; };            // byte offsets of an e4m3 image and of its e8m0 scale image (fp8 region)
struct BlkW {
    int64_t qkv, p, w1, w3, w2, qkvT, pT, w13T, w2T; int64_t bqkv;   // element offsets (bf16) / float offsets
    Img8 qkv8, p8, w1_8, w3_8, w2_8, qkvT8, pT8, w13T8, w2T8;         // precision = FP8: encoder blocks only
};
struct WLayout {
    int64_t pe, de, deT, dp, dpT;
    std::vector<BlkW> b1, b2, bf, bd;
    int64_t bf16_elems;      // bf16 region size (elements), multiple of 8
    int64_t f32_elems;       // fp32 region (bias packs)
    int64_t fp8_bytes;       // e4m3 images + scale images of the encoder blocks (precision = FP8), after the fp32 region
    int64_t total_elems;     // in bf16 units
};

inline void make_wlayout(const Geo& g, WLayout& W) {
    int64_t cur = 0, fcur = 0, cur8 = 0;
    auto img = [&](int N, int K) { int64_t o = cur; cur += (int64_t)N * K; return o; };
    auto img8 = [&](int N, int K) {       // [ceil(N/16)][ceil(K/128)][64 lanes][32 B] + one scale dword per (n-tile, 512-chunk, lane)
        const int64_t nt = (N + 15) / 16, ks = (K + 127) / 128, kch = (ks + 3) / 4;
        Img8 o; o.w = cur8; cur8 += nt * ks * 64 * 32; o.s = cur8; cur8 += nt * kch * 64 * 4;
        return o;
    };
    auto blk = [&](int d, int hp, bool f8) {
        BlkW b; std::memset(&b, 0, sizeof(b));
        b.qkv = img(3 * d, d); b.p = img(d, d); b.w1 = img(hp, d); b.w3 = img(hp, d); b.w2 = img(d, hp);
        b.qkvT = img(d, 3 * d); b.pT = img(d, d); b.w13T = img(d, 2 * hp); b.w2T = img(hp, d);
        b.bqkv = fcur; fcur += 3 * d;
        if (f8) {
            b.qkv8 = img8(3 * d, d); b.p8 = img8(d, d); b.w1_8 = img8(hp, d); b.w3_8 = img8(hp, d); b.w2_8 = img8(d, hp);
            b.qkvT8 = img8(d, 3 * d); b.pT8 = img8(d, d); b.w13T8 = img8(d, 2 * hp); b.w2T8 = img8(hp, d);
        }
        return b;
    };
    const bool f8 = g.prec == HSIMAE_PREC_FP8;
    W.pe = img(g.Dp, 96);
    if (g.has_axis) {
        for (int i = 0; i < g.sdepth; ++i) W.b1.push_back(blk(g.Dp, g.hp, f8));
        for (int i = 0; i < g.sdepth; ++i) W.b2.push_back(blk(g.Dp, g.hp, f8));
    }
    for (int i = 0; i < g.nfus; ++i) W.bf.push_back(blk(g.Dp, g.hp, f8));
    W.de = img(g.Ddp, g.Dp); W.deT = img(g.Dp, g.Ddp);
    for (int i = 0; i < g.ddepth; ++i) W.bd.push_back(blk(g.Ddp, g.hpd, false));
    W.dp = img(80, g.Ddp); W.dpT = img(g.Ddp, 96);
    W.bf16_elems = (cur + 7) & ~7ll;
    W.f32_elems = (fcur + 3) & ~3ll;            // keeps the fp8 region 16-B aligned
    W.fp8_bytes = cur8;
    W.total_elems = W.bf16_elems + 2 * W.f32_elems + (cur8 + 1) / 2;
}

inline void pack_descs(const Geo& g, const PLayout& L, const WLayout& W, const float* P, hs_bf16* wpk,
                std::vector<PackDesc>& out) {
    float* fbase = reinterpret_cast<float*>(wpk + W.bf16_elems);
    unsigned char* base8 = reinterpret_cast<unsigned char*>(fbase + W.f32_elems);
    auto mat = [&](int64_t src, int rows, int cols, int tr, int n_off, int k_off, int K_img, int64_t dst) {
        PackDesc d; std::memset(&d, 0, sizeof(d));
        d.src = P + src; d.rows = rows; d.cols = cols; d.transpose = tr; d.n_off = n_off; d.k_off = k_off;
        d.KS = K_img / 32; d.dst = wpk + dst; out.push_back(d);
    };
    auto mat8 = [&](int64_t src, int rows, int cols, int tr, int n_off, int k_off, int K_img, const Img8& im) {
        PackDesc d; std::memset(&d, 0, sizeof(d));
        d.src = P + src; d.rows = rows; d.cols = cols; d.transpose = tr; d.n_off = n_off; d.k_off = k_off;
        d.KS = (K_img + 127) / 128; d.dst = reinterpret_cast<hs_bf16*>(base8 + im.w); d.fp8 = 1; d.scales = base8 + im.s;
        out.push_back(d);
    };
    auto fcopy = [&](int64_t src, int n, int64_t dst_f, int off) {
        PackDesc d; std::memset(&d, 0, sizeof(d));
        d.src = P + src; d.rows = 1; d.cols = n; d.transpose = 0; d.n_off = off; d.k_off = 0; d.KS = 0;
        d.dst = reinterpret_cast<hs_bf16*>(fbase + dst_f); out.push_back(d);
    };
    // d: true width of the block, dp: its storage width (K extents and the q | k | v placement use dp; the sources keep d)
    auto blk = [&](const BlkOff& b, const BlkW& w, int d, int dp, int h, int hp, bool f8) {
        mat(b.qw, d, d, 0, 0, 0, dp, w.qkv); mat(b.kw, d, d, 0, dp, 0, dp, w.qkv); mat(b.vw, d, d, 0, 2 * dp, 0, dp, w.qkv);
        mat(b.pw, d, d, 0, 0, 0, dp, w.p);
        mat(b.w1w, h, d, 0, 0, 0, dp, w.w1); mat(b.w3w, h, d, 0, 0, 0, dp, w.w3);
        mat(b.w2w, d, h, 0, 0, 0, hp, w.w2);
        // transposed images for the data gradients
        mat(b.qw, d, d, 1, 0, 0, 3 * dp, w.qkvT); mat(b.kw, d, d, 1, 0, dp, 3 * dp, w.qkvT); mat(b.vw, d, d, 1, 0, 2 * dp, 3 * dp, w.qkvT);
        mat(b.pw, d, d, 1, 0, 0, dp, w.pT);
        mat(b.w1w, h, d, 1, 0, 0, 2 * hp, w.w13T); mat(b.w3w, h, d, 1, 0, hp, 2 * hp, w.w13T);
        mat(b.w2w, d, h, 1, 0, 0, dp, w.w2T);
        fcopy(b.qb, d, w.bqkv, 0); fcopy(b.kb, d, w.bqkv, dp); fcopy(b.vb, d, w.bqkv, 2 * dp);
        if (f8) {                                     // the same images as MX e4m3 (encoder blocks, precision = FP8)
            mat8(b.qw, d, d, 0, 0, 0, dp, w.qkv8); mat8(b.kw, d, d, 0, dp, 0, dp, w.qkv8); mat8(b.vw, d, d, 0, 2 * dp, 0, dp, w.qkv8);
            mat8(b.pw, d, d, 0, 0, 0, dp, w.p8);
            mat8(b.w1w, h, d, 0, 0, 0, dp, w.w1_8); mat8(b.w3w, h, d, 0, 0, 0, dp, w.w3_8);
            mat8(b.w2w, d, h, 0, 0, 0, hp, w.w2_8);
            mat8(b.qw, d, d, 1, 0, 0, 3 * dp, w.qkvT8); mat8(b.kw, d, d, 1, 0, dp, 3 * dp, w.qkvT8); mat8(b.vw, d, d, 1, 0, 2 * dp, 3 * dp, w.qkvT8);
            mat8(b.pw, d, d, 1, 0, 0, dp, w.pT8);
            mat8(b.w1w, h, d, 1, 0, 0, 2 * hp, w.w13T8); mat8(b.w3w, h, d, 1, 0, hp, 2 * hp, w.w13T8);
            mat8(b.w2w, d, h, 1, 0, 0, dp, w.w2T8);
        }
    };
    mat(L.pew, g.D, 72, 0, 0, 0, 96, W.pe);
    const bool f8 = g.prec == HSIMAE_PREC_FP8;
    for (size_t i = 0; i < L.b1.size(); ++i) blk(L.b1[i], W.b1[i], g.D, g.Dp, g.h, g.hp, f8);
    for (size_t i = 0; i < L.b2.size(); ++i) blk(L.b2[i], W.b2[i], g.D, g.Dp, g.h, g.hp, f8);
    for (size_t i = 0; i < L.bf.size(); ++i) blk(L.bf[i], W.bf[i], g.D, g.Dp, g.h, g.hp, f8);
    mat(L.dew, g.Dd, g.D, 0, 0, 0, g.Dp, W.de); mat(L.dew, g.Dd, g.D, 1, 0, 0, g.Ddp, W.deT);
    for (size_t i = 0; i < L.bd.size(); ++i) blk(L.bd[i], W.bd[i], g.Dd, g.Ddp, g.hdec, g.hpd, false);
    mat(L.dpw, 72, g.Dd, 0, 0, 0, g.Ddp, W.dp); mat(L.dpw, 72, g.Dd, 1, 0, 0, 96, W.dpT);
}

// ------------------------------------------------------------------ workspace
// rows between the planes of a planar weight-gradient operand beyond M (round 5): with exactly M rows the planes of C2 start
// 27 x 2^19 bytes apart and the two streams of a dW tile's operand slice meet in the same HBM channels (wgrad_dma 118.8 -> 123.5 us)
#ifndef HS_PLANE_PAD_ROWS
#define HS_PLANE_PAD_ROWS 48
#endif
constexpr int kPlanePadRows = 64;          // what the arena reserves per plane (>= HS_PLANE_PAD_ROWS)
static_assert(HS_PLANE_PAD_ROWS <= kPlanePadRows && HS_PLANE_PAD_ROWS % 16 == 0,
              "a -DHS_PLANE_PAD_ROWS variant must stay inside the rows the arena reserves per plane (ADVICE r05)");
struct BlkBuf { hs_bf16* u; hs_bf16* qkv; float* lse; hs_bf16* o; float* x1; hs_bf16* u2; hs_bf16* h13; hs_bf16* g; float* x2; };

struct Scr { float* G1; float* du; hs_bf16* dh13; hs_bf16* dob; hs_bf16* dqkv; hs_bf16* g0b; hs_bf16* g1b; float* slab; };   // per-stream backward scratch (g0b/g1b: bf16 dY / dx1; slab: weight-gradient partials)

struct Ws {
    Scr sc, sc2;                      // sc2: encoder-sized second set for the side stream (spectral stack)
    // Second operand set of each stream for the paired weight-gradient launches (wgrad_pairable below): the launch of two encoder
    // blocks reads dqkv / g0b / g1b / dh13 of both, so consecutive blocks of a stack alternate between sc and scb (sc2 and sc2b).
    // G1 / du / dob / slab are shared with the first set: no weight-gradient task of the fused path reads them.
    Scr scb, sc2b;
    hs_bf16* a_pe; float* x0;
    std::vector<BlkBuf> b1, b2, bf, bd;
    hs_bf16* lat; float* y; float* yfull; hs_bf16* zn; float* pred; hs_bf16* dpred; float* partial;
    float *G0, *G1, *G2, *du; hs_bf16 *dh13, *dob, *dqkv, *dyb;
    float* G3;                        // the spectral stack's own dX: both axis stacks read d(x1 + x2) from G0, neither writes it
    float* dec_slabs;                 // one more slab per decoder block after the first (dec_slab below), NULL without the fused decoder
    float* slab;                      // weight-gradient partials of the persistent kernels: [workgroup][slot][thread] (slab_bytes())
    int64_t bytes;
};
// Weight-gradient slabs, sized from the geometry (every arena used to carry 2 x 64 MiB whatever ran in it):
//   * the 256 x 256-tile weight-gradient launch (wgrad.hip, all matrices >= 256 wide: Large / Huge): 256 workgroups x 256 KB,
//     one slab per stream — the caller's and, for the forked spectral stack, the side stream's;
//   * the fused decoder's backward: HSIMAE_DEC_BLOCK_SLAB_FLOATS (checked against fused_dec.hip's own constants there), caller's stream.
//   The caller's stream also runs the DECODER's weight-gradient launches when the decoder goes layer at a time (block_bwd with
//   w.sc): a decoder of width >= 256 takes the 256 x 256-tile path whatever the encoder's width is (embed_dim 128 +
//   decoder_embed_dim 256 wrote 247 x 256 KB into a 56.7 MB slab), so the caller's slab is sized from BOTH widths; the side
//   stream only ever runs encoder blocks.
constexpr int64_t kSlabBytes = 256ll * 256 * 256 * 4;
inline int64_t slab_bytes(const Geo& g, bool side_stream) {
    if (side_stream) return (g.has_axis && g.Dp >= 256) ? kSlabBytes : 0;
    const int64_t wg = std::max(g.Dp, g.Ddp) >= 256 ? kSlabBytes : 0;
    return std::max<int64_t>(wg, HSIMAE_DEC_BLOCK_SLAB_FLOATS * 4);
}

inline bool mlp_fusable(int d, int hidden);
inline bool dec_fusable(int d, int heads, int hidden, int Ts);
constexpr int kDecReduceBlocks = 8;        // decoder blocks one dec_dw_reduce launch takes (fused_dec.hip)
inline void carve(const Geo& g, int N, int K, char* base, Ws& w) {
    int64_t cur = 0;
    auto take = [&](int64_t bytes) { char* p = base ? base + cur : nullptr; cur += (bytes + 255) & ~255ll; return p; };
    const int64_t Me = (int64_t)N * K, Md = (int64_t)N * g.TL;
    // (g and dh1|dh3 are sized for the planar operand layout of round 5 — 64-column planes of M + kPlanePadRows rows,
    //  hsimae_wgrad_task — whose padded width is hp rounded up to 64)
    auto blk = [&](int64_t M, int d, int heads, int hp) {
        BlkBuf b;
        b.u = (hs_bf16*)take(M * d * 2); b.qkv = (hs_bf16*)take(M * 3 * d * 2); b.lse = (float*)take(M * heads * 4);
        b.o = (hs_bf16*)take(M * d * 2); b.x1 = (float*)take(M * d * 4); b.u2 = (hs_bf16*)take(M * d * 2);
        b.h13 = (hs_bf16*)take(M * 2 * hp * 2); b.g = (hs_bf16*)take((M + kPlanePadRows) * rup(hp, 64) * 2); b.x2 = (float*)take(M * d * 4);
        return b;
    };
    w.a_pe = (hs_bf16*)take(Me * 96 * 2);
    w.x0 = (float*)take(Me * g.Dp * 4);
    w.b1.clear(); w.b2.clear(); w.bf.clear(); w.bd.clear();
    if (g.has_axis) {
        for (int i = 0; i < g.sdepth; ++i) w.b1.push_back(blk(Me, g.Dp, g.H, g.hp));
        for (int i = 0; i < g.sdepth; ++i) w.b2.push_back(blk(Me, g.Dp, g.H, g.hp));
    }
    for (int i = 0; i < g.nfus; ++i) w.bf.push_back(blk(Me, g.Dp, g.H, g.hp));
    w.lat = (hs_bf16*)take(Me * g.Dp * 2);
    w.y = (float*)take(Me * g.Ddp * 4);
    w.yfull = (float*)take(Md * g.Ddp * 4);
    for (int i = 0; i < g.ddepth; ++i) w.bd.push_back(blk(Md, g.Ddp, g.Hd, g.hpd));
    w.zn = (hs_bf16*)take(Md * g.Ddp * 2);
    w.pred = (float*)take(Md * 72 * 4);
    w.dpred = (hs_bf16*)take(Md * 96 * 2);
    w.partial = (float*)take((int64_t)loss_partials(N, g.T) * 4);
    const int64_t gmax = std::max(Me * g.Dp, Md * g.Ddp);
    w.G0 = (float*)take(gmax * 4); w.G1 = (float*)take(gmax * 4); w.G2 = (float*)take(gmax * 4); w.du = (float*)take(gmax * 4);
    w.dh13 = (hs_bf16*)take(std::max((Me + kPlanePadRows) * 2 * rup(g.hp, 64), (Md + kPlanePadRows) * 2 * rup(g.hpd, 64)) * 2);
    w.dob = (hs_bf16*)take(gmax * 2);
    w.dqkv = (hs_bf16*)take(gmax * 3 * 2);
    w.dyb = (hs_bf16*)take(Me * g.Ddp * 2);
    w.sc.G1 = w.G1; w.sc.du = w.du; w.sc.dh13 = w.dh13; w.sc.dob = w.dob; w.sc.dqkv = w.dqkv;
    w.sc2.G1 = (float*)take(Me * g.Dp * 4); w.sc2.du = (float*)take(Me * g.Dp * 4);
    w.sc2.dh13 = (hs_bf16*)take((Me + kPlanePadRows) * 2 * rup(g.hp, 64) * 2); w.sc2.dob = (hs_bf16*)take(Me * g.Dp * 2);
    w.sc2.dqkv = (hs_bf16*)take(Me * g.Dp * 3 * 2);
    w.sc.g0b = (hs_bf16*)take(gmax * 2); w.sc.g1b = (hs_bf16*)take(gmax * 2);     // (also decoder rows on the layer-at-a-time path)
    w.sc2.g0b = (hs_bf16*)take(Me * g.Dp * 2); w.sc2.g1b = (hs_bf16*)take(Me * g.Dp * 2);
    w.slab = (float*)take(slab_bytes(g, false));
    w.sc.slab = w.slab;
    w.sc2.slab = slab_bytes(g, true) ? (float*)take(slab_bytes(g, true)) : nullptr;      // (NULL: that launch commits with atomics)
    // only the 128-tile fused path pairs its launches (plan_block: wgrad_pair), and only encoder blocks do
    w.scb = w.sc; w.sc2b = w.sc2;
    if (mlp_fusable(g.D, g.h) && g.Dp < 256) {
        auto second = [&](Scr& b) {
            b.dh13 = (hs_bf16*)take((Me + kPlanePadRows) * 2 * rup(g.hp, 64) * 2); b.dqkv = (hs_bf16*)take(Me * g.Dp * 3 * 2);
            b.g0b = (hs_bf16*)take(Me * g.Dp * 2); b.g1b = (hs_bf16*)take(Me * g.Dp * 2);
        };
        second(w.scb);
        if (g.has_axis) second(w.sc2b);
    }
    w.G3 = g.has_axis ? (float*)take(Me * g.Dp * 4) : nullptr;
    // the fused decoder backward: every block of a reduce launch keeps its partials until that launch (block i % 8: w.slab for 0)
    const int nslab = std::min(g.ddepth, kDecReduceBlocks);
    w.dec_slabs = (dec_fusable(g.Dd, g.Hd, g.hdec, g.TL) && nslab > 1) ? (float*)take((nslab - 1) * HSIMAE_DEC_BLOCK_SLAB_FLOATS * 4) : nullptr;
    w.bytes = cur;
}

inline int wgrad_msplit(int tiles, int64_t M, int concurrent = 1) {
    const int chunks = (int)((M + 63) / 64);
    // the kernel holds 2 workgroups per CU (196 registers: 64 accumulators + the prefetched next chunk): keep the
    // launch to one resident wave of workgroups
    const int budget = 512;
    // `concurrent` launches resident at once (the forked axis stacks) share the budget as long as each still gets whole
    // groups of 8 row slices: slice ms runs on XCD ms % 8, so fewer than 8 slices leave XCDs idle (D = 256: 52 tiles,
    // sharing made the step 13 % slower; D = 128: 13 tiles, 2 % faster).
    int ms = std::max(1, budget / std::max(1, concurrent) / std::max(1, tiles));
    if (ms < 8) ms = std::max(1, budget / std::max(1, tiles));
    if (ms >= 8) ms &= ~7;              // whole XCD groups (wgrad.hip places row slice ms on XCD ms % 8)
    return std::max(1, std::min(ms, chunks));
}

// ------------------------------------------------------------------ which gemm_kernel a call launches (gemm.hip)
// hs_gemm launches ONE gemm_kernel<AK, EPI, KC, BM, F8, NCH> per call.  plan_gemm() below picks (KC, BM, F8, NCH) from the A kind,
// the epilogue, the precision, N, K and the tile override of hsimae_gemm_tiled (0 = this rule); HS_GEMM_INSTANCES lists every
// tuple it can answer, and gemm.hip instantiates exactly that list.  csrc/plan_sched_main.cpp prints both without a GPU and
// tests/test_launch_plan_cpu.py holds them against each other and against the tables of the GPU tests (tests/gemm_ref.py).
//
// Tiling of the wide layers, from scripts/gemm_sweep.py at the Large / Huge shapes (profiles/r02_gemm_sweep.txt):
// 64-row panels (two to three workgroups per CU: one panel's staging / epilogue overlaps another's MFMA loop) win
// wherever the weight image is small enough that streaming it once per 64 rows instead of once per 128 costs less than
// the overlap gains: q|k|v at d = 256 235 -> 175 us, gate backward 461 -> 216 us; they lose at d = 512 when K is deep
// (w2 303 -> 355 us).  256-deep A chunks pay only together with 64-row panels (alone: 1.3-1.7x slower).
struct GemmInst { int kc, bm, f8, nch; };          // A chunk depth, rows per workgroup, MX e4m3 operands, accumulator sets (1 = n outer)

inline bool small_weights(int N, int K, bool dual) {
    const int64_t nk = (int64_t)N * K;
    if (K < 256) return false;
    if (dual) return nk <= 400 * 1024;
    return K <= 512 ? nk <= 800 * 1024 : nk <= 400 * 1024;
}

// (A kind, epilogue, precision) combinations that have a kernel at some shape.  The MX form has no position-embedding epilogue.
inline bool gemm_has_kernel(int akind, int epi, int prec) {
    if (prec == HSIMAE_PREC_FP8 && epi == HSIMAE_E_POS_F32) return false;
    switch (akind) {
    case HSIMAE_A_F32_LN: return epi == HSIMAE_E_BF16 || epi == HSIMAE_E_SWIGLU || epi == HSIMAE_E_F32;
    case HSIMAE_A_BF16: return epi == HSIMAE_E_RES_F32 || epi == HSIMAE_E_POS_F32 || epi == HSIMAE_E_F32 || epi == HSIMAE_E_BF16 || epi == HSIMAE_E_LN_BWD;
    case HSIMAE_A_F32: return epi == HSIMAE_E_SWIGLU_BWD || epi == HSIMAE_E_BF16 || epi == HSIMAE_E_F32;
    }
    return false;
}

// HSIMAE_OK and the instantiation, or the refusal the shape alone decides (HSIMAE_EUNSUPPORTED; `out` is then all zeros).  What
// depends on the other members of the parameter block — strides, pointers — stays with hs_gemm.  force_bm: 0 / 64 / 128,
// force_kc: 0 / 128 / 256 (hsimae_gemm_tiled, tile sweeps); the LayerNorm-backward epilogue has one tile shape per N and ignores both.
inline int plan_gemm(int akind, int epi, int prec, int N, int K, int force_bm, int force_kc, GemmInst& out) {
    out = GemmInst{0, 0, 0, 0};
    if (!gemm_has_kernel(akind, epi, prec)) return HSIMAE_EUNSUPPORTED;
    const bool f8 = prec == HSIMAE_PREC_FP8, ln = akind == HSIMAE_A_F32_LN, dual = epi == HSIMAE_E_SWIGLU;
    if (epi == HSIMAE_E_LN_BWD) {
        // rows of one 128-column chunk: the one-chunk epilogue (bf16 only).  256- / 512-wide rows: k outer, all chunks' accumulators
        // live, bf16 or MX fp8 operands; four accumulator sets sit on 32-row panels (on 64-row panels they and the per-thread
        // dgamma / dbeta sums spilled 100 registers, and an LDS table for those sums with ds_add was 9 ms slower per Huge step than
        // the separate ln_bwd pass), and so do the register-prefetched A chunks of the fp8 form
        if (N == 128 && !f8) out = GemmInst{128, 128, 0, 1};
        else if (N == 256) out = f8 ? GemmInst{512, 32, 1, 2} : GemmInst{256, 64, 0, 2};
        else if (N == 512) out = f8 ? GemmInst{512, 32, 1, 4} : GemmInst{256, 32, 0, 4};
        else return HSIMAE_EUNSUPPORTED;
        return HSIMAE_OK;
    }
    if (ln && K > 512) return HSIMAE_EUNSUPPORTED;          // the LayerNorm prologue stages the whole row as one chunk
    const bool deep = !ln && !dual && N > 128 && N <= 512;  // at most 4 n-chunks, no prologue, no gate pair: k outer where K is deep
    if (f8) {
        // fp8 (MX) form: 512-deep e4m3 chunks.  64-row panels for every fp8 product: the e4m3 weight stream per panel is half the
        // bf16 one, and two to three resident workgroups hide the fragment fetches that one 128-row workgroup exposes (Huge step
        // 57.7 -> 55.6 ms; 128 rows everywhere: 76.8 ms, and a deeper fragment prefetch there does not help: 87.8 ms).
        // Deep K (several 512-chunks): k outer, every chunk quantised once; bf16 A chunks are prefetched into registers, and
        // 32-row panels keep them at 32 registers.
        if (deep && K > 512 && force_bm != 128) out = GemmInst{512, akind == HSIMAE_A_BF16 ? 32 : 64, 1, N <= 256 ? 2 : 4};
        else out = GemmInst{512, force_bm == 128 ? 128 : 64, 1, 1};
        return HSIMAE_OK;
    }
    const bool bm64 = force_bm ? force_bm == 64 : small_weights(N, K, dual);
    if (ln) out = GemmInst{K <= 128 ? 128 : K <= 256 ? 256 : 512, (K > 128 && bm64) ? 64 : 128, 0, 1};
    else if (deep && epi != HSIMAE_E_SWIGLU_BWD && !force_bm && K > 256) out = GemmInst{256, 64, 0, N <= 256 ? 2 : 4};
    else {
        const bool kc256 = force_kc ? force_kc == 256 : (bm64 && K >= 256 && K <= 1024);
        out = GemmInst{kc256 ? 256 : 128, bm64 ? 64 : 128, 0, 1};
    }
    return HSIMAE_OK;
}

// Every (AK, EPI, KC, BM, F8, NCH) plan_gemm can answer: 90.  gemm.hip expands the list into its launch switch, the only place
// that instantiates gemm_kernel; a tuple missing here is HSIMAE_EUNSUPPORTED at the launch, and the CPU test proves there is none.
#define HS_GI_LN(X, EPI)            /* LayerNorm prologue: the whole row is one chunk (KC from K); fp8: 512 */ \
    X(HSIMAE_A_F32_LN, EPI, 128, 128, 0, 1) X(HSIMAE_A_F32_LN, EPI, 256, 64, 0, 1) X(HSIMAE_A_F32_LN, EPI, 256, 128, 0, 1) \
    X(HSIMAE_A_F32_LN, EPI, 512, 64, 0, 1) X(HSIMAE_A_F32_LN, EPI, 512, 128, 0, 1) X(HSIMAE_A_F32_LN, EPI, 512, 64, 1, 1) \
    X(HSIMAE_A_F32_LN, EPI, 512, 128, 1, 1)
#define HS_GI_BF(X, AK, EPI)        /* bf16: k outer with 2 / 4 accumulator sets, else n outer, 128- / 256-deep chunks, 64 / 128 rows */ \
    X(AK, EPI, 256, 64, 0, 2) X(AK, EPI, 256, 64, 0, 4) X(AK, EPI, 256, 64, 0, 1) X(AK, EPI, 256, 128, 0, 1) \
    X(AK, EPI, 128, 64, 0, 1) X(AK, EPI, 128, 128, 0, 1)
#define HS_GI_F8(X, AK, EPI, KOBM)  /* fp8: k outer on KOBM-row panels, else n outer on 64 / 128 rows */ \
    X(AK, EPI, 512, KOBM, 1, 2) X(AK, EPI, 512, KOBM, 1, 4) X(AK, EPI, 512, 64, 1, 1) X(AK, EPI, 512, 128, 1, 1)
#define HS_GEMM_INSTANCES(X) \
    HS_GI_LN(X, HSIMAE_E_BF16) HS_GI_LN(X, HSIMAE_E_SWIGLU) HS_GI_LN(X, HSIMAE_E_F32) \
    HS_GI_BF(X, HSIMAE_A_BF16, HSIMAE_E_RES_F32) HS_GI_BF(X, HSIMAE_A_BF16, HSIMAE_E_POS_F32) HS_GI_BF(X, HSIMAE_A_BF16, HSIMAE_E_F32) \
    HS_GI_BF(X, HSIMAE_A_BF16, HSIMAE_E_BF16) HS_GI_BF(X, HSIMAE_A_F32, HSIMAE_E_BF16) HS_GI_BF(X, HSIMAE_A_F32, HSIMAE_E_F32) \
    X(HSIMAE_A_F32, HSIMAE_E_SWIGLU_BWD, 128, 64, 0, 1) X(HSIMAE_A_F32, HSIMAE_E_SWIGLU_BWD, 128, 128, 0, 1) \
    X(HSIMAE_A_F32, HSIMAE_E_SWIGLU_BWD, 256, 64, 0, 1) X(HSIMAE_A_F32, HSIMAE_E_SWIGLU_BWD, 256, 128, 0, 1) \
    HS_GI_F8(X, HSIMAE_A_BF16, HSIMAE_E_RES_F32, 32) HS_GI_F8(X, HSIMAE_A_BF16, HSIMAE_E_F32, 32) HS_GI_F8(X, HSIMAE_A_BF16, HSIMAE_E_BF16, 32) \
    HS_GI_F8(X, HSIMAE_A_F32, HSIMAE_E_SWIGLU_BWD, 64) HS_GI_F8(X, HSIMAE_A_F32, HSIMAE_E_BF16, 64) HS_GI_F8(X, HSIMAE_A_F32, HSIMAE_E_F32, 64) \
    X(HSIMAE_A_BF16, HSIMAE_E_LN_BWD, 128, 128, 0, 1) X(HSIMAE_A_BF16, HSIMAE_E_LN_BWD, 256, 64, 0, 2) X(HSIMAE_A_BF16, HSIMAE_E_LN_BWD, 256, 32, 0, 4) \
    X(HSIMAE_A_BF16, HSIMAE_E_LN_BWD, 512, 32, 1, 2) X(HSIMAE_A_BF16, HSIMAE_E_LN_BWD, 512, 32, 1, 4)
#define HS_GI_ONE(AK, EPI, KC, BM, F8, NCH) +1
static_assert(0 HS_GEMM_INSTANCES(HS_GI_ONE) == 90, "HS_GEMM_INSTANCES: one more or fewer kernel is a decision (tests/gemm_ref.py TABLE)");
#undef HS_GI_ONE

// ------------------------------------------------------------------ which kernel a weight-gradient launch runs (wgrad.hip)
constexpr int kWgradDmaRows = 32;          // rows per LDS stage of the LDS-DMA kernels (one MFMA k-step); planar operands come in whole ones
// T x T dW tiles of a launch.  (constexpr: the kernels of wgrad.hip count their tiles with it too.)
constexpr int wg_tiles(const hsimae_wgrad_params& p, int T) {
    int tiles = 0;
    for (int i = 0; i < p.ntasks; ++i) tiles += ((p.t[i].N + T - 1) / T) * ((p.t[i].K + T - 1) / T);
    return tiles;
}

// WG_REG: wgrad_kernel, register-staged 128 x 128 tiles (fp32 dO, unaligned or >= 4 GB operands); WG_DMA6 / WG_DMA3:
// wgrad_dma_kernel<6 / 3, false>, 128 x 128 tiles fed by LDS-DMA; WG_BIG: wgrad_dma_kernel<4, true>, 256 x 256 tiles committed with
// float atomics; WG_BIG_SLAB: the same through the caller's slab + wgrad_slab_reduce_kernel.
enum WgradPath { WG_REG, WG_DMA6, WG_DMA3, WG_BIG, WG_BIG_SLAB };
struct WgradPlan {
    WgradPath path;
    int msplit;          // row slices the launch uses: p.msplit on 128-tiles, its own on 256-tiles
    int grid;            // workgroups of the main launch; 0: nothing to launch
    int reduce_grid;     // workgroups of the slab reduce launch (WG_BIG_SLAB), else 0
};

// Everything hs_wgrad decides before it launches: its refusals, in its order, then the path and the grids.  Pointers are looked at
// (NULL or not, 16-byte alignment), never through.
inline int plan_wgrad(const hsimae_wgrad_params& p, WgradPlan& out) {
    constexpr int DC = kWgradDmaRows;
    out = WgradPlan{WG_REG, 0, 0, 0};
    if (p.ntasks <= 0 || p.M <= 0) return HSIMAE_OK;
    if (p.ntasks > 16 || p.msplit < 1) return HSIMAE_EDIMS;
    bool any_planar = false;
    for (int i = 0; i < p.ntasks; ++i) {
        const hsimae_wgrad_task& t = p.t[i];
        if (t.ldo % 8 || t.lda % 8) return HSIMAE_EDIMS;
        // the row factor is applied where an fp32 dO is rounded to bf16 (load_rows); no kernel scales a bf16 dO
        if (t.dO_rowscale && !t.dO_f32) return HSIMAE_EUNSUPPORTED;
        // planar operands: padded width a multiple of 64, whole 32-row DMA chunks (a row past M would be the next plane's row 0)
        if (t.dO_plane_rows && (t.ldo % 64 || t.dO_f32 || p.M % DC || t.dO_plane_rows < p.M)) return HSIMAE_EDIMS;
        if (t.A_plane_rows && (t.lda % 64 || p.M % DC || t.A_plane_rows < p.M)) return HSIMAE_EDIMS;
        // 32-bit byte offsets: an edge tile's lanes address plane index (n0 + 255) / 64, i.e. up to 256 columns past ld, and rely on
        // the buffer bounds check to return zeros there — which holds only while that offset does not wrap
        if ((int64_t)std::max(t.dO_plane_rows, t.A_plane_rows) * (std::max(t.ldo, t.lda) + 256) * 2 >= (1ll << 32)) return HSIMAE_EDIMS;
        any_planar = any_planar || t.dO_plane_rows || t.A_plane_rows;
    }
    // all operands bf16 and addressable with 32-bit buffer offsets -> LDS-DMA kernels; fp32 dO (the layer-at-a-time schedule) or larger
    // extents -> the register-staged wgrad_kernel.  (The switches that forced the older choice — HSIMAE_WGRAD_DMA, _WGRAD_BIG, _WGRAD_DS —
    // and the ring depths nobody ran went in round 6.)
    bool dma = true, big = true;
    for (int i = 0; i < p.ntasks; ++i) {
        const hsimae_wgrad_task& t = p.t[i];
        if (t.dO_f32 || (int64_t)(p.M + DC) * t.ldo * 2 >= (1ll << 32) || (int64_t)(p.M + DC) * t.lda * 2 >= (1ll << 32)) dma = false;
        if ((reinterpret_cast<uintptr_t>(t.dO) | reinterpret_cast<uintptr_t>(t.A)) & 15) dma = false;
        if (t.N < 256 || t.K < 256) big = false;            // wide layers only: a 256-tile of a 128-wide matrix is half padding
    }
    if (any_planar && !dma) return HSIMAE_EUNSUPPORTED;     // only the LDS-DMA kernels address planes
    if (dma && big) {
        // 256 x 256 tiles, one workgroup per CU: the row split that fills the chip once (p.msplit is sized for 128-tiles)
        const int t256 = wg_tiles(p, 256), nchunks = (p.M + DC - 1) / DC;
        constexpr int wgs = 256;
        out.msplit = std::max(1, std::min(wgs / std::max(1, t256), nchunks));
        const int total = t256 * out.msplit;
        out.grid = 8 * ((total + 7) / 8);
        // slab + reduce pays where many row slices meet in one tile (Large: 13 tiles x 19 slices, 264 -> 196 us of atomics out,
        // 35.70 -> 35.27 ms per step); with few slices per tile (Huge: 52 tiles x 4) the atomics are uncontended and the extra
        // 64 MB pass costs more than it saves (48.86 -> 49.06 ms): atomics there, whether a slab is given or not
        const bool slab = p.slab && !(total > 256 || out.msplit < 8);
        out.path = slab ? WG_BIG_SLAB : WG_BIG;
        out.reduce_grid = slab ? t256 * 128 : 0;
        return HSIMAE_OK;
    }
    const int tiles = wg_tiles(p, 128);
    out.msplit = p.msplit;
    out.grid = (p.msplit & 7) == 0 ? 8 * tiles * (p.msplit / 8) : 8 * ((tiles + 7) / 8) * p.msplit;      // wgrad.hip decode_wg
    // ring depth: a launch of at most one workgroup per CU has the LDS to itself (6 stages = 96 KB); larger launches keep 3
    // stages so that three workgroups fit a CU
    out.path = !dma ? WG_REG : out.grid > 256 ? WG_DMA3 : WG_DMA6;
    return HSIMAE_OK;
}

// ------------------------------------------------------------------ the schedule of a pass, decided ONCE, by its forward
// Every choice between two kernel generations that changes what the forward leaves in the workspace for the backward — fused
// or layer-at-a-time halves (which intermediates exist), q|k|v saved or recomputed, fp8 GEMMs or fused bf16 kernels — is read from
// the environment exactly once per pass: by the forward entry point (api.hip sched_from_env), which records the word for its
// workspace arena.  The backward entry points look the record up and follow it (HSIMAE_ENOFORWARD if there is none); they never
// read the environment, so a switch flipped between a forward and its backward has no effect on that pass.  What a word means
// for a stack of blocks is worked out in ONE place, plan_block() below, and both directions switch on its result (rounds 1-4
// re-derived each decision where it was needed: a forward that skipped the q|k|v store followed by a backward that decided not to
// recompute read an unwritten buffer and returned HSIMAE_OK — VERDICT r04 item 5).  Only this list names the switches.
enum : uint32_t {
    SC_FUSED_DEC = 1u << 0,        // HSIMAE_FUSED_DEC=0 clears: layer-at-a-time decoder
    SC_DEC_SPLIT = 1u << 1,        // HSIMAE_DEC_SPLIT=0 clears: one-kernel decoder block forward
    SC_FP8_UNFUSED = 1u << 2,      // HSIMAE_FP8_UNFUSED=1 sets: every linear of an fp8 encoder block on the MX GEMMs, no fused kernel
    SC_FUSED_MLP = 1u << 3,        // HSIMAE_FUSED_MLP=0 clears: layer-at-a-time MLP half of the encoder blocks
    SC_ATTN_BLOCK = 1u << 4,       // HSIMAE_FUSED_ATTN_BLOCK=0 clears: blk128_fwd
    SC_ATTN_BLOCK256 = 1u << 5,    // HSIMAE_FUSED_ATTN_BLOCK256=0 clears: blk256_fwd
    SC_ATTN_BLOCK_BWD = 1u << 6,   // HSIMAE_FUSED_ATTN_BLOCK_BWD=0 clears: blk128_bwd
    SC_PROJ_BWD = 1u << 7,         // HSIMAE_FUSED_PROJ_BWD=0 clears: the projection's data gradient as its own GEMM
    SC_LNBWD = 1u << 8,            // HSIMAE_FUSED_LNBWD=0 clears: du store + separate ln_bwd pass
    SC_LNBWD_512 = 1u << 9,        // HSIMAE_FUSED_LNBWD_512=0 clears it at d = 512 only
    SC_RECOMPUTE = 1u << 10,       // HSIMAE_ATTN_BWD_RECOMPUTE=0 clears: the forward saves q|k|v
    SC_WGRAD_SLAB = 1u << 11,      // HSIMAE_WGRAD_SLAB=0 clears: float atomics in the 256 x 256-tile weight-gradient launches
    SC_DEC_SLAB = 1u << 12,        // HSIMAE_DEC_SLAB=0 clears: float atomics in the fused decoder backward
    SC_PLANAR = 1u << 13,          // HSIMAE_WGRAD_PLANAR=0 clears: g / dh1|dh3 of the fused MLP backward row-major instead of 64-column planes
    SC_ATTN_BLOCK256_BWD = 1u << 14,   // HSIMAE_FUSED_ATTN_BLOCK256_BWD=0 clears: blk256_bwd (three launches instead)
    SC_WGRAD_PAIR = 1u << 15,      // HSIMAE_WGRAD_PAIR=0 clears: one weight-gradient launch per encoder block instead of one per two
    SC_DEC_REDUCE_ONCE = 1u << 16, // HSIMAE_DEC_REDUCE_ONCE=0 clears: one slab reduce per fused decoder block instead of one per 8
};

// Shapes the fused kernels are instantiated for.  Each kernel unit ties its template constants to these with static_assert and
// keeps its own refusals at launch; whether a pass USES a kernel is plan_block()'s / plan_dec()'s answer.
constexpr int kAttnTile = 16, kAttnMaxTs = 2 * kAttnTile;   // blk128_* / blk256_*: one or two 16-token tiles per sample
constexpr int kAttn128D = 128, kAttn128Heads = 8;           // attn.hip blk128_fwd / blk128_bwd: 8 heads of 16, unpadded rows
constexpr int kAttn256D = 256, kAttn256Heads = 16;          // attn_wide.hip blk256_fwd / blk256_bwd: 16 waves = 16 heads of 16
constexpr bool mlp_shape(int d, int hp) {                   // fused_enc.hip enc_mlp_*_kernel<D, HP>: (d, rup(hidden, 32))
    return (d == 128 && hp == 352) || (d == 256 && hp == 704) || (d == 64 && hp == 192);
}
constexpr int kDecD = 64, kDecHeads = 8, kDecHp = 192, kDecMinTs = 16, kDecMaxTs = 112;    // fused_dec.hip: up to 7 m-tiles of a sample in LDS
inline bool attn128_fusable(int d, int heads, int Ts) { return d == kAttn128D && heads == kAttn128Heads && Ts <= kAttnMaxTs; }
// (the kernels index q|k|v with 32-bit element offsets: a larger launch takes the layer-at-a-time kernels)
inline bool attn256_fusable(int d, int heads, int Ts, int nsamples) {
    return d == kAttn256D && heads == kAttn256Heads && Ts >= 1 && Ts <= kAttnMaxTs && (int64_t)nsamples * Ts * 3 * kAttn256D < (1ll << 31);
}
inline bool mlp_fusable(int d, int hidden) { return mlp_shape(d, rup(hidden, 32)); }   // (declared above carve())
inline bool dec_fusable(int d, int heads, int hidden, int Ts) {
    return d == kDecD && heads == kDecHeads && rup(hidden, 32) == kDecHp && hidden % 4 == 0 && Ts <= kDecMaxTs && Ts >= kDecMinTs;
}

// precision = FP8 puts the MX e4m3 images on the encoder linears that run as stand-alone GEMMs, where it pays: K >= 512.  At
// d = 256 the MX GEMMs are no faster than the bf16 ones (Large: 37.8 vs 37.2 ms per step, r03_k) and at d = 128 every linear sits
// inside a fused bf16 kernel; SC_FP8_UNFUSED forces them at every width (tests of the generic path).  The decoder's blocks never are.
inline bool enc_linears_fp8(int model_prec, int D, uint32_t sc) {
    return model_prec == HSIMAE_PREC_FP8 && (D >= 512 || (sc & SC_FP8_UNFUSED));
}

enum AttnFwd { ATTN_FWD_LAYERED, ATTN_FWD_BLK128, ATTN_FWD_BLK256 };
enum AttnBwd { ATTN_BWD_LAYERED, ATTN_BWD_BLK128, ATTN_BWD_BLK128_RECOMPUTE, ATTN_BWD_BLK256 };
enum LnBwd { LN_SEPARATE, LN_GEMM_EPILOGUE, LN_IN_KERNEL };     // du store + ln_bwd pass / epilogue of the du GEMM / inside a fused kernel
struct BlockPlan {
    int d, dp, heads, h, hp, Ts, nsamples; int64_t M;      // d: true width, dp / hp: storage widths (Geo::Dp), M rows of Ts-token samples
    AttnFwd attn_fwd;
    bool save_qkv;           // the forward stores q|k|v (false: attn_bwd recomputes them from u)
    bool mlp_fused;          // MLP half as enc_mlp_fwd / enc_mlp_bwd (both directions)
    bool gemm_fp8;           // the stand-alone linears on MX e4m3 images
    AttnBwd attn_bwd;
    bool proj_bwd_fused;     // the projection's data gradient inside the attention backward kernel: derived, attn_bwd != LAYERED
    LnBwd ln1_bwd, ln2_bwd;
    bool planar; int plane_rows;     // g / dh1|dh3 as 64-column planes of plane_rows rows (hsimae_wgrad_task), 0 = row-major
    bool wgrad_slab;         // the 256 x 256-tile weight-gradient launches commit through the stream's slab
    bool wgrad_pair;         // the weight gradients of two consecutive blocks of a stack as one launch (api.hip WgPair)
};

// fp8: enc_linears_fp8 for encoder stacks, false for the decoder.  Where a fused bf16 kernel covers the shape it is kept: it beats
// the layer-at-a-time fp8 form (round 2: Base 26.9 vs 19.4 ms, Large 44.1 vs 39.5 ms); SC_FP8_UNFUSED restores that all-fp8 schedule.
inline BlockPlan plan_block(int d, int heads, int hidden, int Ts, int nsamples, int64_t M, bool fp8, uint32_t sc) {
    BlockPlan p;
    p.d = d; p.dp = rup(d, 32); p.heads = heads; p.h = hidden; p.hp = rup(hidden, 32); p.Ts = Ts; p.nsamples = nsamples; p.M = M;
    auto on = [sc](uint32_t bits) { return (sc & bits) == bits; };
    const bool unpadded = p.dp == d;                     // the fused kernels have no pad columns
    const bool all_fp8 = fp8 && on(SC_FP8_UNFUSED);
    const bool a128 = !all_fp8 && attn128_fusable(d, heads, Ts), a256 = !fp8 && unpadded && attn256_fusable(d, heads, Ts, nsamples);
    p.gemm_fp8 = fp8;
    p.mlp_fused = !all_fp8 && on(SC_FUSED_MLP) && mlp_fusable(d, hidden);
    p.attn_fwd = (a128 && on(SC_ATTN_BLOCK)) ? ATTN_FWD_BLK128 : (a256 && on(SC_ATTN_BLOCK256)) ? ATTN_FWD_BLK256 : ATTN_FWD_LAYERED;
    // dO, the attention backward, du and the LayerNorm-1 backward as ONE persistent launch; its dx1 operand is the fused MLP
    // backward's bf16 copy.  With q|k|v recomputed from u when the forward ran blk128_fwd, which then does not store them.
    const bool b128 = a128 && p.mlp_fused && on(SC_ATTN_BLOCK_BWD | SC_PROJ_BWD | SC_LNBWD);
    const bool b256 = a256 && on(SC_ATTN_BLOCK256_BWD | SC_PROJ_BWD | SC_LNBWD);          // from the saved q|k|v
    p.attn_bwd = !b128 ? (b256 ? ATTN_BWD_BLK256 : ATTN_BWD_LAYERED)
                       : (p.attn_fwd == ATTN_FWD_BLK128 && on(SC_RECOMPUTE)) ? ATTN_BWD_BLK128_RECOMPUTE : ATTN_BWD_BLK128;
    p.save_qkv = p.attn_bwd != ATTN_BWD_BLK128_RECOMPUTE;
    p.proj_bwd_fused = p.attn_bwd != ATTN_BWD_LAYERED;
    // d = 256 / 512 (rows of exactly two / four 128-column chunks): LayerNorm backward as the epilogue of the k-outer GEMM
    // (gemm.hip epilogue_ln_ko; d = 512 on 32-row panels, fp8 only: Huge fp8 49.9 -> 48.9 ms per step, but bf16 60.2 -> 61.5);
    // at d = 128 LayerNorm-1's is the epilogue of the row-panel GEMM (du never goes to HBM)
    const bool wide_ln = on(SC_LNBWD) && unpadded && (d == 256 || (d == 512 && fp8 && on(SC_LNBWD_512)));
    p.ln1_bwd = p.proj_bwd_fused ? LN_IN_KERNEL : ((on(SC_LNBWD) && d == 128 && !all_fp8) || wide_ln) ? LN_GEMM_EPILOGUE : LN_SEPARATE;
    p.ln2_bwd = p.mlp_fused ? LN_IN_KERNEL : wide_ln ? LN_GEMM_EPILOGUE : LN_SEPARATE;
    // planes need whole 32-row DMA chunks and 32-bit byte offsets
    p.planar = p.mlp_fused && on(SC_PLANAR) && M % 32 == 0 && (M + kPlanePadRows) * 2 * (int64_t)(rup(p.hp, 64) + 256) * 2 < (1ll << 32);
    p.plane_rows = p.planar ? (int)M + HS_PLANE_PAD_ROWS : 0;
    p.wgrad_slab = on(SC_WGRAD_SLAB);
    // Every operand of the block's 7 tasks is then a bf16 buffer that lives until the next block but one of its stream (Ws::scb) or to
    // the end of the pass, and every matrix is narrower than 256: 128-tiles, 13 per block, so two blocks fit one launch of at most
    // 16 tasks whose grid wgrad_msplit keeps to the same workgroup count with half the row slices.
    p.wgrad_pair = on(SC_WGRAD_PAIR) && p.mlp_fused && p.attn_bwd != ATTN_BWD_LAYERED && p.attn_bwd != ATTN_BWD_BLK256 && p.dp < 256;
    return p;
}

// The decoder stack: fused Block kernels (fused_dec.hip), else layer at a time (plan_block of its own shape).  split: the fused
// forward as the attention half (q / k / v in registers, 16 waves per CU) + the row-panel MLP half enc_mlp_fwd_kernel<64, 192>
// (default since round 3) instead of the one-kernel form; slab: the fused backward commits its in-register weight gradients
// through the slab + one reduce launch instead of float atomics.
// reduce_once: the blocks' partials stay in a slab each (Ws::dec_slabs) and one reduce launch takes up to kDecReduceBlocks of them.
struct DecPlan { bool fused, split, slab, reduce_once; };
inline DecPlan plan_dec(int Dd, int heads, int hidden, int TL, uint32_t sc) {
    const bool fused = (sc & SC_FUSED_DEC) && dec_fusable(Dd, heads, hidden, TL), slab = (sc & SC_DEC_SLAB) != 0;
    return DecPlan{fused, (sc & SC_DEC_SPLIT) && mlp_fusable(Dd, hidden), slab, fused && slab && (sc & SC_DEC_REDUCE_ONCE)};
}
// slab of decoder block i of a pass (carve(): w.slab, then w.dec_slabs)
inline float* dec_slab(float* slab0, float* more, int i) {
    const int k = i % kDecReduceBlocks;
    return (k == 0 || !more) ? slab0 : more + (int64_t)(k - 1) * HSIMAE_DEC_BLOCK_SLAB_FLOATS;
}

// ------------------------------------------------------------------ bodies of the host-only C entry points
inline int param_layout(const hsimae_config* cfg, int64_t* offsets, int64_t* sizes, int max_entries) {
    Geo g; int e = make_geo(cfg, g); if (e) return e;
    PLayout L; make_playout(g, L);
    const int n = (int)L.offs.size();
    for (int i = 0; i < n && i < max_entries; ++i) {
        if (offsets) offsets[i] = L.offs[i];
        if (sizes) sizes[i] = L.sizes[i];
    }
    return n;
}
inline int64_t wpk_elems(const hsimae_config* cfg) {
    Geo g; if (make_geo(cfg, g)) return -1;
    WLayout W; make_wlayout(g, W);
    return W.total_elems;
}
inline int64_t pack_table_bytes(const hsimae_config* cfg) {
    Geo g; if (make_geo(cfg, g)) return -1;
    PLayout L; make_playout(g, L); WLayout W; make_wlayout(g, W);
    std::vector<PackDesc> d; pack_descs(g, L, W, nullptr, nullptr, d);
    return (int64_t)d.size() * sizeof(PackDesc);
}
inline int build_pack_table(const hsimae_config* cfg, const float* params_dev, hs_bf16* wpk_dev, void* table_host) {
    Geo g; int e = make_geo(cfg, g); if (e) return e;
    if (!params_dev || !wpk_dev || !table_host) return HSIMAE_ENULL;
    PLayout L; make_playout(g, L); WLayout W; make_wlayout(g, W);
    std::vector<PackDesc> d; pack_descs(g, L, W, params_dev, wpk_dev, d);
    std::memcpy(table_host, d.data(), d.size() * sizeof(PackDesc));
    return HSIMAE_OK;
}
inline int64_t wgrad_slab_bytes(const hsimae_config* cfg, int32_t side_stream) {
    Geo g; if (make_geo(cfg, g)) return -1;
    return slab_bytes(g, side_stream != 0);
}
inline int64_t workspace_bytes(const hsimae_config* cfg, int32_t N, int32_t len_t, int32_t len_l) {
    Geo g; if (make_geo(cfg, g)) return -1;
    if (N <= 0 || len_t < 1 || len_l < 1) return -1;
    Ws w; carve(g, N, len_t * len_l, nullptr, w);
    return w.bytes;
}

}  // namespace hsplan
