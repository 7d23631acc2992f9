// Stand-alone program that prints what the planners of plan.h decide — the schedule of a pass (plan_block / plan_dec /
// enc_linears_fp8) and the launch rules of the GEMM and weight-gradient kernels (plan_gemm, HS_GEMM_INSTANCES, plan_wgrad) — for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan plan_sched_main.cpp -o plan_sched_asan
// (hsimae_amd.build.build_sched_probe).  Never part of the library; tests/test_sched_plan_cpu.py and tests/test_launch_plan_cpu.py
// run it and check its output.
// stdin, one query per line; stdout, binary int32:
//   B d heads hidden Ts nsamples M fp8 sc0 count -> out[count][3], the plans of the schedule words sc0 .. sc0 + count - 1:
//       [0] attn_fwd | save_qkv << 2 | mlp_fused << 3 | gemm_fp8 << 4 | attn_bwd << 5 | proj_bwd_fused << 7 | ln1_bwd << 8 |
//           ln2_bwd << 10 | planar << 12 | wgrad_slab << 13 | (the shape fields echo the arguments) << 14 | wgrad_pair << 15
//       [1] plane_rows   [2] dp << 16 | hp
//   D Dd heads hidden TL sc0 count                -> out[count]: fused | split << 1 | slab << 2
//   F model_prec D sc                             -> out[1]: enc_linears_fp8
//   S tiles M concurrent                          -> out[1]: wgrad_msplit, the row split api.hip passes for a launch of `tiles` 128-tiles
//   P                                             -> out[1]: HS_PLANE_PAD_ROWS
//   G akind epi prec bm kc N0 N1 K0 K1            -> out[(N1 - N0) / 16 + 1][(K1 - K0) / 32 + 1][5]: plan_gemm at N = N0, N0 + 16 .. N1 and
//                                                    K = K0, K0 + 32 .. K1: return code, kc, bm, f8, nch
//   I                                             -> out[1 + 6 n]: n, then the n tuples (akind, epi, kc, bm, f8, nch) of HS_GEMM_INSTANCES
//   W ntasks n {N K f32 ldo lda rs dpr apr} x n  nM {M} x nM  nS {msplit} x nS
//                                                 -> out[nM][nS][slab: no, yes][operands: aligned, 4 bytes off][5]: plan_wgrad's return
//       code, path, msplit, grid, reduce_grid for a launch that declares `ntasks` tasks and fills the first n (<= 16) of them: ldo / lda
//       0 = N / K rounded up to 8, rs = a row factor is given, dpr / apr = dO_plane_rows / A_plane_rows.  The pointers are made-up
//       addresses of the alignment asked for; nothing reads through them.
#include "plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hsplan;

int main() {
    char line[1024];
    while (std::fgets(line, sizeof(line), stdin)) {
        std::vector<int32_t> out;
        long long d, heads, hidden, Ts, ns, M, fp8, sc0, count;
        if (std::sscanf(line, "B %lld %lld %lld %lld %lld %lld %lld %lld %lld", &d, &heads, &hidden, &Ts, &ns, &M, &fp8, &sc0, &count) == 9) {
            out.resize((size_t)count * 3);                     // exactly count rows: an overrun is a sanitizer report
            for (long long i = 0; i < count; ++i) {
                const BlockPlan p = plan_block((int)d, (int)heads, (int)hidden, (int)Ts, (int)ns, M, fp8 != 0, (uint32_t)(sc0 + i));
                const bool echo = p.d == d && p.heads == heads && p.h == hidden && p.Ts == Ts && p.nsamples == ns && p.M == M;
                out[i * 3] = p.attn_fwd | p.save_qkv << 2 | p.mlp_fused << 3 | p.gemm_fp8 << 4 | p.attn_bwd << 5 | p.proj_bwd_fused << 7 |
                             p.ln1_bwd << 8 | p.ln2_bwd << 10 | p.planar << 12 | p.wgrad_slab << 13 | echo << 14 | p.wgrad_pair << 15;
                out[i * 3 + 1] = p.plane_rows;
                out[i * 3 + 2] = p.dp << 16 | p.hp;
            }
        } else if (std::sscanf(line, "D %lld %lld %lld %lld %lld %lld", &d, &heads, &hidden, &Ts, &sc0, &count) == 6) {
            out.resize((size_t)count);
            for (long long i = 0; i < count; ++i) {
                const DecPlan p = plan_dec((int)d, (int)heads, (int)hidden, (int)Ts, (uint32_t)(sc0 + i));
                out[i] = (int32_t)p.fused | (int32_t)p.split << 1 | (int32_t)p.slab << 2;
            }
        } else if (std::sscanf(line, "F %lld %lld %lld", &fp8, &d, &sc0) == 3) {
            out.push_back(enc_linears_fp8((int)fp8, (int)d, (uint32_t)sc0));
        } else if (long long tiles, conc; std::sscanf(line, "S %lld %lld %lld", &tiles, &M, &conc) == 3) {
            out.push_back(wgrad_msplit((int)tiles, M, (int)conc));
        } else if (line[0] == 'P') {
            out.push_back(HS_PLANE_PAD_ROWS);
        } else if (int akind, epi, prec, bm, kc, N0, N1, K0, K1;
                   std::sscanf(line, "G %d %d %d %d %d %d %d %d %d", &akind, &epi, &prec, &bm, &kc, &N0, &N1, &K0, &K1) == 9) {
            for (int N = N0; N <= N1; N += 16)
                for (int K = K0; K <= K1; K += 32) {
                    GemmInst g;
                    out.push_back(plan_gemm(akind, epi, prec, N, K, bm, kc, g));
                    out.insert(out.end(), {g.kc, g.bm, g.f8, g.nch});
                }
        } else if (line[0] == 'I') {
            out.push_back(0);
#define HS_PROBE_INST(AK, EPI, KC, BM, F8, NCH) out.insert(out.end(), {AK, EPI, KC, BM, F8, NCH});
            HS_GEMM_INSTANCES(HS_PROBE_INST)
#undef HS_PROBE_INST
            out[0] = (int32_t)(out.size() / 6);
        } else if (line[0] == 'W') {
            char* c = line + 1;
            auto next = [&c]() { return std::strtol(c, &c, 10); };
            hsimae_wgrad_params p;
            std::memset(&p, 0, sizeof(p));
            p.ntasks = (int32_t)next();
            const long n = next();
            if (n < 0 || n > 16) return 2;
            for (long i = 0; i < n; ++i) {
                hsimae_wgrad_task& t = p.t[i];
                t.N = (int32_t)next(); t.K = (int32_t)next(); t.dO_f32 = (int32_t)next();
                t.ldo = (int32_t)next(); t.lda = (int32_t)next();
                if (!t.ldo) t.ldo = rup(t.N, 8);
                if (!t.lda) t.lda = rup(t.K, 8);
                t.dO_rowscale = next() ? reinterpret_cast<const float*>(uintptr_t(0x7000000)) : nullptr;
                t.dO_plane_rows = (int32_t)next(); t.A_plane_rows = (int32_t)next();
            }
            std::vector<long> Ms(next()); for (long& m : Ms) m = next();
            std::vector<long> splits(next()); for (long& m : splits) m = next();
            for (long m : Ms)
                for (long ms : splits)
                    for (int slab = 0; slab < 2; ++slab)
                        for (int off = 0; off < 8; off += 4) {
                            p.M = (int32_t)m; p.msplit = (int32_t)ms;
                            p.slab = slab ? reinterpret_cast<float*>(uintptr_t(0x6000000)) : nullptr;
                            for (long i = 0; i < n; ++i) {
                                p.t[i].dO = reinterpret_cast<const void*>(uintptr_t(0x10000000 + 0x2000000 * i + off));
                                p.t[i].A = reinterpret_cast<const hs_bf16*>(uintptr_t(0x11000000 + 0x2000000 * i + off));
                            }
                            WgradPlan w;
                            out.push_back(plan_wgrad(p, w));
                            out.insert(out.end(), {(int32_t)w.path, w.msplit, w.grid, w.reduce_grid});
                        }
        } else {
            std::fprintf(stderr, "bad query: %s", line);
            return 2;
        }
        if (std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size()) return 3;
    }
    return 0;
}
