// Stand-alone program that prints what the schedule planner (plan.h plan_block / plan_dec / enc_linears_fp8) decides, for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan plan_sched_main.cpp -o plan_sched_asan
// (hsimae_amd.build.build_sched_probe).  Never part of the library; tests/test_sched_plan_cpu.py runs it and checks its output.
// stdin, one query per line; stdout, binary int32:
//   B d heads hidden Ts nsamples M fp8 sc0 count -> out[count][3], the plans of the schedule words sc0 .. sc0 + count - 1:
//       [0] attn_fwd | save_qkv << 2 | mlp_fused << 3 | gemm_fp8 << 4 | attn_bwd << 5 | proj_bwd_fused << 7 | ln1_bwd << 8 |
//           ln2_bwd << 10 | planar << 12 | wgrad_slab << 13 | (the shape fields echo the arguments) << 14
//       [1] plane_rows   [2] dp << 16 | hp
//   D Dd heads hidden TL sc0 count                -> out[count]: fused | split << 1 | slab << 2
//   F model_prec D sc                             -> out[1]: enc_linears_fp8
//   P                                             -> out[1]: HS_PLANE_PAD_ROWS
#include "plan.h"
#include <cstdio>
#include <vector>

using namespace hsplan;

int main() {
    char line[256];
    while (std::fgets(line, sizeof(line), stdin)) {
        std::vector<int32_t> out;
        long long d, heads, hidden, Ts, ns, M, fp8, sc0, count;
        if (std::sscanf(line, "B %lld %lld %lld %lld %lld %lld %lld %lld %lld", &d, &heads, &hidden, &Ts, &ns, &M, &fp8, &sc0, &count) == 9) {
            out.resize((size_t)count * 3);                     // exactly count rows: an overrun is a sanitizer report
            for (long long i = 0; i < count; ++i) {
                const BlockPlan p = plan_block((int)d, (int)heads, (int)hidden, (int)Ts, (int)ns, M, fp8 != 0, (uint32_t)(sc0 + i));
                const bool echo = p.d == d && p.heads == heads && p.h == hidden && p.Ts == Ts && p.nsamples == ns && p.M == M;
                out[i * 3] = p.attn_fwd | p.save_qkv << 2 | p.mlp_fused << 3 | p.gemm_fp8 << 4 | p.attn_bwd << 5 | p.proj_bwd_fused << 7 |
                             p.ln1_bwd << 8 | p.ln2_bwd << 10 | p.planar << 12 | p.wgrad_slab << 13 | echo << 14;
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
        } else if (line[0] == 'P') {
            out.push_back(HS_PLANE_PAD_ROWS);
        } else {
            std::fprintf(stderr, "bad query: %s", line);
            return 2;
        }
        if (std::fwrite(out.data(), sizeof(int32_t), out.size(), stdout) != out.size()) return 3;
    }
    return 0;
}
