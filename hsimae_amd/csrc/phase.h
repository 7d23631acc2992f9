// Per-phase cycle accounting of the instrumented kernels (scripts/phase_timing.py, phase_wide.py, phase_blk128_bwd.py).  Compiled
// only with -DHS_PHASE_TIMING, never in the shipped library: without it every macro below expands to nothing.
//   HS_PHASE_COUNTERS(array, reader, n)   at file scope: the unit's n device counters and the exported C function that copies them
//                                         out (and zeroes them when `reset`);
//   PH_DECL(n)                            in a kernel: start the clock, n per-thread accumulators;
//   PH(i)                                 add the cycles since the previous stamp to accumulator i;
//   PH_FLUSH(array, base, n, tid)         thread `tid` of every workgroup adds its n accumulators to array[base ..].
// PHS_*(set, ...) is the same family with a named stamp set, for a second clock inside one phase; its clock starts at PHS_START.
#pragma once
#ifdef HS_PHASE_TIMING
#define HS_PHASE_COUNTERS(array, reader, n) \
    __device__ unsigned long long array[n]; \
    extern "C" __attribute__((visibility("default"))) int reader(unsigned long long* out, int reset) { \
        int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(array), sizeof(unsigned long long) * (n)); \
        if (reset) { unsigned long long z[n] = {0}; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(array), z, sizeof(z)); } \
        return rc; \
    }
#define PHS_DECL(set, n) unsigned long long ph_t##set = 0, ph_acc##set[n] = {};
#define PHS_START(set) ph_t##set = __builtin_readcyclecounter();
#define PHS(set, i) { const unsigned long long ph_now = __builtin_readcyclecounter(); ph_acc##set[i] += ph_now - ph_t##set; ph_t##set = ph_now; }
#define PHS_FLUSH(set, array, base, n, tid) \
    if (threadIdx.x == (tid)) { for (int i = 0; i < (n); ++i) atomicAdd(&array[(base) + i], ph_acc##set[i]); }
#else
#define HS_PHASE_COUNTERS(array, reader, n)
#define PHS_DECL(set, n)
#define PHS_START(set)
#define PHS(set, i)
#define PHS_FLUSH(set, array, base, n, tid)
#endif
#define PH_DECL(n) PHS_DECL(0, n) PHS_START(0)
#define PH(i) PHS(0, i)
#define PH_FLUSH(array, base, n, tid) PHS_FLUSH(0, array, base, n, tid)
