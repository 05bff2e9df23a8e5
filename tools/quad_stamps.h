// s_memtime stamps of the quad kernel's PROLOGUE (estep_quad.h QUAD_PROLOGUE_*; development builds only:
// tools/phase_stamps_quad.py compiles a COPY of the package with -DPYLDA_QUAD_STAMPS=1, the library never includes this
// file otherwise).  A stamp waits for everything the wavefront has in flight (vmcnt / lgkmcnt 0), so the sub-phases are
// what the hardware needs for them when nothing later overlaps them; their split is what counts.  Stamps:
//   0  kernel entry -> this lane's term ids landed
//   1  -> last row of the gather landed (register slots, LDS slots written)
//   2  -> first barrier passed (token total, sum alpha; not taken with packed launch slots: stays 0)
//   3  -> first t stored, last barrier in front of the loop passed
// Every wavefront leaves its ticks and its iteration count over the document's gamma row at the training fast-path exit
// (needs K >= 16 x wavefronts; run with compact = 0 and doc_values = 0 so that every document takes that exit).
#pragma once
#define QUAD_PROLOGUE_BEGIN()                                                                   \
    long long stamp_acc[4] = {0, 0, 0, 0};                                                      \
    long long stamp_prev = __builtin_amdgcn_s_memtime();                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define QUAD_PROLOGUE_STAMP(j)                                                 \
    do {                                                                       \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");            \
        const long long now_ = __builtin_amdgcn_s_memtime();                   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
        stamp_acc[j] = now_ - stamp_prev;                                      \
        stamp_prev = now_;                                                     \
    } while (0)
#define QUAD_PROLOGUE_DUMP()                                                                    \
    do {                                                                                        \
        __syncthreads();                                                                        \
        if (lane == 0) {                                                                        \
            double* dbg = p.gamma + (size_t)doc * K + wave * 16;                                \
            for (int j = 0; j < 4; ++j) dbg[j] = (double)stamp_acc[j];                          \
            dbg[4] = (double)it;                                                                \
        }                                                                                       \
    } while (0)
