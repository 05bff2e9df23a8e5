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
//
// The HAND-OVER exit (estep_quad.h quad_hand_over, QUAD_HANDOVER_*) is stamped in three parts:
//   0  entry -> second barrier passed (live ballot, the two barriers, pos[], live list, gamma)
//   1  -> tile stores issued AND landed (the stamp waits for vmcnt 0)
//   2  -> the rest (live count, iteration and status of the document)
// A document handed over leaves them at entries 6 .. 8 of its wavefronts' 16 gamma entries, its iteration count at 4 and
// the marker -1 at 5 (gamma is positive), and is marked FINISHED instead of handed over, so that the live-topic kernel
// leaves the row alone: a stamped build computes nothing useful for these documents.
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
#define QUAD_HANDOVER_BEGIN()                                                                   \
    long long ho_acc[3] = {0, 0, 0};                                                            \
    long long ho_prev = __builtin_amdgcn_s_memtime();                                           \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#define QUAD_HANDOVER_STAMP(j)                                                 \
    do {                                                                       \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");            \
        const long long now_ = __builtin_amdgcn_s_memtime();                   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
        ho_acc[j] = now_ - ho_prev;                                            \
        ho_prev = now_;                                                        \
    } while (0)
#define QUAD_HANDOVER_DUMP()                                                                    \
    do {                                                                                        \
        __syncthreads();                                                                        \
        if (lane == 0) {                                                                        \
            double* dbg = p.gamma + (size_t)doc * K + wave * 16;                                \
            dbg[4] = (double)it;                                                                \
            dbg[5] = -1.0;                                                                      \
            for (int j = 0; j < 3; ++j) dbg[6 + j] = (double)ho_acc[j];                         \
        }                                                                                       \
        if (tid == 0) p.status[doc] = 0;                                                        \
    } while (0)
