// Sizes and small parameter blocks that BOTH the kernels and the host-side planner need (the kernel headers define
// __global__ functions and can be included by one translation unit each; this header by all of them).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#elif !defined(__host__)        // the planner alone under g++ (host_plan.cpp, sanitizer build)
#define __host__
#define __device__
#endif
#include <stddef.h>
#include <stdint.h>

namespace pylda {

// ---- estep_generic.h: LDS carve (all offsets multiples of 16 bytes, G17) ----
struct GenericLds {
    size_t tile, t, lt, gam, r, lognrm, cts, ids, red, scratch, total;
};

__host__ __device__ inline GenericLds generic_lds_layout(int K, int n_cap, int tile_stride,
                                                          int nthreads, bool tile_global)
{
    auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    GenericLds L;
    size_t off = 0;
    L.tile = off;   off = a16(off + (tile_global ? 0 : (size_t)n_cap * tile_stride * 8));
    L.t = off;      off = a16(off + (size_t)K * 8);
    L.lt = off;     off = a16(off + (size_t)K * 8);
    L.gam = off;    off = a16(off + (size_t)K * 8);
    L.r = off;      off = a16(off + (size_t)n_cap * 8);
    L.lognrm = off; off = a16(off + (size_t)n_cap * 8);
    L.cts = off;    off = a16(off + (size_t)n_cap * 8);
    L.ids = off;    off = a16(off + (size_t)n_cap * 4);
    // cross-group partials of pass 2: G x K doubles, G = nthreads / KL <= nthreads / min(K', nthreads)
    int kl = 1;
    while (kl < K && kl < nthreads) kl <<= 1;
    int groups = nthreads / kl;
    L.red = off;    off = a16(off + (size_t)groups * K * 8);
    L.scratch = off; off = a16(off + (size_t)(nthreads / 64) * 8);
    L.total = off;
    return L;
}

// ---- estep_logspace.h ----
__host__ __device__ inline size_t logspace_lds_bytes(int K)
{
    // psi[K], gam[K], gacc[4][K], scratch[4]
    return (size_t)(6 * K + 4) * 8 + 64;
}
// What estep_logspace_kernel is launched with: a document's arrays, rounded up to 16 bytes, then the chunk's list of flagged
// documents (256 + 1 ints).  The ONE figure both the launch and the creation of a corpus go by: a K whose launch would not fit
// the LDS is refused there, not in every E-step.  48 K + 1124 bytes: with the margin below K <= 3325 of gfx950's 160 KiB.
// kLdsMargin: a dynamic-LDS request within 3 KiB of the CU's 160 KiB is refused by hipFuncSetAttribute (found with 540-term
// documents at K = 32 in a generic kernel, 162 608 bytes; the quad kernel's 160 512 are accepted) - the planner
// (host_plan.cpp) and the creation of a corpus keep every request that far below the limit.
constexpr size_t kLdsMargin = 3072;
constexpr int kLogspaceListDocs = 256;
__host__ __device__ inline size_t logspace_list_offset(int K) { return (logspace_lds_bytes(K) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t logspace_launch_lds_bytes(int K)
{
    return logspace_list_offset(K) + (size_t)(kLogspaceListDocs + 1) * sizeof(int32_t);
}

// ---- doc_terms.h: work_count_partial_kernel ----
constexpr int kWorkCountBlocks = 1024;        // at most this many workgroups (of 1024 documents per trip), one row of 8 sums each

// ---- estep_qfuse.h / estep_qfusek.h ----
#ifndef PYLDA_QF_SLOTS
#define PYLDA_QF_SLOTS 128
#endif
constexpr int kQfMaxSlots = PYLDA_QF_SLOTS;   // word slots per wavefront: documents up to 1024 distinct terms

// ---- estep_qgroup.h ----
constexpr int kQgMaxWords = 1024;           // distinct terms per document

// ---- estep_quad.h: word slots, and the packed launch slots of its classes (prepare_kernels.h quad_pack_kernel) ----
// A document's 16 word groups gg deal its terms to word slots s: term s * 16 + gg in the on-chip slots (s < wpr: registers
// and LDS rows), and in REVERSE group order in the streamed slots behind them (estep_quad.h, "streamed slots").
__host__ __device__ constexpr int quad_slot_term(int s, int gg, int wpr) { return s * 16 + (s < wpr ? gg : 15 - gg); }
// slot counts of a geometry code SWL * 1000000 + TL * 10000 + RWL * 100 + TWL: on chip, and with the streamed ones
__host__ __device__ constexpr int quad_wpr_of(int rn) { return rn % 10000 / 100 + rn % 100; }
__host__ __device__ constexpr int quad_wpg_of(int rn) { return quad_wpr_of(rn) + rn / 1000000; }
// Which classes get packed launch slots: table stride 256 (TL = 32), where a document owns its CU and every tick of the
// prologue is idle time of the whole CU.  At stride 128 (TL = 16) the CU's other document runs its loop meanwhile, and
// the <16, 10, 4, 0> hand-over kernel answers the second prologue with two tile rows spilled inside its loop
// (tests/test_kernel_resources.py holds the ceilings): those classes keep addressing through order / doc_ptr / term_id.
__host__ __device__ constexpr bool quad_packs_slots(int tl) { return tl == 32; }
__host__ __device__ constexpr int quad_tl_of(int rn) { return rn % 1000000 / 10000; }
// term ids a word group holds per launch slot in the packed array: its wpg slots, rounded up to whole 16-byte loads
__host__ __device__ constexpr int quad_ids_stride(int wpg) { return (wpg + 3) & ~3; }
// ... and where the ids of word group gg of a class's launch slot start in the class's part of that array (int32 units)
__host__ __device__ constexpr int64_t quad_ids_at(int64_t slot, int gg, int stride) { return (slot * 16 + gg) * stride; }
// Two compile-time predicates of the stride-256 quad kernels, each with a macro so that tools/ab_build.py can build a copy
// of the library without it for an A/B on the same sources (python tools/ab_build.py NAME -DPYLDA_QUAD_...=0; LABNOTES
// has the figures of both):
//   quad_prologue_at_once - the packed prologue issues ids, alpha and sum alpha in front of the record, requests the two
//     counts in front of the gather and stores them behind it, and requests ALL rows of the LDS slots before it stores the
//     first: one round trip to memory in front of the gather and one for the gather, where there were four and 1 + TWL;
//   quad_early_handoff - the hand-over to the live-topic kernel is decided at the BOTTOM of an inner iteration, where the
//     live count is read, instead of behind the first chunk of the next iteration's pass A (same iteration, same bits).
// Stride 128 keeps its code (two documents per CU hide a prologue; `<16,10,4,0>` sits at its scratch ceiling).
#ifndef PYLDA_QUAD_PROLOGUE_AT_ONCE
#define PYLDA_QUAD_PROLOGUE_AT_ONCE 1
#endif
#ifndef PYLDA_QUAD_EARLY_HANDOFF
#define PYLDA_QUAD_EARLY_HANDOFF 1
#endif
__host__ __device__ constexpr bool quad_prologue_at_once(int tl) { return PYLDA_QUAD_PROLOGUE_AT_ONCE && tl == 32; }
__host__ __device__ constexpr bool quad_early_handoff(int tl) { return PYLDA_QUAD_EARLY_HANDOFF && tl == 32; }
// A third one, of the hand-over exit (estep_quad.h quad_hand_over), with the same A/B macro:
//   quad_handover_pairs - the tile goes out in 16-byte stores.  At stride 256 the lanes i and i + 32 of a wavefront hold
//     the same topics of two ADJACENT terms (word groups 2 wave and 2 wave + 1: terms 16 s + 2 wave + {0, 1} of an
//     on-chip slot s), 16 contiguous bytes of a column of the tile.  Over a pair of slots (2 q, 2 q + 1) the half-waves
//     swap: the lower one ends up with both values of slot 2 q, the upper one with both of slot 2 q + 1, and every lane
//     stores 16 bytes where it stored 8 twice - half the store instructions, the same bytes at the same addresses.
//     The streamed slots (reverse group order, values from the table) keep their 8-byte stores.
#ifndef PYLDA_QUAD_HANDOVER_PAIRS
#define PYLDA_QUAD_HANDOVER_PAIRS 1
#endif
__host__ __device__ constexpr bool quad_handover_pairs(int tl) { return PYLDA_QUAD_HANDOVER_PAIRS && tl == 32; }
// What thread `tid` of a stride-256 document (512 threads: wavefront tid / 64, half-wave tid / 32 % 2) stores into EVERY
// live column of the tile for store index q, at N terms, wpr on-chip slots (even register count, so that a pair never
// straddles registers and LDS) and wpg slots in all:
//   q < (wpr + 1) / 2: the slot pair (2 q, 2 q + 1) - the lower half-wave stores slot 2 q, the upper one slot 2 q + 1
//     (nothing if wpr is odd and that slot does not exist), both from the EVEN term of the slot's two;
//   the wpg - wpr indices behind them: a streamed slot each, one term per lane as before.
// bytes: 16 (terms `term` and `term + 1`, both below N), 8 (`term` alone: the last term of a document of odd length - 16
// bytes there would reach into the next column and, in the last column, past the document's region) or 0 (nothing).
struct QuadPairStore {
    int term, bytes;
};
__host__ __device__ constexpr int quad_pair_stores(int wpr, int wpg) { return (wpr + 1) / 2 + (wpg - wpr); }
// the term a thread stores from in pair 0 (the even term of its wavefront's two in slot 0 or 1); pair q: 32 q further
__host__ __device__ constexpr int quad_pair_first_term(int tid) { return 16 * (tid / 32 % 2) + 2 * (tid / 64); }
// a slot pair, from that term (the kernel keeps it, and nothing per pair, in a register)
__host__ __device__ constexpr QuadPairStore quad_pair_store_from(int N, int wpr, int first, int q)
{
    const int left = N - (first + 32 * q);              // terms of the document from this one on
    return QuadPairStore{first + 32 * q, (2 * q + 1 >= wpr && first >= 16) || left <= 0 ? 0 : left >= 2 ? 16 : 8};
}
// the whole table, as tests/test_quad_handover_pairs_host.py walks it.  The kernel calls quad_pair_store_from for the pairs and
// takes `bytes` from it; the address it forms as (thread's first term) * 8 + 256 q in the store's offset field, which is
// `term` = first + 32 q by the line above.  For the streamed slots it keeps the expression it always had,
// quad_slot_term(s, gg, wpr) with gg = tid / 32 and n < N: the branch below restates exactly that, for the coverage count.
__host__ __device__ constexpr QuadPairStore quad_pair_store(int N, int wpr, int wpg, int tid, int q)
{
    const int pairs = (wpr + 1) / 2;
    if (q < pairs) return quad_pair_store_from(N, wpr, quad_pair_first_term(tid), q);
    const int s = wpr + (q - pairs);
    const int n = quad_slot_term(s, tid / 32, wpr);
    return QuadPairStore{n, s < wpg && n < N ? 8 : 0};
}
// ---- estep_compact.h: three compile-time predicates of the live-topic kernels, each with a macro for the same A/B
// (python tools/ab_build.py NAME -DPYLDA_LIVE_...=0; LABNOTES has the figures).  None of them changes a bit of a result:
//   live_stop_shortcut - the stop sum of an iteration is formed only when no single lane's |delta gamma| exceeds the
//     threshold on its own (a sum of non-negative terms is never below its largest term, in any order of summation);
//   live_guard_once - a normaliser outside the fp64 range is looked for once per document, on the running minimum the
//     exactness guard keeps anyway, instead of per slot and iteration;
//   live_raw_extremes - that minimum and the maximum of r are kept with one v_min_f64 / v_max_f64 per slot, without the
//     canonicalising instruction fmin / fmax put in front of each operand.
#ifndef PYLDA_LIVE_STOP_SHORTCUT
#define PYLDA_LIVE_STOP_SHORTCUT 1
#endif
#ifndef PYLDA_LIVE_GUARD_ONCE
#define PYLDA_LIVE_GUARD_ONCE 1
#endif
#ifndef PYLDA_LIVE_RAW_EXTREMES
#define PYLDA_LIVE_RAW_EXTREMES 1
#endif
__host__ __device__ constexpr bool live_stop_shortcut() { return PYLDA_LIVE_STOP_SHORTCUT != 0; }
__host__ __device__ constexpr bool live_guard_once() { return PYLDA_LIVE_GUARD_ONCE != 0; }
__host__ __device__ constexpr bool live_raw_extremes() { return PYLDA_LIVE_RAW_EXTREMES != 0; }
// What a workgroup of the quad kernel needs to know of its document, one aligned 32-byte load from its launch slot.
// ids[launch slot][gg][quad_ids_stride]: term id of word slot s of group gg (-1: beyond the document, or padding).
struct alignas(32) QuadSlot {
    int32_t doc, N;       // document, distinct terms
    int64_t lo;           // its first (term, count) pair
    double tokens;        // sum of its counts (an integer below 2^53: exact in any order of summation)
    int64_t pad;
};

// ---- mstep_kernels.h: parameters of alpha_newton_kernel (variational_bayes.py:277-324) ----
struct NewtonParams {
    int iterations;             // hyper_parameter_iteration (100)
    int maximum_decay;          // hyper_parameter_maximum_decay (10)
    double threshold;           // hyper_parameter_converge_threshold (1e-6)
    double decay_power[17];     // numpy.power(hyper_parameter_decay_factor, d), d = 0 .. maximum_decay (computed by the host's pow)
};

}  // namespace pylda
