// Internal header of libpylda_hip.so: the context / corpus objects behind the opaque handles of include/pylda_hip.h
// and the host-side functions its translation units share.  Nothing here is part of the ABI.
//
//   context.hip        handles, options, model tables in and out, host memory, marks, RCCL glue, test hooks
//   host_plan.cpp      the planner: launch classes, segment cut, rounds, sweep dealing - pure host functions, no HIP
//   plan.hip           the planner's configuration from the context; pylda_corpus_plan / pylda_corpus_layout
//   launch_small.hip   document kernels, generic / slab / quilt families
//   launch_quad.hip    ... the register + LDS tile kernel (strides 128 / 256), handing documents to the live-topic kernel
//   launch_quad_dense.hip  ... the same without the hand-over (launch_quad.hip compiled again with the flag off)
//   launch_compact.hip ... the live-topic kernel behind them, its buffers, and whether alpha still lets topics die
//   launch_stream.hip  ... the fused streaming families (qfuse, qfusek, qgroup)
//   sstats_gather.hip  postings, segments and the statistics pass (dispatch-paced gather, persistent sweep)
//   estep_api.hip      corpus upload, pylda_estep as a driver over its stages (estep_plan ... estep_finish) and its read-backs
//   sampler_host.h     what the token samplers' launchers (the next five, and launch_completion.hip for the lane layout) share:
//                      the argument checks, the dispatch on the topics per lane, a corpus' token offsets and state words
//   launch_hybrid.hip  the hybrid (Gibbs-within-VB) E-step, its statistics pass and the Philox test hook
//   launch_gibbs.hip   the collapsed Gibbs engine: initial assignment, block-synchronous sweeps, log posterior, counts in and out
//   launch_foldin.hip  held-out fold-in against a frozen Gibbs model: the predictive table, the sampler, the likelihood
//   launch_cvb0.hip    the collapsed variational Bayes engine (CVB0): start, block-synchronous sweeps with an ordered apply pass, likelihood, fold-in
//                      ... and its stochastic (minibatch) form, SCVB0: start, steps with a deterministic blend (scvb_kernels.h)
//   launch_completion.hip  document-completion held-out likelihood: the predictive table of eta, the score of the held halves
//   launch_coherence.hip   topic coherence: the top words of every topic, the co-document counts of their pairs
//   launch_similarity.hip  nearest documents by topic mixture: the base, the fused score and top-N pass, the merge
//   launch_topic_distance.hip  topic distances between two models: the row transform, the tiled pair sums, the ordered combine
//   launch_left_to_right.hip  left-to-right held-out likelihood: a chain per (document, particle), the reduction
//   mstep_api.hip      device M-step, pack, alpha update, the outer iteration's one read-back
#pragma once
#include "../../include/pylda_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "comm.h"
#include "estep_common.h"
#include "estep_limits.h"
#include "host_plan.h"
#include "postings.h"

using namespace pylda;

namespace pylda_host __attribute__((visibility("hidden"))) {
using namespace pylda_plan;     // Variant, Launch, the planner (host_plan.h: HIP-free, sanitizer-tested)
}  // namespace pylda_host

using namespace pylda_host;

struct pylda_corpus;

struct pylda_ctx {
    int device = 0;
    int K = 0, V = 0;
    int ldk = 0;                    // row stride of the word-major tables
    hipStream_t own_stream = nullptr;
    // A corpus whose documents fall into several launch classes (different words-per-lane
    // instantiations) has independent launches: they are fanned out over these streams so a
    // small corpus pays one kernel latency (50 serial inner iterations), not one per class.
    // Only estep_api.hip picks them (the dense classes inside an AuxFork scope, the document-terms pass on
    // aux_stream[0]) and hands them to the launchers, which take the stream they launch on as a parameter.
    static constexpr int kAux = 4;
    hipStream_t aux_stream[kAux] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_event = nullptr;
    hipEvent_t join_event[kAux] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t stream = nullptr;
    size_t lds_limit = 64 * 1024;
    int num_cu = 256;

    double* d_eta = nullptr;        // K x V (numpy layout)
    double* d_elog = nullptr;       // V x ldk shifted E_log_eta
    double* d_expElog = nullptr;    // V x ldk
    double* d_expElog_elog = nullptr; // V x ldk
    double* d_shift = nullptr;      // V
    double* d_psi_rowsum = nullptr; // K
    double* d_topic_lse = nullptr;  // K
    double* d_alpha = nullptr;      // K
    double* d_alpha_wsum = nullptr; // sum_k alpha_k in the quad prologue's order of summation (alpha_wave_sum_kernel, per E-step)
    double* d_alpha_sgn = nullptr;  // K: alpha, sign bit set where the topic never counts as dead (alpha_mortality_kernel, per E-step)
    double* d_sstats = nullptr;     // V x ldk
    double* d_kv_scratch = nullptr; // K x V (export transposes)
    double* d_beta = nullptr;       // V
    double* d_small = nullptr;      // scalars + K-vectors scratch
    double* d_partial = nullptr;    // alpha-ss partials
    std::vector<double> h_beta;     // the beta last handed to pylda_mstep (its lgamma sums are cached)
    double beta_sum = 0.0, beta_lgamma_sum = 0.0;

    std::vector<double> h_alpha;
    // pinned host staging (one allocation, 5K + 8 doubles): two alpha slots (K each), the outer-iteration read-back (3K + 4),
    // the E-step's scalars (4)
    double* h_pin = nullptr;
    hipEvent_t alpha_event[2] = {nullptr, nullptr};
    bool alpha_event_used[2] = {false, false};
    int alpha_slot = 0;
    double* d_outer = nullptr;      // [doc ll, #documents, log-space documents, 0, alpha ss (K) | per-topic ll (K)]
    bool outer_ready = false;
    bool newton_pending = false;    // pylda_mstep_enqueue asked for the alpha update: pylda_outer_fetch runs it
    NewtonParams newton;
    double* d_newton_work = nullptr;   // 4 K
    double* d_eta_ckpt = nullptr;   // pylda_model_checkpoint
    double* d_work = nullptr;       // profiling, accumulated over E-steps: [sum_d I_d, sum_d I_d N_d, tile entries executed, documents handed
                                    // over, shader-clock ticks, constant-rate ticks of the same spans, live-topic iterations that skipped
                                    // the stop sum, ... that formed it]
    double work_cache[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // the last read of d_work (pylda_work_counters)
    hipEvent_t mark_event[4] = {nullptr, nullptr, nullptr, nullptr};
    void* comm = nullptr;           // RCCL communicator of pylda_comm_init (multi-GPU through the C ABI)
    int comm_world = 1;
    double* d_comm_small = nullptr; // staging buffer of pylda_allreduce_doubles
    double* d_foldin_table = nullptr;   // V x ldk: the predictive table of pylda_foldin_set_model (allocated by its first call)
    double* d_foldin_alpha = nullptr;   // K: the alpha of the last pylda_foldin
    bool foldin_ready = false;
    // document completion (launch_completion.hip): its table of eta lives in d_foldin_table - one of the two models at a time
    double* d_completion_rowsum = nullptr;  // K: sum_v eta[k][v]
    bool completion_ready = false;          // the table holds eta's posterior means (pylda_completion_set_model)
    // left-to-right held-out likelihood (launch_left_to_right.hip): the scratch of the last call, kept for the next one
    uint16_t* d_ltr_z = nullptr;            // ltr_capacity: the tokens' topics per particle
    double* d_ltr_p = nullptr;              // ltr_capacity: the tokens' predictive probabilities per particle
    size_t ltr_capacity = 0;                // (token, particle) cells both buffers hold
    int64_t ltr_chunk_tokens = 0;           // test hook: tokens per chunk of documents at most (0: what fits)
    const pylda_corpus* ltr_last_corpus = nullptr;  // what the buffers hold: the last call's corpus, particles and chunks
    int ltr_last_particles = 0, ltr_last_chunks = 0;
    size_t comm_small_cap = 0;
    bool have_eta = false, have_alpha = false, have_sstats = false;
    int force_logspace = 0;
    int force_variant = -1;
    int quilt12 = 0;
    int gather_rows = 2;            // 0: 64-topic chunks; 1: whole rows (ldk 64 / 128 / 256); 2: + postings in bulk (ldk 128 / 256)
    int gather_blocks = -1;         // document blocks of the gather: -1 automatic, 0 / 1 off, n forced (multiple of 8)
    int sweep_xcd = 1;              // the sweep's rendezvous per XCD (32 workgroups) instead of chip-wide (256)
    int sweep_sub = 4;              // sub-blocks a document block is walked in by the sweep (L2 working set 1 / sub of a block)
    int sweep_spin = 4000;          // polls of a rendezvous of the sweep before a workgroup goes on alone
    int gather_sweep = 1;           // the persistent sweep (sstats_sweep.h) at stride 128 / 256: 0 never, 1 when the partial rows of the
                                    // dispatch-paced gather would exceed their budget (rounds), 2 whenever the gather is blocked
    int gather_round_mb = 0;        // budget of the gather's partial rows per round, MiB (0: 4 GiB for the sweep-or-gather decision;
                                    // the rounds themselves are also capped by a quarter of the free device memory)
    int launch_order = 1;           // 0: launch classes in plan order (longest documents first), 1: fewest documents first (cfg 3: -0.5 %)
    int terms_overlap = 1;          // doc_terms_kernel on an auxiliary stream beside the dispatch-paced statistics gather
    int slab_uber = 1;              // small corpora: all slab launch classes in one dispatch
    int wide_postings = 0;          // test hook: 64-bit CSR positions in the postings whatever nnz (automatic from 2^31 pairs)
    int lds_pad = 0;                // A/B: extra dynamic LDS per quad workgroup (forces one workgroup per CU)
    int quad = 1;                   // register + LDS tile kernel (estep_quad.h) for table strides 128 / 256, N <= 208
    int quad_stream = 1;            // ... with streamed word slots for documents of 225-256 terms
    int prepare_path = 0;           // the tables of eta (enqueue_prepare): 0 by size, 1 the one-kernel path of K <= 64, 2 the two passes (same bits)
    int quad_packed = 1;            // ... addressing its documents through packed launch slots (0: through order / doc_ptr / term_id)
    int quilt_odd = 1;              // words-per-lane 6 / 7 instantiations (less padding for 129..224-term documents)
    int doc_values = 1;             // 1: per-document log-likelihoods complete (see EstepParams::want_doc_ll)
    int compact = 1;                // the dense quad kernel hands a document to the live-topic kernel (estep_compact.h) once few topics move
    int gather_live = 1;            // the statistics pass reads the documents' lists of live topics (sstats_live.h) where the corpus hands documents over
    int alpha_ss_moved = 1;         // the alpha statistics of the M-step take psi(alpha_k) from a table where gamma_dk == alpha_k bitwise (A/B switch)
    int compact_phase = 1;          // the live-topic kernels run behind ALL dense kernels of the E-step (0: behind their class, on its stream)
    int compact_stream = 1;         // ... and so do the fused streaming kernels (384 <= table stride <= 1024), without a tile
    int compact_pair = -1;          // hand over at twice one wavefront's columns (two-wavefront body): -1 from table stride 256 on, 0 never, 1 always
    int compact_cap = 0;            // test hook: hand over at this many live topics at most (0: what the class' register tile holds)
    int compact_guard_fail = 0;     // test hook: the live-topic kernel's exactness guard fails for every document
    int64_t compact_underflow_doc = -1;   // test hook: the hand-over tile of this document gets its LAST term scaled by 1e-288
    int64_t coherence_chunk_docs = 0;   // test hook: documents per chunk of pylda_codocument_counts' bitmaps (a multiple of 64; 0: what fits)
    int similarity_doc_slices = 0;      // test hook: document slices of pylda_similar_documents' launch (0: enough to fill the compute units)
    double* d_similarity_base = nullptr;    // similarity_D x K: the base of pylda_similarity_set_base, transformed
    int64_t similarity_D = 0;
    int topic_distance_segment_groups = 0;  // test hook: groups of segments of pylda_topic_distances' launch (0: by the number of tiles)
    int plan_epoch = 0;
    bool exact_stop = false;        // this E-step's threshold is outside the fixed-point stop test's range

    // profiling (pylda_set_profiling): HIP events on the launch streams
    struct Bracket { hipEvent_t a, b; int slot; };   // slot -1: document kernels, -2: statistics pass, >= 0: launch class
    bool profiling = false;
    std::vector<Bracket> pending_events;
    std::vector<hipEvent_t> event_pool;
    double doc_kernel_ms = 0.0, sstats_kernel_ms = 0.0;
    std::vector<double> class_ms;   // per launch class of the last profiled corpus
    int64_t estep_calls = 0;

    std::string err;
};

struct pylda_corpus {
    pylda_ctx* ctx = nullptr;
    int64_t D = 0, nnz = 0, tokens = 0;
    int32_t max_terms = 0;
    int64_t* d_doc_ptr = nullptr;
    int32_t* d_term_id = nullptr;
    int32_t* d_term_ct = nullptr;
    int32_t* d_order = nullptr;
    double* d_gamma = nullptr;
    double* d_doc_ll = nullptr;
    double* d_doc_wll = nullptr;
    int32_t* d_iters = nullptr;
    int32_t* d_status = nullptr;
    int32_t* d_flag_count = nullptr;   // documents the safety net redid in the last E-step over THIS corpus (in d_scalars[3])
    double* d_scalars = nullptr;   // [0] doc ll, [1] words ll, [2] corpus entropy term (fast path)
    double* d_entropy_partial = nullptr;
    bool last_doc_values = true;
    double* d_tfinal = nullptr;    // D x ldk
    double* d_rfinal = nullptr;    // nnz
    double* d_term_scratch = nullptr;   // nnz, only when a launch class needs it (kGenericHuge)
    // postings (CSC) of the corpus for the sufficient-statistics gather pass
    bool have_postings = false;
    int32_t* d_post_doc = nullptr; // nnz
    void* d_post_pos = nullptr;    // nnz: position in CSR order (int32, or int64 when wide_pos)
    bool wide_pos = false;         // nnz >= 2^31 (or option wide_postings): 64-bit CSR positions in the postings
    int64_t* d_seg_begin = nullptr;
    int64_t* d_seg_end = nullptr;
    int32_t* d_exec_order = nullptr;   // document-blocked gather: segment of every (workgroup, wavefront) slot, or -1
    int64_t exec_slots = 0;
    // The gather runs in ROUNDS over contiguous term ranges that share one set of partial rows (a (term, block)
    // pair costs a row: 45 GB at cfg 4 in one go - and a second for the allocation alone): gather round r, finalize
    // its terms, reuse the rows.  One round unless the rows would exceed the budget.
    using Round = pylda_plan::Round;
    std::vector<Round> rounds;
    int64_t partial_rows = 0, ent_blocks = 0;
    // ... or the persistent sweep (sstats_sweep.h): no partial rows at all
    bool sweep = false;
    int sweep_passes = 0, sweep_terms = 0, sweep_wpb = 0;   // passes over the document blocks, terms per wavefront, wavefronts per workgroup
    int32_t* d_seg_block = nullptr;             // document block of every segment
    int32_t* d_term_of = nullptr;               // [passes][wavefronts][terms per wavefront]
    unsigned* d_rendezvous = nullptr;
    int gather_blocks = 1;
    int gather_rows = 2;            // the context's option at the time the postings were built (it selects the gather kernel)
    int64_t* d_word_seg_ptr = nullptr;  // V+1
    double* d_partial = nullptr;   // nseg x ldk
    int64_t nseg = 0;
    std::vector<int32_t> h_terms_sorted;  // distinct-term counts in schedule order
    std::vector<int32_t> h_order;         // the schedule: document of every slot
    // hand-over to the live-topic kernel (launch_compact.hip): per document the live topics and their tile columns
    int32_t* d_live_n = nullptr;          // D
    char* d_live_list = nullptr;          // D x kLiveListBytes: a document's live topics and their t
    bool live_stats = false;              // the statistics pass of this corpus reads those lists (decided with the postings)
    int64_t* d_tile_ptr = nullptr;        // D
    double* d_live_tile = nullptr;        // sum over the quad classes' documents of N_d x (live topics the class hands over at)
    int32_t* d_handoff_it = nullptr;      // D: inner iterations the dense kernel ran before the hand-over, or -1
    int32_t* d_col_iters = nullptr;       // D: tile columns x iterations the live-topic kernel executed
    bool compact_ready = false;
    bool compact_failed = false;          // the tile buffer did not fit: dense kernels only, for good
    bool live_off_by_alpha = false;       // alpha has grown: too many topics never count as dead for any document to be handed over (alpha_allows_live)
    int compact_plan_epoch = -1, compact_cap_used = -1, compact_stream_used = -1, compact_pair_used = -2;
    // schedule ranges of one lane shape (term slots per lane) inside a launch class that hands documents over
    struct CompactRange { int plan_index, slots; bool from_table; int64_t first, count; };
    std::vector<CompactRange> compact_ranges;
    std::vector<Launch> plan;
    int plan_epoch = 0;
    int plan_serial = 0;           // counts build_plan() calls: what is derived from the plan knows which one it belongs to
    // packed launch slots of the quad classes (estep_limits.h QuadSlot; built by pack_quad_slots for plan number quad_slots_serial)
    pylda::QuadSlot* d_quad_rec = nullptr;
    int32_t* d_quad_ids = nullptr;
    pylda_plan::QuadSlotLayout quad_slots;
    int quad_slots_serial = -1;
    bool plan_exact = false;       // the plan avoids the kernels with the fixed-point stop test
    bool estep_done = false;
    int last_heldout = 0;
    // token samplers (sampler_host.h), each built by the first call that needs it: the terms' token offsets (exclusive scan
    // of term_ct, nnz + 1) and one state word per token (the hybrid E-step's sample histories; the collapsed Gibbs engine's
    // topic and the topic before its last draw; fold-in's topic)
    int64_t* d_tok_off = nullptr;
    uint64_t* d_hyb_state = nullptr;
    // hybrid E-step (launch_hybrid.hip), allocated by the first training one: CSR positions grouped by term for its statistics pass
    int64_t* d_hyb_col_ptr = nullptr;     // V + 1
    int64_t* d_hyb_post_pos = nullptr;    // nnz
    // collapsed Gibbs engine (launch_gibbs.hip), allocated by its first call; it keeps n_dk as exact doubles in d_gamma
    int32_t* d_gibbs_table = nullptr;     // V x ldk word-major topic counts
    int32_t* d_gibbs_nk = nullptr;        // K
    double* d_gibbs_alpha = nullptr;      // K: the priors of the last sweep / log posterior
    double* d_gibbs_beta = nullptr;       // V
    double* d_gibbs_words = nullptr;      // V + 1: the log posterior's per-word sums and its total
    std::vector<double> h_gibbs_alpha, h_gibbs_beta;   // what the two prior buffers hold
    bool gibbs_ready = false;             // gibbs_init or gibbs_set_state has run
    // ... sharded over several ranks (pylda_gibbs_exchange_prepare; gibbs_exchange.h): the move records of a round
    uint64_t* d_gibbs_send = nullptr;     // max(capacity) records: this rank's segment
    uint64_t* d_gibbs_recv = nullptr;     // world x max(capacity): every rank's segment of the round
    int64_t* d_gibbs_rec_off = nullptr;   // D: position of a document's first record in its round's segment
    std::vector<int64_t> h_gibbs_capacity, h_gibbs_round_tokens;   // per round: records a rank sends, records of this one
    int64_t gibbs_exchange_blocks = 0, gibbs_exchange_first = 0;   // the (blocks, first_document) the plan was made for
    int gibbs_exchange_world = 0;         // 0: no plan
    // left-to-right held-out likelihood (launch_left_to_right.hip), built by its first call: the documents' token offsets on the host
    std::vector<int64_t> h_ltr_doc_tok;   // D + 1
    // collapsed variational Bayes (launch_cvb0.hip), allocated by its first call; it keeps N_dk in d_gamma.  A held-out
    // corpus of pylda_cvb0_foldin has d_cvb0_g alone
    double* d_cvb0_g = nullptr;           // nnz x ldk: a row per (document, term) slot
    double* d_cvb0_table = nullptr;       // V x ldk word-major expected topic counts
    double* d_cvb0_nk = nullptr;          // K
    double* d_cvb0_chunk = nullptr;       // ceil(V / 1024) x ldk: the chunk sums of n_k
    double* d_cvb0_alpha = nullptr;       // K: the priors of the last sweep / likelihood
    double* d_cvb0_beta = nullptr;        // V
    double* d_cvb0_change = nullptr;      // D: sum c |df| of a document's last update
    double* d_cvb0_out = nullptr;         // 2: the likelihood's total and the change's
    std::vector<double> h_cvb0_alpha, h_cvb0_beta;     // what the two prior buffers hold
    bool cvb0_ready = false;              // cvb0_init or cvb0_set_state has run
    // ... the postings of the blocks of a sweep (host_plan.h: cvb0_block_postings), built for one (blocks, first_document)
    pylda_plan::Cvb0Postings cvb0_rounds; // (its two nnz-sized lists live on the device only)
    int64_t cvb0_blocks = 0, cvb0_first = 0;
    int64_t* d_cvb0_place = nullptr;      // nnz: a slot's row of the delta buffer
    int64_t* d_cvb0_seg_begin = nullptr;  // segments + 1
    int64_t* d_cvb0_run_seg = nullptr;    // runs + 1
    int32_t* d_cvb0_run_word = nullptr;   // runs
    double* d_cvb0_delta = nullptr;       // (largest block's slots) x ldk
    double* d_cvb0_partial = nullptr;     // (largest block's segments) x ldk
    // stochastic collapsed variational Bayes (launch_cvb0.hip, scvb_kernels.h): the buffers above without d_cvb0_g, and
    bool scvb_ready = false;              // scvb_init or scvb_set_state has run
    int32_t* d_scvb_word_run = nullptr;   // V: a word's run among the step's block, -1 without postings in it
};

namespace pylda_host __attribute__((visibility("hidden"))) {

extern std::string g_create_error;
int fail(pylda_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail((ctx), e_ == hipErrorOutOfMemory ? PYLDA_ERR_OOM : PYLDA_ERR_HIP, \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                        __LINE__);                                                      \
    } while (0)

template <typename T>
int dev_alloc(pylda_ctx* ctx, T** p, size_t n)
{
    *p = nullptr;
    if (n == 0) n = 1;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)));
    return PYLDA_OK;
}

template <typename T>
void dev_free(T*& p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

// keeps the first failure of a series of calls that all have to be attempted or skipped together
struct FirstError {
    pylda_ctx* ctx;
    const char* what;
    int rc = PYLDA_OK;
    void operator()(int r) { if (rc == PYLDA_OK) rc = r; }
    void h2d(void* dst, const void* src, size_t bytes)
    {
        if (rc == PYLDA_OK && bytes && hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(ctx, PYLDA_ERR_HIP, "%s: H2D copy failed", what);
    }
};

// One kernel launch: opt in to more than 64 KiB of dynamic LDS where the launch asks for it, launch, the runtime's verdict.
template <typename... Params, typename... Args>
hipError_t launch_kernel(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args)
{
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    return hipGetLastError();
}

// PYLDA_TIMING=1: wall time of the one-off phases (corpus upload, postings, segment cut) on stderr
struct PhaseTimer {
    bool on = getenv("PYLDA_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[pylda timing] %-34s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
        t0 = now;
    }
};

// ---- plan.hip ----
PlanConfig plan_config(const pylda_ctx* ctx);
void build_plan(pylda_corpus* c);
int slab_uber_from(const pylda_ctx* ctx, const pylda_corpus* c);    // first class of the one-dispatch slab group, or -1

// ---- launch_*.hip: one launch class of the plan on the stream `st` ----
int launch_generic_any(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);
int launch_slab_any(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);
int launch_slab_uber_any(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const pylda_corpus* c, int from);
int launch_quilt_any(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);
int launch_quad_any(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);         // (hands on to the next one where the class hands nothing over)
int launch_quad_dense_any(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);   // launch_quad_dense.hip: the kernels without the hand-over
int launch_qfuse(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);
int launch_qfusek(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);
int launch_qgroup(pylda_ctx* ctx, hipStream_t st, const EstepParams& p, const Launch& L);

// ---- launch_compact.hip: the live-topic kernel behind a quad launch class ----
int compact_handoff_for(const pylda_ctx* ctx, const Launch& L);      // 0: the class keeps its documents, 1: hands over with tile columns, 2: without
void compact_caps(const pylda_ctx* ctx, int (&caps)[9]);             // live topics at which a document of s term slots per lane is handed over
int prepare_compact(pylda_ctx* ctx, pylda_corpus* c);                // buffers and ranges of the hand-over (sets c->compact_ready)
int immortal_topics(const pylda_ctx* ctx);                           // topics whose alpha keeps them from ever counting as dead (kMortalT), by the host's alpha
bool alpha_allows_live(const pylda_ctx* ctx, bool was_off);          // fewer of them than the widest tile has columns (with hysteresis)
void release_postings(pylda_corpus* c);                              // sstats_gather.hip: the next training E-step builds them again
int launch_compact(pylda_ctx* ctx, hipStream_t st, const pylda_corpus* c, EstepParams p, int slots, bool from_table, int64_t first, int64_t count);

// ---- estep_api.hip: the steps every E-step flavour shares ----
int enqueue_prepare(pylda_ctx* ctx, bool heldout);                   // the tables of this eta (prepare_kernels.h)
struct AlphaSums { double sum, lgamma_sum, term; };                  // sum_k alpha_k, sum_k lnG(alpha_k), lnG(sum) - sum lnG  (:195)
AlphaSums alpha_sums(const pylda_ctx* ctx);                          // by the host's alpha
// the tail of every E-step: per-document values -> the scalars of pylda_estep_results (`entropy`: with the fast path's corpus term), bookkeeping
int finish_estep(pylda_ctx* ctx, pylda_corpus* c, int heldout, bool entropy, bool doc_values);

// ---- sstats_gather.hip ----
int build_postings(pylda_corpus* c);
int enqueue_sstats_gather(pylda_ctx* ctx, pylda_corpus* c);

// ---- context.hip: profiling events ----
int open_bracket(pylda_ctx* ctx, int slot, hipStream_t st);         // index into pending_events, or -1 (not profiling, no event)
void close_bracket(pylda_ctx* ctx, int at, hipStream_t st);
void drain_events(pylda_ctx* ctx);

}  // namespace pylda_host
