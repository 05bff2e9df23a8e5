/*
 * pylda_hip.h - C ABI of libpylda_hip.so: the MI355X (gfx950) implementation
 * of PyLDA's variational-Bayes E-step hot path.
 *
 * The reference (kzhai/PyLDA) has no FFI: its seam is two Python methods,
 * VariationalBayes.e_step (variational_bayes.py:132-216) and m_step
 * (:218-235), driven by learning() (:239-261) and inference() (:263-271).
 * Each entry point below names the reference lines it replaces.  The Python
 * binding that calls these (ctypes) is pylda_amd/_capi.py; the stub a
 * maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; the caller owns every host buffer; the library
 *    never keeps a host pointer after the call returns;
 *  - matrices handed over by the host use numpy's C order: eta and sstats
 *    are (K, V) row-major, gamma is (D, K) row-major;
 *  - every function returns 0 on success or a negative pylda_status; the
 *    text of the last failure is pylda_last_error(ctx) (or (NULL) for
 *    failures of pylda_create); no C++ exception crosses the ABI;
 *  - a context is used from one thread at a time (ctypes drops the GIL for
 *    the duration of a call); work is enqueued on the context's HIP stream
 *    and the *_get_* / *_results functions synchronise it;
 *  - there is no CPU fallback: without a usable HIP device pylda_create
 *    fails with PYLDA_ERR_HIP.
 */
#ifndef PYLDA_HIP_H
#define PYLDA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pylda_ctx pylda_ctx;
typedef struct pylda_corpus pylda_corpus;

typedef enum pylda_status {
    PYLDA_OK = 0,
    PYLDA_ERR_INVALID = -1, /* bad argument (shape, range, NULL, unsorted CSR ...) */
    PYLDA_ERR_HIP = -2,     /* HIP runtime error (no device, launch failure ...)   */
    PYLDA_ERR_OOM = -3,     /* host or device allocation failed                    */
    PYLDA_ERR_STATE = -4    /* call sequence error (e.g. results before an e-step) */
} pylda_status;

/* ABI version: bumped whenever an existing entry point changes its signature or meaning.
 *   1  round-1 interface
 *   2  pylda_parse_corpus gained doc_separator, pylda_kernel_time its third output,
 *      pylda_set_stream(NULL) = HIP's null stream (pylda_use_own_stream restores the private one)
 *   3  additions only: pylda_abi_version, pylda_mstep_enqueue / pylda_outer_device / pylda_allreduce_outer /
 *      pylda_outer_fetch (one host wait per outer iteration), pylda_model_checkpoint, pylda_mark_time /
 *      pylda_elapsed_ms, pylda_work_counters, pylda_executed_work, pylda_clock_counters, pylda_host_alloc / pylda_host_free, pylda_test_alpha_update;
 *      pylda_set_alpha no longer waits for the stream (and is a no-op when handed the values the device holds)
 *   4  additions only: pylda_hybrid_estep / pylda_hybrid_scale_sstats (the hybrid Gibbs-within-VB E-step),
 *      pylda_test_philox
 *   5  additions only: pylda_gibbs_init / pylda_gibbs_sweep / pylda_gibbs_log_posterior / pylda_gibbs_get_counts /
 *      pylda_gibbs_set_state (the collapsed Gibbs engine)
 *   6  additions only: pylda_foldin_set_model / pylda_foldin (held-out fold-in against a frozen Gibbs model)
 *   7  additions only: pylda_gibbs_round_tokens / pylda_gibbs_exchange_prepare / pylda_gibbs_round_sample /
 *      pylda_gibbs_round_apply / pylda_gibbs_table_device / pylda_gibbs_log_posterior_parts (the collapsed Gibbs engine
 *      sharded over several ranks)
 *   8  additions only: pylda_mstep_online / pylda_mstep_online_enqueue (online variational Bayes: the M-step that blends
 *      a minibatch's statistics into eta)
 *   9  additions only: pylda_completion_set_model / pylda_completion_score (document-completion held-out likelihood)
 *  10  additions only: pylda_test_special_forms (test hook: every call form of the device special functions);
 *      pylda_top_words / pylda_codocument_counts (topic coherence: the top words of every topic and the co-document
 *      counts of their pairs); pylda_test_tables (test hook: the tables an E-step prepares from eta, and alpha_sgn);
 *      pylda_test_statistics (test hook: the statistics pass on given t, r and lists of live topics),
 *      pylda_compute_units; pylda_similarity_set_base / pylda_similar_documents (nearest documents by topic mixture: a
 *      base of rows on the device, the fused score and top-N pass over it); pylda_test_gibbs_posterior_terms (test hook:
 *      the collapsed Gibbs log posterior's per-document and per-word terms and its three device sums);
 *      pylda_left_to_right / pylda_test_left_to_right_state (the left-to-right held-out likelihood of every engine's
 *      predictive table, and the test hook that copies its last call's topics and predictive probabilities);
 *      pylda_topic_distances (topic distances between two models: the matrix of Bhattacharyya coefficients or of
 *      Jensen-Shannon divergences between the rows of two (K', V) tables); pylda_stop_sum_counters (how often the
 *      live-topic kernel's stop sum was skipped and formed); pylda_cvb0_init / pylda_cvb0_sweep /
 *      pylda_cvb0_log_likelihood / pylda_cvb0_get_state / pylda_cvb0_set_state / pylda_cvb0_foldin (the collapsed
 *      variational Bayes engine, CVB0) and pylda_test_cvb0_postings (test hook: the postings of its blocks);
 *      pylda_test_alpha_statistics (test hook: the M-step's alpha statistics on given rows of gamma);
 *      pylda_scvb_init / pylda_scvb_step / pylda_scvb_get_state / pylda_scvb_set_state (stochastic collapsed variational
 *      Bayes, SCVB0: minibatch steps without per-slot state; pylda_cvb0_log_likelihood also serves its corpora)
 * A host compiled against another version must refuse to run: compare PYLDA_ABI_VERSION with
 * pylda_abi_version() right after loading the library. */
#define PYLDA_ABI_VERSION 10
int pylda_abi_version(void);

/* Library version string, e.g. "pylda_hip 0.9 (gfx950, abi 10)". */
const char* pylda_version(void);

/* Number of visible HIP devices (0 is a valid answer, not an error). */
int pylda_device_count(int* count);

/* Create a context for a model with K topics over V word types on `device`.
 * Allocates the device-resident tables (eta, exp(E_log_eta), sstats: K*V
 * doubles each).  Replaces the per-call numpy allocations of
 * variational_bayes.py:147-152. */
int pylda_create(int device, int K, int V, pylda_ctx** out);
void pylda_destroy(pylda_ctx* ctx);
const char* pylda_last_error(const pylda_ctx* ctx);

/* Run the context's work on an existing HIP stream (e.g. a torch stream, so
 * that an RCCL all-reduce issued through torch.distributed on the same stream
 * is ordered after the E-step without a host sync).  As everywhere in HIP, a
 * NULL handle names the device's default (null) stream - which is what
 * torch.cuda.current_stream().cuda_stream is for torch's default stream.
 * pylda_use_own_stream returns to the context's private (non-blocking)
 * stream.  Both drain the stream in use before switching; the caller keeps a
 * stream it handed over alive. */
int pylda_set_stream(pylda_ctx* ctx, void* hip_stream);
int pylda_use_own_stream(pylda_ctx* ctx);
int pylda_synchronize(pylda_ctx* ctx);

/* Upload a parsed corpus: the (word_ids, word_cts) lists parse_data builds
 * (variational_bayes.py:98-130) flattened to CSR.  doc_ptr has D+1 entries,
 * term ids are in [0, V), counts are >= 1, ids are unique within a document
 * (parse_data builds them from a dict).  Copies to the device once and
 * builds the launch schedule (documents bucketed by distinct-term count). */
int pylda_corpus_create(pylda_ctx* ctx, int64_t D, const int64_t* doc_ptr,
                        const int32_t* term_id, const int32_t* term_ct, pylda_corpus** out);
void pylda_corpus_destroy(pylda_corpus* corpus);
/* D, nnz, token total, largest distinct-term count. */
int pylda_corpus_info(const pylda_corpus* corpus, int64_t* D, int64_t* nnz, int64_t* tokens,
                      int32_t* max_terms);

/* Model state.  eta is self._eta (K, V) (variational_bayes.py:95,226);
 * alpha is self._alpha_alpha (K,) (inferencer.py:57). */
int pylda_set_eta(pylda_ctx* ctx, const double* eta_kv);
int pylda_get_eta(pylda_ctx* ctx, double* eta_kv);
int pylda_set_alpha(pylda_ctx* ctx, const double* alpha_k);

/* THE HOT PATH: one E-step over `corpus` (variational_bayes.py:132-216).
 *   max_iter / tol  local_parameter_iteration / _converge_threshold (:132)
 *   heldout         0: training mode (parsed_corpus == None): accumulates the
 *                      sufficient statistics (:207);
 *                   1: held-out mode (:154-155, :202-204): word log-likelihood,
 *                      no sufficient statistics.
 * Asynchronous: enqueues compute_dirichlet_expectation (inferencer.py:15-18),
 * the per-document phi/gamma loop and the reductions on the context's
 * stream.  Results stay on the device until fetched. */
int pylda_estep(pylda_ctx* ctx, pylda_corpus* corpus, int max_iter, double tol, int heldout);

/* Corpus-level scalars of the last E-step (synchronises):
 * document_log_likelihood (:143,:195-199), words_log_likelihood (:144,:204)
 * and how many documents were finished by the log-space safety-net kernel. */
int pylda_estep_results(pylda_ctx* ctx, pylda_corpus* corpus, double* document_log_likelihood,
                        double* words_log_likelihood, int64_t* logspace_documents);

/* phi_sufficient_statistics (K, V) of the last training-mode E-step (:214). */
int pylda_get_sstats(pylda_ctx* ctx, double* sstats_kv);
/* Upload sufficient statistics (K, V) handed to m_step by the caller (:218). */
int pylda_set_sstats(pylda_ctx* ctx, const double* sstats_kv);
/* gamma_values (D, K) of the last E-step over `corpus` (:213,:216). */
int pylda_get_gamma(pylda_ctx* ctx, pylda_corpus* corpus, double* gamma_dk);
/* Per-document values (any pointer may be NULL): the document's own terms of
 * :195-199, of :204, and the number of inner iterations it ran. */
int pylda_get_doc_values(pylda_ctx* ctx, pylda_corpus* corpus, double* doc_ll,
                         double* doc_words_ll, int32_t* iters);

/* One-shot host-buffer form of the hot path (the signature SURVEY.md 8b
 * proposes): set_alpha + set_eta + estep + fetch.  Output pointers may be
 * NULL.  scalars_out[0] = document_log_likelihood, [1] = words_log_likelihood. */
int pylda_estep_host(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k,
                     const double* eta_kv, int max_iter, double tol, int heldout,
                     double* gamma_dk, double* sstats_kv, double* doc_ll, double* doc_words_ll,
                     int32_t* iters, double* scalars_out);

/* Device-resident views for multi-GPU data parallelism: the sufficient
 * statistics live word-major, (V, ldk) doubles with ldk = pylda_table_stride
 * (K rounded up to 16 / 32 / a multiple of 64; padding columns are zero).
 * The Python side wraps this pointer (zero-copy) and all-reduces its V*ldk
 * elements over RCCL between e_step and m_step.  Also the gamma buffer of a
 * corpus, (D, K). */
int pylda_table_stride(const pylda_ctx* ctx);
/* Compute units of the context's device (0: ctx is NULL).  The persistent sweep of the statistics pass runs one
 * workgroup on each: with "gather_sweep_terms" and "gather_sweep_wpb" of pylda_corpus_layout, the terms a pass covers. */
int pylda_compute_units(const pylda_ctx* ctx);
void* pylda_sstats_device(pylda_ctx* ctx);
void* pylda_eta_device(pylda_ctx* ctx);      /* (K, V) doubles, numpy layout */
void* pylda_gamma_device(pylda_corpus* corpus);

/* Tell the library that the caller wrote eta (have_eta = 1) and/or the
 * sufficient statistics (have_sstats = 1) through the device pointers above
 * (e.g. after an all-reduce); -1 leaves a flag unchanged. */
int pylda_mark_device_state(pylda_ctx* ctx, int have_eta, int have_sstats);

/* Multi-GPU exchange without Python (documents shard across GPUs, ONE all-reduce of the
 * K x V sufficient statistics per outer iteration).  RCCL is bound at run time (dlopen of librccl.so;
 * PYLDA_RCCL_PATH overrides the search), so the library has no link-time dependency on it.
 *   rank 0:      pylda_comm_unique_id(id)        128 opaque bytes; the host hands them to every rank
 *                                                (MPI, a socket, a file)
 *   every rank:  pylda_comm_init(ctx, id, rank, world_size)      collective
 *   per outer iteration, between pylda_estep and pylda_mstep:
 *                pylda_allreduce_sstats(ctx)     in-place sum of the V x ldk device buffer, enqueued on the
 *                                                context's stream (ordered with the kernels, no host sync)
 *                pylda_allreduce_doubles(ctx, v, n)   sum of a short host vector (document log-likelihood,
 *                                                #documents, alpha statistics: variational_bayes.py:232-233)
 * Every rank then runs the identical pylda_mstep.  The Python class does the same through torch.distributed. */
#define PYLDA_COMM_ID_BYTES 128
int pylda_comm_unique_id(void* id_out);
int pylda_comm_init(pylda_ctx* ctx, const void* id, int rank, int world_size);
int pylda_comm_destroy(pylda_ctx* ctx);
int pylda_allreduce_sstats(pylda_ctx* ctx);
int pylda_allreduce_doubles(pylda_ctx* ctx, double* values, int64_t n);

/* Device M-step (variational_bayes.py:218-235) on the resident buffers:
 * topic log-likelihood from the PRE-update eta (:222-224), eta <- sstats +
 * beta (:226), alpha sufficient statistics from the gamma of `corpus`
 * (:232-233).  beta_v is self._alpha_beta (V,).  alpha_ss_k may be NULL. */
int pylda_mstep(pylda_ctx* ctx, pylda_corpus* corpus, const double* beta_v,
                double* topic_log_likelihood, double* alpha_ss_k);

/* learning() (variational_bayes.py:239-261) with ONE host wait per outer iteration.  After pylda_estep (and the
 * all-reduce of the sufficient statistics when there are several ranks):
 *   pylda_mstep_enqueue   the device half of m_step (:218-235) - topic log-likelihood terms of the PRE-update eta,
 *                         eta <- sstats + beta, alpha sufficient statistics from the gamma of `corpus` - plus a
 *                         pack of every value the host half needs into one device vector; nothing is waited for;
 *                         hyper_parameter_iteration > 0 also asks for the alpha update of the iteration
 *                         (optimize_hyperparameters, :277-324, the reference's defaults: 100, 0.9, 10, 1e-6) ON THE
 *                         DEVICE - it runs inside pylda_outer_fetch, behind the sum over the ranks, and leaves the new
 *                         alpha where the next E-step reads it; 0: alpha stays (hyper_parameter_optimize_interval);
 *   pylda_outer_device    that vector (3K + 4 doubles) and how many of its LEADING elements are rank-local sums:
 *                         [document log-likelihood (:214), #documents, documents redone in log space, 0,
 *                          alpha sufficient statistics (K) (:232-233) | per-topic likelihood terms (K) | alpha (K),
 *                          both replicated];
 *                         a multi-rank host sums the leading *n_reduce elements over the ranks in place, on the
 *                         context's stream (the Python class: torch.distributed; a C host: pylda_allreduce_outer);
 *   pylda_outer_fetch     [the alpha update] + one device-to-host copy + the wait; any output pointer may be NULL;
 *                         alpha_k receives the alpha the device now holds (updated or not). */
int pylda_mstep_enqueue(pylda_ctx* ctx, pylda_corpus* corpus, const double* beta_v, int hyper_parameter_iteration,
                        double hyper_parameter_decay_factor, int hyper_parameter_maximum_decay,
                        double hyper_parameter_converge_threshold);
void* pylda_outer_device(pylda_ctx* ctx, int64_t* n_reduce);
int pylda_allreduce_outer(pylda_ctx* ctx);
int pylda_outer_fetch(pylda_ctx* ctx, double* document_log_likelihood, double* number_of_documents,
                      int64_t* logspace_documents, double* topic_log_likelihood, double* alpha_ss_k, double* alpha_k);

/* Online variational Bayes (Hoffman, Blei & Bach 2010): the twins of pylda_mstep and pylda_mstep_enqueue for a step on a
 * minibatch.  After pylda_estep in training mode on the minibatch's corpus they compute the topic log-likelihood terms of
 * the PRE-update eta and the alpha sufficient statistics of the minibatch's gamma as their twins do, and in place of
 * eta <- sstats + beta
 *     eta[k][v] <- (1 - rho) * eta[k][v] + rho * (scale * sstats[v][k] + beta[v])
 * in place, each element rounded in the order m = scale * s, a = m + beta, b = rho * a, c = (1 - rho) * eta, c + b, with
 * 1 - rho computed once on the host: numpy's elementwise form of the expression gives the same bits, and rho = scale = 1
 * gives pylda_mstep's eta.  rho is the step size, in (0, 1]; scale is #documents of the corpus / #documents of the
 * minibatch, finite and positive (otherwise PYLDA_ERR_INVALID, as for a NULL beta_v).  PYLDA_ERR_STATE as for the twins.
 * pylda_mstep_online_enqueue schedules no alpha update - alpha is fixed in an online run - and packs the minibatch's
 * document log-likelihood and document count (unscaled) for pylda_outer_fetch, which is unchanged. */
int pylda_mstep_online(pylda_ctx* ctx, pylda_corpus* corpus, const double* beta_v, double rho, double scale,
                       double* topic_log_likelihood, double* alpha_ss_k);
int pylda_mstep_online_enqueue(pylda_ctx* ctx, pylda_corpus* corpus, const double* beta_v, double rho, double scale);

/* Page-locked host memory for the arrays of the public e_step() / m_step() contract (eta, the sufficient
 * statistics and gamma as host ndarrays, variational_bayes.py:212-216): buffers from here move at the PCIe rate
 * (~50 GB/s) instead of through the runtime's staging copy of pageable memory (cfg 3: e_step() 52 -> about 25 ms).
 * Any host pointer is still accepted everywhere; this is an allocator, not a requirement. */
int pylda_host_alloc(int64_t bytes, void** out);
int pylda_host_free(void* p);

/* Device-side model checkpoint: restore = 0 saves eta (the model; the counterpart of the reference's
 * snapshot pickles, launch_train.py:203-204, without the trip through the host), restore = 1 puts the saved
 * eta back.  Asynchronous on the context's stream.  bench.py uses it to time the same outer iterations
 * repeatedly. */
int pylda_model_checkpoint(pylda_ctx* ctx, int restore);

/* Time stamps on the context's stream (4 slots): pylda_mark_time records an event NOW in stream order,
 * pylda_elapsed_ms waits for slot_to and returns the device time between the two.  learning() uses them
 * for the reference's "e_step and m_step ... finished in" line (variational_bayes.py:254) now that the
 * host no longer waits between the two steps. */
int pylda_mark_time(pylda_ctx* ctx, int slot);
int pylda_elapsed_ms(pylda_ctx* ctx, int slot_from, int slot_to, double* ms);

/* Profiling: when enabled, every pylda_estep brackets (HIP events on the launch
 * streams) its document kernels as a group, each launch class on its own, and
 * the sufficient-statistics pass (gather + finalize).  pylda_kernel_time
 * returns the accumulated group times (ms) and the number of E-steps since the
 * last reset, and resets them. */
int pylda_set_profiling(pylda_ctx* ctx, int enabled);
int pylda_kernel_time(pylda_ctx* ctx, double* doc_kernel_ms, double* sstats_kernel_ms,
                      int64_t* estep_calls);
/* With profiling enabled every pylda_estep also accumulates, on the device, the inner iterations its documents
 * actually ran (sum_d I_d) and their terms (sum_d I_d N_d: 4 K flops each, :177-185).  Returns and resets them
 * (synchronises). */
int pylda_work_counters(pylda_ctx* ctx, double* inner_iterations, double* inner_iteration_terms);
/* ... and the rest of the SAME read (no device access: the values of the last pylda_work_counters call):
 * what the kernels really ran - tile_entries = sum_d N_d (K x iterations of the dense kernel + tile columns x iterations
 * of the live-topic kernel), two FMAs each, and the documents handed to the live-topic kernel (estep_compact.h: the
 * iterations of :174-190 on the topics whose gamma still differs from alpha); tile_entries / (K x inner_iteration_terms)
 * is the fraction of the dense N_d x K work that was executed - */
int pylda_executed_work(pylda_ctx* ctx, double* tile_entries, double* handed_over);
/* ... of the live-topic kernel's iterations in those E-steps (wavefront 0's of a document), how many skipped the stop
 * sum - one topic's |delta gamma| alone exceeded the threshold, so the sum could not be below it - and how many formed it
 * (a document the kernel flagged for the log-space kernel counts there with all its remaining iterations) - */
int pylda_stop_sum_counters(pylda_ctx* ctx, double* skipped, double* formed);
/* ... and the shader clock under that load: spans of resident kernels of the profiled E-steps (one in 64 live-topic
 * wavefronts, the work counter's own kernel) measured twice - in shader cycles (s_memtime) and in ticks of the constant
 * wall_hz counter (s_memrealtime).  Sustained clock in Hz = shader_ticks / wall_ticks * wall_hz. */
int pylda_clock_counters(pylda_ctx* ctx, double* shader_ticks, double* wall_ticks, double* wall_hz);

/* The launch schedule of a corpus: documents are bucketed by distinct-term
 * count into launch classes (one kernel instantiation each; the classes of one
 * E-step run concurrently on separate streams).  Fills up to `capacity`
 * entries per array (any may be NULL): kernel variant index (see
 * "force_variant"), its geometry code, documents and distinct (doc, term)
 * pairs in the class, and the profiled kernel time accumulated for the class
 * since the last call (ms; reset by the call).  Returns the number of classes
 * (>= 0) or a negative status. */
int pylda_corpus_plan(pylda_corpus* corpus, int32_t capacity, int32_t* variant, int32_t* geometry,
                      int64_t* documents, int64_t* terms, double* kernel_ms);

/* Layout facts of an uploaded corpus (measurement / test hook): "gather_blocks" - document blocks of the
 * statistics gather (1: unblocked; set when the first training E-step builds the postings, 0 before),
 * "gather_segments" - its posting segments, "gather_rounds" - the term ranges the gather is run in so that their
 * segments share one set of partial rows, "gather_partial_rows" - those rows, "gather_sweep_passes" - passes of the
 * persistent sweep that replaces rows and rounds (0: not in use), "gather_sweep_terms" / "gather_sweep_wpb" - the terms a
 * wavefront of the sweep owns per pass and its wavefronts per workgroup (0: not in use; one workgroup per compute
 * unit, pylda_compute_units), "gather_live" - 1: the pass reads the documents' lists of live topics (sstats_live.h), "live_off_by_alpha" - 1: alpha keeps more topics from ever dying than a tile of the
 * live-topic kernel has columns, so the corpus runs on the dense kernels alone (decided before every E-step; when it
 * changes the postings are rebuilt once in the layout that fits), "quad_slot_bytes" - device bytes of the packed launch
 * slots of the stride-256 quad classes (a 32-byte record and the term ids in lane order per document; 0: none - no such
 * class, or the allocation did not fit and the classes address through the schedule).  Returns the value, or a negative
 * pylda_status. */
int64_t pylda_corpus_layout(pylda_corpus* corpus, const char* name);

/* Tuning / test options:
 *   "doc_values"     1 (default): pylda_get_doc_values returns complete per-document
 *                    log-likelihoods.  0: training fast path - the corpus-level
 *                    document_log_likelihood is identical, but its log-B entropy term is
 *                    taken once per corpus from the sufficient statistics instead of a
 *                    second table gather per document; doc_ll[] is then unavailable;
 *   "force_logspace" 0|1  run every document through the log-space
 *                         safety-net kernel (the reference's formulation);
 *   "force_variant"  -1 (automatic) or a kernel variant index: 0..2 generic LDS 64/256/512
 *                    threads, 3 generic global, 4 slab, 6 quilt, 9 group-fused streaming (more than 256 terms at
 *                    table stride 64 / 128 / 256), 10 quad, 11 fused streaming, 12 generic with the per-term scalars
 *                    in global memory (documents of any length), 13 fused streaming for 512 < K <= 1024 (5, 7, 8 were
 *                    the column, two-pass streaming and hybrid kernels of rounds 1-2, removed);
 *                    a variant that cannot take a document falls back to the automatic choice;
 *   "gather_rows"    statistics gather (variational_bayes.py:207): 0 64-topic chunks, 1 whole rows,
 *                    2 (default) whole rows with the postings fetched in bulk (table stride 128 / 256);
 *   "gather_blocks"  document blocks of that gather, for corpora created afterwards: -1 (default)
 *                    automatic - blocks of about one L2 while a (term, block) pair keeps >= 8
 *                    postings, else unblocked; 0 / 1 off; n > 1 forced (a multiple of 8);
 *   "gather_sweep"   the document-blocked gather as ONE persistent kernel in which every wavefront owns a few terms
 *                    and all workgroups sweep the document blocks together (no partial rows; table stride 128 / 256):
 *                    0 never, 1 (default) where the partial rows of the dispatch-paced gather would exceed their
 *                    budget, 2 whenever the gather is blocked;
 *   "gather_round_mb" budget of the gather's partial rows (one per (term, document block) pair) in MiB, 0 = 4 GiB:
 *                    beyond it the statistics pass is the sweep (gather_sweep = 1) or the gather runs in rounds over term
 *                    ranges that reuse the rows.  The sweep-or-gather decision is taken against this figure only; the rounds
 *                    are additionally capped by a quarter of the device memory free at the time (more, smaller rounds on
 *                    a busy device) - which changes no bit of the result: partial rows are summed in segment order and the
 *                    likelihood's entropy partials are laid out by blocks of the whole table, whatever the rounds;
 *   "wide_postings"  1: 64-bit CSR positions in the postings whatever the corpus size (automatic from 2^31 pairs);
 *   "sweep_xcd"      1 (default): the sweep's rendezvous per XCD (the 32 workgroups that share an L2), 0: chip-wide;
 *   "sweep_spin"     polls of a rendezvous before a workgroup goes on alone (pacing only, never correctness);
 *   "sweep_sub"      sub-steps the sweep walks a document block's range in (default 4; results are bitwise the same);
 *   "terms_overlap"  1 (default): the document-terms pass of the training fast path runs on an auxiliary stream beside
 *                    the dispatch-paced statistics gather, 0: in front of it;
 *   "launch_order"   1 (default): launch classes with the fewest documents go out first, 0: longest documents first
 *                    (scheduling options never change a bit of the results);
 *   "slab_uber"      1 (default): the slab launch classes of a small corpus go out as one dispatch;
 *   "gather_live"    1 (default): where a corpus hands documents to the live-topic kernel ("compact") the statistics pass
 *                    reads the lists of live topics those documents leave (10 bytes per live topic instead of a row of K
 *                    doubles per posting; one plain walk of the postings: no document blocks, sweep or rounds); 0: the
 *                    row gathers above.  Takes effect for corpora whose postings are built afterwards;
 *   "alpha_ss_moved" 1 (default): the M-step's alpha statistics evaluate digamma only for the gamma_dk that differ from
 *                    alpha_k bitwise and take psi(alpha_k) from a table for the rest (after a live-topic E-step: nearly
 *                    all); 0: digamma of all D x K entries.  The same bits either way - an A/B switch;
 *   "compact_phase"  1 (default): the live-topic kernels of an E-step run behind ALL its dense kernels, 0: behind their
 *                    launch class on its stream (scheduling only);
 *   "compact"        1 (default): at 64 < K <= 512 a document leaves the dense kernel once few enough topics still move
 *                    (gamma_k != alpha_k bitwise; 8-64 by document length and table stride) and finishes on the live-topic
 *                    kernel; 0: dense kernels only.  Same iteration counts, results equal to rounding (another summation order);
 *   "compact_pair"   -1 (default): from table stride 256 on a document is handed over at twice the columns one wavefront
 *                    holds and starts on two wavefronts that split the columns; 0: never, 1: always;
 *   "compact_stream" 1 (default): the fused streaming kernel (table stride 384 / 512) hands over too - without a tile, the
 *                    live-topic kernel gathers its entries from the table; 0: the quad kernel only;
 *   "compact_cap"    test hook: hand over at this many live topics at most (0: the kernel's capacity; <= 64);
 *   "compact_guard_fail" test hook: the live-topic kernel's exactness guard fails for every document (they are redone by
 *                    the log-space kernel);
 *   "compact_underflow_doc" test hook (-1, default: off): between the dense kernel and the live-topic kernel the entries
 *                    of this document's LAST term in its hand-over tile are scaled by 1e-288, so that the term's normaliser
 *                    leaves the fp64 range inside the live-topic kernel and nowhere else (a per-term scale cancels in
 *                    everything but the normaliser; the document is redone by the log-space kernel, from the table);
 *   "quad" (1: documents of <= 224 distinct terms at 64 < K <= 256 run on the quad kernel), "quad_stream" (1: ... and
 *   those of 225-256 terms too, with word slots streamed from the table), "quad_packed" (1: the quad kernel at table
 *   stride 256 addresses its document through packed launch slots - one memory round trip in front of the row gather -
 *   and forms the first t while the gather is in flight; 0: through the schedule, doc_ptr and term_id; same bits),
 *   "quilt_odd",
 *   "prepare_path"   which kernels turn eta into the word-major tables at the head of every E-step: 0 (default) by size -
 *                    one kernel, a wavefront per word, when K <= 64 and K * V <= 2^21, else a transposing pass and a
 *                    shift pass; 1: the one kernel whatever V (PYLDA_ERR_INVALID at K > 64); 2: the two passes.  The
 *                    same operations in the same order: the tables agree bit for bit (tests/test_gpu_tables.py);
 *   "quilt12", "lds_pad"  A/B switches of kernel geometry ("Tried and measured");
 *   "coherence_chunk_docs" test hook: pylda_codocument_counts walks the reference corpus in chunks of this many documents
 *                    (a multiple of 64; 0, the default: as many as a quarter of the free device memory holds bitmaps for).
 *                    The counts are the same whatever the chunk;
 *   "similarity_doc_slices" test hook: pylda_similar_documents cuts the base into this many slices of documents, one
 *                    workgroup per (block of 64 queries, slice) (1 .. 1024, clamped to the base's tiles of 128 documents;
 *                    0, the default: as many as put three workgroups on every compute unit; anything else
 *                    PYLDA_ERR_INVALID).  The result is the same whatever the slices;
 *   "topic_distance_segment_groups" test hook: pylda_topic_distances deals the segments of 1024 words to this many
 *                    workgroups per tile of pairs (1 .. 65535, clamped to the segments there are; 1: a workgroup adds all
 *                    of a tile's segments in registers; 0, the default: 1 once the tiles alone put two workgroups on every
 *                    compute unit, else as many as bring the launch to four; anything else PYLDA_ERR_INVALID).  The result
 *                    is the same whatever the groups;
 *   "ltr_chunk_tokens" test hook: pylda_left_to_right keeps the scratch of at most this many tokens (times the particles)
 *                    and walks the documents in chunks that fit it (0, the default: what the free device memory holds).
 *                    The result is the same whatever the chunks. */
int pylda_set_option(pylda_ctx* ctx, const char* name, int64_t value);

/* Test hook: evaluate the device special functions on n host values. */
int pylda_test_special(pylda_ctx* ctx, int64_t n, const double* x, double* digamma_out,
                       double* lgamma_out);

/* Native corpus ingest: parse_data (variational_bayes.py:98-130) without the Python
 * interpreter.  `text` holds the documents, each ended by the byte `doc_separator`
 * ('\n' for the contents of a train.dat file; the Python binding joins the caller's strings
 * with a byte that occurs in none of them) except possibly the last; tokens are separated by
 * the white space Python's str.split() splits on (the Unicode set, UTF-8 encoded - a '\n'
 * inside a document is just white space when it is not the separator).  `vocab` holds the
 * word types, one per line ('\n'), in id order (id = index among the distinct lines).
 * Rules kept from the reference: tokens not in the vocabulary are skipped (:108-109),
 * documents left without tokens are dropped (:116-118); the caller lower-cases/strips
 * lines beforehand if it wants launch_train.py:106 semantics (ASCII lower-casing can be
 * requested with lowercase=1).  Within a document, term ids appear in first-occurrence
 * order (what the reference's dict gives on CPython >= 3.7).
 * Two-call protocol: call with term_id == NULL to get the sizes (*n_docs, *nnz), then
 * with buffers of n_docs+1 / nnz / nnz elements.  Pure host code: no GPU needed. */
int pylda_parse_corpus(const char* text, int64_t text_bytes, int doc_separator, const char* vocab,
                       int64_t vocab_bytes, int lowercase, int64_t* n_docs, int64_t* nnz,
                       int64_t* doc_ptr, int32_t* term_id, int32_t* term_ct, int64_t* dropped_docs);

/* Test hook: the device alpha update (optimize_hyperparameters, variational_bayes.py:277-324) on host vectors:
 * alpha_k, alpha_ss_k (K each), #documents -> alpha_out_k. */
int pylda_test_alpha_update(pylda_ctx* ctx, const double* alpha_k, const double* alpha_ss_k, double number_of_documents,
                            int hyper_parameter_iteration, double hyper_parameter_decay_factor,
                            int hyper_parameter_maximum_decay, double hyper_parameter_converge_threshold,
                            double* alpha_out_k);

/* Test hook: the alpha sufficient statistics of the M-step (variational_bayes.py:232-233) on a caller's gamma (D x K, row
 * major; D >= 0): out_k[k] = sum_d psi(gamma_dk) - psi(sum_k gamma_dk), by the very launch pylda_mstep makes - with the
 * alpha the context holds (pylda_set_alpha, or the device alpha update) and the option "alpha_ss_moved" as it stands.
 * Changes no state of the context but its scratch.  PYLDA_ERR_STATE: alpha was never set. */
int pylda_test_alpha_statistics(pylda_ctx* ctx, const double* gamma_dk, int64_t D, double* out_k);

/* The hybrid E-step (hybrid.py:85-171 of the reference: Mimno, Hoffman & Blei 2012): per document a Gibbs sampler
 * over its tokens - number_of_samples sweeps, the samples of the sweeps from burn_in_samples on kept - inside the
 * variational outer loop.  Reads the same model state as pylda_estep (set_eta / set_alpha, or the device M-step) and
 * fills the same device slots: gamma (alpha + the final topic counts), the per-document values (iters =
 * number_of_samples) and the scalars of pylda_estep_results, so that pylda_get_gamma, pylda_get_doc_values,
 * pylda_mstep_enqueue and pylda_outer_fetch work unchanged.
 *   seed, stream     key and stream of the counter-based random numbers (Philox4x32-10): every draw is a function of
 *                    (seed, stream, global document index, sweep, token position) - independent of the launch shape,
 *                    the document order and the sharding.  stream < 2^32 (the Python class: the iteration counter in
 *                    training, a range of its own for held-out calls)
 *   first_document   global index of the corpus' first document (shards of one corpus: the offsets of their ranges)
 *   heldout          0: training mode - the sufficient statistics are the RAW post-burn-in topic counts per word
 *                    (exact doubles, word-major as pylda_sstats_device describes); divide them with
 *                    pylda_hybrid_scale_sstats (after the all-reduce of a sharded run, so that the sum is exact);
 *                    1: held-out mode - words_log_likelihood with the unnormalised E_log_eta, as the reference.
 * Tokens of a document are visited term by term in CSR order (the copies of a term back to back).  The first call on a
 * corpus allocates its token offsets and sample histories (8 bytes per token, 16 per distinct (document, term) pair);
 * PYLDA_ERR_OOM when they do not fit.  PYLDA_ERR_INVALID: burn_in_samples >= number_of_samples, or
 * (number_of_samples - burn_in_samples + 1) * ceil(log2 K) > 64 (a token's history is one 64-bit word). */
int pylda_hybrid_estep(pylda_ctx* ctx, pylda_corpus* corpus, int number_of_samples, int burn_in_samples, uint64_t seed,
                       uint64_t stream, int64_t first_document, int heldout);
/* sufficient statistics /= divisor (number_of_samples - burn_in_samples), on the context's stream. */
int pylda_hybrid_scale_sstats(pylda_ctx* ctx, double divisor);

/* Test hook: Philox4x32-10 on the device.  counter_key holds n records of six words (counter 0..3, key 0..1),
 * out receives n blocks of four words. */
int pylda_test_philox(pylda_ctx* ctx, int64_t n, const uint32_t* counter_key, uint32_t* out);

/* The collapsed Gibbs engine (monte_carlo.py of the reference) as a document-parallel chain with block-synchronous
 * counts.  State of a corpus: a topic per token (CSR order, a term's copies back to back), n_dk
 * (exact doubles in the gamma buffer: pylda_get_gamma returns them), the word-topic counts and n_k (int32; a corpus of
 * 2^31 tokens or more is PYLDA_ERR_INVALID).  The state belongs to the CORPUS: two corpora of one context are two chains.
 * It needs neither set_eta nor set_alpha; K <= 1024.  Random numbers as the hybrid E-step's (Philox4x32-10): a draw is a
 * function of (seed, stream, global document index, token position).
 *
 * pylda_gibbs_init: every token's topic uniformly (stream 0), then the three count tables.  The first call on a corpus
 * allocates its buffers (4 bytes per table entry, 8 per token); PYLDA_ERR_OOM when they do not fit. */
int pylda_gibbs_init(pylda_ctx* ctx, pylda_corpus* corpus, uint64_t seed, int64_t first_document);
/* One sweep, enqueued on the context's stream: `blocks` rounds; round g samples the documents whose global index
 * (first_document + local index) is g modulo blocks, one wavefront each, against the word-topic counts and n_k of the
 * round's start plus the document's own changes, then adds the block's changes to them.  Rounds without documents launch
 * nothing.  blocks >= the number of documents is the sequential sampler; blocks = 1 freezes the counts for the sweep.
 *   alpha_k (K), beta_v (V), beta_sum   the priors and sum_v beta_v as the caller computed it
 *   stream                              < 2^32 (the Python class: the iteration counter, from 1) */
int pylda_gibbs_sweep(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v, double beta_sum,
                      int64_t blocks, uint64_t seed, uint64_t stream, int64_t first_document);
/* log_posterior (monte_carlo.py:217-256) of the corpus' counts under (alpha_k, beta_v), reduced in a fixed order: the
 * same state and priors give the same bits on every call.  Waits for the stream. */
int pylda_gibbs_log_posterior(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v, double* out);
/* Read-backs (any pointer may be NULL): n_kv (K, V) row-major, n_k (K), the tokens' topics (token total of
 * pylda_corpus_info).  Waits for the stream. */
int pylda_gibbs_get_counts(pylda_ctx* ctx, pylda_corpus* corpus, int32_t* n_kv, int32_t* n_k, int32_t* topics);
/* Restore a state (snapshots; shards of one corpus that start a round from the whole corpus' table): NULL keeps what the
 * corpus holds; n_dk is counted again from `topics` when they are given.  n_kv and n_k are taken as they are - they need
 * not be the counts of this corpus' own tokens.  A corpus without a state needs all three. */
int pylda_gibbs_set_state(pylda_ctx* ctx, pylda_corpus* corpus, const int32_t* n_kv, const int32_t* n_k, const int32_t* topics);

/* The collapsed Gibbs engine sharded over several ranks.  Every rank holds a contiguous range of
 * the documents (first_document: the documents before it) and a full replica of the word-topic counts and n_k.  Round g of
 * a sweep on every rank, in stream order: pylda_gibbs_round_sample (the sampler of pylda_gibbs_sweep on the rank's
 * documents of block g, then one move record per token of the block into `send`), an all-gather of the ranks' `send`
 * segments into `recv` (the caller's: torch.distributed, RCCL, MPI ...), pylda_gibbs_round_apply (the records of all
 * ranks, this one's included, into the replica).  The replicas receive exactly the integer updates the one-GPU table
 * receives: after every round they equal it and each other, and every token's topic is the one-GPU run's.
 *   record    uint64: word << 32 | topic before the draw << 16 | topic after it; a record whose two topics are equal
 *             changes nothing (tokens that stayed, and the zeroed padding)
 *   segment   the block's documents in local order, a document's tokens in the order of its state words; every rank
 *             sends capacity[g] records in round g, its own first, zeros behind them
 * Before the first sweep the replicas must hold the counts of the WHOLE corpus: after pylda_gibbs_init on every rank, sum
 * the tables and n_k over the ranks (pylda_gibbs_table_device).
 *
 * pylda_gibbs_round_tokens: tokens[g], g < blocks: the tokens of this corpus in round g's block (host arithmetic on the
 * corpus' CSR; no kernel).  capacity[g] is the maximum of tokens[g] over the ranks. */
int pylda_gibbs_round_tokens(pylda_ctx* ctx, pylda_corpus* corpus, int64_t blocks, int64_t first_document, int64_t* tokens);
/* Allocates the exchange's buffers of a corpus - max(capacity) records to send, world x max(capacity) to receive, D
 * record offsets - and returns the two device pointers.  A second call replaces the first (the pointers of the first
 * die); the buffers are freed with the corpus.  Waits for the stream.
 * PYLDA_ERR_INVALID: world < 1, rank outside [0, world), blocks < 1 or > 2^24 (more rounds than the corpus has documents
 * are the chain of blocks = the global document count: pass that), a capacity[g] below pylda_gibbs_round_tokens' figure
 * for this corpus.  PYLDA_ERR_OOM: the buffers do not fit in the free device memory (the buffers of the plan before
 * counted as free).  A call refused with either code leaves the plan before in place and usable. */
int pylda_gibbs_exchange_prepare(pylda_ctx* ctx, pylda_corpus* corpus, int64_t blocks, int64_t first_document, int world, int rank,
                                 const int64_t* capacity, void** send, void** recv);
/* Round `round` of a sweep, first half, enqueued: samples the block, writes its records to send[0, tokens[round]) and
 * zeros up to capacity[round].  A round whose block is empty on this rank only zeroes.  Arguments and checks as
 * pylda_gibbs_sweep; round = global document index modulo blocks, so blocks >= the global document count numbers the
 * rounds by global document, as pylda_gibbs_sweep does.
 * PYLDA_ERR_STATE: no pylda_gibbs_exchange_prepare before, or one for another (blocks, first_document); round outside
 * [0, blocks). */
int pylda_gibbs_round_sample(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v, double beta_sum,
                             int64_t blocks, int64_t round, uint64_t seed, uint64_t stream, int64_t first_document);
/* Round `round`, second half, enqueued: applies the world x capacity[round] records at `recv` to the word-topic counts
 * and n_k.  A record that names a word >= V or a topic >= K is skipped.  PYLDA_ERR_STATE as above. */
int pylda_gibbs_round_apply(pylda_ctx* ctx, pylda_corpus* corpus, int64_t round);
/* The corpus' word-topic counts (word-major int32, *table_elements = V x pylda_table_stride) and n_k (K int32) on the
 * device, for the one exchange after pylda_gibbs_init; any pointer may be NULL.  PYLDA_ERR_STATE without a Gibbs state. */
int pylda_gibbs_table_device(pylda_ctx* ctx, pylda_corpus* corpus, void** table, int64_t* table_elements, void** n_k);
/* pylda_gibbs_log_posterior in two parts: out[0] the documents' part with its D-scaled scalar term (sum it over the
 * ranks), out[1] the words' and n_k's part with its K-scaled scalar term (of the replica: the same on every rank).
 * Each in a fixed order.  Waits for the stream. */
int pylda_gibbs_log_posterior_parts(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v, double* out);

/* Held-out fold-in for the collapsed Gibbs engine: topic proportions and a likelihood for
 * documents the model was not trained on, with the word-topic counts frozen.  Frozen counts make the documents
 * independent chains: one wavefront per document, all sweeps in one launch, no blocks and no apply pass.
 *
 * pylda_foldin_set_model: the predictive table P[w][k] = (n_kv[k][w] + beta_w) / (n_k[k] + beta_sum) of the CONTEXT,
 * replaced by the next call and freed with the context.  trained != NULL takes the counts from that corpus' Gibbs state
 * on the device (no read-back; PYLDA_ERR_STATE when it has none); otherwise n_kv (K, V) row-major and n_k (K) from the
 * host.  beta_v (V) and beta_sum as the caller computed it.  The first call allocates the table (8 bytes per table entry;
 * PYLDA_ERR_OOM when it does not fit).  Waits for the stream.  K <= 1024. */
int pylda_foldin_set_model(pylda_ctx* ctx, pylda_corpus* trained, const int32_t* n_kv, const int32_t* n_k,
                           const double* beta_v, double beta_sum);
/* Folds the documents of `heldout` into the model: a uniformly random topic per token, number_of_samples sweeps with
 * weight (n_dk + alpha_k) P[w][k], the document's topic counts summed after each sweep from burn_in_samples on.  Fills
 * the corpus' gamma buffer (pylda_get_gamma): alpha_k + the mean kept count; the per-document slot pylda_get_doc_values
 * returns as doc_words_ll: sum over the document's distinct terms of c_n log(sum_k theta_k P[w_n][k]), theta = gamma /
 * sum(gamma) - the plug-in estimate, theta from the same tokens - with iters = number_of_samples and doc_ll = 0; and
 * *words_log_likelihood, their sum in a fixed order (the same input gives the same bits).  Waits for the stream once.
 *   seed, stream, first_document   as pylda_gibbs_sweep: a draw is a function of (seed, stream, global document index,
 *                                  sweep, token position); stream < 2^32 (the Python class: 2^31 + the call's number)
 * PYLDA_ERR_INVALID: burn_in_samples >= number_of_samples, number_of_samples < 1 or > 65534, K > 1024, stream >= 2^32.
 * PYLDA_ERR_STATE: no model; or `heldout` holds a Gibbs training state (its n_dk and topics live in the buffers this call
 * fills: a training corpus is never touched - fold in a corpus of its own).  The first call on a corpus allocates its
 * token offsets and state words (8 bytes per token, as the hybrid E-step); PYLDA_ERR_OOM when they do not fit. */
int pylda_foldin(pylda_ctx* ctx, pylda_corpus* heldout, const double* alpha_k, int number_of_samples, int burn_in_samples,
                 uint64_t seed, uint64_t stream, int64_t first_document, double* words_log_likelihood);

/* The collapsed variational Bayes engine in its zero-order form (CVB0): a token carries a
 * distribution over the topics in place of one sampled topic, the counts are expected counts, and an update is add,
 * multiply and divide - deterministic after the start.  The state lives in the corpus: a row of K doubles per distinct
 * (document, term) slot of the CSR (the copies of a term in a document share it), the word-major table of expected
 * word-topic counts, n_k, and N_dk in the gamma buffer (pylda_get_gamma).  All of it is fp64: 8 bytes x ldk per slot
 * (ldk = pylda_table_stride) and per word; PYLDA_ERR_OOM, asked before anything is allocated, when it does not fit one
 * GPU.  K <= 1024 (PYLDA_ERR_INVALID).  A corpus that holds a collapsed Gibbs state is refused (PYLDA_ERR_STATE).
 *
 * pylda_cvb0_init: every copy of a slot draws a uniform topic exactly as pylda_gibbs_init does (seed, stream 0,
 * first_document: the corpus' first document's index in the whole collection); the slot's row is the histogram of its
 * copies divided by their number; the table, n_k and N_dk are the integer histograms.  Enqueued. */
int pylda_cvb0_init(pylda_ctx* ctx, pylda_corpus* corpus, uint64_t seed, int64_t first_document);
/* One sweep, enqueued (no host wait; the first call for a (blocks, first_document) pair builds the blocks' postings on
 * the host and waits for the stream once).  Block b = the documents whose global index is b modulo `blocks`; a round per
 * block that holds a document: the update (one wavefront per document against the table and n_k of the round's start),
 * the apply pass (the round's changes into the table, summed in a fixed order: no floating-point atomics) and n_k
 * recomputed from the table.  alpha_k (K), beta_v (V), beta_sum as the caller computed it.  The same state gives the same
 * bits.  PYLDA_ERR_INVALID: blocks < 1, a prior missing.  PYLDA_ERR_STATE: no state.  PYLDA_ERR_OOM: the largest block's
 * delta rows (8 bytes x ldk per slot of the block) do not fit. */
int pylda_cvb0_sweep(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v, double beta_sum,
                     int64_t blocks, int64_t first_document);
/* The training plug-in log-likelihood sum_d sum_q c_q log(sum_k theta_dk P[w_q][k]), theta_d = (N_dk + alpha) / sum,
 * P[w][k] = (T[w][k] + beta_w) / (n_k[k] + beta_sum), and *change = the sum over the slots of c |new row - old row| of
 * every document's last update (0 before the first sweep); both totals in a fixed order.  The per-document likelihoods
 * go into the slot pylda_get_doc_values returns as doc_words_ll.  Either output may be NULL.  Waits for the stream once.
 * PYLDA_ERR_STATE: no state. */
int pylda_cvb0_log_likelihood(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v,
                              double beta_sum, double* log_likelihood, double* change);
/* The state out and in: n_kv (K, V) row-major, n_k (K), n_dk (D, K), g (nnz, K) - the slots' rows in CSR order - all
 * doubles; any pointer may be NULL.  pylda_cvb0_set_state takes what it is given as given (n_k is not recomputed), so a
 * restored run continues bit for bit; a corpus without a state needs all four (PYLDA_ERR_STATE otherwise).  Both wait for
 * the stream.  pylda_cvb0_get_state: PYLDA_ERR_STATE without a state. */
int pylda_cvb0_get_state(pylda_ctx* ctx, pylda_corpus* corpus, double* n_kv, double* n_k, double* n_dk, double* g);
int pylda_cvb0_set_state(pylda_ctx* ctx, pylda_corpus* corpus, const double* n_kv, const double* n_k, const double* n_dk,
                         const double* g);
/* Held-out fold-in against the context's predictive table - pylda_set_eta(n_kv + beta) and pylda_completion_set_model
 * build it - with the table frozen: one wavefront per document, `sweeps` sweeps in one launch, per slot
 * w[k] = ((nd[k] - g[k]) + alpha[k]) P[w][k], normalised as in a training sweep.  The start as pylda_cvb0_init, with the
 * caller's stream.  Fills the gamma buffer (alpha + nd), the per-document likelihoods (doc_words_ll of
 * pylda_get_doc_values; iters = sweeps, doc_ll = 0) and *words_log_likelihood exactly as pylda_foldin does.  Waits for
 * the stream once.  PYLDA_ERR_INVALID: sweeps < 1, stream >= 2^32, K > 1024.  PYLDA_ERR_STATE: no predictive table; or
 * `heldout` holds a training state.  The first call on a corpus allocates its rows (8 bytes x ldk per slot);
 * PYLDA_ERR_OOM when they do not fit. */
int pylda_cvb0_foldin(pylda_ctx* ctx, pylda_corpus* heldout, const double* alpha_k, int sweeps, uint64_t seed, uint64_t stream,
                      int64_t first_document, double* words_log_likelihood);
/* Test hook, pure host code (ctx-free): the postings pylda_cvb0_sweep builds for (blocks, first_document) over a CSR of
 * `documents` documents.  counts (5): rounds, segments, runs, the largest round's postings and segments.  Every other
 * output may be NULL: rounds (rounds x 6: block, first local document, documents, and the ends of the round's postings,
 * segments and runs), post_slot (nnz: CSR slots by (block, word, document)), slot_place (nnz: a slot's place among its
 * round's postings), seg_begin (segments + 1), run_word (runs), run_seg (runs + 1).  A segment holds 256 postings of one
 * word at most. */
int pylda_test_cvb0_postings(int64_t documents, const int64_t* doc_ptr, const int32_t* term_id, int64_t blocks,
                             int64_t first_document, int64_t* counts, int64_t* rounds, int64_t* post_slot, int64_t* slot_place,
                             int64_t* seg_begin, int32_t* run_word, int64_t* run_seg);

/* Stochastic collapsed variational Bayes (SCVB0: Foulds et al. 2013): the collapsed variational
 * engine in minibatches, without its row per (document, term) slot.  The state in the corpus is the word-major table of
 * expected word-topic counts, n_k, and N_dk in the gamma buffer: 8 bytes x ldk per word and 8 bytes x K per document,
 * plus one minibatch's delta rows; PYLDA_ERR_OOM, asked before anything is allocated, when it does not fit.  K <= 1024.
 * A corpus holds one training state: these entries refuse a corpus with a CVB0 or a collapsed Gibbs state, and
 * pylda_cvb0_init / _sweep / _get_state / _set_state / _foldin refuse one with this state (PYLDA_ERR_STATE).
 * pylda_cvb0_log_likelihood serves both; after a step *change is the sum over the documents of sum_k |N_dk after - before|
 * of every document's last visit.
 *
 * pylda_scvb_init: the start of pylda_cvb0_init without the rows (same seed, same table, n_k and N_dk).  Enqueued. */
int pylda_scvb_init(pylda_ctx* ctx, pylda_corpus* corpus, uint64_t seed, int64_t first_document);
/* One minibatch step, enqueued (no host wait; the first call for a (batches, first_document) pair builds the blocks'
 * postings on the host and waits for the stream once).  The minibatch is block `block` of `batches`: the documents whose
 * global index is `block` modulo `batches`.  Every document of it runs `passes` (burn_in + 1: 1 to 16) passes over its
 * slots against the table and n_k of the step's start, pass p with the step size rho_theta[p]; one_minus[p] is the
 * caller's 1 - rho_theta[p].  Then table = keep * table + gain * (the block's expected counts per word, summed in a fixed
 * order) over every word, and n_k is recomputed from the table.  keep = 1 - rho_phi and gain = rho_phi * (the corpus'
 * tokens / the block's), as the caller computed them: the device calls no power function (a slot's (1 - rho_theta) ** c is
 * formed by adds and multiplies in a fixed order).  A block without tokens
 * changes nothing.  The same state gives the same bits.  PYLDA_ERR_INVALID: batches < 1, block outside [0, batches),
 * passes outside [1, 16], a prior or a step size missing, keep outside [0, 1), gain not positive and finite, a rho_theta
 * outside (0, 1].  PYLDA_ERR_STATE: no state.  PYLDA_ERR_OOM: the largest block's delta rows do not fit. */
int pylda_scvb_step(pylda_ctx* ctx, pylda_corpus* corpus, int64_t block, int64_t batches, int64_t first_document,
                    const double* alpha_k, const double* beta_v, double beta_sum, double keep, double gain, int passes,
                    const double* rho_theta, const double* one_minus);
/* The state out and in: n_kv (K, V) row-major, n_k (K), n_dk (D, K), all doubles; any pointer may be NULL.  doc_change (D,
 * out only): sum_k |N_dk after - before| of every document's last visit, 0 before it - what the likelihood's *change sums.
 * pylda_scvb_set_state takes what it is given as given (n_k is not recomputed), so a restored run continues bit for bit; a
 * corpus without a state needs all three (PYLDA_ERR_STATE otherwise).  Both wait for the stream. */
int pylda_scvb_get_state(pylda_ctx* ctx, pylda_corpus* corpus, double* n_kv, double* n_k, double* n_dk, double* doc_change);
int pylda_scvb_set_state(pylda_ctx* ctx, pylda_corpus* corpus, const double* n_kv, const double* n_k, const double* n_dk);

/* Document-completion held-out likelihood: theta is fitted on one half of every test document - by
 * a held-out pylda_estep, pylda_hybrid_estep or pylda_foldin over a corpus of the observed halves - and the OTHER half is
 * scored: sum over the held terms of c_n log(sum_k theta_k P[w_n][k]), theta = gamma / sum(gamma).  The split itself is the
 * host's (pylda_amd.corpus.split_for_completion: token position p of a document is observed when p is even, held when odd).
 *
 * pylda_completion_set_model: the predictive table P[w][k] = eta[k][w] / sum_v eta[k][v] - the posterior mean of topic k -
 * from the context's current device eta (PYLDA_ERR_STATE when it has none), enqueued.  The table belongs to the CONTEXT
 * and shares its storage with pylda_foldin_set_model's: each call replaces what the other built, and after this one
 * pylda_foldin needs its model set again.  The first call allocates the table (8 bytes per table entry; PYLDA_ERR_OOM
 * when it does not fit).  Row sums in a fixed order: the same eta gives the same bits.  K <= 1024. */
int pylda_completion_set_model(pylda_ctx* ctx);
/* Scores the documents of `held` against the context's predictive table - the one pylda_completion_set_model built, or,
 * for a collapsed Gibbs model, the one pylda_foldin_set_model built from the counts.  Document d's gamma is row d of
 * `observed`'s device gamma buffer (what a held-out E-step or a fold-in left there) when that corpus is given; otherwise
 * row d of gamma_dk (D, K) from the host, uploaded into `held`'s own gamma buffer.  Fills the held corpus' per-document
 * slot pylda_get_doc_values returns as doc_words_ll, with doc_ll = 0 and iters = 0; *held_log_likelihood is their sum and
 * *held_tokens the held corpus' tokens, both from one reduction in a fixed order (the same input gives the same bits,
 * however the documents are dealt to corpora).  An empty held document scores exactly 0.  Per-word perplexity is
 * exp(-held_log_likelihood / held_tokens).  Waits for the stream once.
 * PYLDA_ERR_STATE: no predictive table; `observed` has had no E-step or fold-in; `observed` or `held` holds a Gibbs
 * training state (n_dk lives in its gamma buffer).
 * PYLDA_ERR_INVALID: the two corpora differ in their number of documents; both or neither of `observed` and gamma_dk
 * given; K > 1024; a gamma row whose sum is not positive and finite (such a document scores 0; the message counts them). */
int pylda_completion_score(pylda_ctx* ctx, pylda_corpus* observed, pylda_corpus* held, const double* gamma_dk,
                           double* held_log_likelihood, int64_t* held_tokens);

/* Left-to-right held-out likelihood (Wallach, Murray, Salakhutdinov & Mimno 2009, Algorithm 3): an
 * estimate of log p(w | Phi, alpha) of every document of `heldout`, theta integrated out, from the context's predictive
 * table - the one pylda_completion_set_model built from eta or the one pylda_foldin_set_model built from the counts - and
 * alpha_k (K) alone: the same quantity for every engine.  A document's tokens are its CSR terms in order, a term's copies
 * back to back.  Per document `particles` independent chains; for token n in order a chain - if `resample` - draws the
 * topics of tokens 0 .. n - 1 again, one after the other, from (n_dk + alpha_k) P[w][k] with the token itself left out,
 * records p_n = sum_k (n_dk + alpha_k) P[w_n][k] / (n + sum alpha), and draws token n's topic from the same weights.  The
 * document's estimate is sum_n log(mean over the particles of p_n).  resample = 0 is the sequential sampler (N_d steps per
 * particle), resample = 1 Algorithm 3 (N_d (N_d + 1) / 2 steps).
 *   seed, stream, first_document   a draw is a function of (seed, stream + particle, global document index, n, n'): the call
 *                                  takes `particles` consecutive streams (the Python classes: (3 << 30) + 256 calls)
 *   step_budget                    token-steps (all particles counted) of one kernel launch at most, so that a launch ends
 *                                  in bounded time: consecutive documents share a launch up to it, a document over it runs
 *                                  as a launch of its own; 0: the library's default.  The cut never changes a bit.
 * Fills the per-document slot pylda_get_doc_values returns as doc_words_ll, with doc_ll = 0 and iters = particles;
 * *log_likelihood is their sum and *tokens the corpus' tokens, both from one reduction in a fixed order.  The same input
 * gives the same bits, however the documents are dealt to corpora, launches or chunks.  An empty document scores exactly 0.
 * The topics (2 bytes) and p (8 bytes) of every (token, particle) live in a scratch buffer the context keeps for the next
 * call; where they do not fit the free device memory the documents run in several chunks (option "ltr_chunk_tokens").
 * Waits for the stream once (the first call on a corpus also reads its term counts back).
 * PYLDA_ERR_INVALID: particles < 1 or > 256; K > 1024; stream + particles > 2^32; resample not 0 or 1; step_budget < 0.
 * PYLDA_ERR_STATE: no predictive table; `heldout` holds a Gibbs training state.
 * PYLDA_ERR_OOM: one document's scratch does not fit. */
int pylda_left_to_right(pylda_ctx* ctx, pylda_corpus* heldout, const double* alpha_k, int particles, int resample,
                        uint64_t seed, uint64_t stream, int64_t first_document, int64_t step_budget,
                        double* log_likelihood, int64_t* tokens);
/* Test hook: the scratch of the last pylda_left_to_right call, which must have been on `heldout` with `particles`
 * particles: z_out (tokens x particles uint16: document d's block starts at (its first token) x particles and holds
 * particle r's N_d topics at r N_d) and p_out (tokens x particles doubles: token t's particles side by side); either may
 * be NULL.  PYLDA_ERR_STATE: no such call, or it ran in several chunks (the buffers hold the last chunk only). */
int pylda_test_left_to_right_state(pylda_ctx* ctx, pylda_corpus* heldout, int particles, uint16_t* z_out, double* p_out);

/* Topic coherence: what the topics are, and whether their top words occur together.  The device
 * produces integers and copies of table entries only; the logs and sums over them are the host's (pylda_amd/coherence.py).
 *
 * pylda_top_words: the first M entries of every row of a (K, V) row-major table of finite doubles under the total order
 * "larger value first, among equal values the smaller word id first": ids_km (K, M) and values_km (K, M), the table's own
 * bits, in rank order.  table_kv from the host is uploaded to a scratch buffer of the call (PYLDA_ERR_OOM when it does not
 * fit); NULL ranks the context's device eta in place - the same order as the topics' posterior means - and is
 * PYLDA_ERR_STATE when the context holds none.  One pass over the table; the result is a set under a total order: the
 * same table gives the same bits.  Behaviour on NaN or inf is not specified.  Waits for the stream.
 * PYLDA_ERR_INVALID: M < 1, M > 64, M > V, a NULL output. */
int pylda_top_words(pylda_ctx* ctx, const double* table_kv /* host K x V; NULL: the context's eta */,
                    int M, int32_t* ids_km, double* values_km);
/* For the M words ids_km[k] of every topic k (host, (K, M); any ids in [0, V): shared between topics or repeated inside
 * one), the documents of `reference` that contain them: doc_freq_km[k][m] = D(v_m), the documents that contain the word,
 * and co_kmm[k][m][l] = D(v_m, v_l), those that contain both - symmetric, its diagonal doc_freq.  Term counts are ignored;
 * an empty document contains nothing.  Only the corpus' CSR is read: a corpus in any state, a Gibbs state included.  One
 * bitmap of the documents per distinct word, at most a quarter of the free device memory; a corpus whose bitmaps do not fit
 * is walked in chunks of documents (option "coherence_chunk_docs"), PYLDA_ERR_OOM when not even 64 documents fit.  Exact
 * integers, whatever the chunk.  Every buffer is the call's own and freed before it returns.  Waits for the stream.  With
 * profiling enabled pylda_kernel_time returns this call's mark pass (and pylda_top_words' selection) as its document
 * kernels and the pair pass as its statistics pass.
 * PYLDA_ERR_INVALID: M < 1, M > 64, an id outside [0, V), a corpus without documents or of another context, a NULL
 * pointer.  Every error is returned before anything is launched. */
int pylda_codocument_counts(pylda_ctx* ctx, pylda_corpus* reference, int M, const int32_t* ids_km /* host */,
                            int64_t* doc_freq_km, int64_t* co_kmm);

/* Nearest documents by topic mixture: for every query row the first N rows of a base by their
 * score, the Q x D score matrix never stored.  Rows are K doubles (the context's K).
 *   transform of a row g   0: the row as given (any finite doubles); 1: theta_k = g_k / s with
 *                          s = (((+0.0 + g_0) + g_1) + ...) in k order, one s per row; 2: sqrt(theta_k)
 *   score                  s[q][d] = (((+0.0 + a_0 b_0) + a_1 b_1) + ...) over k = 0 .. K - 1 in that order, every multiply
 *                          and every add rounded once: no FMA, the sum never split.  numpy's
 *                          acc = acc + a[:, k, None] * b[None, :, k] gives the same bits
 *   order                  larger score first, among equal scores the smaller document index first: a total order, so the
 *                          answer depends on neither tiling nor launch shape (option "similarity_doc_slices")
 * With transform 2 on both sides the score is the Bhattacharyya coefficient (Hellinger distance sqrt(max(0, 1 - score)),
 * left to the host); with transform 1 on the base and one-hot queries under transform 0 it is theta_dk itself.
 *
 * pylda_similarity_set_base: uploads rows_dk (D, K), transforms it on the device and keeps it on the context: at most a
 * quarter of the device memory free at the time (PYLDA_ERR_OOM; the base it was to replace is gone then).  A later call
 * replaces the base; it is freed with the context.  Waits for the stream.
 * PYLDA_ERR_INVALID: D < 1, D >= 2^31, a transform outside 0 .. 2, NULL rows, and - checked on the host before anything
 * is launched, the message counting the rows - under transform 0 a row with a non-finite entry, under 1 and 2 a row with
 * a negative entry or whose s is not positive and finite. */
int pylda_similarity_set_base(pylda_ctx* ctx, int64_t D, const double* rows_dk /* host */, int transform);
/* ids_qn (Q, N) and scores_qn (Q, N): for query q the first N documents of the base in the order above, leaving out
 * document self_ids[q] (-1: none; self_ids NULL: none for any query).  Fewer than N candidates: the trailing entries are
 * id -1 and score -infinity.  The queries, the slices' lists and the results are buffers of the call.  Waits for the
 * stream once.  With profiling enabled pylda_kernel_time returns the transform and the top-N pass (of both entry points)
 * as the document kernels and the merge of the slices' lists as the statistics pass.
 * PYLDA_ERR_STATE: no base.  PYLDA_ERR_INVALID: Q < 1, N < 1, N > 64, a transform outside 0 .. 2, a self id outside
 * [-1, D), a NULL pointer other than self_ids, a bad row as above.  Every error is returned before anything is launched. */
int pylda_similar_documents(pylda_ctx* ctx, int64_t Q, const double* rows_qk /* host */, int transform, int N,
                            const int32_t* self_ids /* Q or NULL */, int32_t* ids_qn, double* scores_qn);

/* Topic distances between two models: out_ab (Ka, Kb), for every row i of a (Ka, V) and every row
 * j of b (Kb, V) - host, row-major, V the context's, Ka and Kb any counts in 1 .. 2^15 - one number between the two rows as
 * distributions over the words.
 *   transform of a row t   p_v = t_v / s, one s per row: lane l of 64 adds the entries with v = l (mod 64) in ascending v
 *                          from +0.0, then the 64 partials go through the tree x_l = x_l + x_(l xor m), m = 32, 16 .. 1
 *   metric 0, "hellinger"  the Bhattacharyya coefficient sum_v sqrt(p_v) sqrt(q_v), the roots rounded once each (the
 *                          Hellinger distance sqrt(max(0, 1 - out)) is left to the host)
 *   metric 1, "jensen_shannon"  in nats: 0.5 sum_v p (lp - lm) + q (lq - lm) with lp = log(p) (0 where p is 0),
 *                          m = 0.5 (p + q), lm = log(m); the term is exactly 0 where m is 0, and the half is applied once,
 *                          to the finished sum (exact).  One log per (pair, word); a row against itself gives exactly 0,
 *                          rows with disjoint supports ln 2
 *   sum over v             V is cut into segments of 1024 words.  A segment's sum starts at +0.0 and adds its terms in
 *                          ascending v; the segments' sums are added in ascending order from +0.0.  Every multiply and
 *                          every add is rounded once: no FMA, no sum split over lanes.  The result depends on neither the
 *                          tiling nor the launch shape (option "topic_distance_segment_groups")
 * a_kv NULL: the context's eta, Ka = K.  b_kv NULL: a against itself, Kb = Ka; only the tiles on or above the diagonal
 * are computed and mirrored.  Both terms commute in (p, q), so a against itself - as NULL or passed twice - is symmetric
 * bit for bit.  The transformed tables, the segments' sums and the result are buffers of the call, at most three quarters
 * of the device memory free at the time (PYLDA_ERR_OOM), freed before it returns.  Waits for the stream.  With profiling
 * enabled pylda_kernel_time returns the transform as the document kernels and the pair sums as the statistics pass.
 * PYLDA_ERR_STATE: a_kv NULL and eta was never set.  PYLDA_ERR_INVALID: a metric outside 0 .. 1, Ka or Kb outside
 * 1 .. 2^15, Ka != K with a_kv NULL, Kb != Ka with b_kv NULL, a NULL out_ab, and - checked on the host, the message
 * counting the rows - a row with a negative or non-finite entry or whose s is not positive and finite.  Every error is
 * returned before anything is launched. */
int pylda_topic_distances(pylda_ctx* ctx, const double* a_kv /* host; NULL: the context's eta, Ka = K */, int Ka,
                          const double* b_kv /* host; NULL: a against itself */, int Kb, int metric, double* out_ab);

/* Test hook: out[i] = exp(digamma(x[i]) - c), the fused form the inner loop uses. */
int pylda_test_expdigamma(pylda_ctx* ctx, int64_t n, const double* x, double c, double* out);

/* Test hook: out[i] = one call form of the device special functions (special_device.h) at x[i], one thread per element,
 * c a kernel argument (wave-uniform, as the E-step kernels' psi(sum gamma) is).  form:
 *   0 digamma   1 lgamma_pos   2 trigamma   3 exp_shallow (c ignored)   4 rcp_newton (c ignored)
 *   5 exp_digamma_minus(x, c)            exp(psi(x) - c), coefficients as literals
 *   6 exp_digamma_minus_levels(x, c)     the level-ordered form, both coefficient tables fetched inside
 *   7 ... (x, c, A)                      the first table fetched by the caller (estep_compact.h)
 *   8 ... <true>(x, c, A, &B)            both tables fetched by the caller ahead of a barrier (estep_quad.h,
 *                                        estep_quilt.h, estep_compact.h)
 * Forms 6-8 are one instruction sequence and agree bit for bit.  PYLDA_ERR_INVALID: any other form. */
int pylda_test_special_forms(pylda_ctx* ctx, int64_t n, const double* x, double c, int form, double* out);

/* Test hook: what every E-step prepares from the context's eta before its document kernels run
 * (compute_dirichlet_expectation, inferencer.py:15-18, called at variational_bayes.py:152; the held-out normaliser of
 * :155), by the production launches with the held-out normaliser on, read back to the host:
 *   psi_rowsum_k       K          psi(sum_v eta[k][v])
 *   elog_vldk          V x ldk    E_log_eta[k][w] - shift_v[w], word-major (ldk: pylda_table_stride)
 *   expElog_vldk       V x ldk    exp of it: in [0, 1], the largest of a row exactly 1
 *   expElog_elog_vldk  V x ldk    the product of the two, +0 where expElog is 0
 *   shift_v            V          max_k E_log_eta[k][w]
 *   topic_lse_k        K          logsumexp_v E_log_eta[k][v]
 *   alpha_sgn_k        K          the context's alpha, its sign bit set where the topic may never count as dead: where
 *                                 exp(psi(alpha_k) - psi(sum alpha + 8)) is not below 1e-33 (the live-topic hand-over)
 * The V x ldk arrays come back whole: columns K .. ldk-1 are the zero padding the dense kernels read.  Any pointer may be
 * NULL (its array is not copied; alpha_sgn is then not computed either).  *path_out: 1 when the one-kernel path filled the
 * tables, 2 for the two passes (option "prepare_path").  Waits for the stream.
 * PYLDA_ERR_STATE: eta was never set, or alpha_sgn_k is asked for and alpha was never set. */
int pylda_test_tables(pylda_ctx* ctx, double* psi_rowsum_k, double* elog_vldk, double* expElog_vldk,
                      double* expElog_elog_vldk, double* shift_v, double* topic_lse_k, double* alpha_sgn_k, int* path_out);

/* Test hook: the sufficient-statistics pass (variational_bayes.py:207) of a corpus on GIVEN inputs instead of what the
 * document kernels of an E-step leave behind:
 *   t_dldk          D x ldk    the documents' rows of t, padding columns K .. ldk-1 included (ldk: pylda_table_stride)
 *   r_nnz           nnz        r of every (document, term) pair, in the order of the term_id array handed to
 *                              pylda_corpus_create (the device corpus keeps that order)
 *   live_n_d        D          NULL, or per document the entries of its list of live topics (0 .. 60), -1: no list
 *   live_topic_d60  D x 60     the listed topics (each below K), entries 0 .. live_n - 1 of a row
 *   live_t_d60      D x 60     their t
 * In this order: the tables of the context's eta by the production launch; what pylda_estep does in front of its
 * document kernels - the launch plan, alpha's say on the hand-over, the packed launch slots, the hand-over buffers - and
 * the postings exactly as the first training E-step builds them (every option that shapes them - gather_rows,
 * gather_blocks, gather_sweep, gather_round_mb, wide_postings, gather_live, sweep_xcd, sweep_sub - applies; postings the
 * corpus already has are kept; pylda_estep derives from its threshold whether the plan avoids the kernels with the
 * fixed-point stop test - this entry has no threshold and keeps what the context's last E-step decided, "does not" in a
 * fresh context); t and r into the buffers the document kernels write; the lists, packed in the layout the live-topic
 * kernel writes; NaN (all bits set) into everything the pass must write - the statistics, padding columns included, the
 * partial rows, the entropy partials and their sum - so that what a launch leaves unwritten cannot pass for a result; the
 * production statistics pass; the sum of its entropy partials by the job pylda_estep uses, returned in *entropy_out
 * (sum_wk (B log B)[w][k] sum_d r_dw t_d[k]).  The statistics are then read with pylda_get_sstats.  No kernel and no
 * decision of the planner is duplicated or bypassed, with ONE exception: when lists are passed and no launch class of the
 * corpus hands documents to the live-topic kernel (K <= 64, table strides above 512, option compact = 0), the entry
 * allocates the per-document hand-over buffers itself and lets the postings be built as for a corpus that hands over, so
 * that the pass over the lists can be tested at every table stride; the option gather_live and the pass' LDS limit (four
 * rows of ldk doubles in 64 KiB) still decide.  Where the pass reads lists and live_n_d is NULL every document adds its
 * row.  Waits for the stream.
 * PYLDA_ERR_STATE: eta was never set, or a document is listed and the pass of this corpus reads rows ("gather_live" 0);
 * PYLDA_ERR_INVALID: a list length outside -1 .. 60, a listed topic >= K. */
int pylda_test_statistics(pylda_ctx* ctx, pylda_corpus* corpus, const double* t_dldk, const double* r_nnz,
                          const int32_t* live_n_d, const uint16_t* live_topic_d60, const double* live_t_d60,
                          double* entropy_out);

/* Test hook: the terms of the collapsed Gibbs log posterior (monte_carlo.py:217-256) instead of their sum only.  Runs
 * exactly the launches of pylda_gibbs_log_posterior and pylda_gibbs_log_posterior_parts on the corpus' state - the
 * document kernel, the word kernel, then BOTH sum kernels - and reads back what they leave on the device:
 *   doc_terms   D   sum_k lnG(n_dk[d][k] + alpha_k) - lnG(N_d + sum alpha), per document (nothing is written at D = 0)
 *   word_terms  V   sum_k lnG(n_kv[k][v] + beta_v), per word
 *   sums        3   [0] sum_d doc_terms + sum_v word_terms - sum_k lnG(n_k + sum beta), as pylda_gibbs_log_posterior's
 *                   kernel sums it; [1] sum_d doc_terms and [2] sum_v word_terms - sum_k lnG(n_k + sum beta), as
 *                   pylda_gibbs_log_posterior_parts' kernel sums them.  All three WITHOUT the host's scalar terms
 *                   (lnG(sum alpha) - sum_k lnG(alpha_k)) D and (lnG(sum beta) - sum_v lnG(beta_v)) K.
 * sum alpha and sum beta are summed on the host as those two entries sum them.  No kernel of its own; the sampler's
 * state is read, never written (the priors the device holds are replaced, as by every entry that takes them).  Waits for
 * the stream.
 * PYLDA_ERR_STATE: neither pylda_gibbs_init nor pylda_gibbs_set_state was called on the corpus;
 * PYLDA_ERR_INVALID: a NULL argument, a corpus of another context, more than 1024 topics. */
int pylda_test_gibbs_posterior_terms(pylda_ctx* ctx, pylda_corpus* corpus, const double* alpha_k, const double* beta_v,
                                     double* doc_terms, double* word_terms, double* sums);

#ifdef __cplusplus
}
#endif
#endif /* PYLDA_HIP_H */
