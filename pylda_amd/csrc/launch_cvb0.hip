// libpylda_hip.so - the collapsed variational Bayes engine (CVB0): the start, sweeps of block-synchronous rounds with a
// deterministic apply pass, the training plug-in likelihood, the state in and out, and the held-out fold-in; and its
// stochastic form (SCVB0): the start, one minibatch step with its deterministic blend, the state in and out - the same
// buffers without the slots' rows, the same postings, likelihood and held-out entries.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the chains' specifications: estep_cvb0.h,
// scvb_kernels.h.  One translation unit: the two engines launch the same partial-sum and n_k kernels)
#include "sampler_host.h"
#include "estep_cvb0.h"
#include "scvb_kernels.h"

namespace {

int cvb0_chunks(const pylda_ctx* ctx) { return (ctx->V + kCvb0Chunk - 1) / kCvb0Chunk; }

// The engine's buffers of a corpus, allocated by its first call: the slots' rows (with_rows: CVB0 alone keeps them), the
// table, n_k and its chunk sums, the priors, the documents' changes and the two totals.
int prepare_cvb0(pylda_ctx* ctx, pylda_corpus* c, const char* what, bool with_rows = true)
{
    if (c->d_cvb0_table) return PYLDA_OK;
    const size_t cells = (size_t)ctx->V * ctx->ldk, rows = with_rows ? (size_t)c->nnz * ctx->ldk : 0;
    const size_t need = (rows + cells + (size_t)cvb0_chunks(ctx) * ctx->ldk + 2 * (size_t)ctx->K + (size_t)ctx->V + (size_t)c->D + 2) * sizeof(double) +
                        token_offsets_bytes(c);
    int rc = check_device_room(ctx, what, with_rows ? "the slots' rows and the expected-count table" : "the expected-count table", need);
    if (rc != PYLDA_OK || (rc = ensure_token_offsets(ctx, c, what)) != PYLDA_OK) return rc;
    FirstError A{ctx, what};
    if (with_rows && !c->d_cvb0_g) A(dev_alloc(ctx, &c->d_cvb0_g, rows));
    A(dev_alloc(ctx, &c->d_cvb0_nk, (size_t)ctx->K));
    A(dev_alloc(ctx, &c->d_cvb0_chunk, (size_t)cvb0_chunks(ctx) * ctx->ldk));
    A(dev_alloc(ctx, &c->d_cvb0_alpha, (size_t)ctx->K));
    A(dev_alloc(ctx, &c->d_cvb0_beta, (size_t)ctx->V));
    A(dev_alloc(ctx, &c->d_cvb0_change, (size_t)c->D));
    A(dev_alloc(ctx, &c->d_cvb0_out, (size_t)2));
    A(dev_alloc(ctx, &c->d_cvb0_table, cells));
    if (A.rc != PYLDA_OK) {
        dev_free(c->d_cvb0_g); dev_free(c->d_cvb0_nk); dev_free(c->d_cvb0_chunk); dev_free(c->d_cvb0_alpha); dev_free(c->d_cvb0_beta);
        dev_free(c->d_cvb0_change); dev_free(c->d_cvb0_out); dev_free(c->d_cvb0_table);
    }
    return A.rc;
}

// the priors on the device; copied only when they differ from what it holds (a sweep stays asynchronous)
int upload_cvb0_priors(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v)
{
    const size_t K = (size_t)ctx->K, V = (size_t)ctx->V;
    if (c->h_cvb0_alpha.size() != K || memcmp(c->h_cvb0_alpha.data(), alpha_k, K * sizeof(double)) != 0) {
        c->h_cvb0_alpha.assign(alpha_k, alpha_k + K);
        HIP_TRY(ctx, hipMemcpyAsync(c->d_cvb0_alpha, c->h_cvb0_alpha.data(), K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (c->h_cvb0_beta.size() != V || memcmp(c->h_cvb0_beta.data(), beta_v, V * sizeof(double)) != 0) {
        c->h_cvb0_beta.assign(beta_v, beta_v + V);
        HIP_TRY(ctx, hipMemcpyAsync(c->d_cvb0_beta, c->h_cvb0_beta.data(), V * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    return PYLDA_OK;
}

Cvb0Params cvb0_params(const pylda_ctx* ctx, const pylda_corpus* c)
{
    Cvb0Params p{};
    p.K = ctx->K;
    p.V = ctx->V;
    p.ldk = ctx->ldk;
    p.doc_ptr = c->d_doc_ptr;
    p.term_id = c->d_term_id;
    p.term_ct = c->d_term_ct;
    p.tok_off = c->d_tok_off;
    p.g = c->d_cvb0_g;
    p.n_dk = c->d_gamma;
    p.table = c->d_cvb0_table;
    p.n_k = c->d_cvb0_nk;
    p.alpha = c->d_cvb0_alpha;
    p.beta = c->d_cvb0_beta;
    p.delta = c->d_cvb0_delta;
    p.slot_place = c->d_cvb0_place;
    p.doc_change = c->d_cvb0_change;
    p.D = c->D;
    return p;
}

// n_k from the table: the chunk sums, then their sum
hipError_t launch_nk(const pylda_ctx* ctx, const pylda_corpus* c, hipStream_t st)
{
    const unsigned kb = (unsigned)((ctx->K + 255) / 256);
    const hipError_t e = launch_kernel(cvb0_nk_chunk_kernel, dim3((unsigned)cvb0_chunks(ctx), kb), dim3(256), 0, st,
                                       (const double*)c->d_cvb0_table, ctx->V, ctx->K, ctx->ldk, c->d_cvb0_chunk);
    if (e != hipSuccess) return e;
    return launch_kernel(cvb0_nk_sum_kernel, dim3(kb), dim3(256), 0, st, (const double*)c->d_cvb0_chunk, cvb0_chunks(ctx), ctx->K, ctx->ldk,
                         c->d_cvb0_nk);
}

// The postings of the sweep's blocks, built on the host once per (blocks, first_document), and the block buffers.
int ensure_cvb0_rounds(pylda_ctx* ctx, pylda_corpus* c, int64_t blocks, int64_t first_document, const char* what = "cvb0_sweep")
{
    if (c->d_cvb0_place && c->cvb0_blocks == blocks && c->cvb0_first == first_document) return PYLDA_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));        // (a round of the plan before may still read its buffers)
    std::vector<int64_t> ptr((size_t)c->D + 1, 0);
    std::vector<int32_t> ids((size_t)c->nnz);
    HIP_TRY(ctx, hipMemcpy(ptr.data(), c->d_doc_ptr, ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (c->nnz) HIP_TRY(ctx, hipMemcpy(ids.data(), c->d_term_id, ids.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    Cvb0Postings post = cvb0_block_postings(ptr.data(), ids.data(), c->D, blocks, first_document);
    dev_free(c->d_cvb0_place); dev_free(c->d_cvb0_seg_begin); dev_free(c->d_cvb0_run_seg); dev_free(c->d_cvb0_run_word);
    dev_free(c->d_cvb0_delta); dev_free(c->d_cvb0_partial);
    c->cvb0_blocks = 0;
    const size_t need = ((size_t)(post.widest_postings + post.widest_segments) * ctx->ldk) * sizeof(double) +
                        (post.slot_place.size() + post.seg_begin.size() + post.run_seg.size()) * sizeof(int64_t) +
                        post.run_word.size() * sizeof(int32_t);
    const int rc = check_device_room(ctx, what, "the block's delta rows and postings", need);
    if (rc != PYLDA_OK) return rc;
    FirstError A{ctx, what};
    A(dev_alloc(ctx, &c->d_cvb0_place, post.slot_place.size()));
    A(dev_alloc(ctx, &c->d_cvb0_seg_begin, post.seg_begin.size()));
    A(dev_alloc(ctx, &c->d_cvb0_run_seg, post.run_seg.size()));
    A(dev_alloc(ctx, &c->d_cvb0_run_word, post.run_word.size()));
    A(dev_alloc(ctx, &c->d_cvb0_delta, (size_t)post.widest_postings * ctx->ldk));
    A(dev_alloc(ctx, &c->d_cvb0_partial, (size_t)post.widest_segments * ctx->ldk));
    A.h2d(c->d_cvb0_place, post.slot_place.data(), post.slot_place.size() * sizeof(int64_t));
    A.h2d(c->d_cvb0_seg_begin, post.seg_begin.data(), post.seg_begin.size() * sizeof(int64_t));
    A.h2d(c->d_cvb0_run_seg, post.run_seg.data(), post.run_seg.size() * sizeof(int64_t));
    A.h2d(c->d_cvb0_run_word, post.run_word.data(), post.run_word.size() * sizeof(int32_t));
    if (A.rc != PYLDA_OK) {
        dev_free(c->d_cvb0_place); dev_free(c->d_cvb0_seg_begin); dev_free(c->d_cvb0_run_seg); dev_free(c->d_cvb0_run_word);
        dev_free(c->d_cvb0_delta); dev_free(c->d_cvb0_partial);
        return A.rc;
    }
    std::vector<int64_t>().swap(post.post_slot);            // (the nnz-sized lists are on the device now)
    std::vector<int64_t>().swap(post.slot_place);
    std::vector<int64_t>().swap(post.seg_begin);
    std::vector<int64_t>().swap(post.run_seg);
    std::vector<int32_t>().swap(post.run_word);
    c->cvb0_rounds = std::move(post);
    c->cvb0_blocks = blocks;
    c->cvb0_first = first_document;
    return PYLDA_OK;
}

// Whose training state an entry takes: CVB0's (the table, n_k, N_dk and the slots' rows), the stochastic engine's (the same
// without the rows), or either one's (the likelihood reads what both keep).
enum class Engine { cvb0, scvb, either };

int check_corpus(pylda_ctx* ctx, pylda_corpus* c, const char* what, int64_t first_document, bool needs_state, Engine engine)
{
    const int rc = check_sampler_call(ctx, c, what, first_document);
    if (rc != PYLDA_OK) return rc;
    if (c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "%s: the corpus holds a Gibbs training state", what);
    if (engine == Engine::scvb && c->cvb0_ready) return fail(ctx, PYLDA_ERR_STATE, "%s: the corpus holds a CVB0 training state", what);
    if (engine == Engine::cvb0 && c->scvb_ready)
        return fail(ctx, PYLDA_ERR_STATE, "%s: the corpus holds a stochastic (SCVB0) training state", what);
    const bool has_state = (engine != Engine::scvb && c->cvb0_ready) || (engine != Engine::cvb0 && c->scvb_ready);
    if (needs_state && !has_state)
        return fail(ctx, PYLDA_ERR_STATE, engine == Engine::scvb ? "%s: scvb_init or scvb_set_state must be called first"
                                                                 : "%s: cvb0_init or cvb0_set_state must be called first", what);
    return PYLDA_OK;
}

// the buffers of CVB0 without the slots' rows, and the words' run map
int prepare_scvb(pylda_ctx* ctx, pylda_corpus* c, const char* what)
{
    if (c->d_scvb_word_run) return PYLDA_OK;
    int rc = check_device_room(ctx, what, "the words' run map", (size_t)ctx->V * sizeof(int32_t));
    if (rc != PYLDA_OK || (rc = prepare_cvb0(ctx, c, what, false)) != PYLDA_OK) return rc;
    return dev_alloc(ctx, &c->d_scvb_word_run, (size_t)ctx->V);
}

// The start of either engine on a prepared corpus: the table (with_rows: and the slots' rows) zeroed, launch_init(params) -
// the engine's init kernel over the documents -, then n_k.
template <typename LaunchInit>
int init_state(pylda_ctx* ctx, pylda_corpus* c, uint64_t seed, int64_t first_document, bool with_rows, LaunchInit launch_init)
{
    Cvb0Params p = cvb0_params(ctx, c);
    p.first_document = (uint32_t)first_document;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    HIP_TRY(ctx, hipMemsetAsync(c->d_cvb0_table, 0, (size_t)ctx->V * ctx->ldk * sizeof(double), ctx->stream));
    if (with_rows && c->nnz) HIP_TRY(ctx, hipMemsetAsync(c->d_cvb0_g, 0, (size_t)c->nnz * ctx->ldk * sizeof(double), ctx->stream));
    if (c->D > 0) {
        const hipError_t e = launch_init(p);
        HIP_TRY(ctx, e);
    }
    HIP_TRY(ctx, launch_nk(ctx, c, ctx->stream));
    c->estep_done = true;           // (pylda_get_gamma hands out N_dk)
    return PYLDA_OK;
}

// The apply pass of round r, which has postings: the segments' partial sums of the block's delta rows, into_table(topics) -
// the engine's pass from the partial rows into the table, on `topics` threads a workgroup -, then n_k.
template <typename IntoTable>
hipError_t apply_round(pylda_ctx* ctx, pylda_corpus* c, size_t r, IntoTable into_table)
{
    const Cvb0Postings& R = c->cvb0_rounds;
    const dim3 topics(ctx->K <= kWave ? kWave : 256);
    hipError_t e = launch_kernel(cvb0_partial_kernel, dim3((unsigned)(R.seg_ptr[r + 1] - R.seg_ptr[r])), topics, 0, ctx->stream,
                                 (const double*)c->d_cvb0_delta, (const int64_t*)(c->d_cvb0_seg_begin + R.seg_ptr[r]), R.post_ptr[r], ctx->K,
                                 ctx->ldk, c->d_cvb0_partial);
    if (e == hipSuccess) e = into_table(topics);
    if (e == hipSuccess) e = launch_nk(ctx, c, ctx->stream);
    return e;
}

// The state out: the table as K x V, n_k, N_dk, and what the engine keeps beside them - the slots' rows g (CVB0) or the
// documents' last changes (SCVB0).  NULL: not wanted.
int get_state(pylda_ctx* ctx, pylda_corpus* c, const char* what, Engine engine, double* n_kv, double* n_k, double* n_dk, double* g,
              double* doc_change)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, what, 0, true, engine);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int K = ctx->K, ldk = ctx->ldk;
    if (n_kv && (rc = table_to_host(ctx, c->d_cvb0_table, n_kv)) != PYLDA_OK) return rc;
    if (n_k) HIP_TRY(ctx, hipMemcpy(n_k, c->d_cvb0_nk, (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
    if (n_dk && c->D > 0) HIP_TRY(ctx, hipMemcpy(n_dk, c->d_gamma, (size_t)c->D * K * sizeof(double), hipMemcpyDeviceToHost));
    if (g && c->nnz > 0)
        HIP_TRY(ctx, hipMemcpy2D(g, (size_t)K * sizeof(double), c->d_cvb0_g, (size_t)ldk * sizeof(double), (size_t)K * sizeof(double),
                                 (size_t)c->nnz, hipMemcpyDeviceToHost));
    if (doc_change && c->D > 0) HIP_TRY(ctx, hipMemcpy(doc_change, c->d_cvb0_change, (size_t)c->D * sizeof(double), hipMemcpyDeviceToHost));
    return PYLDA_OK;
}

// The state in, each part as given; a corpus without a state needs all of its engine's parts (g: CVB0 alone).
int set_state(pylda_ctx* ctx, pylda_corpus* c, const char* what, Engine engine, const double* n_kv, const double* n_k, const double* n_dk,
              const double* g)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, what, 0, false, engine);
    const bool scvb = engine == Engine::scvb;
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool& ready = scvb ? c->scvb_ready : c->cvb0_ready;
    const bool fresh = !ready;
    if (fresh && (!n_kv || !n_k || !n_dk || (!scvb && !g)))
        return fail(ctx, PYLDA_ERR_STATE, scvb ? "%s: a corpus without a state needs the table, n_k and n_dk"
                                               : "%s: a corpus without a state needs the table, n_k, n_dk and the slots' rows", what);
    if ((rc = scvb ? prepare_scvb(ctx, c, what) : prepare_cvb0(ctx, c, what)) != PYLDA_OK) return rc;
    const int K = ctx->K, ldk = ctx->ldk;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_kv && (rc = table_from_host(ctx, c->d_cvb0_table, n_kv)) != PYLDA_OK) return rc;
    if (n_k) HIP_TRY(ctx, hipMemcpy(c->d_cvb0_nk, n_k, (size_t)K * sizeof(double), hipMemcpyHostToDevice));
    if (n_dk && c->D > 0) HIP_TRY(ctx, hipMemcpy(c->d_gamma, n_dk, (size_t)c->D * K * sizeof(double), hipMemcpyHostToDevice));
    if (g && c->nnz > 0) {
        if (fresh) HIP_TRY(ctx, hipMemset(c->d_cvb0_g, 0, (size_t)c->nnz * ldk * sizeof(double)));     // (the padding)
        HIP_TRY(ctx, hipMemcpy2D(c->d_cvb0_g, (size_t)ldk * sizeof(double), g, (size_t)K * sizeof(double), (size_t)K * sizeof(double),
                                 (size_t)c->nnz, hipMemcpyHostToDevice));
    }
    if (fresh && c->D > 0) HIP_TRY(ctx, hipMemset(c->d_cvb0_change, 0, (size_t)c->D * sizeof(double)));
    ready = true;
    c->estep_done = true;
    return PYLDA_OK;
}

}  // namespace

extern "C" {

int pylda_cvb0_init(pylda_ctx* ctx, pylda_corpus* c, uint64_t seed, int64_t first_document)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, "cvb0_init", first_document, false, Engine::cvb0);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = prepare_cvb0(ctx, c, "cvb0_init")) != PYLDA_OK) return rc;
    rc = init_state(ctx, c, seed, first_document, true, [&](const Cvb0Params& p) {
        return with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(cvb0_init_kernel<decltype(S)::value>, dim3((unsigned)((c->D + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
    });
    if (rc == PYLDA_OK) c->cvb0_ready = true;
    return rc;
}

int pylda_cvb0_sweep(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double beta_sum, int64_t blocks,
                     int64_t first_document)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, "cvb0_sweep", first_document, true, Engine::cvb0);
    if (rc != PYLDA_OK) return rc;
    if (!alpha_k || !beta_v || !(beta_sum > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "cvb0_sweep: alpha, beta or beta_sum missing");
    if (blocks < 1) return fail(ctx, PYLDA_ERR_INVALID, "cvb0_sweep: blocks=%lld (at least 1)", (long long)blocks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_cvb0_rounds(ctx, c, blocks, first_document)) != PYLDA_OK) return rc;
    if ((rc = upload_cvb0_priors(ctx, c, alpha_k, beta_v)) != PYLDA_OK) return rc;
    Cvb0Params p = cvb0_params(ctx, c);
    p.beta_sum = beta_sum;
    p.first_document = (uint32_t)first_document;
    p.step = blocks;
    const Cvb0Postings& R = c->cvb0_rounds;
    const int bracket = open_bracket(ctx, -1, ctx->stream);
    for (size_t r = 0; r < R.round_block.size(); ++r) {
        p.first = R.round_first[r];
        p.count = R.round_docs[r];
        hipError_t e = with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(cvb0_update_kernel<decltype(S)::value>, dim3((unsigned)((p.count + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
        const int64_t segments = R.seg_ptr[r + 1] - R.seg_ptr[r], runs = R.run_ptr[r + 1] - R.run_ptr[r];
        if (e == hipSuccess && segments > 0)
            e = apply_round(ctx, c, r, [&](dim3 topics) {
                return launch_kernel(cvb0_combine_kernel, dim3((unsigned)runs), topics, 0, ctx->stream, (const double*)c->d_cvb0_partial,
                                     (const int32_t*)(c->d_cvb0_run_word + R.run_ptr[r]), (const int64_t*)(c->d_cvb0_run_seg + R.run_ptr[r]),
                                     R.seg_ptr[r], ctx->K, ctx->ldk, c->d_cvb0_table);
            });
        if (e != hipSuccess) {
            close_bracket(ctx, bracket, ctx->stream);
            HIP_TRY(ctx, e);
        }
    }
    close_bracket(ctx, bracket, ctx->stream);
    return PYLDA_OK;
}

int pylda_cvb0_log_likelihood(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double beta_sum,
                              double* log_likelihood, double* change)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, "cvb0_log_likelihood", 0, true, Engine::either);
    if (rc != PYLDA_OK) return rc;
    if (!alpha_k || !beta_v || !(beta_sum > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "cvb0_log_likelihood: alpha, beta or beta_sum missing");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = upload_cvb0_priors(ctx, c, alpha_k, beta_v)) != PYLDA_OK) return rc;
    Cvb0Params p = cvb0_params(ctx, c);
    p.beta_sum = beta_sum;
    if (c->D > 0) {
        const hipError_t e = with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(cvb0_likelihood_kernel<decltype(S)::value>, dim3((unsigned)((c->D + 3) / 4)), dim3(256), 0, ctx->stream, p,
                                 c->d_doc_ll, c->d_doc_wll);
        });
        HIP_TRY(ctx, e);
    }
    HIP_TRY(ctx, launch_kernel(cvb0_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)c->d_doc_wll,
                               (const double*)c->d_cvb0_change, c->D, c->d_scalars, c->d_cvb0_out));
    c->last_heldout = 0;
    c->last_doc_values = true;
    double* sc = ctx->h_pin + (size_t)5 * ctx->K + 4;       // the context's page-locked staging area, as pylda_estep_results
    HIP_TRY(ctx, hipMemcpyAsync(sc, c->d_cvb0_out, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (log_likelihood) *log_likelihood = sc[0];
    if (change) *change = sc[1];
    return PYLDA_OK;
}

int pylda_cvb0_get_state(pylda_ctx* ctx, pylda_corpus* c, double* n_kv, double* n_k, double* n_dk, double* g)
{
    return get_state(ctx, c, "cvb0_get_state", Engine::cvb0, n_kv, n_k, n_dk, g, nullptr);
}

int pylda_cvb0_set_state(pylda_ctx* ctx, pylda_corpus* c, const double* n_kv, const double* n_k, const double* n_dk, const double* g)
{
    return set_state(ctx, c, "cvb0_set_state", Engine::cvb0, n_kv, n_k, n_dk, g);
}

int pylda_cvb0_foldin(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, int sweeps, uint64_t seed, uint64_t stream,
                      int64_t first_document, double* words_log_likelihood)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "cvb0_foldin", first_document);
    if (rc != PYLDA_OK) return rc;
    if (!alpha_k) return fail(ctx, PYLDA_ERR_INVALID, "cvb0_foldin: alpha is NULL");
    if (sweeps < 1) return fail(ctx, PYLDA_ERR_INVALID, "cvb0_foldin: sweeps=%d (at least 1)", sweeps);
    if (stream > 0xffffffffull) return fail(ctx, PYLDA_ERR_INVALID, "cvb0_foldin: stream %llu >= 2^32", (unsigned long long)stream);
    // the table of either model: the context's eta (completion_set_model) or frozen Gibbs counts (foldin_set_model)
    if (!ctx->completion_ready && !ctx->foldin_ready)
        return fail(ctx, PYLDA_ERR_STATE, "cvb0_foldin: no predictive table (set_eta and completion_set_model first)");
    // (N_dk of a training state lives in the gamma buffer, its rows in the slot buffer: both are this call's outputs)
    if (c->cvb0_ready || c->scvb_ready || c->gibbs_ready)
        return fail(ctx, PYLDA_ERR_STATE, "cvb0_foldin: the corpus holds a training state; fold in a corpus of its own");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)c->nnz * ctx->ldk;
    rc = check_device_room(ctx, "cvb0_foldin", "the token offsets and the slots' rows",
                           token_offsets_bytes(c) + (c->d_cvb0_g ? 0 : rows * sizeof(double)));
    if (rc != PYLDA_OK || (rc = ensure_token_offsets(ctx, c, "cvb0_foldin")) != PYLDA_OK) return rc;
    if (!c->d_cvb0_g && (rc = dev_alloc(ctx, &c->d_cvb0_g, rows)) != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_foldin_alpha, alpha_k, (size_t)ctx->K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

    Cvb0FoldinParams p{};
    p.K = ctx->K;
    p.V = ctx->V;
    p.ldk = ctx->ldk;
    p.doc_ptr = c->d_doc_ptr;
    p.term_id = c->d_term_id;
    p.term_ct = c->d_term_ct;
    p.tok_off = c->d_tok_off;
    p.g = c->d_cvb0_g;
    p.P = ctx->d_foldin_table;
    p.alpha = ctx->d_foldin_alpha;
    p.gamma = c->d_gamma;
    p.doc_ll = c->d_doc_ll;
    p.doc_wll = c->d_doc_wll;
    p.iters = c->d_iters;
    p.D = c->D;
    p.sweeps = sweeps;
    p.first_document = (uint32_t)first_document;
    p.stream = (uint32_t)stream;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);

    const int bracket = open_bracket(ctx, -1, ctx->stream);
    if (c->D > 0) {
        const hipError_t e = with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(cvb0_foldin_kernel<decltype(S)::value>, dim3((unsigned)((p.D + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
        HIP_TRY(ctx, e);
    }
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, launch_kernel(cvb0_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)c->d_doc_wll, (const double*)nullptr, c->D,
                               c->d_scalars, (double*)nullptr));
    c->estep_done = true;
    c->last_heldout = 1;
    c->last_doc_values = true;
    double* sc = ctx->h_pin + (size_t)5 * ctx->K + 4;       // the total through the context's page-locked staging area
    HIP_TRY(ctx, hipMemcpyAsync(sc, c->d_scalars + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (words_log_likelihood) *words_log_likelihood = sc[0];
    return PYLDA_OK;
}

int pylda_test_cvb0_postings(int64_t documents, const int64_t* doc_ptr, const int32_t* term_id, int64_t blocks, int64_t first_document,
                             int64_t* counts, int64_t* rounds, int64_t* post_slot, int64_t* slot_place, int64_t* seg_begin,
                             int32_t* run_word, int64_t* run_seg)
{
    if (documents < 0 || !doc_ptr || blocks < 1 || first_document < 0 || !counts) return PYLDA_ERR_INVALID;
    const Cvb0Postings post = cvb0_block_postings(doc_ptr, term_id, documents, blocks, first_document);
    const size_t n = post.round_block.size();
    counts[0] = (int64_t)n;
    counts[1] = (int64_t)post.seg_begin.size() - 1;
    counts[2] = (int64_t)post.run_word.size();
    counts[3] = post.widest_postings;
    counts[4] = post.widest_segments;
    if (rounds)
        for (size_t r = 0; r < n; ++r) {
            int64_t* row = rounds + 6 * r;
            row[0] = post.round_block[r];
            row[1] = post.round_first[r];
            row[2] = post.round_docs[r];
            row[3] = post.post_ptr[r + 1];
            row[4] = post.seg_ptr[r + 1];
            row[5] = post.run_ptr[r + 1];
        }
    if (post_slot) std::copy(post.post_slot.begin(), post.post_slot.end(), post_slot);
    if (slot_place) std::copy(post.slot_place.begin(), post.slot_place.end(), slot_place);
    if (seg_begin) std::copy(post.seg_begin.begin(), post.seg_begin.end(), seg_begin);
    if (run_word) std::copy(post.run_word.begin(), post.run_word.end(), run_word);
    if (run_seg) std::copy(post.run_seg.begin(), post.run_seg.end(), run_seg);
    return PYLDA_OK;
}


// ---- the stochastic form (SCVB0) ----
int pylda_scvb_init(pylda_ctx* ctx, pylda_corpus* c, uint64_t seed, int64_t first_document)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, "scvb_init", first_document, false, Engine::scvb);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = prepare_scvb(ctx, c, "scvb_init")) != PYLDA_OK) return rc;
    rc = init_state(ctx, c, seed, first_document, false, [&](const Cvb0Params& p) {
        return with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(scvb_init_kernel<decltype(S)::value>, dim3((unsigned)((c->D + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
    });
    if (rc == PYLDA_OK) c->scvb_ready = true;
    return rc;
}

int pylda_scvb_step(pylda_ctx* ctx, pylda_corpus* c, int64_t block, int64_t batches, int64_t first_document, const double* alpha_k,
                    const double* beta_v, double beta_sum, double keep, double gain, int passes, const double* rho_theta,
                    const double* one_minus)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_corpus(ctx, c, "scvb_step", first_document, true, Engine::scvb);
    if (rc != PYLDA_OK) return rc;
    if (!alpha_k || !beta_v || !(beta_sum > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: alpha, beta or beta_sum missing");
    if (batches < 1) return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: batches=%lld (at least 1)", (long long)batches);
    if (block < 0 || block >= batches)
        return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: block=%lld of %lld minibatches", (long long)block, (long long)batches);
    if (passes < 1 || passes > kScvbMaxPasses)
        return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: passes=%d (burn_in + 1: 1 to %d)", passes, kScvbMaxPasses);
    if (!rho_theta || !one_minus) return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: the documents' step sizes are missing");
    if (!(keep >= 0.0 && keep < 1.0) || !(gain > 0.0 && gain <= 1.7976931348623157e308))
        return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: keep=%g (1 - rho: in [0, 1)) or gain=%g (positive and finite)", keep, gain);
    ScvbParams sp{};
    sp.passes = passes;
    for (int i = 0; i < passes; ++i) {
        if (!(rho_theta[i] > 0.0 && rho_theta[i] <= 1.0) || !(one_minus[i] >= 0.0 && one_minus[i] < 1.0))
            return fail(ctx, PYLDA_ERR_INVALID, "scvb_step: pass %d has rho=%g, 1 - rho=%g (rho in (0, 1])", i, rho_theta[i], one_minus[i]);
        sp.one_minus[i] = one_minus[i];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_cvb0_rounds(ctx, c, batches, first_document, "scvb_step")) != PYLDA_OK) return rc;
    if ((rc = upload_cvb0_priors(ctx, c, alpha_k, beta_v)) != PYLDA_OK) return rc;
    const Cvb0Postings& R = c->cvb0_rounds;
    const auto at = std::lower_bound(R.round_block.begin(), R.round_block.end(), block);
    if (at == R.round_block.end() || *at != block) return PYLDA_OK;         // a block without documents changes nothing
    const size_t r = (size_t)(at - R.round_block.begin());
    const int64_t segments = R.seg_ptr[r + 1] - R.seg_ptr[r], runs = R.run_ptr[r + 1] - R.run_ptr[r];
    if (segments == 0) return PYLDA_OK;                                     // ... nor does one without tokens
    sp.c = cvb0_params(ctx, c);
    sp.c.beta_sum = beta_sum;
    sp.c.first_document = (uint32_t)first_document;
    sp.c.step = batches;
    sp.c.first = R.round_first[r];
    sp.c.count = R.round_docs[r];
    const int bracket = open_bracket(ctx, -1, ctx->stream);
    hipError_t e = with_sampler_slots(ctx->K, [&](auto S) {
        return launch_kernel(scvb_update_kernel<decltype(S)::value>, dim3((unsigned)((sp.c.count + 3) / 4)), dim3(256), 0, ctx->stream, sp);
    });
    if (e == hipSuccess)
        e = apply_round(ctx, c, r, [&](dim3 topics) {
            hipError_t b = hipMemsetAsync(c->d_scvb_word_run, 0xff, (size_t)ctx->V * sizeof(int32_t), ctx->stream);
            if (b == hipSuccess)
                b = launch_kernel(scvb_run_map_kernel, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, ctx->stream,
                                  (const int32_t*)(c->d_cvb0_run_word + R.run_ptr[r]), runs, c->d_scvb_word_run);
            if (b == hipSuccess)
                b = launch_kernel(scvb_blend_kernel, dim3((unsigned)ctx->V), topics, 0, ctx->stream, (const double*)c->d_cvb0_partial,
                                  (const int32_t*)c->d_scvb_word_run, (const int64_t*)(c->d_cvb0_run_seg + R.run_ptr[r]), R.seg_ptr[r], ctx->K,
                                  ctx->ldk, keep, gain, c->d_cvb0_table);
            return b;
        });
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, e);
    return PYLDA_OK;
}

int pylda_scvb_get_state(pylda_ctx* ctx, pylda_corpus* c, double* n_kv, double* n_k, double* n_dk, double* doc_change)
{
    return get_state(ctx, c, "scvb_get_state", Engine::scvb, n_kv, n_k, n_dk, nullptr, doc_change);
}

int pylda_scvb_set_state(pylda_ctx* ctx, pylda_corpus* c, const double* n_kv, const double* n_k, const double* n_dk)
{
    return set_state(ctx, c, "scvb_set_state", Engine::scvb, n_kv, n_k, n_dk, nullptr);
}

}  // extern "C"
