// libpylda_hip.so - left-to-right held-out likelihood: per (held-out document, particle) a chain over the document's
// tokens against the context's predictive table, the particles' predictive probabilities averaged per token, their logs
// summed per document.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the estimator's specification: left_to_right.h)
#include "sampler_host.h"
#include "left_to_right.h"

namespace {

// Token-steps of one launch unless the caller says otherwise: a good second at the 3.5e9 token-steps/s measured with
// resampling on cfg 3.
constexpr int64_t kDefaultStepBudget = (int64_t)1 << 32;
constexpr int64_t kMaxItems = (int64_t)1 << 30;          // work items of one launch (four to a workgroup)

hipError_t launch_particles(const LtrParams& p, hipStream_t st)
{
    const int64_t items = p.doc_count * p.R;
    return with_sampler_slots(p.K, [&](auto S) {
        return launch_kernel(ltr_particle_kernel<decltype(S)::value>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, p);
    });
}

int check_arguments(pylda_ctx* ctx, const pylda_corpus* c, const double* alpha_k, int particles, int resample, uint64_t stream,
                    int64_t first_document, int64_t step_budget)
{
    const int rc = check_sampler_call(ctx, c, "left_to_right", first_document);
    if (rc != PYLDA_OK) return rc;
    if (!alpha_k) return fail(ctx, PYLDA_ERR_INVALID, "left_to_right: alpha is NULL");
    if (particles < 1 || particles > 256) return fail(ctx, PYLDA_ERR_INVALID, "left_to_right: particles=%d (1 to 256)", particles);
    if (resample != 0 && resample != 1) return fail(ctx, PYLDA_ERR_INVALID, "left_to_right: resample=%d (0 or 1)", resample);
    if (stream > ((uint64_t)1 << 32) - (uint64_t)particles)
        return fail(ctx, PYLDA_ERR_INVALID, "left_to_right: stream %llu + %d particles > 2^32", (unsigned long long)stream, particles);
    if (step_budget < 0) return fail(ctx, PYLDA_ERR_INVALID, "left_to_right: step_budget=%lld (0: the default)", (long long)step_budget);
    // the table of either model: the context's eta (completion_set_model) or the frozen counts (foldin_set_model)
    if (!ctx->completion_ready && !ctx->foldin_ready)
        return fail(ctx, PYLDA_ERR_STATE, "left_to_right: no predictive table (completion_set_model or foldin_set_model first)");
    // (the per-document slots this call fills belong to the training state there: a training corpus is never touched)
    if (c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "left_to_right: the corpus holds a Gibbs training state; score a corpus of its own");
    return PYLDA_OK;
}

// The topics and the predictive probabilities: 10 bytes per token and particle, all documents at once where they fit the
// free device memory; *chunk_tokens: the tokens a chunk of documents may hold.
int prepare_scratch(pylda_ctx* ctx, const pylda_corpus* c, int particles, int64_t* chunk_tokens)
{
    const int64_t D = c->D;
    const std::vector<int64_t>& doc_tok = c->h_ltr_doc_tok;
    int64_t longest = 0;
    for (int64_t d = 0; d < D; ++d) longest = std::max(longest, doc_tok[(size_t)d + 1] - doc_tok[(size_t)d]);
    const size_t per_token = (size_t)particles * (sizeof(uint16_t) + sizeof(double));
    const size_t held = ctx->ltr_capacity * (sizeof(uint16_t) + sizeof(double));
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const size_t reserve = (size_t)256 << 20;
    const size_t usable = free_bytes + held > reserve ? free_bytes + held - reserve : 0;
    int64_t fit = (int64_t)std::min<size_t>((size_t)doc_tok[(size_t)D], usable / per_token);
    if (ctx->ltr_chunk_tokens > 0) fit = std::min(fit, ctx->ltr_chunk_tokens);
    if (longest > fit)
        return fail(ctx, PYLDA_ERR_OOM, "left_to_right: a document of %lld tokens with %d particles needs %zu MiB of scratch, %lld tokens fit",
                    (long long)longest, particles, ((size_t)longest * per_token) >> 20, (long long)fit);
    const size_t need = (size_t)fit * (size_t)particles;
    if (need > ctx->ltr_capacity) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        dev_free(ctx->d_ltr_z); dev_free(ctx->d_ltr_p);
        ctx->ltr_capacity = 0;
        FirstError A{ctx, "left_to_right"};
        A(dev_alloc(ctx, &ctx->d_ltr_z, need));
        A(dev_alloc(ctx, &ctx->d_ltr_p, need));
        if (A.rc != PYLDA_OK) {
            dev_free(ctx->d_ltr_z); dev_free(ctx->d_ltr_p);
            return A.rc;
        }
        ctx->ltr_capacity = need;
    }
    *chunk_tokens = fit;
    return PYLDA_OK;
}

// Work items in document order.  A chunk: consecutive documents whose tokens fit the scratch; inside it a launch:
// consecutive documents up to the budget of token-steps (all particles counted), a document over it on its own; then the
// chunk's reduction.
int enqueue_chunks(pylda_ctx* ctx, const pylda_corpus* c, LtrParams p, int64_t chunk_tokens, double budget, int* chunks)
{
    const int64_t D = c->D, R = p.R;
    const std::vector<int64_t>& doc_tok = c->h_ltr_doc_tok;
    *chunks = 0;
    for (int64_t d0 = 0; d0 < D;) {
        int64_t d1 = d0;
        while (d1 < D && doc_tok[(size_t)d1 + 1] - doc_tok[(size_t)d0] <= chunk_tokens) ++d1;
        p.tok_base = doc_tok[(size_t)d0];
        for (int64_t a = d0; a < d1;) {
            int64_t b = a;
            double steps = 0.0;
            while (b < d1 && (b - a + 1) * R <= kMaxItems) {
                const double n = (double)(doc_tok[(size_t)b + 1] - doc_tok[(size_t)b]);
                const double more = (double)R * (p.resample ? n * (n - 1.0) / 2.0 + n : n);
                if (b > a && steps + more > budget) break;
                steps += more;
                ++b;
            }
            p.doc_first = a;
            p.doc_count = b - a;
            HIP_TRY(ctx, launch_particles(p, ctx->stream));
            a = b;
        }
        for (int64_t a = d0; a < d1; a += kMaxItems) {
            p.doc_first = a;
            p.doc_count = std::min(kMaxItems, d1 - a);
            HIP_TRY(ctx, launch_kernel(ltr_reduce_kernel, dim3((unsigned)((p.doc_count + 3) / 4)), dim3(256), 0, ctx->stream, p));
        }
        d0 = d1;
        ++*chunks;
    }
    return PYLDA_OK;
}

}  // namespace

extern "C" {

int pylda_left_to_right(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, int particles, int resample, uint64_t seed,
                        uint64_t stream, int64_t first_document, int64_t step_budget, double* log_likelihood, int64_t* tokens)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_arguments(ctx, c, alpha_k, particles, resample, stream, first_document, step_budget);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->ltr_last_corpus = nullptr;
    rc = ensure_token_offsets(ctx, c, "left_to_right", true);      // (with the documents' offsets on the host)
    if (rc != PYLDA_OK) return rc;
    int64_t chunk_tokens = 0;
    rc = prepare_scratch(ctx, c, particles, &chunk_tokens);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_foldin_alpha, alpha_k, (size_t)ctx->K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

    LtrParams p{};
    p.K = ctx->K;
    p.ldk = ctx->ldk;
    p.R = particles;
    p.resample = resample;
    p.doc_ptr = c->d_doc_ptr;
    p.term_id = c->d_term_id;
    p.term_ct = c->d_term_ct;
    p.tok_off = c->d_tok_off;
    p.P = ctx->d_foldin_table;
    p.alpha = ctx->d_foldin_alpha;
    p.z = ctx->d_ltr_z;
    p.p = ctx->d_ltr_p;
    p.doc_ll = c->d_doc_ll;
    p.doc_wll = c->d_doc_wll;
    p.iters = c->d_iters;
    p.first_document = (uint32_t)first_document;
    p.stream = (uint32_t)stream;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);

    const int bracket = open_bracket(ctx, -1, ctx->stream);
    int chunks = 0;
    rc = enqueue_chunks(ctx, c, p, chunk_tokens, (double)(step_budget > 0 ? step_budget : kDefaultStepBudget), &chunks);
    close_bracket(ctx, bracket, ctx->stream);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, launch_kernel(ltr_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, c->d_doc_wll, c->d_doc_ptr, c->d_tok_off, c->D,
                               c->d_scalars, c->d_flag_count));
    // the scalars through the context's page-locked staging area, as pylda_estep_results
    double* sc = ctx->h_pin + (size_t)5 * ctx->K + 4;
    HIP_TRY(ctx, hipMemcpyAsync(sc, c->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    c->estep_done = true;
    c->last_heldout = 1;
    c->last_doc_values = true;
    ctx->ltr_last_corpus = c;
    ctx->ltr_last_particles = particles;
    ctx->ltr_last_chunks = chunks;
    if (log_likelihood) *log_likelihood = sc[1];
    if (tokens) *tokens = (int64_t)sc[2];
    return PYLDA_OK;
}

int pylda_test_left_to_right_state(pylda_ctx* ctx, pylda_corpus* c, int particles, uint16_t* z_out, double* p_out)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    if (!c || c->ctx != ctx) return fail(ctx, PYLDA_ERR_INVALID, "test_left_to_right_state: corpus does not belong to this context");
    if (ctx->ltr_last_corpus != c || ctx->ltr_last_particles != particles)
        return fail(ctx, PYLDA_ERR_STATE, "test_left_to_right_state: the last left_to_right call was not on this corpus with %d particles", particles);
    if (ctx->ltr_last_chunks > 1)
        return fail(ctx, PYLDA_ERR_STATE, "test_left_to_right_state: the last call ran in %d chunks, the buffers hold the last one's", ctx->ltr_last_chunks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)c->h_ltr_doc_tok[(size_t)c->D] * (size_t)particles;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (z_out && cells) HIP_TRY(ctx, hipMemcpy(z_out, ctx->d_ltr_z, cells * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (p_out && cells) HIP_TRY(ctx, hipMemcpy(p_out, ctx->d_ltr_p, cells * sizeof(double), hipMemcpyDeviceToHost));
    return PYLDA_OK;
}

}  // extern "C"
