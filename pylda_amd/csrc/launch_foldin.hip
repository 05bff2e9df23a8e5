// libpylda_hip.so - held-out fold-in for the collapsed Gibbs engine: the predictive table of a frozen model, and per
// held-out document a Gibbs chain over its tokens, its topic proportions and its likelihood, in one launch.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the estimator's specification: estep_foldin.h)
#include "sampler_host.h"
#include "estep_foldin.h"

extern "C" {

int pylda_foldin_set_model(pylda_ctx* ctx, pylda_corpus* trained, const int32_t* n_kv, const int32_t* n_k, const double* beta_v,
                           double beta_sum)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    const int K = ctx->K, V = ctx->V, ldk = ctx->ldk;
    if (K > 64 * 16) return fail(ctx, PYLDA_ERR_INVALID, "foldin_set_model: %d topics (at most 1024: 16 per lane)", K);
    if (!beta_v || !(beta_sum > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "foldin_set_model: beta or beta_sum missing");
    if (trained && trained->ctx != ctx) return fail(ctx, PYLDA_ERR_INVALID, "foldin_set_model: corpus does not belong to this context");
    if (trained && !trained->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "foldin_set_model: the corpus holds no Gibbs state");
    if (!trained && (!n_kv || !n_k)) return fail(ctx, PYLDA_ERR_INVALID, "foldin_set_model: neither a trained corpus nor n_kv and n_k");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)V * ldk;
    if (!ctx->d_foldin_table) {
        const size_t need = cells * (sizeof(double) + sizeof(int32_t)) + (size_t)V * sizeof(double);
        size_t free_bytes = 0, total_bytes = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
        if (need + ((size_t)256 << 20) > free_bytes)
            return fail(ctx, PYLDA_ERR_OOM, "foldin_set_model: the predictive table needs %zu MiB, %zu MiB of device memory are free",
                        need >> 20, free_bytes >> 20);
        FirstError A{ctx, "foldin_set_model"};
        A(dev_alloc(ctx, &ctx->d_foldin_table, cells));
        A(dev_alloc(ctx, &ctx->d_foldin_alpha, (size_t)K));
        if (A.rc != PYLDA_OK) {
            dev_free(ctx->d_foldin_table); dev_free(ctx->d_foldin_alpha);
            return A.rc;
        }
    }
    ctx->foldin_ready = false;
    ctx->completion_ready = false;      // (document completion's table of eta shares the storage)
    // what the table kernel reads besides a trained corpus' buffers lives until the kernel has run
    double* d_beta = nullptr;
    int32_t *d_counts = nullptr, *d_nk = nullptr;
    FirstError A{ctx, "foldin_set_model"};
    A(dev_alloc(ctx, &d_beta, (size_t)V));
    A.h2d(d_beta, beta_v, (size_t)V * sizeof(double));
    if (!trained) {
        std::vector<int32_t> table(cells, 0);              // word-major, as a corpus' table
        for (int k = 0; k < K; ++k)
            for (int v = 0; v < V; ++v) table[(size_t)v * ldk + k] = n_kv[(size_t)k * V + v];
        A(dev_alloc(ctx, &d_counts, cells));
        A(dev_alloc(ctx, &d_nk, (size_t)K));
        A.h2d(d_counts, table.data(), cells * sizeof(int32_t));
        A.h2d(d_nk, n_k, (size_t)K * sizeof(int32_t));
    }
    hipError_t e = hipSuccess;
    if (A.rc == PYLDA_OK) {
        e = launch_kernel(foldin_table_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream,
                          trained ? trained->d_gibbs_table : d_counts, trained ? trained->d_gibbs_nk : d_nk, d_beta, beta_sum, K, V, ldk,
                          ctx->d_foldin_table);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    dev_free(d_beta); dev_free(d_counts); dev_free(d_nk);
    if (A.rc != PYLDA_OK) return A.rc;
    HIP_TRY(ctx, e);
    ctx->foldin_ready = true;
    return PYLDA_OK;
}

int pylda_foldin(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, int number_of_samples, int burn_in_samples, uint64_t seed,
                 uint64_t stream, int64_t first_document, double* words_log_likelihood)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "foldin", first_document);
    if (rc != PYLDA_OK) return rc;
    if (!alpha_k) return fail(ctx, PYLDA_ERR_INVALID, "foldin: alpha is NULL");
    if (number_of_samples < 1 || number_of_samples > 65534)
        return fail(ctx, PYLDA_ERR_INVALID, "foldin: number_of_samples=%d (1 to 65534: the sweep is 16 bits of a draw's name)", number_of_samples);
    if (burn_in_samples < 0 || burn_in_samples >= number_of_samples)
        return fail(ctx, PYLDA_ERR_INVALID, "foldin: number_of_samples=%d, burn_in_samples=%d (need 0 <= burn-in < samples)",
                    number_of_samples, burn_in_samples);
    if (stream > 0xffffffffull) return fail(ctx, PYLDA_ERR_INVALID, "foldin: stream %llu >= 2^32", (unsigned long long)stream);
    if (!ctx->foldin_ready) return fail(ctx, PYLDA_ERR_STATE, "foldin: foldin_set_model must be called first");
    // (n_dk of a training state lives in the gamma buffer, its topics in the state words: both are this call's outputs)
    if (c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "foldin: the corpus holds a Gibbs training state; fold in a corpus of its own");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // token offsets and state words, by the first call that needs them
    rc = check_device_room(ctx, "foldin", "the token offsets and states", token_state_bytes(c));
    if (rc != PYLDA_OK || (rc = ensure_token_state(ctx, c, "foldin")) != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_foldin_alpha, alpha_k, (size_t)ctx->K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

    FoldinParams p{};
    p.K = ctx->K;
    p.V = ctx->V;
    p.ldk = ctx->ldk;
    p.doc_ptr = c->d_doc_ptr;
    p.term_id = c->d_term_id;
    p.term_ct = c->d_term_ct;
    p.tok_off = c->d_tok_off;
    p.state = c->d_hyb_state;
    p.P = ctx->d_foldin_table;
    p.alpha = ctx->d_foldin_alpha;
    p.gamma = c->d_gamma;
    p.doc_ll = c->d_doc_ll;
    p.doc_wll = c->d_doc_wll;
    p.iters = c->d_iters;
    p.D = c->D;
    p.samples = number_of_samples;
    p.burn_in = burn_in_samples;
    p.first_document = (uint32_t)first_document;
    p.stream = (uint32_t)stream;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);

    const int bracket = open_bracket(ctx, -1, ctx->stream);
    if (c->D > 0) {
        const hipError_t e = with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(foldin_sample_kernel<decltype(S)::value>, dim3((unsigned)((p.D + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
        HIP_TRY(ctx, e);
    }
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, launch_kernel(foldin_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, c->d_doc_wll, c->D, c->d_scalars));
    c->estep_done = true;
    c->last_heldout = 1;
    c->last_doc_values = true;
    // the total through the context's page-locked staging area, as pylda_estep_results
    double* sc = ctx->h_pin + (size_t)5 * ctx->K + 4;
    HIP_TRY(ctx, hipMemcpyAsync(sc, c->d_scalars + 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (words_log_likelihood) *words_log_likelihood = sc[0];
    return PYLDA_OK;
}

}  // extern "C"
