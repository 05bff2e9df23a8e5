// libpylda_hip.so - document-completion held-out likelihood: the predictive table of the context's eta, and the score of
// the held halves of test documents under a gamma fitted on their observed halves.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the estimator's specification: completion_score.h)
#include "sampler_host.h"
#include "completion_score.h"

extern "C" {

int pylda_completion_set_model(pylda_ctx* ctx)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    const int K = ctx->K, V = ctx->V, ldk = ctx->ldk;
    if (K > 64 * 16) return fail(ctx, PYLDA_ERR_INVALID, "completion_set_model: %d topics (at most 1024: 16 per lane)", K);
    if (!ctx->have_eta) return fail(ctx, PYLDA_ERR_STATE, "completion_set_model: eta was never set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)V * ldk;
    if (!ctx->d_foldin_table) {         // (the table fold-in's model lives in: one of the two at a time)
        const size_t need = cells * sizeof(double);
        size_t free_bytes = 0, total_bytes = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
        if (need + ((size_t)256 << 20) > free_bytes)
            return fail(ctx, PYLDA_ERR_OOM, "completion_set_model: the predictive table needs %zu MiB, %zu MiB of device memory are free",
                        need >> 20, free_bytes >> 20);
        FirstError A{ctx, "completion_set_model"};
        A(dev_alloc(ctx, &ctx->d_foldin_table, cells));
        A(dev_alloc(ctx, &ctx->d_foldin_alpha, (size_t)K));
        if (A.rc != PYLDA_OK) {
            dev_free(ctx->d_foldin_table); dev_free(ctx->d_foldin_alpha);
            return A.rc;
        }
    }
    if (!ctx->d_completion_rowsum) {
        const int rc = dev_alloc(ctx, &ctx->d_completion_rowsum, (size_t)K);
        if (rc != PYLDA_OK) return rc;
    }
    ctx->foldin_ready = false;          // (the counts' table is overwritten)
    ctx->completion_ready = false;
    HIP_TRY(ctx, launch_kernel(completion_rowsum_kernel, dim3((unsigned)K), dim3(256), 0, ctx->stream, ctx->d_eta, K, V,
                               ctx->d_completion_rowsum));
    HIP_TRY(ctx, launch_kernel(completion_table_kernel, dim3((unsigned)((V + 31) / 32), (unsigned)((ldk + 31) / 32)), dim3(256), 0,
                               ctx->stream, ctx->d_eta, ctx->d_completion_rowsum, K, V, ldk, ctx->d_foldin_table));
    ctx->completion_ready = true;
    return PYLDA_OK;
}

int pylda_completion_score(pylda_ctx* ctx, pylda_corpus* observed, pylda_corpus* held, const double* gamma_dk,
                           double* held_log_likelihood, int64_t* held_tokens)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    if (!held || held->ctx != ctx) return fail(ctx, PYLDA_ERR_INVALID, "completion_score: the held corpus does not belong to this context");
    if (observed && observed->ctx != ctx)
        return fail(ctx, PYLDA_ERR_INVALID, "completion_score: the observed corpus does not belong to this context");
    if (ctx->K > 64 * 16) return fail(ctx, PYLDA_ERR_INVALID, "completion_score: %d topics (at most 1024: 16 per lane)", ctx->K);
    if ((observed != nullptr) == (gamma_dk != nullptr))
        return fail(ctx, PYLDA_ERR_INVALID, "completion_score: gamma comes from the observed corpus OR from gamma_dk (%s given)",
                    observed ? "both" : "neither");
    if (observed && observed->D != held->D)
        return fail(ctx, PYLDA_ERR_INVALID, "completion_score: the observed corpus has %lld documents, the held corpus %lld",
                    (long long)observed->D, (long long)held->D);
    // the table of either model: the context's eta (completion_set_model) or the frozen counts (foldin_set_model)
    if (!ctx->completion_ready && !ctx->foldin_ready)
        return fail(ctx, PYLDA_ERR_STATE, "completion_score: no predictive table (completion_set_model or foldin_set_model first)");
    // (n_dk of a training state lives in the gamma buffer: it is no gamma, and the held corpus' buffer is written)
    if (held->gibbs_ready || (observed && observed->gibbs_ready))
        return fail(ctx, PYLDA_ERR_STATE, "completion_score: the %s corpus holds a Gibbs training state; score corpora of their own",
                    held->gibbs_ready ? "held" : "observed");
    if (observed && !observed->estep_done)
        return fail(ctx, PYLDA_ERR_STATE, "completion_score: no E-step or fold-in has run on the observed corpus");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (gamma_dk && held->D > 0)
        HIP_TRY(ctx, hipMemcpyAsync(held->d_gamma, gamma_dk, (size_t)held->D * ctx->K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

    CompletionParams p{};
    p.K = ctx->K;
    p.ldk = ctx->ldk;
    p.doc_ptr = held->d_doc_ptr;
    p.term_id = held->d_term_id;
    p.term_ct = held->d_term_ct;
    p.P = ctx->d_foldin_table;
    p.gamma = observed ? observed->d_gamma : held->d_gamma;
    p.doc_ll = held->d_doc_ll;
    p.doc_wll = held->d_doc_wll;
    p.iters = held->d_iters;
    p.status = held->d_status;
    p.D = held->D;

    const int bracket = open_bracket(ctx, -1, ctx->stream);
    if (held->D > 0) {
        const hipError_t e = with_sampler_slots(ctx->K, [&](auto S) {
            return launch_kernel(completion_score_kernel<decltype(S)::value>, dim3((unsigned)((p.D + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
        HIP_TRY(ctx, e);
    }
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, launch_kernel(completion_sum_kernel, dim3(1), dim3(1024), 0, ctx->stream, held->d_doc_wll, held->d_status, held->D,
                               held->d_doc_ll, held->d_scalars, held->d_flag_count));
    // the scalars through the context's page-locked staging area, as pylda_estep_results
    double* sc = ctx->h_pin + (size_t)5 * ctx->K + 4;
    HIP_TRY(ctx, hipMemcpyAsync(sc, held->d_scalars, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t flagged = *reinterpret_cast<const int32_t*>(sc + 3);
    if (flagged) {
        held->estep_done = false;
        return fail(ctx, PYLDA_ERR_INVALID, "completion_score: %d gamma rows whose sum is not positive and finite", (int)flagged);
    }
    held->estep_done = true;
    held->last_heldout = 1;
    held->last_doc_values = true;
    if (held_log_likelihood) *held_log_likelihood = sc[1];
    if (held_tokens) *held_tokens = (int64_t)sc[2];
    return PYLDA_OK;
}

}  // extern "C"
