// libpylda_hip.so - the hybrid E-step (hybrid.py:85-171 of the reference: a Gibbs sampler per document inside the
// variational outer loop), its statistics pass, the scale step behind the all-reduce and the Philox test hook.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the chain's specification: estep_hybrid.h)
#include "sampler_host.h"
#include "estep_hybrid.h"

namespace {

// Token offsets and sample histories of a corpus (sampler_host.h; training mode also: the CSR positions grouped by term
// that its statistics pass walks, from a host copy of the term ids by a counting sort, O(nnz)): built once, on the first
// hybrid E-step that needs them.
int prepare_hybrid(pylda_ctx* ctx, pylda_corpus* c, bool postings)
{
    const bool need_postings = postings && !c->d_hyb_post_pos;
    const int64_t nnz = c->nnz;
    const int V = ctx->V;
    const size_t need = token_state_bytes(c) + (need_postings ? ((size_t)nnz + (size_t)V + 1) * sizeof(int64_t) : 0);
    int rc = check_device_room(ctx, "hybrid_estep", "the sample histories and offsets", need);
    if (rc != PYLDA_OK || (rc = ensure_token_state(ctx, c, "hybrid_estep")) != PYLDA_OK || !need_postings) return rc;
    std::vector<int32_t> ids((size_t)nnz);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (nnz) HIP_TRY(ctx, hipMemcpy(ids.data(), c->d_term_id, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> col_ptr((size_t)V + 1, 0), post((size_t)nnz);
    for (int64_t q = 0; q < nnz; ++q) col_ptr[(size_t)ids[(size_t)q] + 1] += 1;
    for (int v = 0; v < V; ++v) col_ptr[(size_t)v + 1] += col_ptr[(size_t)v];
    {
        std::vector<int64_t> at(col_ptr.begin(), col_ptr.end() - 1);
        for (int64_t q = 0; q < nnz; ++q) post[(size_t)at[(size_t)ids[(size_t)q]]++] = q;
    }
    FirstError A{ctx, "hybrid_estep"};
    A(dev_alloc(ctx, &c->d_hyb_col_ptr, (size_t)V + 1));
    A(dev_alloc(ctx, &c->d_hyb_post_pos, (size_t)nnz));
    A.h2d(c->d_hyb_col_ptr, col_ptr.data(), col_ptr.size() * sizeof(int64_t));
    A.h2d(c->d_hyb_post_pos, post.data(), post.size() * sizeof(int64_t));
    if (A.rc != PYLDA_OK) {
        dev_free(c->d_hyb_col_ptr); dev_free(c->d_hyb_post_pos);
    }
    return A.rc;
}

// what a hybrid E-step's kernels take from the context and the corpus (the chain's own parameters: the caller's)
HybridParams hybrid_params(const pylda_ctx* ctx, const pylda_corpus* c, int heldout)
{
    HybridParams p{};
    p.K = ctx->K;
    p.V = ctx->V;
    p.ldk = ctx->ldk;
    p.B = ctx->d_expElog;
    p.alpha = ctx->d_alpha;
    p.eta = ctx->d_eta;
    p.psi_rowsum = ctx->d_psi_rowsum;
    p.doc_ptr = c->d_doc_ptr;
    p.term_id = c->d_term_id;
    p.term_ct = c->d_term_ct;
    p.tok_off = c->d_tok_off;
    p.state = c->d_hyb_state;
    p.gamma = c->d_gamma;
    p.doc_ll = c->d_doc_ll;
    p.doc_wll = c->d_doc_wll;
    p.iters = c->d_iters;
    p.status = c->d_status;
    p.D = c->D;
    p.heldout = heldout;
    p.alpha_term = alpha_sums(ctx).term;
    return p;
}

}  // namespace

extern "C" {

int pylda_hybrid_estep(pylda_ctx* ctx, pylda_corpus* c, int number_of_samples, int burn_in_samples, uint64_t seed,
                       uint64_t stream, int64_t first_document, int heldout)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "hybrid_estep", first_document);
    if (rc != PYLDA_OK) return rc;
    const int K = ctx->K, bits = sampler_bits(K);
    if (number_of_samples < 1 || burn_in_samples < 0 || burn_in_samples >= number_of_samples)
        return fail(ctx, PYLDA_ERR_INVALID, "hybrid_estep: number_of_samples=%d, burn_in_samples=%d (need 0 <= burn-in < samples)",
                    number_of_samples, burn_in_samples);
    if ((int64_t)(number_of_samples - burn_in_samples + 1) * bits > 64)
        return fail(ctx, PYLDA_ERR_INVALID, "hybrid_estep: %d post-burn-in samples of %d bits each do not fit a token's 64-bit history",
                    number_of_samples - burn_in_samples, bits);
    if (stream > 0xffffffffull) return fail(ctx, PYLDA_ERR_INVALID, "hybrid_estep: stream %llu >= 2^32", (unsigned long long)stream);
    if (!ctx->have_eta || !ctx->have_alpha)
        return fail(ctx, PYLDA_ERR_STATE, "hybrid_estep: set_eta and set_alpha must be called first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    heldout = heldout ? 1 : 0;
    if ((rc = prepare_hybrid(ctx, c, heldout == 0)) != PYLDA_OK) return rc;
    if ((rc = enqueue_prepare(ctx, false)) != PYLDA_OK) return rc;

    HybridParams p = hybrid_params(ctx, c, heldout);
    p.first_document = (uint32_t)first_document;
    p.stream = (uint32_t)stream;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    p.samples = number_of_samples;
    p.burn_in = burn_in_samples;
    p.bits = bits;

    const int doc_bracket = open_bracket(ctx, -1, ctx->stream);
    if (c->D > 0) {
        const hipError_t e = with_sampler_slots(K, [&](auto S) {
            return launch_kernel(hybrid_sample_kernel<decltype(S)::value>, dim3((unsigned)((p.D + 3) / 4)), dim3(256), 0, ctx->stream, p);
        });
        HIP_TRY(ctx, e);
    }
    close_bracket(ctx, doc_bracket, ctx->stream);
    const int ss_bracket = open_bracket(ctx, -2, ctx->stream);
    if (!heldout) {
        // raw counts; pylda_hybrid_scale_sstats divides them (behind the all-reduce of a sharded run)
        hipLaunchKernelGGL(hybrid_sstats_kernel, dim3((unsigned)ctx->V), dim3(256), (size_t)K * sizeof(unsigned), ctx->stream,
                           c->d_hyb_col_ptr, c->d_hyb_post_pos, c->d_tok_off, c->d_hyb_state, K, ctx->ldk, number_of_samples,
                           burn_in_samples, bits, ctx->d_sstats);
        HIP_TRY(ctx, hipGetLastError());
    }
    close_bracket(ctx, ss_bracket, ctx->stream);
    if (doc_bracket >= 0 && ss_bracket >= 0) ctx->estep_calls += 1;      // (a call counts only with both of its brackets)
    return finish_estep(ctx, c, heldout, false, true);
}

int pylda_hybrid_scale_sstats(pylda_ctx* ctx, double divisor)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    if (!(divisor > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "hybrid_scale_sstats: divisor %g", divisor);
    if (!ctx->have_sstats) return fail(ctx, PYLDA_ERR_STATE, "hybrid_scale_sstats: no training-mode E-step has run");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n = (int64_t)ctx->V * ctx->ldk;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4 * (int64_t)ctx->num_cu));
    hipLaunchKernelGGL(hybrid_scale_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->d_sstats, n, divisor);
    HIP_TRY(ctx, hipGetLastError());
    return PYLDA_OK;
}

int pylda_test_philox(pylda_ctx* ctx, int64_t n, const uint32_t* counter_key, uint32_t* out)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    if (n < 0 || !counter_key || !out) return fail(ctx, PYLDA_ERR_INVALID, "test_philox: bad argument");
    if (n == 0) return PYLDA_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t *din = nullptr, *dout = nullptr;
    int rc = dev_alloc(ctx, &din, (size_t)n * 6);
    if (rc == PYLDA_OK) rc = dev_alloc(ctx, &dout, (size_t)n * 4);
    if (rc == PYLDA_OK) {
        hipError_t e = hipMemcpy(din, counter_key, (size_t)n * 6 * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(philox_test_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, din, n, dout);
            e = hipStreamSynchronize(ctx->stream);
        }
        if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(ctx, PYLDA_ERR_HIP, "test_philox: %s", hipGetErrorString(e));
    }
    dev_free(din);
    dev_free(dout);
    return rc;
}

}  // extern "C"
