// Host side of what the token samplers' launchers share (launch_hybrid.hip, launch_gibbs.hip, launch_foldin.hip,
// launch_left_to_right.hip; launch_completion.hip for the lane layout): the argument checks they all make, the dispatch on
// the topics per lane, and a corpus' token offsets and state words, which every engine lays out the same way and the first
// call that needs them builds.  (A header of its own: sampler_wave.h is device code, which host_internal.h stays free of.)
#pragma once
#include "host_internal.h"
#include "sampler_wave.h"

#include <type_traits>

namespace pylda_host __attribute__((visibility("hidden"))) {

// the checks of every entry point that takes a corpus into a sampler
inline int check_sampler_call(pylda_ctx* ctx, const pylda_corpus* c, const char* what, int64_t first_document)
{
    if (!c || c->ctx != ctx) return fail(ctx, PYLDA_ERR_INVALID, "%s: corpus does not belong to this context", what);
    if (ctx->K > kWave * kSamplerMaxSlots)
        return fail(ctx, PYLDA_ERR_INVALID, "%s: %d topics (at most 1024: 16 per lane)", what, ctx->K);
    if (first_document < 0 || first_document + c->D > ((int64_t)1 << 32))
        return fail(ctx, PYLDA_ERR_INVALID, "%s: first_document=%lld (global indices must stay below 2^32)", what, (long long)first_document);
    return PYLDA_OK;
}

// f(std::integral_constant<int, S>{}) for the S = sampler_slots(K) topics per lane of a kernel's instantiation
template <typename F>
auto with_sampler_slots(int K, F&& f)
{
    switch (sampler_slots(K)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, kSamplerMaxSlots>{});
    }
}

// device bytes ensure_token_offsets / ensure_token_state would allocate for this corpus (0: it has them)
inline size_t token_offsets_bytes(const pylda_corpus* c)
{
    return c->d_tok_off ? 0 : ((size_t)c->nnz + 1) * sizeof(int64_t);
}

inline size_t token_state_bytes(const pylda_corpus* c)
{
    return token_offsets_bytes(c) + (c->d_hyb_state ? 0 : (size_t)c->tokens * sizeof(uint64_t));
}

// PYLDA_ERR_OOM where `need` more bytes (the caller's `things`) would not leave 256 MiB of device memory free: asked
// before anything is allocated
inline int check_device_room(pylda_ctx* ctx, const char* what, const char* things, size_t need)
{
    if (need == 0) return PYLDA_OK;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    if (need + ((size_t)256 << 20) > free_bytes)
        return fail(ctx, PYLDA_ERR_OOM, "%s: %s need %zu MiB, %zu MiB of device memory are free", what, things, need >> 20, free_bytes >> 20);
    return PYLDA_OK;
}

// The terms' token offsets on the device (d_tok_off: the exclusive scan of term_ct, nnz + 1) and, where asked for, the
// documents' on the host (h_ltr_doc_tok, D + 1): from a host copy of the counts, O(nnz).  Nothing to do where they exist.
inline int ensure_token_offsets(pylda_ctx* ctx, pylda_corpus* c, const char* what, bool doc_tokens = false)
{
    const bool need_device = !c->d_tok_off, need_host = doc_tokens && c->h_ltr_doc_tok.empty();
    if (!need_device && !need_host) return PYLDA_OK;
    const int64_t nnz = c->nnz, D = c->D;
    std::vector<int32_t> cts((size_t)nnz);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (nnz) HIP_TRY(ctx, hipMemcpy(cts.data(), c->d_term_ct, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> tok_off((size_t)nnz + 1, 0);
    for (int64_t q = 0; q < nnz; ++q) tok_off[(size_t)q + 1] = tok_off[(size_t)q] + cts[(size_t)q];
    if (need_host) {
        std::vector<int64_t> ptr((size_t)D + 1, 0);
        HIP_TRY(ctx, hipMemcpy(ptr.data(), c->d_doc_ptr, ((size_t)D + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        c->h_ltr_doc_tok.assign((size_t)D + 1, 0);
        for (int64_t d = 0; d <= D; ++d) c->h_ltr_doc_tok[(size_t)d] = tok_off[(size_t)ptr[(size_t)d]];
    }
    if (!need_device) return PYLDA_OK;
    FirstError A{ctx, what};
    A(dev_alloc(ctx, &c->d_tok_off, (size_t)nnz + 1));
    A.h2d(c->d_tok_off, tok_off.data(), tok_off.size() * sizeof(int64_t));
    if (A.rc != PYLDA_OK) dev_free(c->d_tok_off);
    return A.rc;
}

// ... and one state word per token (d_hyb_state; what it holds is the engine's own)
inline int ensure_token_state(pylda_ctx* ctx, pylda_corpus* c, const char* what)
{
    const int rc = ensure_token_offsets(ctx, c, what);
    if (rc != PYLDA_OK || c->d_hyb_state) return rc;
    return dev_alloc(ctx, &c->d_hyb_state, (size_t)c->tokens);
}

// A count table between the device's word-major V x ldk layout and the caller's K x V array (T: double, int32_t); the
// padding columns K .. ldk - 1 go up as zeros.  Plain copies: the callers have waited for the stream.
template <typename T>
int table_to_host(pylda_ctx* ctx, const T* d_table, T* n_kv)
{
    const int K = ctx->K, V = ctx->V, ldk = ctx->ldk;
    std::vector<T> table((size_t)V * ldk);
    HIP_TRY(ctx, hipMemcpy(table.data(), d_table, table.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < K; ++k) n_kv[(size_t)k * V + v] = table[(size_t)v * ldk + k];
    return PYLDA_OK;
}

template <typename T>
int table_from_host(pylda_ctx* ctx, T* d_table, const T* n_kv)
{
    const int K = ctx->K, V = ctx->V, ldk = ctx->ldk;
    std::vector<T> table((size_t)V * ldk, T(0));
    for (int k = 0; k < K; ++k)
        for (int v = 0; v < V; ++v) table[(size_t)v * ldk + k] = n_kv[(size_t)k * V + v];
    HIP_TRY(ctx, hipMemcpy(d_table, table.data(), table.size() * sizeof(T), hipMemcpyHostToDevice));
    return PYLDA_OK;
}

}  // namespace pylda_host
