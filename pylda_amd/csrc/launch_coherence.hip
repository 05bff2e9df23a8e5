// libpylda_hip.so - topic coherence: the top words of every topic, and for every pair of a topic's top words the documents
// of a reference corpus that contain both.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the definitions: coherence_kernels.h)
//
// Memory: every buffer of a call is allocated by the call and freed before it returns (DeviceBuffers below); nothing is
// cached on the context.  The bitmaps take at most a quarter of the device memory free at the time - the rule of the
// gather's rounds - and where the whole corpus does not fit, or the option "coherence_chunk_docs" says so, the documents
// are walked in chunks of a multiple of 64 and the counts accumulate over the chunks: integer sums, the same whatever
// the chunk.
#include "host_internal.h"
#include "coherence_kernels.h"

namespace {

// the device buffers of one call: freed when the call returns, by whichever path
struct DeviceBuffers {
    std::vector<void*> held;
    ~DeviceBuffers()
    {
        for (void* p : held) (void)hipFree(p);
    }
    template <typename T>
    int alloc(pylda_ctx* ctx, T** p, size_t n)
    {
        const int rc = dev_alloc(ctx, p, n);
        if (rc == PYLDA_OK) held.push_back(*p);
        return rc;
    }
};

constexpr size_t kMemoryMargin = (size_t)256 << 20;     // left free beside a scratch table, as the predictive tables leave it

}  // namespace

extern "C" {

int pylda_top_words(pylda_ctx* ctx, const double* table_kv, int M, int32_t* ids_km, double* values_km)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    const int K = ctx->K, V = ctx->V;
    if (M < 1 || M > kCoherenceMaxWords) return fail(ctx, PYLDA_ERR_INVALID, "top_words: M=%d (1 .. %d)", M, kCoherenceMaxWords);
    if (M > V) return fail(ctx, PYLDA_ERR_INVALID, "top_words: M=%d, but the vocabulary has %d words", M, V);
    if (!ids_km || !values_km) return fail(ctx, PYLDA_ERR_INVALID, "top_words: %s is NULL", ids_km ? "values_km" : "ids_km");
    if (!table_kv && !ctx->have_eta) return fail(ctx, PYLDA_ERR_STATE, "top_words: no table given and eta was never set");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DeviceBuffers buffers;
    const size_t cells = (size_t)K * V, out = (size_t)K * M;
    const double* d_table = ctx->d_eta;
    if (table_kv) {
        size_t free_bytes = 0, total_bytes = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
        if (cells * sizeof(double) + kMemoryMargin > free_bytes)
            return fail(ctx, PYLDA_ERR_OOM, "top_words: the table needs %zu MiB, %zu MiB of device memory are free",
                        (cells * sizeof(double)) >> 20, free_bytes >> 20);
        double* d_scratch = nullptr;
        const int rc = buffers.alloc(ctx, &d_scratch, cells);
        if (rc != PYLDA_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_scratch, table_kv, cells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        d_table = d_scratch;
    }
    int32_t* d_ids = nullptr;
    double* d_values = nullptr;
    int rc = buffers.alloc(ctx, &d_ids, out);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_values, out);
    if (rc != PYLDA_OK) return rc;
    const int bracket = open_bracket(ctx, -1, ctx->stream);
    HIP_TRY(ctx, launch_kernel(coherence_select_kernel, dim3((unsigned)K), dim3(kSelectThreads), 0, ctx->stream, d_table, V, M, d_ids,
                               d_values));
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(ids_km, d_ids, out * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(values_km, d_values, out * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PYLDA_OK;
}

int pylda_codocument_counts(pylda_ctx* ctx, pylda_corpus* reference, int M, const int32_t* ids_km, int64_t* doc_freq_km, int64_t* co_kmm)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    const int K = ctx->K, V = ctx->V;
    if (!reference || reference->ctx != ctx)
        return fail(ctx, PYLDA_ERR_INVALID, "codocument_counts: the reference corpus does not belong to this context");
    if (M < 1 || M > kCoherenceMaxWords) return fail(ctx, PYLDA_ERR_INVALID, "codocument_counts: M=%d (1 .. %d)", M, kCoherenceMaxWords);
    if (!ids_km || !doc_freq_km || !co_kmm)
        return fail(ctx, PYLDA_ERR_INVALID, "codocument_counts: %s is NULL", !ids_km ? "ids_km" : !doc_freq_km ? "doc_freq_km" : "co_kmm");
    if (reference->D < 1) return fail(ctx, PYLDA_ERR_INVALID, "codocument_counts: the reference corpus has no documents");
    const size_t tops = (size_t)K * M;
    for (size_t i = 0; i < tops; ++i)
        if (ids_km[i] < 0 || ids_km[i] >= V)
            return fail(ctx, PYLDA_ERR_INVALID, "codocument_counts: ids[%zu][%zu]=%d is not a word id (0 .. %d)", i / M, i % M,
                        (int)ids_km[i], V - 1);
    // the slot map: the distinct words among the ids in order of first appearance; words shared between topics, or
    // repeated inside one, share a slot
    std::vector<int32_t> slot_of_word((size_t)V, -1), slot_of_top(tops);
    int32_t slots = 0;
    for (size_t i = 0; i < tops; ++i) {
        int32_t& slot = slot_of_word[(size_t)ids_km[i]];
        if (slot < 0) slot = slots++;
        slot_of_top[i] = slot;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // documents per chunk: what a quarter of the free memory holds, in multiples of 64, or the option's figure
    const int64_t D = reference->D;
    const int64_t D64 = (D + 63) / 64 * 64;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const int64_t fit_words = (int64_t)(free_bytes / 4 / sizeof(uint64_t) / (size_t)slots);
    if (fit_words < 1)
        return fail(ctx, PYLDA_ERR_OOM, "codocument_counts: %d bitmaps of 64 documents need %zu bytes, a quarter of the free device memory is %zu",
                    (int)slots, (size_t)slots * sizeof(uint64_t), free_bytes / 4);
    int64_t chunk_docs = std::min(D64, fit_words * 64);
    if (ctx->coherence_chunk_docs > 0) chunk_docs = std::min(chunk_docs, ctx->coherence_chunk_docs);
    const int64_t words = chunk_docs / 64;

    DeviceBuffers buffers;
    int32_t *d_slot_of_word = nullptr, *d_slot_of_top = nullptr;
    unsigned long long *d_bits = nullptr, *d_co = nullptr;
    const size_t co_cells = tops * M, bit_words = (size_t)slots * words;
    int rc = buffers.alloc(ctx, &d_slot_of_word, (size_t)V);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_slot_of_top, tops);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_co, co_cells);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_bits, bit_words);
    if (rc != PYLDA_OK) return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_slot_of_word, slot_of_word.data(), (size_t)V * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_slot_of_top, slot_of_top.data(), tops * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_co, 0, co_cells * sizeof(uint64_t), st));
    for (int64_t d0 = 0; d0 < D; d0 += chunk_docs) {
        const int64_t n_docs = std::min(chunk_docs, D - d0);
        const int64_t n_words = (n_docs + 63) / 64;                    // (the words of the chunk that can hold a bit)
        HIP_TRY(ctx, hipMemsetAsync(d_bits, 0, bit_words * sizeof(uint64_t), st));
        int bracket = open_bracket(ctx, -1, st);
        HIP_TRY(ctx, launch_kernel(coherence_mark_kernel, dim3((unsigned)((n_docs + 3) / 4)), dim3(256), 0, st, reference->d_doc_ptr,
                                   reference->d_term_id, d_slot_of_word, d0, n_docs, words, d_bits));
        close_bracket(ctx, bracket, st);
        bracket = open_bracket(ctx, -2, st);
        HIP_TRY(ctx, launch_kernel(coherence_pair_kernel, dim3((unsigned)((n_words + kPairTile - 1) / kPairTile), (unsigned)K),
                                   dim3(kPairThreads), 0, st, d_bits, words, d_slot_of_top, M, d_co));
        close_bracket(ctx, bracket, st);
    }
    HIP_TRY(ctx, hipMemcpyAsync(co_kmm, d_co, co_cells * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < tops; ++i) doc_freq_km[i] = co_kmm[i * M + i % M];     // the diagonal: D(v) = D(v, v)
    return PYLDA_OK;
}

}  // extern "C"
