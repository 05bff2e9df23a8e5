// libpylda_hip.so - nearest documents by topic mixture: a base of rows kept on the device, and for every query row the
// first N rows of the base by their score.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the arithmetic: similarity_kernels.h)
//
// Memory: the base belongs to the context (at most a quarter of the device memory free when it is set); the queries, the
// slices' lists and the results are buffers of the call, freed before it returns.
#include "host_internal.h"
#include "similarity_kernels.h"

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

// rows that the transform cannot take: 0 wants finite entries; 1 and 2 want no negative entry and a positive, finite
// sum - the sum in the device's order, so that host and device agree on which rows those are
int64_t bad_rows(const double* rows, int64_t n, int K, int transform)
{
    int64_t bad = 0;
    for (int64_t r = 0; r < n; ++r) {
        const double* g = rows + r * K;
        bool ok = true;
        if (transform == 0) {
            for (int k = 0; k < K; ++k) ok = ok && std::isfinite(g[k]);
        } else {
            double s = 0.0;
            for (int k = 0; k < K; ++k) {
                ok = ok && !(g[k] < 0.0);
                s = s + g[k];
            }
            ok = ok && s > 0.0 && std::isfinite(s);
        }
        bad += ok ? 0 : 1;
    }
    return bad;
}

const char* const kBadRow[3] = {"a non-finite entry", "a negative entry or a sum that is not positive and finite",
                                "a negative entry or a sum that is not positive and finite"};

// The slices that cost least by "rounds of resident workgroups x (tiles a workgroup walks + its fixed cost)", the fewest
// among equals: the workgroups of a launch run in rounds of `resident`, and a last round that is nearly empty costs as much
// as a full one (157 query blocks x 5 slices on 512 places: two rounds of 157 tiles; x 13 slices: four of 61).  The fixed
// cost of a workgroup - its start, the first loads with nothing to hide behind, the lists filling up from empty, their
// write-out and their share of the merge - is put at kSliceFixedTiles tiles: without it the count runs to one tile a
// slice, which measured at twice the time of 5 slices.
constexpr int64_t kSliceFixedTiles = 4;
int64_t similarity_slices(int64_t qblocks, int64_t tiles, int64_t most, int64_t resident)
{
    int64_t best = 1, best_cost = INT64_MAX;
    for (int64_t s = 1; s <= most; ++s) {
        const int64_t walked = (tiles + s - 1) / s;
        const int64_t used = (tiles + walked - 1) / walked;             // (slices that get a tile)
        const int64_t rounds = (qblocks * used + resident - 1) / resident;
        if (rounds * (walked + kSliceFixedTiles) < best_cost) {
            best_cost = rounds * (walked + kSliceFixedTiles);
            best = s;
        }
    }
    return best;
}

int enqueue_transform(pylda_ctx* ctx, double* d_rows, int64_t n, int transform)
{
    if (transform == 0) return PYLDA_OK;
    HIP_TRY(ctx, launch_kernel(similarity_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_rows, n, ctx->K,
                               transform));
    return PYLDA_OK;
}

}  // namespace

extern "C" {

int pylda_similarity_set_base(pylda_ctx* ctx, int64_t D, const double* rows_dk, int transform)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    const int K = ctx->K;
    if (D < 1 || D > (int64_t)INT32_MAX) return fail(ctx, PYLDA_ERR_INVALID, "similarity_set_base: D=%lld (1 .. 2^31 - 1)", (long long)D);
    if (transform < 0 || transform > 2) return fail(ctx, PYLDA_ERR_INVALID, "similarity_set_base: transform=%d (0 .. 2)", transform);
    if (!rows_dk) return fail(ctx, PYLDA_ERR_INVALID, "similarity_set_base: rows_dk is NULL");
    const int64_t bad = bad_rows(rows_dk, D, K, transform);
    if (bad)
        return fail(ctx, PYLDA_ERR_INVALID, "similarity_set_base: %lld of %lld rows have %s (transform %d)", (long long)bad, (long long)D,
                    kBadRow[transform], transform);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                    // (nothing may still read the base this one replaces)
    dev_free(ctx->d_similarity_base);
    ctx->similarity_D = 0;
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const size_t cells = (size_t)D * K;
    if (cells * sizeof(double) > free_bytes / 4)
        return fail(ctx, PYLDA_ERR_OOM, "similarity_set_base: the base needs %zu MiB, a quarter of the free device memory is %zu MiB",
                    (cells * sizeof(double)) >> 20, (free_bytes / 4) >> 20);
    int rc = dev_alloc(ctx, &ctx->d_similarity_base, cells);
    if (rc != PYLDA_OK) return rc;
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(ctx->d_similarity_base, rows_dk, cells * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const int bracket = open_bracket(ctx, -1, st);
        rc = enqueue_transform(ctx, ctx->d_similarity_base, D, transform);
        close_bracket(ctx, bracket, st);
        if (rc == PYLDA_OK) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess || rc != PYLDA_OK) {
        dev_free(ctx->d_similarity_base);
        return rc != PYLDA_OK ? rc : fail(ctx, PYLDA_ERR_HIP, "similarity_set_base: %s", hipGetErrorString(e));
    }
    ctx->similarity_D = D;
    return PYLDA_OK;
}

int pylda_similar_documents(pylda_ctx* ctx, int64_t Q, const double* rows_qk, int transform, int N, const int32_t* self_ids,
                            int32_t* ids_qn, double* scores_qn)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    const int K = ctx->K;
    const int64_t D = ctx->similarity_D;
    if (Q < 1) return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: Q=%lld", (long long)Q);
    if (N < 1 || N > kSimilarityMaxN) return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: N=%d (1 .. %d)", N, kSimilarityMaxN);
    if (transform < 0 || transform > 2) return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: transform=%d (0 .. 2)", transform);
    if (!rows_qk || !ids_qn || !scores_qn)
        return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: %s is NULL", !rows_qk ? "rows_qk" : !ids_qn ? "ids_qn" : "scores_qn");
    if (!ctx->d_similarity_base || D < 1) return fail(ctx, PYLDA_ERR_STATE, "similar_documents: no base (pylda_similarity_set_base)");
    if (self_ids)
        for (int64_t q = 0; q < Q; ++q)
            if (self_ids[q] < -1 || self_ids[q] >= D)
                return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: self_ids[%lld]=%d (-1 .. %lld)", (long long)q, (int)self_ids[q],
                            (long long)(D - 1));
    const int64_t bad = bad_rows(rows_qk, Q, K, transform);
    if (bad)
        return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: %lld of %lld rows have %s (transform %d)", (long long)bad, (long long)Q,
                    kBadRow[transform], transform);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // the launch shape: (query block, slice) workgroups that fill the compute units in whole rounds, no slice without a tile
    const int64_t tiles = (D + kSimBD - 1) / kSimBD;
    const int64_t qblocks = (Q + kSimBQ - 1) / kSimBQ;
    const int64_t most = std::min<int64_t>(tiles, kSimMaxSlices);
    int64_t want = ctx->similarity_doc_slices;
    if (want <= 0) {
        int resident = 0;
        HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, similarity_topn_kernel, kSimThreads, 0));
        // (the slices' lists are Q x slices x N entries of 12 bytes: the automatic choice keeps them within 1 GiB)
        const int64_t lists_fit = std::max<int64_t>(1, ((int64_t)1 << 30) / (12 * Q * (int64_t)N));
        want = similarity_slices(qblocks, tiles, std::min(most, lists_fit), (int64_t)std::max(resident, 1) * ctx->num_cu);
    }
    want = std::max<int64_t>(1, std::min<int64_t>(want, most));
    const int64_t tiles_per_slice = (tiles + want - 1) / want;
    const int slices = (int)((tiles + tiles_per_slice - 1) / tiles_per_slice);
    if (qblocks > (int64_t)INT32_MAX) return fail(ctx, PYLDA_ERR_INVALID, "similar_documents: Q=%lld is more than one launch takes", (long long)Q);

    DeviceBuffers buffers;
    double *d_rows = nullptr, *d_part_v = nullptr, *d_scores = nullptr;
    int32_t *d_self = nullptr, *d_part_i = nullptr, *d_ids = nullptr;
    const size_t cells = (size_t)Q * K, parts = (size_t)Q * slices * N, out = (size_t)Q * N;
    int rc = buffers.alloc(ctx, &d_rows, cells);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_part_v, parts);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_part_i, parts);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_ids, out);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_scores, out);
    if (rc == PYLDA_OK && self_ids) rc = buffers.alloc(ctx, &d_self, (size_t)Q);
    if (rc != PYLDA_OK) return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_rows, rows_qk, cells * sizeof(double), hipMemcpyHostToDevice, st));
    if (self_ids) HIP_TRY(ctx, hipMemcpyAsync(d_self, self_ids, (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int bracket = open_bracket(ctx, -1, st);
    rc = enqueue_transform(ctx, d_rows, Q, transform);
    if (rc == PYLDA_OK) {
        const hipError_t e = launch_kernel(similarity_topn_kernel, dim3((unsigned)qblocks, (unsigned)slices), dim3(kSimThreads), 0, st,
                                           (const double*)d_rows, Q, (const double*)ctx->d_similarity_base, D, K, N, (const int32_t*)d_self,
                                           tiles, tiles_per_slice, d_part_v, d_part_i);
        if (e != hipSuccess) rc = fail(ctx, PYLDA_ERR_HIP, "similar_documents: launch failed: %s", hipGetErrorString(e));
    }
    close_bracket(ctx, bracket, st);
    if (rc == PYLDA_OK) {
        bracket = open_bracket(ctx, -2, st);
        const hipError_t e = launch_kernel(similarity_merge_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(kSimMergeThreads), 0, st,
                                           (const double*)d_part_v, (const int32_t*)d_part_i, Q, slices, N, d_ids, d_scores);
        if (e != hipSuccess) rc = fail(ctx, PYLDA_ERR_HIP, "similar_documents: launch failed: %s", hipGetErrorString(e));
        close_bracket(ctx, bracket, st);
    }
    if (rc == PYLDA_OK) {
        HIP_TRY(ctx, hipMemcpyAsync(ids_qn, d_ids, out * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(scores_qn, d_scores, out * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));                             // (the buffers are freed on return, whatever rc)
    return rc;
}

}  // extern "C"
