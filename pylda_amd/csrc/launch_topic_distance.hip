// libpylda_hip.so - topic distances between two models: the Ka x Kb matrix of Bhattacharyya coefficients or of
// Jensen-Shannon divergences between the rows of two (K', V) tables.
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the arithmetic: topic_distance_kernels.h)
//
// Memory: the transformed tables, the segments' sums and the result are buffers of the call, at most three quarters of
// the device memory free at the time, freed before it returns.
#include "host_internal.h"
#include "topic_distance_kernels.h"

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

// rows that the transform cannot take: a negative or non-finite entry, or a sum that is not positive and finite - the
// sum in the device's order (lane l adds v = l mod 64 in ascending v, then the tree), so that host and device agree on
// which rows those are
int64_t bad_rows(const double* rows, int n, int V)
{
    int64_t bad = 0;
    for (int r = 0; r < n; ++r) {
        const double* t = rows + (size_t)r * V;
        bool ok = true;
        double lane[kWave];
        for (int l = 0; l < kWave; ++l) lane[l] = 0.0;
        for (int v = 0; v < V; ++v) {
            ok = ok && t[v] >= 0.0 && std::isfinite(t[v]);
            lane[v & (kWave - 1)] = lane[v & (kWave - 1)] + t[v];
        }
        for (int m = kWave / 2; m >= 1; m >>= 1)
            for (int l = 0; l < m; ++l) lane[l] = lane[l] + lane[l + m];    // (lane l of the tree, l < m: x_l + x_(l xor m))
        ok = ok && lane[0] > 0.0 && std::isfinite(lane[0]);
        bad += ok ? 0 : 1;
    }
    return bad;
}

// Groups of segments.  One group needs no scratch and adds in registers; it is the choice once the tiles alone put two
// workgroups on every compute unit (K = 1024 against itself: 528 tiles).  Fewer tiles want segments in flight: as many
// groups as bring the launch to four workgroups a compute unit, no more than there are segments.
int segment_groups(int64_t tiles, int segments, int num_cu)
{
    if (tiles >= 2 * (int64_t)num_cu) return 1;
    const int64_t want = (4 * (int64_t)num_cu + tiles - 1) / tiles;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, segments));
}

// every refusal that needs no device memory: the arguments, then the rows of both tables (the context's eta read back for
// it: a copy, not a launch - its rows are checked on the host like any others)
int check_tables(pylda_ctx* ctx, const double* a_kv, int Ka, const double* b_kv, int Kb, int metric, const double* out_ab)
{
    const int V = ctx->V;
    if (metric < 0 || metric > 1) return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: metric=%d (0 hellinger, 1 jensen_shannon)", metric);
    if (!out_ab) return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: out_ab is NULL");
    if (!a_kv) {
        if (!ctx->have_eta) return fail(ctx, PYLDA_ERR_STATE, "topic_distances: a_kv is NULL and eta was never set");
        if (Ka != ctx->K) return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: a_kv is NULL (the context's eta) and Ka=%d is not K=%d", Ka, ctx->K);
    }
    if (Ka < 1 || Ka > kTdMaxRows) return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: Ka=%d (1 .. %d)", Ka, kTdMaxRows);
    if (!b_kv && Kb != Ka) return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: b_kv is NULL (a against itself) and Kb=%d is not Ka=%d", Kb, Ka);
    if (Kb < 1 || Kb > kTdMaxRows) return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: Kb=%d (1 .. %d)", Kb, kTdMaxRows);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t a_cells = (size_t)Ka * V;
    std::vector<double> eta;
    if (!a_kv) {
        try {
            eta.resize(a_cells);
        } catch (const std::bad_alloc&) {
            return fail(ctx, PYLDA_ERR_OOM, "topic_distances: %zu MiB of host memory for the check of eta", (a_cells * sizeof(double)) >> 20);
        }
        HIP_TRY(ctx, hipMemcpyAsync(eta.data(), ctx->d_eta, a_cells * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    int64_t bad = bad_rows(a_kv ? a_kv : eta.data(), Ka, V);
    if (bad)
        return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: %lld of %d rows of a have a negative or non-finite entry or a sum that is not "
                    "positive and finite", (long long)bad, Ka);
    bad = b_kv ? bad_rows(b_kv, Kb, V) : 0;
    if (bad)
        return fail(ctx, PYLDA_ERR_INVALID, "topic_distances: %lld of %d rows of b have a negative or non-finite entry or a sum that is not "
                    "positive and finite", (long long)bad, Kb);
    return PYLDA_OK;
}

// the launch shape, and what it needs of the device memory
struct Shape {
    int tiles_a, tiles_b, segments, groups, per_group;
    size_t a_cells, b_cells, out_cells;
};

int choose_shape(pylda_ctx* ctx, int Ka, int Kb, bool symmetric, int metric, Shape* shape)
{
    Shape& s = *shape;
    s.tiles_a = (Ka + kTdTile - 1) / kTdTile;
    s.tiles_b = (Kb + kTdTile - 1) / kTdTile;
    s.segments = (ctx->V + kTdSegment - 1) / kTdSegment;
    s.a_cells = (size_t)Ka * ctx->V;
    s.b_cells = symmetric ? 0 : (size_t)Kb * ctx->V;
    s.out_cells = (size_t)Ka * Kb;
    const int64_t tiles = symmetric ? (int64_t)s.tiles_a * (s.tiles_a + 1) / 2 : (int64_t)s.tiles_a * s.tiles_b;
    const size_t fixed_bytes = ((s.a_cells + s.b_cells) * (metric == 1 ? 2 : 1) + s.out_cells) * sizeof(double);
    const size_t part_bytes = (size_t)s.segments * s.out_cells * sizeof(double);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                    // (what the stream still holds may free memory)
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const size_t budget = free_bytes / 4 * 3;
    int groups = ctx->topic_distance_segment_groups;
    if (groups <= 0) {
        groups = segment_groups(tiles, s.segments, ctx->num_cu);
        if (groups > 1 && fixed_bytes + part_bytes > budget) groups = 1;    // (one group needs no segments' sums)
    }
    groups = std::max(1, std::min(groups, s.segments));
    s.per_group = (s.segments + groups - 1) / groups;
    s.groups = (s.segments + s.per_group - 1) / s.per_group;            // (no group without a segment)
    const size_t need = fixed_bytes + (s.groups > 1 ? part_bytes : 0);
    if (need > budget)
        return fail(ctx, PYLDA_ERR_OOM, "topic_distances: the tables, %d segments' sums and the result need %zu MiB, three quarters of the free "
                    "device memory are %zu MiB", s.groups > 1 ? s.segments : 0, need >> 20, budget >> 20);
    return PYLDA_OK;
}

}  // namespace

extern "C" {

int pylda_topic_distances(pylda_ctx* ctx, const double* a_kv, int Ka, const double* b_kv, int Kb, int metric, double* out_ab)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_tables(ctx, a_kv, Ka, b_kv, Kb, metric, out_ab);
    if (rc != PYLDA_OK) return rc;
    const int V = ctx->V;
    const bool symmetric = !b_kv;
    Shape s;
    rc = choose_shape(ctx, Ka, Kb, symmetric, metric, &s);
    if (rc != PYLDA_OK) return rc;
    hipStream_t st = ctx->stream;

    DeviceBuffers buffers;
    double *d_a0 = nullptr, *d_a1 = nullptr, *d_b0 = nullptr, *d_b1 = nullptr, *d_out = nullptr, *d_part = nullptr;
    rc = buffers.alloc(ctx, &d_a0, s.a_cells);
    if (rc == PYLDA_OK && metric == 1) rc = buffers.alloc(ctx, &d_a1, s.a_cells);
    if (rc == PYLDA_OK && !symmetric) rc = buffers.alloc(ctx, &d_b0, s.b_cells);
    if (rc == PYLDA_OK && !symmetric && metric == 1) rc = buffers.alloc(ctx, &d_b1, s.b_cells);
    if (rc == PYLDA_OK) rc = buffers.alloc(ctx, &d_out, s.out_cells);
    if (rc == PYLDA_OK && s.groups > 1) rc = buffers.alloc(ctx, &d_part, (size_t)s.segments * s.out_cells);
    if (rc != PYLDA_OK) return rc;
    if (a_kv) HIP_TRY(ctx, hipMemcpyAsync(d_a0, a_kv, s.a_cells * sizeof(double), hipMemcpyHostToDevice, st));
    if (!symmetric) HIP_TRY(ctx, hipMemcpyAsync(d_b0, b_kv, s.b_cells * sizeof(double), hipMemcpyHostToDevice, st));

    int bracket = open_bracket(ctx, -1, st);
    hipError_t e = launch_kernel(topic_distance_transform_kernel, dim3((unsigned)((Ka + 3) / 4)), dim3(kTdThreads), 0, st,
                                 a_kv ? (const double*)d_a0 : (const double*)ctx->d_eta, Ka, V, metric, d_a0, d_a1);
    if (e == hipSuccess && !symmetric)
        e = launch_kernel(topic_distance_transform_kernel, dim3((unsigned)((Kb + 3) / 4)), dim3(kTdThreads), 0, st, (const double*)d_b0, Kb, V,
                          metric, d_b0, d_b1);
    close_bracket(ctx, bracket, st);
    if (e == hipSuccess) {
        bracket = open_bracket(ctx, -2, st);
        const dim3 grid((unsigned)s.tiles_a, (unsigned)s.tiles_b, (unsigned)s.groups);
        const double* p_b0 = symmetric ? d_a0 : d_b0;
        const double* p_b1 = symmetric ? d_a1 : d_b1;
        if (metric == 1)
            e = launch_kernel(topic_distance_pair_kernel<true>, grid, dim3(kTdThreads), 0, st, (const double*)d_a0, (const double*)d_a1, Ka, p_b0,
                              p_b1, Kb, V, (int)symmetric, s.segments, s.per_group, d_out, d_part);
        else
            e = launch_kernel(topic_distance_pair_kernel<false>, grid, dim3(kTdThreads), 0, st, (const double*)d_a0, (const double*)d_a1, Ka, p_b0,
                              p_b1, Kb, V, (int)symmetric, s.segments, s.per_group, d_out, d_part);
        if (e == hipSuccess && s.groups > 1)
            e = launch_kernel(topic_distance_combine_kernel, dim3((unsigned)((s.out_cells + kTdThreads - 1) / kTdThreads)), dim3(kTdThreads), 0, st,
                              (const double*)d_part, Ka, Kb, s.segments, (int)symmetric, metric, d_out);
        close_bracket(ctx, bracket, st);
    }
    if (e != hipSuccess) rc = fail(ctx, PYLDA_ERR_HIP, "topic_distances: launch failed: %s", hipGetErrorString(e));
    if (rc == PYLDA_OK) HIP_TRY(ctx, hipMemcpyAsync(out_ab, d_out, s.out_cells * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                             // (the buffers are freed on return, whatever rc)
    return rc;
}

}  // extern "C"
