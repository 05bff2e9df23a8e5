// Document-completion held-out likelihood: theta is fitted on one half of every test document by
// the engine's own held-out path, and the OTHER half is scored here.  The stage needs a gamma per document and a word-major
// predictive table, nothing else; tests/completion_restatement.py is the same estimator in numpy with exact sums.
//
//   table       P[w][k] = eta[k][w] / sum_v eta[k][v], the posterior mean of topic k: word-major V x ldk doubles, zero
//               padding - the layout AND the storage of fold-in's table (for a collapsed Gibbs model the table is the one
//               pylda_foldin_set_model builds from the counts).  Row sums: one workgroup per topic, thread t adds
//               v = t, t + 256, .. in turn, then block_sum - a fixed order; the division is rounded once.  The transposing
//               write goes through a 32 x 33 LDS tile: eta is read coalesced along v, P written coalesced along k.
//   document    one wavefront per held document; topic k in lane k / S, slot k % S (sampler_wave.h), so a lane's share of
//               a row of P is S contiguous doubles and the wavefront's read of it one contiguous 64 S 8-byte access
//   theta       gamma[d][k] / sum_k gamma[d][k]: slot sums sequential, the lane sum by wave_sum
//   score       the held terms in batches of T (64, 32, 16 for S = 1, 2, >= 4: the T partials live in registers).  Per
//               batch: part_j = sum_s theta[s] P[w_j][k0 + s] for its T terms, the partials REDUCE-SCATTERED over the
//               lanes (reduce_scatter below: lane j ends with p_j = sum_k theta_k P[w_j][k]; T - 1 exchange-adds plus one
//               per missing level, where a butterfly per term takes 6 T), ONE log per lane - the T logs side by side -
//               times c_j; lanes beyond the batch's terms hold an exact 0 and take no log; one wave_sum per batch, the
//               batches added in order.  A fixed order throughout: the same input gives the same bits, whatever the grid.
//   outputs     the held corpus' doc_wll slot, doc_ll = 0 (completion_sum_kernel; until then the document's held tokens), iters = 0; status 1 where sum_k gamma is not positive and finite
//               (the document scores 0 and the call reports it).  An empty held document scores exactly 0.
#pragma once
#include "estep_common.h"
#include "sampler_wave.h"

namespace pylda {

struct CompletionParams {
    int K, ldk;
    const int64_t* doc_ptr;     // the HELD corpus
    const int32_t* term_id;
    const int32_t* term_ct;
    const double* P;            // V x ldk
    const double* gamma;        // D x K: fitted on the observed halves
    double* doc_ll;             // D: 0
    double* doc_wll;            // D: sum_n c_n log(sum_k theta_k P[w_n][k]) over the held terms
    int32_t* iters;             // D: 0
    int32_t* status;            // D: 1 for a gamma row whose sum is not positive and finite
    int64_t D;
};

// rowsum[k] = sum_v eta[k][v]; one workgroup per topic row, the order of eta_rowsum_psi_kernel.
__global__ __launch_bounds__(256) void completion_rowsum_kernel(const double* __restrict__ eta, int K, int V,
                                                                double* __restrict__ rowsum)
{
    __shared__ double scratch[4];
    const int k = blockIdx.x;
    const double* row = eta + (size_t)k * V;
    double s = 0.0;
    for (int v = threadIdx.x; v < V; v += 256) s += row[v];
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) rowsum[k] = s;
}

// P[w][k] = eta[k][w] / rowsum[k] for k < K, 0 for K <= k < ldk.  grid (ceil(V / 32), ceil(ldk / 32)).
__global__ __launch_bounds__(256) void completion_table_kernel(const double* __restrict__ eta, const double* __restrict__ rowsum,
                                                               int K, int V, int ldk, double* __restrict__ P)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const int v0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + ty + j * 8, v = v0 + tx;
        tile[ty + j * 8][tx] = k < K && v < V ? eta[(size_t)k * V + v] / rowsum[k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = v0 + ty + j * 8, k = k0 + tx;
        if (k < ldk && v < V) P[(size_t)v * ldk + k] = tile[tx][ty + j * 8];
    }
}

template <int S>
struct CompletionBatch {
    static constexpr int value = S == 1 ? 64 : S == 2 ? 32 : 16;
};

// One level of the reduce-scatter inside a row of 16 lanes: 2 H partials -> H.  A lane whose bit `upper` is set keeps
// v[H + i] and hands v[i] to its partner (the lane the DPP control pairs it with, whose bit is clear), and the other way
// round; both then hold the sum over the pair of the partial they keep.
template <int H, int CTRL>
__device__ __forceinline__ void scatter_level(double (&v)[2 * H], bool upper)
{
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const double mine = upper ? v[H + i] : v[i];
        const double other = upper ? v[i] : v[H + i];
        v[i] = mine + dpp_f64<CTRL>(other);
    }
}

// T partials per lane (partial j: this lane's share of term j) -> lane j holds the sum over the 64 lanes of partial j;
// with T < 64 lane l holds term l % T.  The levels of wave_sum taken the other way round, each halving what a lane keeps:
//   halves of the wavefront (T = 64)     lanes 0-31 keep terms 0-31, lanes 32-63 terms 32-63       permlane32_swap
//   pairs of rows (T >= 32)              even rows keep the lower 16 of their terms, odd the upper   permlane16_swap
//   row_mirror, row_half_mirror, quad_perm [2,3,0,1], quad_perm [1,0,3,2]: bits 3, 2, 1, 0 of the lane pick the half kept
// and where T has no level to halve at, the sum over that level's pair (a = b: both lanes keep it).  Exchange-adds:
// 32 + 16 + 8 + 4 + 2 + 1 = 63 for 64 terms, 16 + 15 + 1 = 32 for 32, 15 + 2 = 17 for 16.
template <int T>
__device__ __forceinline__ double reduce_scatter(double (&part)[T], int lane)
{
    double r[16];
    if constexpr (T == 64) {
        double q[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) q[i] = swap32_add(part[i], part[i + 32]);
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = swap16_add(q[i], q[i + 16]);
    } else if constexpr (T == 32) {
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = swap16_add(part[i], part[i + 16]);
    } else {
        static_assert(T == 16, "batch of 64, 32 or 16 terms");
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = part[i];
    }
    scatter_level<8, 0x140>(r, (lane & 8) != 0);        // row_mirror: lane l <-> 15 - l of its row
    double h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = r[i];
    scatter_level<4, 0x141>(h, (lane & 4) != 0);        // row_half_mirror: l <-> l ^ 7
    double f[4] = {h[0], h[1], h[2], h[3]};
    scatter_level<2, 0x4E>(f, (lane & 2) != 0);         // quad_perm [2,3,0,1]: l <-> l ^ 2
    double t[2] = {f[0], f[1]};
    scatter_level<1, 0xB1>(t, (lane & 1) != 0);         // quad_perm [1,0,3,2]: l <-> l ^ 1
    double v = t[0];
    if constexpr (T <= 16) v = swap16_add(v, v);
    if constexpr (T <= 32) v = swap32_add(v, v);
    return v;
}

// a lane's share of row w of the table: S contiguous doubles (16-byte pieces from S = 2 on) from column kl on
template <int S>
__device__ __forceinline__ void completion_load_row(const double* __restrict__ P, int w, int ldk, int kl, double (&row)[S])
{
    const double* at = P + (size_t)w * ldk + kl;
    if constexpr (S == 1) {
        row[0] = at[0];
    } else {
        const f64x2* at2 = reinterpret_cast<const f64x2*>(at);
#pragma unroll
        for (int s = 0; s < S / 2; ++s) {
            const f64x2 two = at2[s];
            row[2 * s] = two.x;
            row[2 * s + 1] = two.y;
        }
    }
}

// The value of one batch of n <= T held terms from CSR position q0 on (FULL: n == T, no term is tested).
template <int S, int T, bool FULL>
__device__ __forceinline__ double completion_batch_value(const CompletionParams& p, const double (&th)[S], int64_t q0, int n, int lane,
                                                         int kl, long long& held)
{
    const bool mine = lane < T && (FULL || lane < n);
    const int w_lane = mine ? p.term_id[q0 + lane] : 0;
    const int c_lane = mine ? p.term_ct[q0 + lane] : 0;
    held += c_lane;
    // the rows of G terms are requested together (32 doubles per lane in flight), then folded into their partials: without
    // the fence the compiler requests all T rows first and, from S = 16 on, spills them
    constexpr int G = S >= 32 ? 1 : 32 / S;
    double part[T];
    static_for<T>([&](auto j) {
        constexpr int J = decltype(j)::value;
        if constexpr (J % G == 0 && J > 0) __builtin_amdgcn_sched_barrier(0);
        if (FULL || J < n) {
            double row[S];
            completion_load_row<S>(p.P, __builtin_amdgcn_readlane(w_lane, J), p.ldk, kl, row);
            double a = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) a = a + th[s] * row[s];
            part[J] = a;
        } else {
            part[J] = 0.0;
        }
    });
    const double pj = reduce_scatter<T>(part, lane);
    double v = 0.0;
    if (mine) v = (double)c_lane * log(pj);
    return wave_sum(v);
}

template <int S>
__global__ __launch_bounds__(256) void completion_score_kernel(CompletionParams p)
{
    constexpr int T = CompletionBatch<S>::value;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (d >= p.D) return;                                    // (whole wavefronts)
    const int K = p.K, k0 = lane * S;
    // where the lane reads a row: its own columns, padding included (the stride is a multiple of S), or - a lane wholly
    // beyond the stride, whose theta is 0 - the row's first: an address inside the table without a branch per row
    const int kl = k0 < p.ldk ? k0 : 0;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    double th[S], gpart = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        th[s] = k0 + s < K ? p.gamma[d * K + k0 + s] : 0.0;
        gpart = gpart + th[s];
    }
    const double gsum = wave_sum(gpart);
    const bool usable = gsum > 0.0 && gsum < INFINITY;
    double ll = 0.0;
    long long held = 0;                                      // this lane's share of the document's held tokens
    if (usable) {
#pragma unroll
        for (int s = 0; s < S; ++s) th[s] = th[s] / gsum;
        int64_t q = pb;
        for (; q + T <= pe; q += T) ll = ll + completion_batch_value<S, T, true>(p, th, q, T, lane, kl, held);
        if (q < pe) ll = ll + completion_batch_value<S, T, false>(p, th, q, __builtin_amdgcn_readfirstlane((int)(pe - q)), lane, kl, held);
    }
    const double tokens = wave_sum((double)held);            // (integers below 2^53: exact)
    if (lane == 0) {
        p.doc_ll[d] = tokens;                                // (on its way to completion_sum_kernel, which leaves 0 here)
        p.doc_wll[d] = ll;
        p.iters[d] = 0;
        p.status[d] = usable ? 0 : 1;
    }
}

// The corpus' scalars in one fixed-order reduction (one workgroup, every thread a fixed share): [0] 0, [1] sum_d doc_wll[d],
// [2] the held tokens - the documents' counts, which the score kernel left in the doc_ll slot and this kernel replaces by
// the slot's value, 0 (integers below 2^53: exact) - and in the fourth scalar's bytes (the corpus' count of flagged
// documents) the documents with status 1.
__global__ __launch_bounds__(1024) void completion_sum_kernel(const double* __restrict__ doc_wll, const int32_t* __restrict__ status,
                                                             int64_t D, double* __restrict__ doc_ll, double* __restrict__ scalars,
                                                             int32_t* __restrict__ flagged)
{
    __shared__ double scratch[16];
    double s = 0.0, bad = 0.0, tokens = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 1024) {
        s += doc_wll[d];
        bad += status[d] ? 1.0 : 0.0;
        tokens += doc_ll[d];
        doc_ll[d] = 0.0;
    }
    s = block_sum<1024>(s, scratch);
    bad = block_sum<1024>(bad, scratch);
    tokens = block_sum<1024>(tokens, scratch);
    if (threadIdx.x == 0) {
        scalars[0] = 0.0;
        scalars[1] = s;
        scalars[2] = tokens;
        flagged[0] = (int32_t)bad;
    }
}

}  // namespace pylda
