// Topic distances between two models: for two tables a (Ka, V) and b (Kb, V) of non-negative
// doubles the Ka x Kb matrix of Bhattacharyya coefficients or of Jensen-Shannon divergences (nats) between their rows,
// each row normalised to a distribution over the V words.  tests/topic_distance_restatement.py is the same arithmetic in
// numpy: the Hellinger path equals it bit for bit, the Jensen-Shannon path up to the device's log.
//
//   transform  one wavefront per row.  s: lane l adds the entries t_v with v = l (mod 64) in ascending v, starting at +0.0;
//              the 64 partials then go through the fixed tree x_l = x_l + x_(l xor m), m = 32, 16, 8, 4, 2, 1 (an add
//              commutes, so every lane ends with the same bits).  p_v = t_v / s.  Metric 0 stores sqrt(p_v) (rounded once);
//              metric 1 stores p_v and log(p_v), the log as 0 where p_v is 0.
//   pair       grid (tile of a's rows, tile of b's rows, group of segments), 256 threads.  V is cut into segments of
//              kTdSegment words.  A segment's sum starts at +0.0 and adds its terms in ascending v, one thread per pair,
//              never split over lanes; every multiply and every add is rounded once (no FMA: -ffp-contract=off, and the
//              pragma below).  A workgroup holds 32 rows of a and 32 of b and walks its segments in chunks of 32 words
//              through LDS (stored v-major, so that a thread reads its operands as 16-byte pairs: a broadcast for a's
//              rows, 16 lanes x 16 bytes contiguous for b's).  A thread owns 2 x 2 pairs.
//                metric 0  term = sa_v * sb_v
//                metric 1  m = 0.5 * (p + q), lm = log(m), term = p * (lp - lm) + q * (lq - lm), exactly 0 where m == 0;
//                          the sum of the terms is KL(p || m) + KL(q || m), and the divergence is half of it: the finished
//                          sum is multiplied by 0.5 once, where it is written (exact: a power of two)
//              One group of segments: the workgroup adds its segments' sums in ascending order in registers, from +0.0,
//              and writes the result.  Several groups: every segment's sum goes to part (segments, Ka, Kb) and the combine
//              kernel adds them in the same order - the same bits.
//              b == a (symmetric): only the tiles on or above the diagonal run; a tile above it also writes its mirror.
//              Both terms commute in (a, b), so the matrix is symmetric bit for bit, a diagonal tile included.
//              Padding: rows beyond Ka or Kb and words beyond V are zeros in LDS (for metric 1: p = 0, lp = 0).  Their
//              terms are +0.0, and a sum is never -0.0 (it starts as +0.0 + x), so adding them changes no bit.
//   combine    one thread per output: out = (((+0.0 + part_0) + part_1) + ...) over the segments in ascending order (times
//              0.5 for metric 1); in the symmetric case an output below the diagonal tiles reads its mirror's sums.
// No atomics: every output element has one owner.
#pragma once
#include "estep_common.h"

#pragma clang fp contract(off)

namespace pylda {

constexpr int kTdMaxRows = 1 << 15;         // rows of either table
constexpr int kTdThreads = 256;
constexpr int kTdTile = 32;                 // rows of a, and of b, of a workgroup
constexpr int kTdChunk = 32;                // words of a chunk
constexpr int kTdSegment = 1024;            // words of a segment
constexpr int kTdCells = kTdChunk * kTdTile;    // doubles of one operand's chunk
static_assert(kTdSegment % kTdChunk == 0, "a chunk lies in one segment");
static_assert(kTdThreads == (kTdTile / 2) * (kTdTile / 2), "a thread owns 2 x 2 pairs of the tile");
static_assert(kTdCells == 4 * kTdThreads, "a thread loads 4 words of one row of either operand");

// grid ceil(rows / 4), 256 threads: one wavefront per row.  src (rows, V); out0, out1 (rows, V), out1 only for metric 1.
// out0 may be src: a lane reads and writes the same entries, after the row's sum.
__global__ __launch_bounds__(kTdThreads) void topic_distance_transform_kernel(const double* src, int rows, int V, int metric, double* out0,
                                                                              double* out1)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int row = blockIdx.x * (kTdThreads / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (row >= rows) return;                                            // (whole wavefronts)
    const double* t = src + (size_t)row * V;
    double s = 0.0;
    for (int v = lane; v < V; v += kWave) s = s + t[v];
    for (int m = kWave / 2; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, kWave);
    double* o0 = out0 + (size_t)row * V;
    double* o1 = metric == 1 ? out1 + (size_t)row * V : nullptr;
    for (int v = lane; v < V; v += kWave) {
        const double p = t[v] / s;
        if (metric == 1) {
            o0[v] = p;
            o1[v] = p == 0.0 ? 0.0 : log(p);
        } else
            o0[v] = __dsqrt_rn(p);
    }
}

// grid (ceil(Ka / 32), ceil(Kb / 32), groups), 256 threads.  a0, b0: sqrt(p) (metric 0) or p (metric 1); a1, b1: log(p)
// (metric 1).  groups == 1: out (Ka, Kb); otherwise part (segments, Ka, Kb).
template <bool JS>
__global__ __launch_bounds__(kTdThreads) void topic_distance_pair_kernel(const double* __restrict__ a0, const double* __restrict__ a1, int Ka,
                                                                         const double* __restrict__ b0, const double* __restrict__ b1, int Kb,
                                                                         int V, int symmetric, int segments, int segments_per_group,
                                                                         double* __restrict__ out, double* __restrict__ part)
{
    __shared__ __attribute__((aligned(16))) double lds[(JS ? 4 : 2) * kTdCells];
    const int ti = blockIdx.x, tj = blockIdx.y;
    if (symmetric && tj < ti) return;                                   // (block-uniform: the tile above the diagonal writes this one)
    double* sa0 = lds;                      // [kTdChunk][kTdTile]
    double* sb0 = lds + kTdCells;
    double* sa1 = lds + (JS ? 2 : 0) * kTdCells;
    double* sb1 = lds + (JS ? 3 : 0) * kTdCells;
    const int tid = threadIdx.x;
    const int ta = tid >> 4, tb = tid & 15;     // the thread's rows ta * 2 + {0, 1} of a's tile, tb * 2 + {0, 1} of b's
    // the loader's share of a chunk: 4 words of one row of a and of one row of b
    const int l_row = tid & (kTdTile - 1), l_w = (tid / kTdTile) * 4;
    const bool a_live = ti * kTdTile + l_row < Ka, b_live = tj * kTdTile + l_row < Kb;
    const size_t a_at = a_live ? (size_t)(ti * kTdTile + l_row) * V : 0;
    const size_t b_at = b_live ? (size_t)(tj * kTdTile + l_row) * V : 0;
    const bool whole = gridDim.z == 1;
    const int seg_begin = blockIdx.z * segments_per_group;
    const int seg_end = seg_begin + segments_per_group < segments ? seg_begin + segments_per_group : segments;

    double total[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int seg = seg_begin; seg < seg_end; ++seg) {                   // (block-uniform)
        const int v_begin = seg * kTdSegment;
        const int v_end = v_begin + kTdSegment < V ? v_begin + kTdSegment : V;
        double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
        for (int v0 = v_begin; v0 < v_end; v0 += kTdChunk) {            // (block-uniform)
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int v = v0 + l_w + u;
                const bool in = v < V;
                sa0[(l_w + u) * kTdTile + l_row] = (a_live && in) ? a0[a_at + v] : 0.0;
                sb0[(l_w + u) * kTdTile + l_row] = (b_live && in) ? b0[b_at + v] : 0.0;
                if (JS) {
                    sa1[(l_w + u) * kTdTile + l_row] = (a_live && in) ? a1[a_at + v] : 0.0;
                    sb1[(l_w + u) * kTdTile + l_row] = (b_live && in) ? b1[b_at + v] : 0.0;
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int w = 0; w < kTdChunk; ++w) {
                const double2 x = *reinterpret_cast<const double2*>(sa0 + w * kTdTile + ta * 2);
                const double2 y = *reinterpret_cast<const double2*>(sb0 + w * kTdTile + tb * 2);
                const double xe[2] = {x.x, x.y}, yf[2] = {y.x, y.y};
                if (JS) {
                    const double2 lx = *reinterpret_cast<const double2*>(sa1 + w * kTdTile + ta * 2);
                    const double2 ly = *reinterpret_cast<const double2*>(sb1 + w * kTdTile + tb * 2);
                    const double lxe[2] = {lx.x, lx.y}, lyf[2] = {ly.x, ly.y};
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int f = 0; f < 2; ++f) {
                            const double m = 0.5 * (xe[e] + yf[f]);
                            const double lm = log(m);
                            const double term = xe[e] * (lxe[e] - lm) + yf[f] * (lyf[f] - lm);
                            acc[e][f] = acc[e][f] + (m == 0.0 ? 0.0 : term);
                        }
                } else {
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int f = 0; f < 2; ++f) acc[e][f] = acc[e][f] + xe[e] * yf[f];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                if (whole)
                    total[e][f] = total[e][f] + acc[e][f];
                else {
                    const int i = ti * kTdTile + ta * 2 + e, j = tj * kTdTile + tb * 2 + f;
                    if (i < Ka && j < Kb) part[((size_t)seg * Ka + i) * Kb + j] = acc[e][f];
                }
            }
    }
    if (!whole) return;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int i = ti * kTdTile + ta * 2 + e, j = tj * kTdTile + tb * 2 + f;
            if (i < Ka && j < Kb) {
                const double x = JS ? 0.5 * total[e][f] : total[e][f];
                out[(size_t)i * Kb + j] = x;
                if (symmetric && ti != tj) out[(size_t)j * Kb + i] = x;             // (Ka == Kb)
            }
        }
}

// grid ceil(Ka Kb / 256), 256 threads: one thread per output.  part (segments, Ka, Kb), out (Ka, Kb); metric 1 halves the sum.
__global__ __launch_bounds__(kTdThreads) void topic_distance_combine_kernel(const double* __restrict__ part, int Ka, int Kb, int segments,
                                                                            int symmetric, int metric, double* __restrict__ out)
{
    const size_t at = (size_t)blockIdx.x * kTdThreads + threadIdx.x;
    const size_t cells = (size_t)Ka * Kb;
    if (at >= cells) return;
    int i = (int)(at / Kb), j = (int)(at % Kb);
    if (symmetric && i / kTdTile > j / kTdTile) {                       // (below the diagonal tiles: the mirror's sums)
        const int t = i;
        i = j;
        j = t;
    }
    double total = 0.0;
    for (int seg = 0; seg < segments; ++seg) total = total + part[(size_t)seg * cells + (size_t)i * Kb + j];
    out[at] = metric == 1 ? 0.5 * total : total;
}

}  // namespace pylda
