// Nearest documents by topic mixture: for every query row the first N rows of a base under the
// total order "larger score first, among equal scores the smaller document index first", the Q x D score matrix never
// stored.  tests/similarity_restatement.py is the same arithmetic in numpy, and every result is tested for equality.
//
//   score      s[q][d] = (((+0.0 + a_0 b_0) + a_1 b_1) + ...) over k = 0 .. K - 1 in that order: every multiply and every add
//              rounded once (no FMA: -ffp-contract=off, and the pragma below), the sum over k never split over lanes.
//   transform  the rows of an uploaded array in place: theta_k = g_k / s with s = (((+0.0 + g_0) + g_1) + ...), one s per
//              row, and sqrt(theta_k) for the Bhattacharyya coefficient.  One thread per row.
//   topn       grid (query block, document slice).  A workgroup of 4 wavefronts holds 64 queries and walks its slice of the
//              base in tiles of 128 documents, k in chunks of 16 through LDS (stored k-major, so that a thread reads its
//              operands as 16-byte pairs: 16 lanes x 16 bytes contiguous for the documents, a broadcast for the queries).
//              A thread owns 4 queries x 8 documents: 32 accumulators, advanced k by k.  The 16 lanes-of-16 of a wavefront
//              own the same 16 queries, so a finished tile goes to LDS in two halves of 32 queries - over the chunks, which
//              are dead by then - and every wavefront offers its 8 queries' 128 scores of the half to their lists, 64
//              documents at a time, one per lane.  The lists are section 16's (topn_list.h): one (score, id) per lane,
//              sorted, behind a threshold; 16 lists a wavefront, 48 registers.  After the first tiles almost nothing
//              passes the threshold and the selection costs a compare per pair.
//              Padding: k beyond K and rows beyond Q or D are zeros in LDS.  A product of zeros is +0.0, and an
//              accumulator is never -0.0 (it starts as +0.0 + x), so adding it changes no bit; documents beyond D are
//              never offered.
//   merge      one wavefront per query: the slices' lists go through the same list, 64 entries at a time.  The ids of a
//              query's candidates are distinct, so the result is the set the order defines, whatever the slices.
//              Entries a list never filled leave as id -1, score -infinity.
// No atomics: every output element has one owner.
#pragma once
#include "estep_common.h"
#include "topn_list.h"

#pragma clang fp contract(off)

namespace pylda {

constexpr int kSimilarityMaxN = 64;         // N <= one wavefront's lanes: a list is one entry per lane
constexpr int kSimThreads = 256;
constexpr int kSimWaves = kSimThreads / kWave;
constexpr int kSimBQ = 64;                  // queries of a workgroup
constexpr int kSimBD = 128;                 // documents of a tile
constexpr int kSimKC = 16;                  // k of a chunk
constexpr int kSimHalfQ = kSimBQ / 2;       // queries of one half of the score tile
constexpr int kSimWaveQ = kSimHalfQ / kSimWaves;    // queries of a wavefront in one half (8): 16 lists a wavefront
constexpr int kSimLds = kSimHalfQ * kSimBD;         // doubles: the score tile's half (32 KiB) over a-chunk + b-chunk (24 KiB)
constexpr int kSimMaxSlices = 1024;
constexpr int kSimMergeThreads = 256;
static_assert(kSimKC * (kSimBQ + kSimBD) <= kSimLds, "the chunks lie under the score tile");

// grid ceil(n / 256), 256 threads: one thread per row.  transform 1: theta; 2: sqrt(theta).
__global__ __launch_bounds__(256) void similarity_transform_kernel(double* __restrict__ rows, int64_t n, int K, int transform)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double* g = rows + r * K;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s = s + g[k];
    for (int k = 0; k < K; ++k) {
        const double theta = g[k] / s;
        g[k] = transform == 2 ? __dsqrt_rn(theta) : theta;
    }
}

// grid (ceil(Q / kSimBQ), slices), kSimThreads threads.  a (Q, K), b (D, K) row-major; self_ids (Q) or NULL.
// part_v / part_i (Q, slices, N): the list of every (query, slice); an unfilled entry has id INT_MAX.
__global__ __launch_bounds__(kSimThreads) void similarity_topn_kernel(const double* __restrict__ a, int64_t Q, const double* __restrict__ b,
                                                                      int64_t D, int K, int N, const int32_t* __restrict__ self_ids,
                                                                      int64_t tiles, int64_t tiles_per_slice,
                                                                      double* __restrict__ part_v, int32_t* __restrict__ part_i)
{
    __shared__ __attribute__((aligned(16))) double lds[kSimLds];
    __shared__ int s_self[kSimBQ];
    double* sa = lds;                       // [kSimKC][kSimBQ]
    double* sb = lds + kSimKC * kSimBQ;     // [kSimKC][kSimBD]
    double* ss = lds;                       // [kSimHalfQ][kSimBD], once the chunks are dead
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int td = tid & 15, tq = tid >> 4;     // the thread's documents j * 32 + td * 2 + {0, 1}, queries i * 32 + tq * 2 + {0, 1}
    const int64_t q0 = (int64_t)blockIdx.x * kSimBQ;
    const int slices = gridDim.y, slice = blockIdx.y;
    const int64_t t_begin = (int64_t)slice * tiles_per_slice;
    const int64_t t_end = t_begin + tiles_per_slice < tiles ? t_begin + tiles_per_slice : tiles;

    if (tid < kSimBQ) s_self[tid] = (self_ids && q0 + tid < Q) ? self_ids[q0 + tid] : -1;
    // the loader's share of a chunk: 4 k of one query, 8 k of one document
    const int a_row = tid & (kSimBQ - 1), a_k = (tid / kSimBQ) * 4;
    const int b_row = tid & (kSimBD - 1), b_k = (tid / kSimBD) * 8;
    const bool a_live = q0 + a_row < Q;
    const double* a_src = a + (a_live ? (q0 + a_row) * K : 0);

    // empty lists: entries that come after every entry there is
    double lv[2 * kSimWaveQ];
    int li[2 * kSimWaveQ];
#pragma unroll
    for (int l = 0; l < 2 * kSimWaveQ; ++l) {
        lv[l] = -INFINITY;
        li[l] = INT_MAX;
    }

    for (int64_t t = t_begin; t < t_end; ++t) {                         // (block-uniform)
        const int64_t d0 = t * kSimBD;
        const bool b_live = d0 + b_row < D;
        const double* b_src = b + (b_live ? (d0 + b_row) * K : 0);
        double acc[2][2][4][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][e][j][0] = acc[i][e][j][1] = 0.0;

        for (int k0 = 0; k0 < K; k0 += kSimKC) {                        // (block-uniform)
            __syncthreads();                                            // the chunk, or the score tile, before it is read out
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + a_k + u;
                sa[(a_k + u) * kSimBQ + a_row] = (a_live && k < K) ? a_src[k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + b_k + u;
                sb[(b_k + u) * kSimBD + b_row] = (b_live && k < K) ? b_src[k] : 0.0;
            }
            __syncthreads();
#pragma unroll 4
            for (int kk = 0; kk < kSimKC; ++kk) {
                double2 av[2], bv[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const double2*>(sa + kk * kSimBQ + i * 32 + tq * 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const double2*>(sb + kk * kSimBD + j * 32 + td * 2);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[i][0][j][0] = acc[i][0][j][0] + av[i].x * bv[j].x;
                        acc[i][0][j][1] = acc[i][0][j][1] + av[i].x * bv[j].y;
                        acc[i][1][j][0] = acc[i][1][j][0] + av[i].y * bv[j].x;
                        acc[i][1][j][1] = acc[i][1][j][1] + av[i].y * bv[j].y;
                    }
            }
        }

        // the tile's scores through LDS, a half of the queries at a time; wavefront w owns queries w * 8 .. w * 8 + 7 of a half
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<double2*>(ss + (tq * 2 + e) * kSimBD + j * 32 + td * 2) = make_double2(acc[i][e][j][0], acc[i][e][j][1]);
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kSimWaveQ; ++r) {
                const int l = i * kSimWaveQ + r;
                const int row = wave * kSimWaveQ + r;
                const int self = s_self[i * kSimHalfQ + row];
                double thr_v = readlane_f64(lv[l], N - 1);
                int thr_i = __builtin_amdgcn_readlane(li[l], N - 1);
#pragma unroll
                for (int c = 0; c < kSimBD / kWave; ++c) {
                    const int64_t d = d0 + c * kWave + lane;
                    const double x = ss[row * kSimBD + c * kWave + lane];
                    const int v = (d < D && d != self) ? (int)d : -1;
                    coherence_offer(lv[l], li[l], thr_v, thr_i, x, v, N, lane);
                }
            }
        }
    }

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < kSimWaveQ; ++r) {
            const int l = i * kSimWaveQ + r;
            const int64_t q = q0 + i * kSimHalfQ + wave * kSimWaveQ + r;
            if (q < Q && lane < N) {
                const size_t at = ((size_t)q * slices + slice) * N + lane;
                part_v[at] = lv[l];
                part_i[at] = li[l];
            }
        }
}

// grid ceil(Q / 4), kSimMergeThreads threads: one wavefront per query.  ids (Q, N), scores (Q, N).
__global__ __launch_bounds__(kSimMergeThreads) void similarity_merge_kernel(const double* __restrict__ part_v, const int32_t* __restrict__ part_i,
                                                                            int64_t Q, int slices, int N, int32_t* __restrict__ ids,
                                                                            double* __restrict__ scores)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = (int64_t)blockIdx.x * (kSimMergeThreads / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (q >= Q) return;                                                 // (whole wavefronts)
    const int candidates = slices * N;
    const double* cv = part_v + (size_t)q * candidates;
    const int32_t* ci = part_i + (size_t)q * candidates;
    double lv = -INFINITY, thr_v = -INFINITY;
    int li = INT_MAX, thr_i = INT_MAX;
    for (int base = 0; base < candidates; base += kWave) {              // (wave-uniform)
        const int at = base + lane;
        const double x = at < candidates ? cv[at] : 0.0;
        int v = at < candidates ? ci[at] : -1;
        if (v == INT_MAX) v = -1;                                       // (a slice with fewer than N candidates)
        coherence_offer(lv, li, thr_v, thr_i, x, v, N, lane);
    }
    if (lane < N) {
        const bool filled = li != INT_MAX;
        ids[(size_t)q * N + lane] = filled ? li : -1;
        scores[(size_t)q * N + lane] = filled ? lv : -INFINITY;
    }
}

}  // namespace pylda
