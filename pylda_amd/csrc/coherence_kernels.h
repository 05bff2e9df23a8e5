// Topic coherence and top words per topic: two exact counting problems.  The device produces
// integers and copies of table entries only; the logs and sums over them are host numpy (pylda_amd/coherence.py), and
// tests/coherence_restatement.py is the same counting in numpy.
//
//   select   the first M entries of every row of a (K, V) table under the total order "larger value first, among equal
//            values the smaller word id first".  One workgroup of 16 wavefronts per topic, one pass over the row, read
//            coalesced along v.  Every wavefront keeps its best 64 as a sorted list IN REGISTERS - lane j holds entry j -
//            behind a threshold, its entry M - 1: lanes compare their element with the threshold, the few that beat it
//            insert one at a time through a ballot loop (the rank of the newcomer is a ballot's population count, the
//            entries behind it move up one lane).  The 16 lists are merged through LDS by rank: an entry's rank is the
//            number of entries before it in the order, and the order is total (a word id occurs once in a row), so the
//            answer is a set with a position for each member - it depends neither on the insertion order nor on the
//            launch shape, and the values are the table's own bits.
//   mark     one bitmap of the documents per SLOT (a distinct word among the K x M top ids): bit d - d0 of row map[w] is
//            set for every (document d, term w) pair of the chunk [d0, d0 + Dc) whose word has a slot.  One wavefront per
//            document, its terms read coalesced; OR is order-free, so the 64-bit atomics give the same bitmap every time.
//   pair     grid (tile of bitmap words, topic): the topic's M bitmap rows of the tile are staged in LDS, a thread owns
//            pairs (m, l <= m) and adds popcount(a & b) over the tile; one integer atomic add per (topic, pair, tile) into
//            co[k][m][l] and its mirror.  Integer sums are order-free.  The diagonal is the document frequency.
#pragma once
#include "estep_common.h"
#include "topn_list.h"     // coherence_before / coherence_insert / coherence_offer: the sorted list of a wavefront

namespace pylda {

constexpr int kCoherenceMaxWords = 64;      // M <= one wavefront's lanes: a list is one entry per lane
constexpr int kSelectThreads = 1024;
constexpr int kSelectWaves = kSelectThreads / kWave;
constexpr int kSelectUnroll = 4;            // elements a lane has in flight
constexpr int kPairTile = 64;               // bitmap words (4096 documents) a workgroup of the pair kernel stages per row
constexpr int kPairRowStride = kPairTile + 1;   // odd: the rows of a tile start in different banks
constexpr int kPairThreads = 256;

// grid K, kSelectThreads threads.  table (K, V) row-major, finite; 1 <= M <= min(64, V).
__global__ __launch_bounds__(kSelectThreads) void coherence_select_kernel(const double* __restrict__ table, int V, int M,
                                                                         int32_t* __restrict__ top_ids, double* __restrict__ top_values)
{
    __shared__ double s_v[kSelectThreads];
    __shared__ int s_i[kSelectThreads];
    const int k = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const double* row = table + (size_t)k * V;
    // an empty list: entries that come after every entry of a finite table
    double lv = -INFINITY, thr_v = -INFINITY;
    int li = INT_MAX, thr_i = INT_MAX;
    for (int base = 0; base < V; base += kSelectThreads * kSelectUnroll) {      // (block-uniform)
        double x[kSelectUnroll];
        int v[kSelectUnroll];
#pragma unroll
        for (int u = 0; u < kSelectUnroll; ++u) {
            const int at = base + u * kSelectThreads + (int)threadIdx.x;
            v[u] = at < V ? at : -1;
            x[u] = at < V ? row[at] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kSelectUnroll; ++u) coherence_offer(lv, li, thr_v, thr_i, x[u], v[u], M, lane);
    }
    // merge by rank: the row's first M are among the lists' first M each; they meet in LDS, packed, and thread t owns
    // candidate t - its position is the number of candidates before it
    if (lane < M) {
        s_v[(threadIdx.x / kWave) * M + lane] = lv;
        s_i[(threadIdx.x / kWave) * M + lane] = li;
    }
    __syncthreads();
    const int candidates = kSelectWaves * M;
    if ((int)threadIdx.x >= candidates) return;
    const double my_v = s_v[threadIdx.x];
    const int my_i = s_i[threadIdx.x];
    int rank = 0;
    for (int j = 0; j < candidates; ++j) rank += coherence_before(s_v[j], s_i[j], my_v, my_i) ? 1 : 0;
    if (my_i != INT_MAX && rank < M) {
        top_ids[(size_t)k * M + rank] = my_i;
        top_values[(size_t)k * M + rank] = my_v;
    }
}

// grid ceil(documents of the chunk / 4), 256 threads: one wavefront per document d0 + i, i < n_docs.
// bits: slots x words 64-bit words, zeroed; slot_of_word (V): slot or -1.
__global__ __launch_bounds__(256) void coherence_mark_kernel(const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ term_id,
                                                             const int32_t* __restrict__ slot_of_word, int64_t d0, int64_t n_docs,
                                                             int64_t words, unsigned long long* __restrict__ bits)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (i >= n_docs) return;                                            // (whole wavefronts)
    const int64_t pb = doc_ptr[d0 + i], pe = doc_ptr[d0 + i + 1];
    const unsigned long long bit = 1ull << (i & 63);
    const int64_t word = i >> 6;
    for (int64_t q = pb + lane; q < pe; q += kWave) {
        const int slot = slot_of_word[term_id[q]];
        if (slot >= 0) atomicOr(bits + (size_t)slot * words + word, bit);
    }
}

// grid (ceil(words / kPairTile), K), kPairThreads threads.  slot_of_top (K x M): the slot of every top word.
// co (K, M, M) 64-bit counts, accumulated over the tiles (and over the chunks of documents).
__global__ __launch_bounds__(kPairThreads) void coherence_pair_kernel(const unsigned long long* __restrict__ bits, int64_t words,
                                                                      const int32_t* __restrict__ slot_of_top, int M,
                                                                      unsigned long long* __restrict__ co)
{
    __shared__ unsigned long long tile[kCoherenceMaxWords * kPairRowStride];
    const int k = blockIdx.y;
    const int64_t w0 = (int64_t)blockIdx.x * kPairTile;
    const int n = (int)(words - w0 < kPairTile ? words - w0 : kPairTile);   // (>= 1 by the grid)
    for (int e = threadIdx.x; e < M * kPairTile; e += kPairThreads) {
        const int m = e / kPairTile, w = e % kPairTile;
        tile[m * kPairRowStride + w] = w < n ? bits[(size_t)slot_of_top[(size_t)k * M + m] * words + w0 + w] : 0ull;
    }
    __syncthreads();
    const int pairs = M * (M + 1) / 2;
    for (int p = threadIdx.x; p < pairs; p += kPairThreads) {
        // p = m (m + 1) / 2 + l, l <= m
        int m = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
        while (m * (m + 1) / 2 > p) --m;
        while ((m + 1) * (m + 2) / 2 <= p) ++m;
        const int l = p - m * (m + 1) / 2;
        const unsigned long long* a = tile + m * kPairRowStride;
        const unsigned long long* b = tile + l * kPairRowStride;
        int count = 0;
#pragma unroll 8
        for (int w = 0; w < kPairTile; ++w) count += __popcll(a[w] & b[w]);
        if (count) {
            atomicAdd(co + ((size_t)k * M + m) * M + l, (unsigned long long)count);
            if (l != m) atomicAdd(co + ((size_t)k * M + l) * M + m, (unsigned long long)count);
        }
    }
}

}  // namespace pylda
