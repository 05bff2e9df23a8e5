// The collapsed Gibbs engine sharded over several ranks: every rank holds a contiguous range of the
// documents and a full replica of the word-topic table T and n_k.  A round samples the rank's documents of the block
// (gibbs_sample_kernel, unchanged), packs one move record per token of the block, the ranks all-gather their records,
// and every rank applies ALL of them - its own included - to its replica.  The replicas therefore receive exactly the
// integer updates the one-GPU table receives (gibbs_apply_kernel is not launched in a sharded round).
//
//   record      one uint64 per token: word << 32 | old topic << 16 | new topic (K <= 1024 fits); old == new is skipped by
//               the apply pass: tokens that kept their topic, and the zeroed padding behind a rank's last record
//   segment     a rank's records of a round: the block's documents in local order, a document's tokens in state-word
//               order; rec_off[d] is the position of document d's first record (built on the host per (blocks,
//               first_document)); every rank sends capacity[round] records, the tail zeroed
#pragma once
#include "estep_gibbs.h"

namespace pylda {

__host__ __device__ constexpr uint64_t gibbs_record(uint32_t word, uint32_t zold, uint32_t znew)
{
    return ((uint64_t)word << 32) | ((uint64_t)zold << 16) | (uint64_t)znew;
}

// One wavefront per document of the block, lanes over its terms (as gibbs_apply_kernel walks them).
__global__ __launch_bounds__(256) void gibbs_pack_kernel(GibbsParams p, const int64_t* __restrict__ rec_off, uint64_t* __restrict__ send)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (i >= p.count) return;
    const int64_t d = p.first + i * p.step;
    const uint64_t topic_mask = ((uint64_t)1 << p.bits) - 1;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t shift = rec_off[d] - p.tok_off[pb];        // from a token's position in the state words to its record's
    for (int64_t q = pb + lane; q < pe; q += kWave) {
        const uint32_t w = (uint32_t)p.term_id[q];
        for (int64_t tk = p.tok_off[q]; tk < p.tok_off[q + 1]; ++tk) {
            const uint64_t st = p.state[tk];
            send[shift + tk] = gibbs_record(w, (uint32_t)((st >> p.bits) & topic_mask), (uint32_t)(st & topic_mask));
        }
    }
}

// One thread per record of the gathered buffer: T[w][old] -= 1, T[w][new] += 1 by global integer atomics, n_k through
// per-workgroup counts in LDS (the idiom of gibbs_apply_kernel).  The records come from other processes: one that names a
// word or a topic outside the model is skipped, never followed.
__global__ __launch_bounds__(256) void gibbs_record_apply_kernel(const uint64_t* __restrict__ recv, int64_t n, int32_t* __restrict__ table,
                                                                 int32_t* __restrict__ n_k, int K, int V, int ldk)
{
    extern __shared__ int record_delta[];                    // K
    for (int k = threadIdx.x; k < K; k += 256) record_delta[k] = 0;
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) {
        const uint64_t rec = recv[r];
        const uint32_t w = (uint32_t)(rec >> 32);
        const int zold = (int)((rec >> 16) & 0xffffu), znew = (int)(rec & 0xffffu);
        if (zold != znew && w < (uint32_t)V && zold < K && znew < K) {
            int32_t* row = table + (size_t)w * ldk;
            atomicAdd(&row[zold], -1);
            atomicAdd(&row[znew], 1);
            atomicAdd(&record_delta[zold], -1);
            atomicAdd(&record_delta[znew], 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256)
        if (record_delta[k]) atomicAdd(&n_k[k], record_delta[k]);
}

// out[0] = sum_d docs[d], out[1] = sum_v words[v] - sum_k lnG(n_k + beta_sum): the two halves of
// gibbs_posterior_sum_kernel apart (a rank's documents; the replicated table), each in a fixed order
__global__ __launch_bounds__(256) void gibbs_posterior_parts_kernel(const double* __restrict__ docs, int64_t D, const double* __restrict__ words,
                                                                    int V, const int32_t* __restrict__ n_k, int K, double beta_sum,
                                                                    double* __restrict__ out)
{
    __shared__ double scratch[4];
    double s = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 256) s += docs[d];
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) out[0] = s;
    s = 0.0;                                                 // (block_sum opens with a barrier: its scratch is free again)
    for (int v = threadIdx.x; v < V; v += 256) s += words[v];
    for (int k = threadIdx.x; k < K; k += 256) s -= lgamma_pos((double)n_k[k] + beta_sum);
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) out[1] = s;
}

}  // namespace pylda
