// The collapsed Gibbs engine (monte_carlo.py of the reference; Griffiths & Steyvers 2004) as a document-parallel chain
// with block-synchronous counts.  DESIGN.md section 11 is the specification; tests/gibbs_restatement.py is the same chain
// in numpy, operation for operation, and the two agree on every token (there is no transcendental in the chain).
//
//   blocks      block g of a sweep = the documents whose GLOBAL index is g modulo `blocks`; a sweep is `blocks` rounds of
//               (gibbs_sample_kernel, gibbs_apply_kernel) in stream order
//   round       one wavefront per document of the block, token after token in CSR order (a term's copies back to back).
//               The word-topic table T (word-major int32, V x ldk) and n_k are read only: they keep their values of the
//               round's start.  The document adds its own changes of the round on top: nd[] its live topic counts,
//               dk[] = nd - nd at the round's start (n_k as the document sees it: n_k + dk), dw[] the moves of the copies
//               of the current term already visited (cleared when the term changes; its row as seen: T[w] + dw)
//   draw        the token leaves its old topic (nd, dk, dw of it minus one), then
//               w[k] = ((double)nd[k] + alpha[k]) * ((double)(T[w][k] + dw[k]) + beta_w) / ((double)(n_k[k] + dk[k]) + beta_sum)
//               - add, add, add, multiply, divide, each rounded once - and the lane layout, slot sums, Hillis-Steele lane
//               scan and owner rule of sampler_wave.h with t = uniform(position, phase 1, global document, stream) * total
//   state       one uint64 per token: bits [0, b) the topic, [b, 2b) the topic before the token's last draw
//               (b = ceil(log2 K)): all the apply pass needs
//   apply       per token of the block that changed topic: T[w][old] -= 1, T[w][new] += 1 (vector integer atomics on
//               global memory: sums of integers, the order does not matter), n_k through per-workgroup counts in LDS
//   start       topic = min(K - 1, (int)(uniform(position, phase 0, global document, stream 0) * K))
#pragma once
#include "estep_common.h"
#include "philox.h"
#include "sampler_wave.h"
#include "special_device.h"

namespace pylda {

struct GibbsParams {
    int K, V, ldk, bits;
    const int64_t* doc_ptr;
    const int32_t* term_id;
    const int32_t* term_ct;
    const int64_t* tok_off;     // nnz + 1
    uint64_t* state;            // tokens
    double* n_dk;               // D x K, exact integers (the corpus' gamma buffer)
    int32_t* table;             // V x ldk
    int32_t* n_k;               // K
    const double* alpha;        // K
    const double* beta;         // V
    double beta_sum;
    int64_t D;                  // documents of the corpus
    int64_t first;              // first local document of this launch's block
    int64_t step;               // ... and the distance to the next (= blocks); count of them:
    int64_t count;
    uint32_t first_document, stream, seed_lo, seed_hi;
};

// Initial assignment: one wavefront per document, lanes over its terms.  n_dk through per-wavefront counts in LDS
// (4 x K), the table by global atomics, n_k from the workgroup's four documents.
__global__ __launch_bounds__(256) void gibbs_init_kernel(GibbsParams p)
{
    extern __shared__ int init_counts[];                     // 4 x K
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t d = (int64_t)blockIdx.x * 4 + wave;
    const int K = p.K;
    int* mine = init_counts + wave * K;
    for (int k = lane; k < K; k += kWave) mine[k] = 0;
    __syncthreads();
    if (d < p.D) {
        const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
        const int64_t t0 = p.tok_off[pb];
        const uint32_t gdoc = p.first_document + (uint32_t)d;
        for (int64_t q = pb + lane; q < pe; q += kWave) {
            int32_t* row = p.table + (size_t)p.term_id[q] * p.ldk;
            for (int64_t tk = p.tok_off[q]; tk < p.tok_off[q + 1]; ++tk) {
                const double u = philox_uniform((uint32_t)(tk - t0), 0u, gdoc, 0u, p.seed_lo, p.seed_hi);
                const int z = uniform_topic(u, K);
                p.state[tk] = (uint64_t)z | ((uint64_t)z << p.bits);
                atomicAdd(&mine[z], 1);
                atomicAdd(&row[z], 1);
            }
        }
    }
    __syncthreads();
    if (d < p.D)
        for (int k = lane; k < K; k += kWave) p.n_dk[d * K + k] = (double)mine[k];
    for (int k = threadIdx.x; k < K; k += 256) {
        const int s = init_counts[k] + init_counts[K + k] + init_counts[2 * K + k] + init_counts[3 * K + k];
        if (s) atomicAdd(&p.n_k[k], s);
    }
}

template <int S>
__global__ __launch_bounds__(256) void gibbs_sample_kernel(GibbsParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (i >= p.count) return;                                // (whole wavefronts)
    const int64_t d = p.first + i * p.step;
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t t0 = p.tok_off[pb];
    const uint32_t gdoc = p.first_document + (uint32_t)d;
    const uint64_t topic_mask = ((uint64_t)1 << p.bits) - 1;
    int nd[S], dk[S], nk[S], dw[S], tn[S];
    double al[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool real = k0 + s < K;
        nd[s] = real ? (int)p.n_dk[d * K + k0 + s] : 0;
        nk[s] = real ? p.n_k[k0 + s] : 0;
        al[s] = real ? p.alpha[k0 + s] : 0.0;
        dk[s] = 0;
        tn[s] = 0;
    }
    if (pb < pe) load_topic_row<S>(p.table, p.term_id[pb], p.ldk, k0, K, tn);
    double bwn = pb < pe ? p.beta[p.term_id[pb]] : 0.0;
    uint32_t pos = 0;
    for (int64_t q = pb; q < pe; ++q) {
        int tr[S];
        const double bw = bwn;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            tr[s] = tn[s];
            dw[s] = 0;
        }
        if (q + 1 < pe) {           // the next term's row, while this one's tokens are drawn
            const int w_next = p.term_id[q + 1];
            load_topic_row<S>(p.table, w_next, p.ldk, k0, K, tn);
            bwn = p.beta[w_next];
        }
        const int c = p.term_ct[q];
        for (int j = 0; j < c; ++j, ++pos) {
            const int zold = (int)(p.state[t0 + pos] & topic_mask);
            double w[S], part = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (k0 + s == zold) {
                    nd[s] -= 1;
                    dk[s] -= 1;
                    dw[s] -= 1;
                }
                const double a = (double)nd[s] + al[s];
                const double b = (double)(tr[s] + dw[s]) + bw;
                const double n = (double)(nk[s] + dk[s]) + p.beta_sum;
                w[s] = k0 + s < K ? a * b / n : 0.0;
                part = part + w[s];
            }
            const int znew = wave_draw<S>([&](int s) { return w[s]; },
                                          [&] { return philox_uniform(pos, 1u << 16, gdoc, p.stream, p.seed_lo, p.seed_hi); }, part, lane, k0);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (k0 + s == znew) {
                    nd[s] += 1;
                    dk[s] += 1;
                    dw[s] += 1;
                }
            if (lane == 0) p.state[t0 + pos] = (uint64_t)znew | ((uint64_t)zold << p.bits);
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (k0 + s < K) p.n_dk[d * K + k0 + s] = (double)nd[s];
}

// The round's changes into the table and n_k: one wavefront per document of the block, lanes over its terms.
__global__ __launch_bounds__(256) void gibbs_apply_kernel(GibbsParams p)
{
    extern __shared__ int apply_delta[];                     // K
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    const int K = p.K;
    for (int k = threadIdx.x; k < K; k += 256) apply_delta[k] = 0;
    __syncthreads();
    if (i < p.count) {
        const int64_t d = p.first + i * p.step;
        const uint64_t topic_mask = ((uint64_t)1 << p.bits) - 1;
        for (int64_t q = p.doc_ptr[d] + lane; q < p.doc_ptr[d + 1]; q += kWave) {
            int32_t* row = p.table + (size_t)p.term_id[q] * p.ldk;
            for (int64_t tk = p.tok_off[q]; tk < p.tok_off[q + 1]; ++tk) {
                const uint64_t st = p.state[tk];
                const int znew = (int)(st & topic_mask), zold = (int)((st >> p.bits) & topic_mask);
                if (znew != zold) {
                    atomicAdd(&row[zold], -1);
                    atomicAdd(&row[znew], 1);
                    atomicAdd(&apply_delta[zold], -1);
                    atomicAdd(&apply_delta[znew], 1);
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256)
        if (apply_delta[k]) atomicAdd(&p.n_k[k], apply_delta[k]);
}

// ---- log posterior (monte_carlo.py:217-256), fixed-order reductions ----
// per document: sum_k lnG(n_dk + alpha_k) - lnG(N_d + sum alpha), one wavefront per document
__global__ __launch_bounds__(256) void gibbs_doc_posterior_kernel(const double* __restrict__ n_dk, const double* __restrict__ alpha,
                                                                  double alpha_sum, int K, int64_t D, double* __restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (d >= D) return;
    double lg = 0.0, n = 0.0;
    for (int k = lane; k < K; k += kWave) {
        const double c = n_dk[d * K + k];
        lg += lgamma_pos(c + alpha[k]);
        n += c;
    }
    lg = wave_sum(lg);
    n = wave_sum(n);
    if (lane == 0) out[d] = lg - lgamma_pos(n + alpha_sum);
}

// per word: sum_k lnG(T[w][k] + beta_w), one workgroup per word
__global__ __launch_bounds__(256) void gibbs_word_posterior_kernel(const int32_t* __restrict__ table, const double* __restrict__ beta,
                                                                   int K, int ldk, double* __restrict__ out)
{
    __shared__ double scratch[4];
    const int v = blockIdx.x;
    const double b = beta[v];
    const double lg_b = lgamma_pos(b);                       // (most of a row is empty)
    double lg = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int c = table[(size_t)v * ldk + k];
        lg += c ? lgamma_pos((double)c + b) : lg_b;
    }
    lg = block_sum<256>(lg, scratch);
    if (threadIdx.x == 0) out[v] = lg;
}

// out[0] = sum_d docs[d] + sum_v words[v] - sum_k lnG(n_k + beta_sum): one workgroup, every thread a fixed share
__global__ __launch_bounds__(256) void gibbs_posterior_sum_kernel(const double* __restrict__ docs, int64_t D, const double* __restrict__ words,
                                                                  int V, const int32_t* __restrict__ n_k, int K, double beta_sum,
                                                                  double* __restrict__ out)
{
    __shared__ double scratch[4];
    double s = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 256) s += docs[d];
    for (int v = threadIdx.x; v < V; v += 256) s += words[v];
    for (int k = threadIdx.x; k < K; k += 256) s -= lgamma_pos((double)n_k[k] + beta_sum);
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) out[0] = s;
}

// n_dk of every document from its tokens' topics (pylda_gibbs_set_state)
__global__ __launch_bounds__(256) void gibbs_recount_kernel(GibbsParams p)
{
    extern __shared__ int recount_counts[];                  // 4 x K
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t d = (int64_t)blockIdx.x * 4 + wave;
    if (d >= p.D) return;                                    // (whole wavefronts; no workgroup barrier below)
    const int K = p.K;
    int* mine = recount_counts + wave * K;
    for (int k = lane; k < K; k += kWave) mine[k] = 0;
    wave_lds_exchange();
    const uint64_t topic_mask = ((uint64_t)1 << p.bits) - 1;
    for (int64_t tk = p.tok_off[p.doc_ptr[d]] + lane; tk < p.tok_off[p.doc_ptr[d + 1]]; tk += kWave)
        atomicAdd(&mine[(int)(p.state[tk] & topic_mask)], 1);
    wave_lds_exchange();
    for (int k = lane; k < K; k += kWave) p.n_dk[d * K + k] = (double)mine[k];
}

}  // namespace pylda
