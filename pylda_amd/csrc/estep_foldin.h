// Held-out fold-in for the collapsed Gibbs engine: topic proportions and a likelihood for documents the model was not
// trained on, with the word-topic counts frozen.  DESIGN.md section 12 is the specification; tests/foldin_restatement.py
// is the same estimator in numpy, operation for operation (there is no transcendental in the chain: gamma agrees bit for
// bit; the likelihood takes one log per distinct term).
//
//   model       P[w][k] = ((double)n_kv[k][w] + beta_w) / ((double)n_k[k] + beta_sum), word-major V x ldk doubles, zero
//               padding: add, add, divide, each rounded once; built once per model (foldin_table_kernel)
//   document    one wavefront, all sweeps in one launch; with the counts frozen the documents are independent chains, so
//               the document-parallel sampler is exact here (no blocks, no apply pass).  Tokens in CSR order, a term's
//               copies back to back; topic k in lane k / S, slot k % S (sampler_wave.h)
//   start       topic = min(K - 1, (int)(uniform(position, phase 0, global document, stream) * K))
//   sweep s     the token leaves its topic, w[k] = ((double)nd[k] + alpha[k]) * P[w][k] - one add, one multiply - then the
//               slot sums, lane scan and owner rule of sampler_wave.h with
//               t = uniform(position, (1 + s) << 16, global document, stream) * total
//   keep        after each sweep s >= burn_in: acc[k] += nd[k] (integers);
//               gamma[k] = alpha[k] + (double)acc[k] / (double)(samples - burn_in)
//   likelihood  theta = gamma / sum(gamma); sum over the distinct terms, in CSR order, of c_n * log(sum_k theta[k] P[w_n][k])
//               (slot sums sequential, lane sums by wave_sum): the plug-in estimate, theta from the same tokens
//   topics      the corpus' state words in global memory; the next token's topic - last sweep's value - is requested before
//               the current draw, so the load is off the per-token dependent chain (topics in LDS were measured and were
//               slower: section 12)
#pragma once
#include "estep_common.h"
#include "philox.h"
#include "sampler_wave.h"

namespace pylda {

struct FoldinParams {
    int K, V, ldk;
    const int64_t* doc_ptr;
    const int32_t* term_id;
    const int32_t* term_ct;
    const int64_t* tok_off;     // nnz + 1
    uint64_t* state;            // tokens: their topics
    const double* P;            // V x ldk
    const double* alpha;        // K
    double* gamma;              // D x K
    double* doc_ll;             // D: 0
    double* doc_wll;            // D: the document's likelihood
    int32_t* iters;             // D: samples
    int64_t D;
    int samples, burn_in;
    uint32_t first_document, stream, seed_lo, seed_hi;
};

// counts: V x ldk word-major (a corpus' Gibbs table, or the host's n_kv transposed)
__global__ __launch_bounds__(256) void foldin_table_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ n_k,
                                                           const double* __restrict__ beta, double beta_sum, int K, int V, int ldk,
                                                           double* __restrict__ P)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)V * ldk) return;
    const int w = (int)(i / ldk), k = (int)(i % ldk);
    P[i] = k < K ? ((double)counts[i] + beta[w]) / ((double)n_k[k] + beta_sum) : 0.0;
}

template <int S>
__global__ __launch_bounds__(256) void foldin_sample_kernel(FoldinParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (d >= p.D) return;                                    // (whole wavefronts)
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t t0 = p.tok_off[pb];
    const uint32_t ntok = (uint32_t)(p.tok_off[pe] - t0);
    const uint32_t gdoc = p.first_document + (uint32_t)d;
    uint64_t* topic = p.state + t0;
    int nd[S];
    long long acc[S];
    double al[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        nd[s] = 0;
        acc[s] = 0;
        al[s] = k0 + s < K ? p.alpha[k0 + s] : 0.0;
    }
    for (uint32_t pos = 0; pos < ntok; ++pos) {
        const double u = philox_uniform(pos, 0u, gdoc, p.stream, p.seed_lo, p.seed_hi);
        const int z = uniform_topic(u, K);
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (k0 + s == z) nd[s] += 1;
        topic[pos] = (uint64_t)z;          // (every lane: each lane's later reads follow its own store)
    }
    for (int it = 0; it < p.samples; ++it) {
        const uint32_t phase = (uint32_t)(1 + it) << 16;
        int znext = ntok ? (int)topic[0] : 0;
        double pn[S];
        if (pb < pe) load_topic_row<S>(p.P, p.term_id[pb], p.ldk, k0, K, pn);
        uint32_t pos = 0;
        for (int64_t q = pb; q < pe; ++q) {
            double pr[S];
#pragma unroll
            for (int s = 0; s < S; ++s) pr[s] = pn[s];
            if (q + 1 < pe) load_topic_row<S>(p.P, p.term_id[q + 1], p.ldk, k0, K, pn);     // the next term's row, while this one's copies are drawn
            const int c = p.term_ct[q];
            for (int j = 0; j < c; ++j, ++pos) {
                const int zold = znext;
                if (pos + 1 < ntok) znext = (int)topic[pos + 1];      // (last sweep's topic: it does not wait for this draw)
                // (the weights are not kept across the scan: the owner computes its own again, the same operations)
                auto weight = [&](int s) { return ((double)nd[s] + al[s]) * pr[s]; };
                double part = 0.0;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (k0 + s == zold) nd[s] -= 1;
                    part = part + weight(s);
                }
                const int znew = wave_draw<S>(weight, [&] { return philox_uniform(pos, phase, gdoc, p.stream, p.seed_lo, p.seed_hi); },
                                              part, lane, k0);
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (k0 + s == znew) nd[s] += 1;
                topic[pos] = (uint64_t)znew;
            }
        }
        if (it >= p.burn_in) {
#pragma unroll
            for (int s = 0; s < S; ++s) acc[s] += nd[s];
        }
    }
    // gamma, theta and the document's likelihood
    const double kept = (double)(p.samples - p.burn_in);
    double th[S], gpart = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        th[s] = k0 + s < K ? al[s] + (double)acc[s] / kept : 0.0;
        if (k0 + s < K) p.gamma[d * K + k0 + s] = th[s];
        gpart = gpart + th[s];
    }
    const double gsum = wave_sum(gpart);
#pragma unroll
    for (int s = 0; s < S; ++s) th[s] = th[s] / gsum;
    double ll = 0.0;
    for (int64_t q = pb; q < pe; ++q) {
        double row[S], part = 0.0;
        load_topic_row<S>(p.P, p.term_id[q], p.ldk, k0, K, row);
#pragma unroll
        for (int s = 0; s < S; ++s) part = part + th[s] * row[s];
        ll = ll + (double)p.term_ct[q] * log(wave_sum(part));
    }
    if (lane == 0) {
        p.doc_ll[d] = 0.0;
        p.doc_wll[d] = ll;
        p.iters[d] = p.samples;
    }
}

// scalars of pylda_estep_results: [0] 0, [1] sum_d doc_wll[d], [2] 0, [3] no flagged documents; one workgroup, every
// thread a fixed share
__global__ __launch_bounds__(256) void foldin_sum_kernel(const double* __restrict__ doc_wll, int64_t D, double* __restrict__ scalars)
{
    __shared__ double scratch[4];
    double s = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 256) s += doc_wll[d];
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) {
        scalars[0] = 0.0;
        scalars[1] = s;
        scalars[2] = 0.0;
        scalars[3] = 0.0;
    }
}

}  // namespace pylda
