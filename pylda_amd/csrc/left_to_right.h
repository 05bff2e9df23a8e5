// Left-to-right held-out likelihood (Wallach, Murray, Salakhutdinov & Mimno 2009, Algorithm 3): log p(w | Phi, alpha) of a
// document with theta integrated out, from the context's word-major predictive table P[w][k] and alpha alone - the same
// quantity for every engine.  DESIGN.md section 19 is the specification; tests/ltr_restatement.py is the same estimator in
// numpy, operation for operation (no transcendental in the chains: the topics agree draw for draw, the predictive
// probabilities bit for bit; the reduction takes one log per token).
//
//   tokens      a document's CSR terms in order, a term's copies back to back (the order of sections 10-12 and 15)
//   work item   one wavefront per (document, particle): particles are independent chains.  Topic k in lane k / S, slot k % S
//               (sampler_wave.h); nd[] - integers, 0 at the start - and alpha in registers
//   position n  0 .. N_d - 1 in order:
//     resample  (if asked) for n' = 0 .. n - 1 in order: the token leaves its topic, wt[k] = ((double)nd[k] + alpha[k]) *
//               P[w_n'][k] - one add, one multiply -, the slot sums, lane scan and owner rule of sampler_wave.h with
//               t = uniform(n', n, global document, stream + particle) * total, the token enters the drawn topic
//     predict   p[n][r] = (sum_k wt[k] over w_n) / ((double)n + alpha_sum): slot sums sequential, the lane sum by wave_sum,
//               one divide; alpha_sum in the order of fold-in's theta sum
//     forward   z_n from the same weights (token n not yet counted) with t = uniform(n, n, ..) * total of the lane scan; it
//               enters its topic
//   rows        the current term's row of P in registers, reused across the term's copies; the next term's row and the next
//               token's topic are requested one step ahead, as fold-in does: neither load is on the per-token chain
//   topics      uint16 per token per particle in a scratch buffer of the call: document d's at (its first token) x R, a
//               particle's N_d topics contiguous; p is tokens x R doubles, a token's R values contiguous
//   reduce      per document, tokens in order: m_n = (p[n][0] + .. + p[n][R - 1]) / R added in r order, one log per token -
//               64 tokens side by side -, wave_sum per batch of 64, the batches added in order; doc_wll, doc_ll = 0,
//               iters = R.  An empty document scores exactly 0.
//   sum         the corpus total and its tokens: one workgroup, every thread a fixed share (completion_sum_kernel's order)
// A fixed order throughout, and every draw named by (seed, stream + particle, global document, n, n'): the same input gives
// the same bits whatever the grid, the chunks, the launches or how the documents are dealt to corpora.
#pragma once
#include "estep_common.h"
#include "philox.h"
#include "sampler_wave.h"

namespace pylda {

struct LtrParams {
    int K, ldk, R, resample;
    const int64_t* doc_ptr;
    const int32_t* term_id;
    const int32_t* term_ct;
    const int64_t* tok_off;     // nnz + 1
    const double* P;            // V x ldk
    const double* alpha;        // K
    uint16_t* z;                // (the chunk's tokens) x R
    double* p;                  // (the chunk's tokens) x R
    int64_t tok_base;           // the chunk's first token
    int64_t doc_first, doc_count;       // the documents of this launch
    double* doc_ll;             // D: 0
    double* doc_wll;            // D: the document's estimate
    int32_t* iters;             // D: R
    uint32_t first_document, stream, seed_lo, seed_hi;
};

template <int S>
__global__ __launch_bounds__(256) void ltr_particle_kernel(LtrParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t item = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (item >= p.doc_count * p.R) return;                   // (whole wavefronts)
    const int64_t d = p.doc_first + item / p.R;
    const int r = (int)(item % p.R);
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t t0 = p.tok_off[pb];
    const uint32_t ntok = (uint32_t)(p.tok_off[pe] - t0);
    const uint32_t gdoc = p.first_document + (uint32_t)d;
    const uint32_t stream = p.stream + (uint32_t)r;
    uint16_t* topic = p.z + (t0 - p.tok_base) * p.R + (int64_t)r * ntok;
    double* pout = p.p + (t0 - p.tok_base) * p.R + r;
    int nd[S];
    double al[S], apart = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        nd[s] = 0;
        al[s] = k0 + s < K ? p.alpha[k0 + s] : 0.0;
        apart = apart + al[s];
    }
    const double asum = wave_sum(apart);

    // the topic drawn (sampler_wave.h) from ((double)nd + alpha) * pr with the uniform named (inner, n); `part` is this
    // lane's slot sum of those weights, which are not kept across the scan: the owner computes its own again
    auto draw = [&](const double (&pr)[S], double part, uint32_t inner, uint32_t n) -> int {
        return wave_draw<S>([&](int s) { return ((double)nd[s] + al[s]) * pr[s]; },
                            [&] { return philox_uniform(inner, n, gdoc, stream, p.seed_lo, p.seed_hi); }, part, lane, k0);
    };

    double pon[S];
    if (pb < pe) load_topic_row<S>(p.P, p.term_id[pb], p.ldk, k0, K, pon);
    uint32_t n = 0;
    for (int64_t q = pb; q < pe; ++q) {
        double po[S];
#pragma unroll
        for (int s = 0; s < S; ++s) po[s] = pon[s];
        if (q + 1 < pe) load_topic_row<S>(p.P, p.term_id[q + 1], p.ldk, k0, K, pon);          // the next term's row, while this one's copies are drawn
        const int c = p.term_ct[q];
        for (int j = 0; j < c; ++j, ++n) {
            if (p.resample && n > 0) {
                // positions 0 .. n - 1 again: they end inside term q at the latest
                int znext = (int)topic[0];
                double pn[S];
                load_topic_row<S>(p.P, p.term_id[pb], p.ldk, k0, K, pn);
                uint32_t pos = 0;
                for (int64_t qq = pb; pos < n; ++qq) {
                    double pr[S];
#pragma unroll
                    for (int s = 0; s < S; ++s) pr[s] = pn[s];
                    if (qq < q) load_topic_row<S>(p.P, p.term_id[qq + 1], p.ldk, k0, K, pn);
                    const uint32_t copies = (uint32_t)p.term_ct[qq];
                    const uint32_t end = n - pos < copies ? n : pos + copies;
                    for (; pos < end; ++pos) {
                        const int zold = znext;
                        if (pos + 1 < n) znext = (int)topic[pos + 1];     // (its last value: it does not wait for this draw)
                        double part = 0.0;
#pragma unroll
                        for (int s = 0; s < S; ++s) {
                            if (k0 + s == zold) nd[s] -= 1;
                            part = part + ((double)nd[s] + al[s]) * pr[s];
                        }
                        const int znew = draw(pr, part, pos, n);
#pragma unroll
                        for (int s = 0; s < S; ++s)
                            if (k0 + s == znew) nd[s] += 1;
                        topic[pos] = (uint16_t)znew;      // (every lane: each lane's later reads follow its own store)
                    }
                }
            }
            double part = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) part = part + ((double)nd[s] + al[s]) * po[s];
            const double predictive = wave_sum(part) / ((double)n + asum);
            if (lane == 0) pout[(int64_t)n * p.R] = predictive;
            const int znew = draw(po, part, n, n);
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (k0 + s == znew) nd[s] += 1;
            topic[n] = (uint16_t)znew;
        }
    }
}

// one wavefront per document of the launch
__global__ __launch_bounds__(256) void ltr_reduce_kernel(LtrParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t item = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (item >= p.doc_count) return;                         // (whole wavefronts)
    const int64_t d = p.doc_first + item;
    const int64_t t0 = p.tok_off[p.doc_ptr[d]];
    const int64_t ntok = p.tok_off[p.doc_ptr[d + 1]] - t0;
    const double* pp = p.p + (t0 - p.tok_base) * p.R;
    const double particles = (double)p.R;
    double ll = 0.0;
    for (int64_t at = 0; at < ntok; at += kWave) {
        double v = 0.0;
        if (at + lane < ntok) {
            const double* row = pp + (at + lane) * p.R;
            double m = row[0];
            for (int r = 1; r < p.R; ++r) m = m + row[r];
            v = log(m / particles);
        }
        ll = ll + wave_sum(v);
    }
    if (lane == 0) {
        p.doc_ll[d] = 0.0;
        p.doc_wll[d] = ll;
        p.iters[d] = p.R;
    }
}

// The corpus' scalars in one fixed-order reduction (one workgroup, every thread a fixed share): [0] 0, [1] sum_d doc_wll[d],
// [2] the corpus' tokens (integers below 2^53: exact), and no flagged documents in the fourth scalar's bytes.
__global__ __launch_bounds__(1024) void ltr_sum_kernel(const double* __restrict__ doc_wll, const int64_t* __restrict__ doc_ptr,
                                                      const int64_t* __restrict__ tok_off, int64_t D, double* __restrict__ scalars,
                                                      int32_t* __restrict__ flagged)
{
    __shared__ double scratch[16];
    double s = 0.0, tokens = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 1024) {
        s += doc_wll[d];
        tokens += (double)(tok_off[doc_ptr[d + 1]] - tok_off[doc_ptr[d]]);
    }
    s = block_sum<1024>(s, scratch);
    tokens = block_sum<1024>(tokens, scratch);
    if (threadIdx.x == 0) {
        scalars[0] = 0.0;
        scalars[1] = s;
        scalars[2] = tokens;
        flagged[0] = 0;
    }
}

}  // namespace pylda
