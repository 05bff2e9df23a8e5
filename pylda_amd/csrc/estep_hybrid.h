// The hybrid E-step (hybrid.py:85-171 of the reference; Mimno, Hoffman & Blei 2012): a collapsed Gibbs sampler per
// document inside the variational outer loop.  One wavefront per document; topic k lives in lane k / S, slot k % S
// (S = sampler_slots(K): 1, 2, 4, 8 or 16 topics per lane).  The chain is a function of (seed, stream, global document
// index, sweep, token position) alone - every random number comes from Philox (philox.h) - so a document's samples do
// not depend on the launch shape, the document order or the sharding.  tests/hybrid_restatement.py is the same chain
// in numpy, operation for operation; DESIGN.md ("Hybrid E-step") is the specification both follow:
//
//   tokens      a document's terms in CSR order, the c_n copies of a term back to back (token position = index in
//               that order); the reference walks the text order, which LDA's exchangeability makes equivalent
//   start       r[k] = uniform(pos, phase 0, index k); colsum = wave_sum of the lanes' sequential slot sums;
//               phi[k] = r[k] / colsum; phi_sum[k] = sequential sum over the positions (fp64, as the reference)
//   sweep 1     phi_sum -= phi[:, pos] (regenerated), clamp negatives to 0, draw, phi_sum[z] += 1
//   sweeps > 1  phi_sum[z_old] -= 1, clamp, draw, phi_sum[z] += 1
//   draw        w[k] = (phi_sum[k] + alpha[k]) * B[w][k]  (B = exp(E_log_eta - shift[w]), the shifted table: the
//               shift cancels in the normalisation); the slot sums, lane scan and owner rule of sampler_wave.h with
//               t = uniform(pos, phase 1 + sweep, index 0) * total
//   state       one uint64 per token: bits [0, b) the current topic, [(j + 1) b, (j + 2) b) the j-th post-burn-in
//               sample (b = ceil(log2 K), at least 1)
//   epilogue    gamma = alpha + phi_sum; document likelihood of hybrid.py:146-159 from the histories (entropy of the
//               per-token sample frequencies with the 1e-100 floor of the K - distinct entries); held-out words
//               likelihood with E_log_eta[z][w] = psi(eta[z][w]) - psi(sum_v eta[z][v]) (not the normalised form)
#pragma once
#include "estep_common.h"
#include "philox.h"
#include "sampler_wave.h"
#include "special_device.h"

namespace pylda {

struct HybridParams {
    int K, V, ldk;
    const double* B;            // V x ldk: exp(E_log_eta - shift[w]) (padding columns zero)
    const double* alpha;        // K
    const double* eta;          // K x V (held-out words likelihood)
    const double* psi_rowsum;   // K
    const int64_t* doc_ptr;
    const int32_t* term_id;
    const int32_t* term_ct;
    const int64_t* tok_off;     // nnz + 1: exclusive scan of term_ct
    uint64_t* state;            // tokens
    double* gamma;              // D x K
    double* doc_ll;
    double* doc_wll;
    int32_t* iters;
    int32_t* status;
    int64_t D;
    uint32_t first_document, stream, seed_lo, seed_hi;
    int samples, burn_in, bits, heldout;
    double alpha_term;          // lgamma(sum alpha) - sum lgamma(alpha)
};

template <int S>
__global__ __launch_bounds__(256) void hybrid_sample_kernel(HybridParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (d >= p.D) return;                                    // (whole wavefronts)
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t t0 = p.tok_off[pb];
    const uint32_t gdoc = p.first_document + (uint32_t)d;
    double ps[S], al[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        ps[s] = 0.0;
        al[s] = k0 + s < K ? p.alpha[k0 + s] : 0.0;
    }
    // random start: phi[:, pos] = r / colsum, phi_sum = sum over the positions
    auto start_column = [&](uint32_t pos, double (&phi)[S]) {
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            phi[s] = k0 + s < K ? philox_uniform(pos, (uint32_t)(k0 + s), gdoc, p.stream, p.seed_lo, p.seed_hi) : 0.0;
            part = part + phi[s];
        }
        const double colsum = wave_sum(part);
#pragma unroll
        for (int s = 0; s < S; ++s) phi[s] = phi[s] / colsum;
    };
    const uint32_t ntok = (uint32_t)(p.tok_off[pe] - t0);
    for (uint32_t pos = 0; pos < ntok; ++pos) {
        double phi[S];
        start_column(pos, phi);
#pragma unroll
        for (int s = 0; s < S; ++s) ps[s] = ps[s] + phi[s];
    }
    const uint64_t topic_mask = ((uint64_t)1 << p.bits) - 1;
    for (int it = 0; it < p.samples; ++it) {
        const uint32_t phase = (uint32_t)(1 + it) << 16;
        const int hist_shift = it >= p.burn_in ? (it - p.burn_in + 1) * p.bits : 0;
        uint32_t pos = 0;
        double bn[S];
        if (pb < pe) load_topic_row<S>(p.B, p.term_id[pb], p.ldk, k0, K, bn);
        for (int64_t q = pb; q < pe; ++q) {
            double b[S];
#pragma unroll
            for (int s = 0; s < S; ++s) b[s] = bn[s];
            // the next term's row, while this one's tokens are drawn (the chain needs phi_sum only)
            if (q + 1 < pe) load_topic_row<S>(p.B, p.term_id[q + 1], p.ldk, k0, K, bn);
            const int c = p.term_ct[q];
            for (int j = 0; j < c; ++j, ++pos) {
                uint64_t st = 0;
                if (it == 0) {
                    double phi[S];
                    start_column(pos, phi);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const double v = ps[s] - phi[s];
                        ps[s] = v > 0.0 ? v : 0.0;
                    }
                } else {
                    st = p.state[t0 + pos];
                    const int zold = (int)(st & topic_mask);
#pragma unroll
                    for (int s = 0; s < S; ++s)
                        if (k0 + s == zold) {
                            const double v = ps[s] - 1.0;
                            ps[s] = v > 0.0 ? v : 0.0;
                        }
                }
                double w[S], part = 0.0;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    w[s] = (ps[s] + al[s]) * b[s];
                    part = part + w[s];
                }
                const int znew = wave_draw<S>([&](int s) { return w[s]; },
                                              [&] { return philox_uniform(pos, phase, gdoc, p.stream, p.seed_lo, p.seed_hi); }, part, lane, k0);
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (k0 + s == znew) ps[s] = ps[s] + 1.0;
                st = (st & ~topic_mask) | (uint64_t)znew;
                if (it >= p.burn_in) st |= (uint64_t)znew << hist_shift;
                p.state[t0 + pos] = st;          // (every lane: each lane's later reads follow its own store)
            }
        }
    }
    // epilogue: gamma (:146), document likelihood (:151-159), held-out words likelihood (:162)
    double gsum = 0.0, lg = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (k0 + s < K) {
            const double g = al[s] + ps[s];
            p.gamma[d * K + k0 + s] = g;
            gsum += g;
            lg += lgamma_pos(g);
        }
    }
    gsum = wave_sum(gsum);
    lg = wave_sum(lg);
    const int m = p.samples - p.burn_in;
    const double floor_term = 1e-100 * log(1e-100);
    double ent = 0.0, wll = 0.0;
    for (int64_t q = pb + lane; q < pe; q += kWave) {
        const int w = p.term_id[q];
        for (int64_t tk = p.tok_off[q]; tk < p.tok_off[q + 1]; ++tk) {
            const uint64_t st = p.state[tk];
            int distinct = 0;
            for (int a = 0; a < m; ++a) {
                const int za = (int)((st >> ((a + 1) * p.bits)) & topic_mask);
                bool seen = false;
                for (int e = 0; e < a; ++e) seen = seen || (int)((st >> ((e + 1) * p.bits)) & topic_mask) == za;
                if (seen) continue;
                int cnt = 0;
                for (int e = a; e < m; ++e) cnt += (int)((st >> ((e + 1) * p.bits)) & topic_mask) == za;
                const double f = (double)cnt / (double)m;
                ent += f * log(f);
                if (p.heldout) wll += f * (digamma(p.eta[(size_t)za * p.V + w]) - p.psi_rowsum[za]);
                ++distinct;
            }
            ent += (double)(K - distinct) * floor_term;
        }
    }
    ent = wave_sum(ent);
    wll = wave_sum(wll);
    if (lane == 0) {
        p.doc_ll[d] = p.alpha_term + lg - lgamma_pos(gsum) - ent;
        p.doc_wll[d] = p.heldout ? wll : 0.0;
        p.iters[d] = p.samples;
        p.status[d] = 0;
    }
}

// Sufficient statistics of the post-burn-in samples: one workgroup per word row over the postings (CSR positions
// grouped by term), integer counts in LDS (order-free, exact), written as exact doubles into the word-major V x ldk
// buffer.  The division by (samples - burn-in) is a separate step (hybrid_scale_kernel), behind any all-reduce.
__global__ __launch_bounds__(256) void hybrid_sstats_kernel(const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ post_pos,
                                                            const int64_t* __restrict__ tok_off, const uint64_t* __restrict__ state,
                                                            int K, int ldk, int samples, int burn_in, int bits,
                                                            double* __restrict__ sstats)
{
    extern __shared__ unsigned counts[];
    const int v = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += 256) counts[k] = 0u;
    __syncthreads();
    const uint64_t topic_mask = ((uint64_t)1 << bits) - 1;
    const int m = samples - burn_in;
    for (int64_t i = col_ptr[v] + threadIdx.x; i < col_ptr[v + 1]; i += 256) {
        const int64_t q = post_pos[i];
        for (int64_t tk = tok_off[q]; tk < tok_off[q + 1]; ++tk) {
            const uint64_t st = state[tk];
            for (int a = 0; a < m; ++a) {
                const unsigned z = (unsigned)((st >> ((a + 1) * bits)) & topic_mask);
                if (z < (unsigned)K) atomicAdd(&counts[z], 1u);
            }
        }
    }
    __syncthreads();
    double* row = sstats + (size_t)v * ldk;
    for (int k = threadIdx.x; k < ldk; k += 256) row[k] = k < K ? (double)counts[k] : 0.0;
}

__global__ __launch_bounds__(256) void hybrid_scale_kernel(double* __restrict__ x, int64_t n, double divisor)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = x[i] / divisor;
}

__global__ void philox_test_kernel(const uint32_t* __restrict__ in, int64_t n, uint32_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* c = in + 6 * i;
    const Philox4x32 r = philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5]);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = r.v[j];
}

}  // namespace pylda
