// Stochastic collapsed variational Bayes (SCVB0: Foulds, Boyles, DuBois, Smyth & Welling 2013) as minibatch steps over the
// blocks of the CVB0 engine, without its per-slot rows.  DESIGN.md section 22 is the specification;
// tests/scvb_restatement.py is the same chain in numpy, operation for operation, and the two agree on every bit (a step is
// add, multiply and divide; the step sizes are the host's, the power below is adds and multiplies only).
//
//   state       T word-major V x ldk doubles, the expected word-topic counts; n_k its column sums; N_dk in the corpus' gamma
//               buffer.  Nothing per (document, term) slot
//   start       CVB0's without the rows: every copy of a slot draws uniform_topic(uniform(token position, phase 0, global
//               document, stream 0), K); T and N_dk the integer histograms (atomics here and only here), n_k from T
//   step        block b = the documents whose GLOBAL index is b modulo B: scvb_update_kernel, cvb0_partial_kernel, the run
//               map, scvb_blend_kernel, the two n_k kernels, in stream order
//   update      one wavefront per document of the block, topic k in lane k / S, slot k % S (sampler_wave.h); T and n_k are
//               read only.  nd = N_dk, den = n_k + beta_sum, Cj the document's tokens.  For pass p = 0 .. P, for slot q in
//               CSR order, tr = T[w_q]: a = nd + al, b = tr + beta_w, w = a * b / den (0 in the padding); part the
//               sequential sum of the lane's slots from 0.0, total lane 63 of wave_inclusive_scan(part); total not positive
//               and finite: nothing moves, and in the last pass the slot's delta row is zeros; else gn = w / total,
//               qm = one_minus[p] ** c by binary exponentiation in double-double arithmetic (scvb_power),
//               nd = (qm * nd) + (((1.0 - qm) * Cj) * gn), and in the last pass
//               delta[q's place in the block] = (double)c * gn.  At the end doc_change = lane 63 of the scan of the
//               lanes' sequential sums of |nd - N_dk| (the old row read again), then N_dk = nd
//   blend       partial[segment][k] exactly CVB0's; then over EVERY word s = the sequential sum from 0.0 of the partial rows of
//               the word's run in segment order (0.0 without postings in the block) and
//               T[w][k] = (keep * T[w][k]) + (gain * s).  No floating-point atomics
//   n_k         recomputed from T by CVB0's chunk kernels
#pragma once
#include "estep_cvb0.h"

namespace pylda {

constexpr int kScvbMaxPasses = 16;          // burn_in <= 15

struct ScvbParams {
    Cvb0Params c;                           // (g unused; first, step, count: the block's documents)
    int passes;                             // burn_in + 1
    double one_minus[kScvbMaxPasses];       // 1 - rho_theta of every pass
};

// The start: cvb0_init_kernel without the slots' rows.
template <int S>
__global__ __launch_bounds__(256) void scvb_init_kernel(Cvb0Params p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (d >= p.D) return;                                    // (whole wavefronts)
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t t0 = p.tok_off[pb];
    const uint32_t gdoc = p.first_document + (uint32_t)d;
    double nd[S];
#pragma unroll
    for (int s = 0; s < S; ++s) nd[s] = 0.0;
    for (int64_t q = pb; q < pe; ++q) {
        double m[S];
        cvb0_start_counts<S>((uint32_t)(p.tok_off[q] - t0), p.term_ct[q], gdoc, 0u, p.seed_lo, p.seed_hi, K, k0, m);
        double* trow = p.table + (size_t)p.term_id[q] * p.ldk + k0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (k0 + s < K && m[s] != 0.0) atomicAdd(&trow[s], m[s]);
            nd[s] = nd[s] + m[s];
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (k0 + s < K) p.n_dk[d * K + k0 + s] = nd[s];
    if (lane == 0) p.doc_change[d] = 0.0;
}

// (ah + al) * (bh + bl) as a double-double (the restatement's _dd_mul): Dekker's exact product of the high parts through
// Veltkamp splits - no fused multiply-add; the translation unit is built with -ffp-contract=off -, the cross terms, one
// renormalisation.  Every operation is a rounded add, subtract or multiply, in this order.
__device__ __forceinline__ void scvb_dd_mul(double ah, double al, double bh, double bl, double& hi, double& lo)
{
    const double p = ah * bh;
    const double ta = 134217729.0 * ah, a1 = ta - (ta - ah), a2 = ah - a1;
    const double tb = 134217729.0 * bh, b1 = tb - (tb - bh), b2 = bh - b1;
    double e = (((a1 * b1 - p) + a1 * b2) + a2 * b1) + a2 * b2;
    e = e + (ah * bl + al * bh);
    hi = p + e;
    lo = e - (hi - p);
}

// x ** n for x in [0, 1], n >= 1 (the restatement's binary_power): binary exponentiation in double-double arithmetic,
// rounded to a double at the end.  The same loop in plain doubles is 54 ulp off at 0.874 ** 300 - a squaring doubles the
// relative error it inherits.  n = 1 is x itself there too (1 * x is exact), so it skips the loop.
__device__ __forceinline__ double scvb_power(double x, int n)
{
    if (n == 1) return x;
    double rh = 1.0, rl = 0.0, xh = x, xl = 0.0;
    while (n) {
        if (n & 1) scvb_dd_mul(rh, rl, xh, xl, rh, rl);
        n >>= 1;
        if (n) scvb_dd_mul(xh, xl, xh, xl, xh, xl);
    }
    return rh;
}

template <int S>
__global__ __launch_bounds__(256) void scvb_update_kernel(ScvbParams sp)
{
    const Cvb0Params& p = sp.c;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (i >= p.count) return;                                // (whole wavefronts)
    const int64_t d = p.first + i * p.step;
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const double Cj = (double)(p.tok_off[pe] - p.tok_off[pb]);
    double nd[S], den[S], al[S], tn[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool real = k0 + s < K;
        nd[s] = real ? p.n_dk[d * K + k0 + s] : 0.0;
        den[s] = real ? p.n_k[k0 + s] + p.beta_sum : 1.0;
        al[s] = real ? p.alpha[k0 + s] : 0.0;
        tn[s] = 0.0;
    }
    if (pb < pe) load_topic_row<S>(p.table, p.term_id[pb], p.ldk, k0, K, tn);
    double bwn = pb < pe ? p.beta[p.term_id[pb]] : 0.0;
    for (int pass = 0; pass < sp.passes; ++pass) {
        const double one_minus = sp.one_minus[pass];
        const bool last = pass + 1 == sp.passes;
        for (int64_t q = pb; q < pe; ++q) {
            double tr[S], w[S];
            const double bw = bwn;
#pragma unroll
            for (int s = 0; s < S; ++s) tr[s] = tn[s];
            if (q + 1 < pe || !last) {      // the next term's row (the next pass' first), while this one is updated
                const int w_next = p.term_id[q + 1 < pe ? q + 1 : pb];
                load_topic_row<S>(p.table, w_next, p.ldk, k0, K, tn);
                bwn = p.beta[w_next];
            }
            const int c = p.term_ct[q];
            double part = 0.0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double a = nd[s] + al[s];
                const double b = tr[s] + bw;
                w[s] = k0 + s < K ? a * b / den[s] : 0.0;
                part = part + w[s];
            }
            const double total = __shfl(wave_inclusive_scan(part, lane), kWave - 1, kWave);
            const bool moves = total > 0.0 && total <= 1.7976931348623157e308;       // (positive and finite; NaN fails both)
            if (moves) {
                const double qm = scvb_power(one_minus, c);
                const double pull = (1.0 - qm) * Cj;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    w[s] = w[s] / total;
                    nd[s] = (qm * nd[s]) + (pull * w[s]);
                }
            }
            if (last) {
                double* drow = p.delta + (size_t)p.slot_place[q] * p.ldk + k0;
                const double cd = (double)c;
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (k0 + s < K) drow[s] = moves ? cd * w[s] : 0.0;
            }
        }
    }
    double change = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (k0 + s < K) {
            double* at = p.n_dk + d * K + k0 + s;
            change = change + fabs(nd[s] - *at);
            *at = nd[s];
        }
    }
    const double doc_change = wave_inclusive_scan(change, lane);
    if (lane == kWave - 1) p.doc_change[d] = doc_change;
}

// word_run[w] = the word's run among the block's (the map was filled with -1 before): one thread per run
__global__ __launch_bounds__(256) void scvb_run_map_kernel(const int32_t* __restrict__ run_word, int64_t runs, int32_t* __restrict__ word_run)
{
    const int64_t run = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (run < runs) word_run[run_word[run]] = (int32_t)run;
}

// T[w][k] = (keep * T[w][k]) + (gain * s), s the word's partial rows summed in segment order from 0.0: one workgroup per
// word (64 threads up to 64 topics, else 256), threads over the topics.  run_seg: the block's runs + 1, segment numbers of
// the whole list; seg0 the block's first segment.
__global__ __launch_bounds__(256) void scvb_blend_kernel(const double* __restrict__ partial, const int32_t* __restrict__ word_run,
                                                         const int64_t* __restrict__ run_seg, int64_t seg0, int K, int ldk, double keep,
                                                         double gain, double* __restrict__ table)
{
    const int64_t word = blockIdx.x;
    const int32_t run = word_run[word];
    const int64_t lo = run < 0 ? 0 : run_seg[run] - seg0, hi = run < 0 ? 0 : run_seg[run + 1] - seg0;
    double* row = table + (size_t)word * ldk;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        double s = 0.0;
        for (int64_t seg = lo; seg < hi; ++seg) s = s + partial[(size_t)seg * ldk + k];
        row[k] = (keep * row[k]) + (gain * s);
    }
}

}  // namespace pylda
