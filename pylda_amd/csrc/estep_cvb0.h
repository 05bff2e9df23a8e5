// The collapsed variational Bayes engine in its zero-order form (CVB0: Teh, Newman & Welling 2006; Asuncion, Welling, Smyth
// & Teh 2009) as a document-parallel chain with block-synchronous expected counts.  DESIGN.md section 21 is the
// specification; tests/cvb0_restatement.py is the same chain in numpy, operation for operation, and the two agree on every
// bit (an update is add, multiply and divide: there is no transcendental and, after the start, no random number).
//
//   state       per distinct (document, term) slot q of the CSR a row g[q][0 .. K) of doubles (nnz x ldk, zero padding): the
//               c_q copies of a term in a document share one row; T word-major V x ldk doubles, the expected word-topic
//               counts; n_k; N_dk in the corpus' gamma buffer
//   start       every copy of slot q draws uniform_topic(uniform(token position, phase 0, global document, stream), K), m[k]
//               the copies that drew k; g[q][k] = (double)m[k] / (double)c_q; T, n_k and N_dk the integer histograms (small
//               integers in doubles add exactly in any order: atomics here and only here)
//   blocks      block b of a sweep = the documents whose GLOBAL index is b modulo `blocks`; a sweep is a round per block
//               that holds a document: cvb0_update_kernel, the two apply kernels, the two n_k kernels, in stream order
//   update      one wavefront per document of the block, topic k in lane k / S, slot k % S (sampler_wave.h); T and n_k are
//               read only and keep their values of the round's start.  For slot q in CSR order, go = g[q], tr = T[w_q]:
//               a = (nd - go) + al, b = (tr - go) + beta_w, n = (nks - go) + beta_sum, w = a * b / n (0 in the padding),
//               part the sequential sum of the lane's slots from 0.0, total lane 63 of wave_inclusive_scan(part); total
//               not positive and finite: the slot keeps go, its delta is 0; else gn = w / total, df = gn - go,
//               dl = c * df, nd += dl, nks += dl, g[q] = gn, delta[q's place in the block] = dl.  Every lane adds
//               c * |df| to a sum of its own; one lane scan at the document's end is the document's change
//   apply       partial[segment][k] = the sequential sum, from 0.0, of delta[posting][k] over the segment's postings (a
//               word's postings within the block in document order, cut into segments of 256); then
//               T[w][k] = ((T[w][k] + partial_0[k]) + partial_1[k]) + .. in segment order.  No floating-point atomics
//   n_k         recomputed from T after every apply: chunks of 1024 words summed sequentially from 0.0 in word order, the
//               chunk sums summed sequentially from 0.0
//   likelihood  per document sum_q c_q log(sum_k theta_k P[w_q][k]), theta = (N_dk + alpha) / sum,
//               P[w][k] = (T[w][k] + beta_w) / (n_k[k] + beta_sum) on the fly: the scoring form of estep_foldin.h
//   fold-in     one wavefront per held-out document, all sweeps in one launch against the context's predictive table P:
//               w = ((nd - go) + al) * P[w_q][k], the update's normalisation, nd += c * (gn - go); gamma = alpha + nd
#pragma once
#include "estep_common.h"
#include "philox.h"
#include "sampler_wave.h"

namespace pylda {

constexpr int kCvb0Chunk = 1024;            // words per chunk of the n_k sums

struct Cvb0Params {
    int K, V, ldk;
    const int64_t* doc_ptr;
    const int32_t* term_id;
    const int32_t* term_ct;
    const int64_t* tok_off;     // nnz + 1
    double* g;                  // nnz x ldk
    double* n_dk;               // D x K (the corpus' gamma buffer)
    double* table;              // V x ldk
    double* n_k;                // K
    const double* alpha;        // K
    const double* beta;         // V
    double beta_sum;
    double* delta;              // (largest block's slots) x ldk
    const int64_t* slot_place;  // nnz: a slot's row of delta
    double* doc_change;         // D
    int64_t D;                  // documents of the corpus
    int64_t first;              // first local document of this launch's block
    int64_t step;               // ... and the distance to the next (= blocks); count of them:
    int64_t count;
    uint32_t first_document, stream, seed_lo, seed_hi;
};

// The start of slot q: m[s] = the copies of the term that drew this lane's topic k0 + s, as doubles (exact integers).
template <int S>
__device__ __forceinline__ void cvb0_start_counts(uint32_t pos, int c, uint32_t gdoc, uint32_t stream, uint32_t seed_lo, uint32_t seed_hi,
                                                  int K, int k0, double (&m)[S])
{
#pragma unroll
    for (int s = 0; s < S; ++s) m[s] = 0.0;
    for (int j = 0; j < c; ++j) {
        const double u = philox_uniform(pos + (uint32_t)j, 0u, gdoc, stream, seed_lo, seed_hi);
        const int z = uniform_topic(u, K);
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (k0 + s == z) m[s] = m[s] + 1.0;
    }
}

// Initial state: one wavefront per document, term after term.  T by atomics (sums of small integers: exact in any order).
template <int S>
__global__ __launch_bounds__(256) void cvb0_init_kernel(Cvb0Params p)
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
        const int c = p.term_ct[q];
        double m[S];
        cvb0_start_counts<S>((uint32_t)(p.tok_off[q] - t0), c, gdoc, 0u, p.seed_lo, p.seed_hi, K, k0, m);
        double* row = p.g + (size_t)q * p.ldk + k0;
        double* trow = p.table + (size_t)p.term_id[q] * p.ldk + k0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (k0 + s < K) {               // (the padding of g was cleared before the launch)
                row[s] = m[s] / (double)c;
                if (m[s] != 0.0) atomicAdd(&trow[s], m[s]);
            }
            nd[s] = nd[s] + m[s];
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (k0 + s < K) p.n_dk[d * K + k0 + s] = nd[s];
    if (lane == 0) p.doc_change[d] = 0.0;
}

// The normalisation the update and the fold-in share: w[] the lane's weights (0 in the padding), go[] the slot's row.
// Returns whether the row moved; then gn[] is the new row and df[] = gn - go.
template <int S>
__device__ __forceinline__ bool cvb0_normalise(const double (&w)[S], const double (&go)[S], int lane, double (&gn)[S], double (&df)[S])
{
    double part = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) part = part + w[s];
    const double total = __shfl(wave_inclusive_scan(part, lane), kWave - 1, kWave);
    const bool moves = total > 0.0 && total <= 1.7976931348623157e308;       // (positive and finite; NaN fails both)
#pragma unroll
    for (int s = 0; s < S; ++s) {
        gn[s] = moves ? w[s] / total : go[s];
        df[s] = moves ? gn[s] - go[s] : 0.0;
    }
    return moves;
}

template <int S>
__global__ __launch_bounds__(256) void cvb0_update_kernel(Cvb0Params p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (i >= p.count) return;                                // (whole wavefronts)
    const int64_t d = p.first + i * p.step;
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    double nd[S], nks[S], al[S], tn[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool real = k0 + s < K;
        nd[s] = real ? p.n_dk[d * K + k0 + s] : 0.0;
        nks[s] = real ? p.n_k[k0 + s] : 0.0;
        al[s] = real ? p.alpha[k0 + s] : 0.0;
        tn[s] = 0.0;
    }
    if (pb < pe) load_topic_row<S>(p.table, p.term_id[pb], p.ldk, k0, K, tn);
    double bwn = pb < pe ? p.beta[p.term_id[pb]] : 0.0;
    double change = 0.0;
    for (int64_t q = pb; q < pe; ++q) {
        double tr[S], go[S], w[S], gn[S], df[S];
        const double bw = bwn;
#pragma unroll
        for (int s = 0; s < S; ++s) tr[s] = tn[s];
        if (q + 1 < pe) {           // the next term's row, while this one is updated
            const int w_next = p.term_id[q + 1];
            load_topic_row<S>(p.table, w_next, p.ldk, k0, K, tn);
            bwn = p.beta[w_next];
        }
        double* row = p.g + (size_t)q * p.ldk + k0;
#pragma unroll
        for (int s = 0; s < S; ++s) go[s] = k0 + s < K ? row[s] : 0.0;
        const double c = (double)p.term_ct[q];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const double a = (nd[s] - go[s]) + al[s];
            const double b = (tr[s] - go[s]) + bw;
            const double n = (nks[s] - go[s]) + p.beta_sum;
            w[s] = k0 + s < K ? a * b / n : 0.0;
        }
        cvb0_normalise<S>(w, go, lane, gn, df);
        double* drow = p.delta + (size_t)p.slot_place[q] * p.ldk + k0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const double dl = c * df[s];
            nd[s] = nd[s] + dl;
            nks[s] = nks[s] + dl;
            change = change + c * fabs(df[s]);
            if (k0 + s < K) {
                row[s] = gn[s];
                drow[s] = dl;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
        if (k0 + s < K) p.n_dk[d * K + k0 + s] = nd[s];
    const double doc_change = wave_inclusive_scan(change, lane);
    if (lane == kWave - 1) p.doc_change[d] = doc_change;
}

// partial[segment][k]: one workgroup (64 threads up to 64 topics, else 256) per segment of the round, threads over the topics.  seg_begin: the round's
// segments + 1, positions in the whole posting list; post0 the round's first posting (a posting's delta row: its
// position - post0).
__global__ __launch_bounds__(256) void cvb0_partial_kernel(const double* __restrict__ delta, const int64_t* __restrict__ seg_begin,
                                                           int64_t post0, int K, int ldk, double* __restrict__ partial)
{
    const int64_t seg = blockIdx.x;
    const int64_t lo = seg_begin[seg] - post0, hi = seg_begin[seg + 1] - post0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        double s = 0.0;
        for (int64_t at = lo; at < hi; ++at) s = s + delta[(size_t)at * ldk + k];
        partial[(size_t)seg * ldk + k] = s;
    }
}

// T[w] += its run's partial rows, in segment order: one workgroup per run (a word with postings in the block).
// run_seg: the round's runs + 1, segment numbers of the whole list; seg0 the round's first segment.
__global__ __launch_bounds__(256) void cvb0_combine_kernel(const double* __restrict__ partial, const int32_t* __restrict__ run_word,
                                                           const int64_t* __restrict__ run_seg, int64_t seg0, int K, int ldk,
                                                           double* __restrict__ table)
{
    const int64_t run = blockIdx.x;
    const int64_t lo = run_seg[run] - seg0, hi = run_seg[run + 1] - seg0;
    double* row = table + (size_t)run_word[run] * ldk;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        double t = row[k];
        for (int64_t seg = lo; seg < hi; ++seg) t = t + partial[(size_t)seg * ldk + k];
        row[k] = t;
    }
}

// chunk[c][k] = the sequential sum from 0.0 of T[w][k] over the chunk's words: one workgroup per (chunk, 256 topics)
__global__ __launch_bounds__(256) void cvb0_nk_chunk_kernel(const double* __restrict__ table, int V, int K, int ldk, double* __restrict__ chunk)
{
    const int k = blockIdx.y * 256 + threadIdx.x;
    if (k >= K) return;
    const int w0 = blockIdx.x * kCvb0Chunk, w1 = min(V, w0 + kCvb0Chunk);
    double s = 0.0;
    for (int w = w0; w < w1; ++w) s = s + table[(size_t)w * ldk + k];
    chunk[(size_t)blockIdx.x * ldk + k] = s;
}

// n_k[k] = the sequential sum from 0.0 of the chunk sums
__global__ __launch_bounds__(256) void cvb0_nk_sum_kernel(const double* __restrict__ chunk, int chunks, int K, int ldk, double* __restrict__ n_k)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s = s + chunk[(size_t)c * ldk + k];
    n_k[k] = s;
}

// theta, then the document's plug-in likelihood against rows formed by `row_of` (int64 q, double (&row)[S]); the scoring
// form of foldin_sample_kernel's tail.  th[]: the lane's gamma entries (0 in the padding).
template <int S, typename RowOf>
__device__ __forceinline__ double cvb0_plug_in(double (&th)[S], int64_t pb, int64_t pe, const int32_t* term_ct, RowOf row_of)
{
    double gpart = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) gpart = gpart + th[s];
    const double gsum = wave_sum(gpart);
#pragma unroll
    for (int s = 0; s < S; ++s) th[s] = th[s] / gsum;
    double ll = 0.0;
    for (int64_t q = pb; q < pe; ++q) {
        double row[S], part = 0.0;
        row_of(q, row);
#pragma unroll
        for (int s = 0; s < S; ++s) part = part + th[s] * row[s];
        ll = ll + (double)term_ct[q] * log(wave_sum(part));
    }
    return ll;
}

// The training plug-in likelihood: one wavefront per document.
template <int S>
__global__ __launch_bounds__(256) void cvb0_likelihood_kernel(Cvb0Params p, double* __restrict__ doc_ll, double* __restrict__ doc_wll)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (d >= p.D) return;                                    // (whole wavefronts)
    const int K = p.K, k0 = lane * S;
    double th[S], den[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool real = k0 + s < K;
        th[s] = real ? p.n_dk[d * K + k0 + s] + p.alpha[k0 + s] : 0.0;
        den[s] = real ? p.n_k[k0 + s] + p.beta_sum : 1.0;
    }
    const double ll = cvb0_plug_in<S>(th, p.doc_ptr[d], p.doc_ptr[d + 1], p.term_ct, [&](int64_t q, double (&row)[S]) {
        const int w = p.term_id[q];
        const double bw = p.beta[w];
        load_topic_row<S>((const double*)p.table, w, p.ldk, k0, K, row);
#pragma unroll
        for (int s = 0; s < S; ++s) row[s] = k0 + s < K ? (row[s] + bw) / den[s] : 0.0;
    });
    if (lane == 0) {
        doc_ll[d] = 0.0;
        doc_wll[d] = ll;
    }
}

// scalars of pylda_estep_results as foldin_sum_kernel leaves them ([1] = sum_d doc_wll[d]); with doc_change (training)
// out[0] = that sum, out[1] = sum_d doc_change[d].  One workgroup, every thread a fixed share.
__global__ __launch_bounds__(256) void cvb0_sum_kernel(const double* __restrict__ doc_wll, const double* __restrict__ doc_change, int64_t D,
                                                       double* __restrict__ scalars, double* __restrict__ out)
{
    __shared__ double scratch[4];
    double s = 0.0, c = 0.0;
    for (int64_t d = threadIdx.x; d < D; d += 256) {
        s += doc_wll[d];
        if (doc_change) c += doc_change[d];
    }
    s = block_sum<256>(s, scratch);
    c = block_sum<256>(c, scratch);
    if (threadIdx.x == 0) {
        scalars[0] = 0.0;
        scalars[1] = s;
        scalars[2] = 0.0;
        scalars[3] = 0.0;
        if (doc_change) {
            out[0] = s;
            out[1] = c;
        }
    }
}

struct Cvb0FoldinParams {
    int K, V, ldk;
    const int64_t* doc_ptr;
    const int32_t* term_id;
    const int32_t* term_ct;
    const int64_t* tok_off;     // nnz + 1
    double* g;                  // nnz x ldk: the slots' rows (scratch of the held-out corpus)
    const double* P;            // V x ldk
    const double* alpha;        // K
    double* gamma;              // D x K
    double* doc_ll;             // D: 0
    double* doc_wll;            // D: the document's likelihood
    int32_t* iters;             // D: sweeps
    int64_t D;
    int sweeps;
    uint32_t first_document, stream, seed_lo, seed_hi;
};

template <int S>
__global__ __launch_bounds__(256) void cvb0_foldin_kernel(Cvb0FoldinParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (d >= p.D) return;                                    // (whole wavefronts)
    const int K = p.K, k0 = lane * S;
    const int64_t pb = p.doc_ptr[d], pe = p.doc_ptr[d + 1];
    const int64_t t0 = p.tok_off[pb];
    const uint32_t gdoc = p.first_document + (uint32_t)d;
    double nd[S], al[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        nd[s] = 0.0;
        al[s] = k0 + s < K ? p.alpha[k0 + s] : 0.0;
    }
    for (int64_t q = pb; q < pe; ++q) {
        const int c = p.term_ct[q];
        double m[S];
        cvb0_start_counts<S>((uint32_t)(p.tok_off[q] - t0), c, gdoc, p.stream, p.seed_lo, p.seed_hi, K, k0, m);
        double* row = p.g + (size_t)q * p.ldk + k0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (k0 + s < K) row[s] = m[s] / (double)c;      // (every lane reads back only what it stored itself)
            nd[s] = nd[s] + m[s];
        }
    }
    for (int it = 0; it < p.sweeps; ++it) {
        double pn[S];
        if (pb < pe) load_topic_row<S>(p.P, p.term_id[pb], p.ldk, k0, K, pn);
        for (int64_t q = pb; q < pe; ++q) {
            double pr[S], go[S], w[S], gn[S], df[S];
#pragma unroll
            for (int s = 0; s < S; ++s) pr[s] = pn[s];
            if (q + 1 < pe) load_topic_row<S>(p.P, p.term_id[q + 1], p.ldk, k0, K, pn);     // the next term's row
            double* row = p.g + (size_t)q * p.ldk + k0;
#pragma unroll
            for (int s = 0; s < S; ++s) go[s] = k0 + s < K ? row[s] : 0.0;
            const double c = (double)p.term_ct[q];
#pragma unroll
            for (int s = 0; s < S; ++s) w[s] = k0 + s < K ? ((nd[s] - go[s]) + al[s]) * pr[s] : 0.0;
            cvb0_normalise<S>(w, go, lane, gn, df);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                nd[s] = nd[s] + c * df[s];
                if (k0 + s < K) row[s] = gn[s];
            }
        }
    }
    double th[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        th[s] = k0 + s < K ? al[s] + nd[s] : 0.0;
        if (k0 + s < K) p.gamma[d * K + k0 + s] = th[s];
    }
    const double ll = cvb0_plug_in<S>(th, pb, pe, p.term_ct, [&](int64_t q, double (&row)[S]) {
        load_topic_row<S>(p.P, p.term_id[q], p.ldk, k0, K, row);
    });
    if (lane == 0) {
        p.doc_ll[d] = 0.0;
        p.doc_wll[d] = ll;
        p.iters[d] = p.sweeps;
    }
}

}  // namespace pylda
