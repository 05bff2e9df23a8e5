// What the token samplers share - hybrid_sample_kernel (estep_hybrid.h), gibbs_sample_kernel (estep_gibbs.h),
// foldin_sample_kernel (estep_foldin.h), ltr_particle_kernel (left_to_right.h): where a topic lives in the wavefront, a
// lane's share of a table row, and the draw of a topic from the lanes' weights.  One wavefront per chain; topic k lives in
// lane k / S, slot k % S (S = sampler_slots(K): 1, 2, 4, 8 or 16 topics per lane), b = sampler_bits(K) bits per topic in a
// state word.  The weights, the state and the order of a chain's steps are each kernel's own.
//
//   draw        w[k] the caller's weights (0 in the padding slots); lane partial = sequential sum of its slots; inclusive
//               Hillis-Steele scan of the partials over the lanes (distances 1, 2, .., 32); total = lane 63's value;
//               t = u * total, u the caller's uniform; lane L = first lane with non-zero weight whose inclusive value
//               exceeds t;
//               in lane L the running sum from the exclusive value picks the first slot that exceeds t (none: the last
//               slot of L with non-zero weight); no lane exceeds t: the last topic with non-zero weight (no such
//               topic: topic 0)
#pragma once
#include "estep_common.h"

namespace pylda {

constexpr int kSamplerMaxSlots = 16;         // 64 x 16 = 1024 topics

__host__ __device__ constexpr int sampler_slots(int K)
{
    return K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
}

__host__ __device__ constexpr int sampler_bits(int K)
{
    int b = 1;
    while ((1 << b) < K) ++b;
    return b;
}

// Inclusive scan over the 64 lanes (Hillis-Steele: v_l += v_{l - d} for d = 1, 2, .., 32), in every lane.
__device__ __forceinline__ double wave_inclusive_scan(double v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double o = __shfl_up(v, d, kWave);
        if (lane >= d) v = v + o;
    }
    return v;
}

// the uniform start topic of a token
__device__ __forceinline__ int uniform_topic(double u, int K)
{
    const int z = (int)(u * (double)K);
    return z < K - 1 ? z : K - 1;
}

// this lane's S slots of row w of a word-major V x ldk table, zero past K
template <int S, typename T>
__device__ __forceinline__ void load_topic_row(const T* table, int w, int ldk, int k0, int K, T (&row)[S])
{
    const T* at = table + (size_t)w * ldk + k0;
#pragma unroll
    for (int s = 0; s < S; ++s) row[s] = k0 + s < K ? at[s] : T(0);
}

// The draw (above), in every lane: the topic drawn from the weights weight(0 .. S - 1) of this lane's slots, whose
// sequential sum is `part`.  weight: int s -> double, called again in the lane that owns the draw (a kernel short of
// registers recomputes there, the same operations, what another keeps); uniform: () -> double, called once, behind the scan.
template <int S, typename Weight, typename Uniform>
__device__ __forceinline__ int wave_draw(Weight weight, Uniform uniform, double part, int lane, int k0)
{
    const double incl = wave_inclusive_scan(part, lane);
    const double excl_raw = __shfl_up(incl, 1, kWave);
    const double excl = lane == 0 ? 0.0 : excl_raw;
    const double total = __shfl(incl, kWave - 1, kWave);
    const double t = uniform() * total;
    // (a lane without weight - padding, or a table entry underflowed to 0 - never owns the draw, even where its inclusive
    //  value exceeds t by a rounding difference of the scan)
    const uint64_t over = __ballot(incl > t && part > 0.0);
    int owner, z = -1;
    if (over) {
        owner = __ffsll((unsigned long long)over) - 1;
        if (lane == owner) {
            double run = excl;
            int last = -1;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double w = weight(s);
                run = run + w;
                if (z < 0 && run > t) z = s;
                if (w > 0.0) last = s;
            }
            if (z < 0) z = last;
        }
    } else {
        // (no weight at all - alpha zero and the counts empty, or NaN - topic 0)
        const uint64_t nonzero = __ballot(part > 0.0);
        owner = nonzero ? 63 - __clzll((long long)nonzero) : 0;
        if (lane == owner) {
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (weight(s) > 0.0) z = s;
            if (z < 0) z = 0;
        }
    }
    return __shfl(k0 + z, owner, kWave);
}

}  // namespace pylda
