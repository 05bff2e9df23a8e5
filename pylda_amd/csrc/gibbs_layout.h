// What the collapsed Gibbs sampler (estep_gibbs.h) and the held-out fold-in (estep_foldin.h) share: where a topic lives
// in the wavefront, and the lane scan a draw is read from.
#pragma once
#include "estep_common.h"

namespace pylda {

// (the hybrid sampler's layout, estep_hybrid.h: topic k in lane k / S, slot k % S; b bits per topic)
__host__ __device__ constexpr int gibbs_slots(int K)
{
    return K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
}

__host__ __device__ constexpr int gibbs_bits(int K)
{
    int b = 1;
    while ((1 << b) < K) ++b;
    return b;
}

// Inclusive scan over the 64 lanes (Hillis-Steele: v_l += v_{l - d} for d = 1, 2, .., 32), in every lane.
__device__ __forceinline__ double gibbs_inclusive_scan(double v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double o = __shfl_up(v, d, kWave);
        if (lane >= d) v = v + o;
    }
    return v;
}

}  // namespace pylda
