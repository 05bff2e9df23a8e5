// Philox4x32-10 (Salmon, Moraes, Dror & Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC 2011): a counter-based
// generator - every output block is a pure function of (counter, key), so a draw can be recomputed anywhere, in any
// order, on any launch shape.  The hybrid E-step (estep_hybrid.h) names every draw by
//   key     = seed (64 bits: low word, high word)
//   counter = [token position in the document, phase << 16 | index, global document index, stream]
// with phase 0 / index k for the random start phi[k][pos] and phase 1 + sweep / index 0 for the topic draw of a
// sweep ("Hybrid E-step").  Host and device share this code (the known-answer test runs both).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pylda {

struct Philox4x32 {
    uint32_t v[4];
};

__host__ __device__ __forceinline__ Philox4x32 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                             uint32_t k1)
{
    constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += kW0;
            k1 += kW1;
        }
        const uint64_t p0 = (uint64_t)kM0 * c0, p1 = (uint64_t)kM1 * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
    return Philox4x32{{c0, c1, c2, c3}};
}

// A double in [0, 1) from the first 64 bits of a block: (x0 | x1 << 32) >> 11, times 2^-53.
__host__ __device__ __forceinline__ double philox_uniform(uint32_t pos, uint32_t phase_index, uint32_t doc, uint32_t stream,
                                                          uint32_t seed_lo, uint32_t seed_hi)
{
    const Philox4x32 r = philox4x32_10(pos, phase_index, doc, stream, seed_lo, seed_hi);
    const uint64_t u = (uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32);
    return (double)(u >> 11) * 0x1.0p-53;
}

}  // namespace pylda
