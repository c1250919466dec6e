// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator of the sampled
// decode step (elem.hip: sample_step_k). Plain integer code that compiles for the host and for the device: the draw of (seed, row, draw index) is a
// pure function, the same on every run, on both sides and inside or outside a captured graph.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDX_PHILOX_HD __host__ __device__ inline
#else
#define RDX_PHILOX_HD inline
#endif

namespace rdx {

// out[0 .. 3] = philox4x32_10(counter ctr[0 .. 3], key key[0 .. 1])
RDX_PHILOX_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the 24 random bits of row `row` at draw index `draw` (the number of tokens the row has generated): counter (row, draw, 0, 0), key = the seed's halves
RDX_PHILOX_HD uint32_t sample_u24(uint64_t seed, uint32_t row, uint32_t draw) {
    const uint32_t ctr[4] = {row, draw, 0u, 0u}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t out[4];
    philox4x32_10(ctr, key, out);
    return out[0] >> 8;
}

}  // namespace rdx
