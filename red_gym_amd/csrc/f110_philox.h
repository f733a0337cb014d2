// f110_philox.h -- Philox4x64-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11; NumPy's
// numpy/random/src/philox/philox.h) as one block function: a 256-bit counter and a 128-bit key give four 64-bit words, and nothing
// is carried from block to block, so any block of any stream is computed without walking another.
// Plain C++ without HIP, F110_HD: the device (f110_gauss.h) and a host program (tests/test_gauss_cpu.py) run the same text.
// The 64 x 64 -> 128-bit products are written in 32-bit halves, which is what gfx950 issues them as (v_mul_lo_u32 / v_mul_hi_u32;
// there is no 64-bit integer multiplier): four partial products of 64 bits each, the carries of the middle column added once.
#pragma once
#include "f110_launch.h"

namespace f110 {

constexpr uint64_t PHILOX_M0 = 0xD2E7470EE14C6C93ull, PHILOX_M1 = 0xCA5A826395121157ull;   // the multipliers of words 0 and 2
constexpr uint64_t PHILOX_W0 = 0x9E3779B97F4A7C15ull, PHILOX_W1 = 0xBB67AE8584CAA73Bull;   // the Weyl increments of the key
constexpr int PHILOX_ROUNDS = 10;

F110_HD inline void philox_mulhilo(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo)
{
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;      // (at most 3 * (2^32 - 1): no overflow)
    lo = (mid << 32) | (uint32_t)p00;
    hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// out[0..3] = philox4x64-10(counter c[0..3], key k[0..1]); c[0] is the least significant counter word, as in NumPy's `counter`
F110_HD inline void philox4x64_10(const uint64_t c[4], const uint64_t k[2], uint64_t out[4])
{
    uint64_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
    for (int r = 0; r < PHILOX_ROUNDS; r++) {
        uint64_t hi0, lo0, hi1, lo1;
        philox_mulhilo(PHILOX_M0, c0, hi0, lo0);
        philox_mulhilo(PHILOX_M1, c2, hi1, lo1);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;      // (the bump behind the last round is not used)
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

} // namespace f110
