// f110_gauss.h -- the policy's Gaussian draws (Actor.sample's normal.rsample(), src/SAL.py:414-421) made on the device: element
// (row r, column j) of call t of stream s under seed is
//     float32( numpy.random.Generator( numpy.random.Philox(key=[seed, s], counter=[0, j, r, t]) ).standard_normal() ),
// NumPy's bits (include/f110_hip.h, "The policy's Gaussian draws").  Every element owns a Philox stream: word 0 of the counter counts
// the element's own blocks (NumPy increments it BEFORE it produces a block, so the first four raw words are the block of counter
// [1, j, r, t]), and no lane reads a word of another's.  98.5 % of the elements take one raw word; the other three of the block are
// thrown away, which is the price of a row that does not depend on the batch around it.
// The normal is random_standard_normal's 256-layer ziggurat (numpy/random/src/distributions/distributions.c) on the tables of
// f110_ziggurat.h with glibc's log1p for the tail (log1p_glibc, f110_noise.h), one raw word per ziggurat trial and two per tail trial.
// It is a second copy of the per-draw decision of noise_rows_kernel (f110_noise_kernels.h) and not a function both call: there the
// decision is woven into a wave that walks ONE sequential PCG64 stream -- tables in LDS, a rejected candidate steps a private copy of
// the generator speculatively, and which lanes are candidates at all is settled across the wave afterwards -- so a shared function
// would have to take the source of the next word as a parameter and would change that kernel's code; its bits and registers stay
// where they are.  Here a lane simply loops over trials until it emits; a wave ends when all of its lanes have.
// No LDS, no atomics, no scratch; the tables (2 KiB each, read at a random index) come through the vector cache.  Nothing contracted.
#pragma once
#include <hip/hip_runtime.h>
#include "f110_gauss_plan.h"
#include "f110_noise.h"
#include "f110_philox.h"

#pragma clang fp contract(off)

namespace f110 {

// One draw.  The words of the element's stream are consumed in order, block after block; `state` says what the next word is for:
// 0 a new ziggurat trial, 1 the wedge test of the trial in (idx, x), 2 and 3 the two uniforms of a tail trial.  (One loop over the
// words with the Philox block at its head, not a next_word() at every place NumPy calls next_uint64: the block function is 20
// 64-bit products and would be inlined four times.)
__device__ inline float gauss_draw(uint64_t seed, uint64_t stream, uint64_t t, uint64_t r, uint64_t j)
{
    uint64_t c[4] = {0, j, r, t};
    const uint64_t k[2] = {seed, stream};
    int state = 0, idx = 0;
    uint64_t rabs = 0;
    double x = 0.0, xx = 0.0;
    for (;;) {
        uint64_t w[4];
        c[0]++;
        philox4x64_10(c, k, w);
#pragma unroll 1
        for (int pos = 0; pos < 4; pos++) {
            uint64_t raw = pos == 0 ? w[0] : pos == 1 ? w[1] : pos == 2 ? w[2] : w[3];
            if (state == 0) {
                // r = next_uint64; idx = r & 0xff; r >>= 8; sign = r & 1; rabs = (r >> 1) & 0x000fffffffffffff; x = rabs * wi[idx];
                // if (sign) x = -x; if (rabs < ki[idx]) return x;
                idx = (int)(raw & 0xffull);
                raw >>= 8;
                const bool neg = (raw & 1ull) != 0;
                rabs = (raw >> 1) & 0x000fffffffffffffull;
                x = (double)rabs * ZIG_WI[idx];
                if (neg) x = -x;
                if (rabs < ZIG_KI[idx]) return (float)x;
                state = idx == 0 ? 2 : 1;
                continue;
            }
            const double u = (double)(raw >> 11) * (1.0 / 9007199254740992.0);      // next_double
            if (state == 1) {
                // wedge: ((fi[idx-1] - fi[idx]) * U + fi[idx]) < exp(-0.5 * x * x) ? return x : draw again
                if (((ZIG_FI[idx - 1] - ZIG_FI[idx]) * u + ZIG_FI[idx]) < exp(-0.5 * x * x)) return (float)x;
                state = 0;
                continue;
            }
            // tail: xx = -inv_r * log1p(-U1), yy = -log1p(-U2) until yy + yy > xx * xx
            const double l = log1p_glibc(-u);
            if (state == 2) { xx = -ZIG_NOR_INV_R * l; state = 3; continue; }
            const double yy = -l;
            if (yy + yy > xx * xx) return (float)(((rabs >> 8) & 1ull) ? -(ZIG_NOR_R + xx) : ZIG_NOR_R + xx);
            state = 2;
        }
    }
}

// grid: gauss_plan(); one lane per element e = i * A + j of out [n, A], striding by the grid where n * A exceeds it
static __global__ __launch_bounds__(GS_THREADS) void gauss_fill_kernel(GaussArgs a)
{
    uint64_t seed = a.seed, t = a.t;
    if (a.state) { seed = a.state->seed; t = a.state->calls[a.stream]; }
    const uint32_t stride = gridDim.x * GS_THREADS;
    for (uint32_t base = blockIdx.x * GS_THREADS; base < a.total; base += stride) {       // (uniform across the workgroup)
        const uint32_t e = base + threadIdx.x;
        float v = 0.0f;
        if (e < a.total) {
            const uint32_t i = e / a.A, j = e - i * a.A;
            const uint64_t r = a.rows ? (uint64_t)a.rows[i] : (uint64_t)i;
            v = gauss_draw(seed, a.stream, t, r, j);
        }
        if (a.vec) {
            // the lane on a 16-byte boundary stores its three neighbours' values with its own; a last group that is not whole stores singly
            const float v1 = __shfl_down(v, 1), v2 = __shfl_down(v, 2), v3 = __shfl_down(v, 3);
            if ((e | 3u) < a.total) {
                if ((e & 3u) == 0) *reinterpret_cast<float4 *>(a.out + e) = make_float4(v, v1, v2, v3);
            } else if (e < a.total) a.out[e] = v;
        } else if (e < a.total) a.out[e] = v;
    }
}

// behind a fill on the same stream: the next fill of this stream of draws reads t + 1 (a captured pair replays with a fresh t)
static __global__ void gauss_advance_kernel(f110_gauss_state *state, int stream)
{
    if (threadIdx.x == 0) state->calls[stream] += 1;
}

} // namespace f110
