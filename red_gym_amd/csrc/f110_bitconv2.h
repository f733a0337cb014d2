// f110_bitconv2.h -- the stem of the reference's policy for acting (src/SAL.py:397-398, 405-406, 429-430, 436-437:
// relu(conv2(relu(conv1(x)))) with conv2 = nn.Conv2d(16, 32, kernel_size=4, stride=2)) in one kernel: the first layer's
// activations are made from the frame's bits as f110_bitconv.h makes them, live in LDS only, and the second layer is a GEMM on
// the fp32 matrix cores whose result is all that reaches memory (32 x 30 x 30 fp32 per frame instead of 16 x 63 x 63 as well).
//   bitconv2_forward_kernel<false>  a workgroup walks work items (sample, band of BR rows of conv2 outputs), item = blockIdx.x,
//                            + gridDim.x, ...  Per item: the band's image rows -> LDS words (bitconv_stage); lane = column, wave =
//                            row of the (BR - 1) s2 + k2 conv1 rows under the band: mask (bitconv_mask), the first layer's
//                            fma chain per channel, result to a1[ci][row][x] in LDS; then per wave M-tiles of 16 output pixels x
//                            one N-tile of 16 output channels on v_mfma_f32_16x16x4_f32, K = (ci, ky, kx) in steps of 4.
//   bitconv2_forward_kernel<true>  the same with a first layer of `stack` input channels, each a frame named by index [n, stack]:
//                            the frames of an item pass through `words` one after the other and every lane carries the running
//                            sums of its pixel's channels in a1 itself (unrounded fp32, so the chain is f110_bitconv_forward_stack's);
//                            the last frame applies `on`, bias and relu.  No LDS beyond the one-frame kernel's, the same bands.
// The two are one body: template <bool STACK> picks the argument struct and the staging / first-layer block, everything else is
// written once.  A template is safe where an inline function shared by two kernels was not (that changed the one-frame kernel's
// register allocation, 219 -> 288 SGPR spills): each instantiation is compiled as a kernel of its own with the other's block
// absent from its source, so nothing is outlined or merged across them, and both keep the registers and spills of the two
// hand-written kernels they replace (profiles/r28_bitconv_one_body.txt).
// The first layer reaches at most 64 columns (OW1 <= 64): a band is whole rows, there is no tiling in x and no halo.
// LDS: [image rows][BC_LWORDS] words, koff[4 BC2_KSTEPS] (where in a1 the k-th term of a window lies, relative to its first
// element; -1 for the padding of K to a multiple of 4), a1[C1][NR1][XW] fp32 with XW = s2 (OW2 - 1) + k2 the columns conv2 uses.
// The host sizes BR so that all of it stays inside BC2_LDS_BYTES.
// A wave keeps its N-tile's weights in registers (b[ks] = w2[co = 16 nt + (lane & 15)][k = 4 ks + (lane >> 4)]) across items;
// with 3 N-tiles two waves own two each and load them per item.  The waves of one N-tile share the band's M-tiles in
// contiguous runs, six accumulators at a time -- independent accumulators are different output tiles, never a split of K.
// Numerics (the contract of include/f110_hip.h): the MFMA is a k-ordered fmaf chain through C, so acc = fma(w2[co][k], a1[k],
// acc) for k = (ci major, ky, kx minor) from acc = 0; the padding terms are fma(0, 0, acc); out = acc + bias2, relu2.
#pragma once
#include "f110_bitconv.h"
#include "f110_bounds.h" // F110_BOUNDS_ONLY

#include <type_traits>

#pragma clang fp contract(off)

namespace f110 {

typedef float bc2_f32x4 __attribute__((ext_vector_type(4)));

// The band as the tile bitconv_stage and bitconv_mask understand: all columns from word 0, the image rows under conv1 rows
// y1 .. y1 + nr1 - 1.
__device__ inline BitconvTile bitconv2_tile(const Bitconv2Args &a, long long sample, int y1, int nr1)
{
    const f110_bitconv_config &c = a.l1.cfg;
    BitconvTile t;
    t.i = sample;
    t.oy0 = y1; t.ox0 = 0;
    t.r0 = y1 * c.stride;
    t.wbase = 0; t.off = 0;
    t.nrows = (nr1 - 1) * c.stride + c.kernel;
    t.nwords = ((a.XW - 1) * c.stride + c.kernel + 63) >> 6;
    const long long s = a.l1.index ? a.l1.index[sample] : sample;
    t.src = s >= 0 && s < a.l1.n_frames ? s : -1;
    return t;
}

// The first layer for conv1 rows wave, wave + 4, ... of the band, lane = column.  <K, false> (stack = 1, j = 0): f110_bitconv_forward's
// own arithmetic.  <K, true>: the share of frame j of a stack -- every channel's running sum is taken from a1 (0 at the first frame),
// frame j's taps are added ky major, kx minor with w1[c][j], and the sum goes back to a1 -- after the last frame through `on`, bias
// and relu.  A lane reads and writes its own elements of a1 only.
template <int K, bool STACK>
__device__ inline void bitconv2_layer1(const Bitconv2Args &a, const BitconvTile &t, const uint64_t *words, float *a1, int nr1,
                                       const float *__restrict__ w1, const float *__restrict__ b1, int stack, int j, int lane, int wave)
{
    const f110_bitconv_config &c = a.l1.cfg;
    if (lane >= a.XW) return;
    const bool first = !STACK || j == 0, last = !STACK || j == stack - 1;
    for (int r = wave; r < nr1; r += BC_THREADS / 64) {
        const uint64_t m = bitconv_mask<K>(words, t, c.stride, r, lane);
        float bit[K * K];
#pragma unroll
        for (int k = 0; k < K * K; k++) bit[k] = (m >> k) & 1ull ? 1.0f : 0.0f;
        for (int ch = 0; ch < c.channels; ch++) {
            const float *w = w1 + (STACK ? ch * stack + j : ch) * (K * K);      // wave-uniform: scalar loads
            float *at = a1 + (ch * a.NR1 + r) * a.XW + lane;
            float acc = first ? 0.0f : *at;
#pragma unroll
            for (int k = 0; k < K * K; k++) acc = __builtin_fmaf(w[k], bit[k], acc);
            if (last) {
                float v = acc * c.on;
                v = v + (b1 ? b1[ch] : 0.0f);
                if (c.relu) v = v < 0.0f ? 0.0f : v;
                acc = v;
            }
            *at = acc;
        }
    }
}

// 16 Q steps of K for BC2_ACCS M-tiles against one N-tile: acc[j] = mfma(a1 at pixel fm[j] + koff[k], b[ks], acc[j]), ks ascending.
// A padding term (koff < 0; b[ks] is 0 there) multiplies 0 by 0.
template <int Q>
__device__ inline void bitconv2_mma(const float *a1, const int *koff, const float (&b)[BC2_KSTEPS], const int (&fm)[BC2_ACCS],
                                    bc2_f32x4 (&acc)[BC2_ACCS], int quad, int a1_len)
{
#pragma unroll
    for (int ks = 0; ks < 16 * Q; ks++) {
        const int ko = koff[4 * ks + quad];
#pragma unroll
        for (int j = 0; j < BC2_ACCS; j++) {
            int at = fm[j] + max(ko, 0);
            F110_BOUNDS_ONLY(if (at < 0 || at >= a1_len) at = 0;)
            const float av = ko >= 0 ? a1[at] : 0.0f;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[ks], acc[j], 0, 0, 0);
        }
    }
}

// What the two launches hand the kernel: the one-frame arguments themselves, or those inside the stacked ones.
__device__ inline const Bitconv2Args &bitconv2_args(const Bitconv2Args &a) { return a; }
__device__ inline const Bitconv2Args &bitconv2_args(const Bitconv2StackArgs &s) { return s.a; }

// grid: min(items, BC2_MAX_GRID); dynamic LDS of a.a1_off + 4 C1 NR1 XW bytes.  w2 [C2, C1, k2, k2], b1 / b2 or NULL, out [n, C2,
// OH2, OW2].  <false>: w1 [C1, K, K], the frame of a sample by a.l1.index.  <true>: w1 [C1, stack, K, K], index [n, stack]; per item
// the frames j = 0 .. stack - 1 are staged into `words` one after the other, with a barrier between a frame's mask reads and the
// next frame's staging.
template <bool STACK>
static __global__ __launch_bounds__(BC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void bitconv2_forward_kernel(
    typename std::conditional<STACK, Bitconv2StackArgs, Bitconv2Args>::type s, const float *__restrict__ w1, const float *__restrict__ b1,
    const float *__restrict__ w2, const float *__restrict__ b2, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bc2_lds[];
    const Bitconv2Args &a = bitconv2_args(s);
    uint64_t *words = reinterpret_cast<uint64_t *>(bc2_lds);
    int *koff = reinterpret_cast<int *>(bc2_lds + a.koff_off);
    float *a1 = reinterpret_cast<float *>(bc2_lds + a.a1_off);
    const f110_bitconv_config &c = a.l1.cfg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int kk2 = a.k2 * a.k2;
    for (int k = tid; k < 4 * BC2_KSTEPS; k += BC_THREADS) {
        const int ci = k / kk2, rem = k - ci * kk2, ky = rem / a.k2, kx = rem - ky * a.k2;
        koff[k] = k < a.ktot ? (ci * a.NR1 + ky) * a.XW + kx : -1;
    }
    // the wave's share of the output tiles: N-tiles nt0, nt0 + nwn, ...; of the M-tiles the mg-th of mw contiguous runs
    const int NT = (a.C2 + 15) >> 4;
    const int nwn = NT >= 4 ? 4 : NT >= 2 ? 2 : 1, mw = 4 / nwn;
    const int nt0 = wave % nwn, mg = wave / nwn;
    float b[BC2_KSTEPS];
    int held = -1;                  // the N-tile whose weights b[] holds
    const size_t plane2 = (size_t)a.OH2 * (size_t)a.OW2;
    const int a1_len = c.channels * a.NR1 * a.XW;

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long sample = item / a.bands;
        const int band = (int)(item - sample * a.bands);
        const int oy0 = band * a.BR, nyb = min(a.BR, a.OH2 - oy0);
        const int nr1 = (nyb - 1) * a.s2 + a.k2;
        BitconvTile t = bitconv2_tile(a, sample, oy0 * a.s2, nr1);
        // (the item's first words are staged while other waves may still multiply the previous item: they read a1 and koff only, and
        // a1 is written after the barrier behind the staging)
        if constexpr (STACK) {
            for (int j = 0; j < s.stack; j++) {
                const long long src = s.index[(size_t)sample * (size_t)s.stack + (size_t)j];
                t.src = src >= 0 && src < a.l1.n_frames ? src : -1;
                bitconv_stage<false>(a.l1, t, words, tid);      // (at j > 0 every wave has left frame j - 1's masks behind the barrier below)
                __syncthreads();
#define BC2_L1S(K) bitconv2_layer1<K, true>(a, t, words, a1, nr1, w1, b1, s.stack, j, lane, wave)
                BITCONV_BY_KERNEL(c.kernel, BC2_L1S)
#undef BC2_L1S
                __syncthreads();
            }
        } else {
            if (a.u8) bitconv_stage<true>(a.l1, t, words, tid);
            else bitconv_stage<false>(a.l1, t, words, tid);
            __syncthreads();
#define BC2_L1(K) bitconv2_layer1<K, false>(a, t, words, a1, nr1, w1, b1, 1, 0, lane, wave)
            BITCONV_BY_KERNEL(c.kernel, BC2_L1)
#undef BC2_L1
            __syncthreads();
        }

        const int mband = nyb * a.OW2, MT = (mband + 15) >> 4;
        const int per = (MT + mw - 1) / mw, mt_end = min(MT, (mg + 1) * per);
        for (int nt = nt0; nt < NT; nt += nwn) {
            const int co = nt * 16 + col;
            if (nt != held) {
#pragma unroll
                for (int ks = 0; ks < BC2_KSTEPS; ks++) {
                    const int k = 4 * ks + quad;
                    b[ks] = ks < a.ksteps && k < a.ktot && co < a.C2 ? w2[(size_t)co * (size_t)a.ktot + (size_t)k] : 0.0f;
                }
                held = nt;
            }
            const float bias = b2 && co < a.C2 ? b2[co] : 0.0f;
            for (int mt0 = mg * per; mt0 < mt_end; mt0 += BC2_ACCS) {
                const int nj = min(BC2_ACCS, mt_end - mt0);
                int fm[BC2_ACCS];
                bc2_f32x4 acc[BC2_ACCS];
#pragma unroll
                for (int j = 0; j < BC2_ACCS; j++) {
                    const int m = (mt0 + j) * 16 + col, mm = m < mband ? m : 0;       // (a pixel beyond the band repeats pixel 0; it is not written)
                    const int oyl = mm / a.OW2, ox = mm - oyl * a.OW2;
                    fm[j] = a.s2 * (oyl * a.XW + ox);
                    acc[j] = bc2_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
#define BC2_MMA(Q) bitconv2_mma<Q>(a1, koff, b, fm, acc, quad, a1_len)
                switch ((a.ksteps + 15) >> 4) { case 1: BC2_MMA(1); break; case 2: BC2_MMA(2); break; case 3: BC2_MMA(3); break; default: BC2_MMA(4); break; }
#undef BC2_MMA
                // lane: channel co, pixels m0 .. m0 + 3 of the band, which are neighbours in memory
                if (co < a.C2) {
                    float *o = out + ((size_t)sample * (size_t)a.C2 + (size_t)co) * plane2 + (size_t)oy0 * (size_t)a.OW2;
#pragma unroll
                    for (int j = 0; j < BC2_ACCS; j++) {
                        if (j < nj) {
                            const int m0 = (mt0 + j) * 16 + quad * 4;
                            float v[4];
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                v[q] = acc[j][q] + bias;
                                if (a.relu2) v[q] = v[q] < 0.0f ? 0.0f : v[q];
                            }
                            if (m0 + 4 <= mband && ((uintptr_t)(o + m0) & 15) == 0) {
                                *reinterpret_cast<float4 *>(o + m0) = make_float4(v[0], v[1], v[2], v[3]);
                            } else {
#pragma unroll
                                for (int q = 0; q < 4; q++)
                                    if (m0 + q < mband) o[m0 + q] = v[q];
                            }
                        }
                    }
                }
            }
        }
    }
}

} // namespace f110
