// f110_bitconv.h -- the first layer of the reference's policy (src/SAL.py:397, 429: nn.Conv2d(1, C, kernel, stride) on the FILL
// bitmap) computed from bits.  An image with two pixel values needs no multiplications by pixels: a window of kernel x kernel
// taps is one 64-bit mask (tap (ky, kx) = bit ky * kernel + kx) and the layer's output is bias + on * sum of w[taps that are set].
// The frames are read as the replay ring keeps them (f110_replay.h: bit k of word w = pixel 64 w + k) or as uint8 images that are
// thresholded (== 255) while they are staged; no fp32 image and no packed copy ever exists in memory.
//   bitconv_forward_kernel   one workgroup per (image, tile of 4 x 64 outputs): the tile's rows of words go to LDS, a lane
//                            assembles its window's mask from them (a window that straddles a word boundary takes two words
//                            per row, once) and expands it to 0.0 / 1.0; per channel one fma per tap with the weight wave-uniform
//   bitconv_backward_kernel  stage 1 of grad_weight / grad_bias: a workgroup walks tiles g, g + G, ... (G fixed by the shape), a
//                            lane owns one tap, a wave one row of the tile, and sums grad_out * bit in a fixed order
//   bitconv_reduce_kernel<false>  stage 2: the G partials of every element summed in a fixed order, times `on`
//   bitconv_forward_stack_kernel  the layer with `stack` input channels, each a frame named by index [n, stack]: the masks of all
//                            frames of a tile go to LDS, then chunks of BCS_CHUNK channels accumulate over the frames in registers
//   bitconv_index_columns_kernel, bitconv_reduce_kernel<true>  the stacked backward is the one-frame backward per index column: the
//                            index transposed once, and stage 2 written with the [C, stack, K, K] stride
// Forward numerics (the contract of include/f110_hip.h): acc = 0; taps ky major, kx minor: acc = fma(w, bit, acc) with bit 0.0 or
// 1.0 -- w * bit is exact, so this is acc + w for a set tap and acc for a clear one, rounded once per tap; out = (acc * on) + bias.
// Limits, BitconvArgs and the host's checks and launch plans are in f110_bitconv_plan.h (f110_bitconv_abi.hip launches them); it
// includes f110_replay_bits.h for the frame format read here: replay_bits16 (16 pixels -> 16 bits).
#pragma once
#include "f110_bitconv_plan.h"

#pragma clang fp contract(off)

namespace f110 {

struct BitconvTile {                // what a workgroup knows about its tile
    long long i, src;               // sample, and the frame it reads (-1: a frame of zeros)
    int oy0, ox0, r0, wbase, off;   // first output, first image row, first word, and the bit of that word where output ox0 starts
    int nrows, nwords;              // rows and words of the image the tile's windows reach
};

__device__ inline BitconvTile bitconv_tile(const BitconvArgs &a, long long tile)
{
    const f110_bitconv_config &c = a.cfg;
    BitconvTile t;
    const long long per = (long long)a.tiles_x * a.tiles_y;
    t.i = tile / per;
    const int rem = (int)(tile - t.i * per), ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
    t.oy0 = ty * BC_TY; t.ox0 = tx * BC_TX;
    const int ny = min(BC_TY, a.OH - t.oy0), nx = min(BC_TX, a.OW - t.ox0);
    t.r0 = t.oy0 * c.stride;
    const int col0 = t.ox0 * c.stride;
    t.wbase = col0 >> 6; t.off = col0 & 63;
    t.nrows = (ny - 1) * c.stride + c.kernel;
    t.nwords = (t.off + (nx - 1) * c.stride + c.kernel + 63) >> 6;
    const long long s = a.index ? a.index[t.i] : t.i;
    t.src = s >= 0 && s < a.n_frames ? s : -1;
    return t;
}

// The tile's words -> lds[r * BC_LWORDS + j] = word wbase + j of image row r0 + r (0 beyond the row's words).  From uint8 a word
// is 64 pixels thresholded in registers (four 16-byte loads where the row has them, byte by byte at the row's end).
template <bool U8>
__device__ inline void bitconv_stage(const BitconvArgs &a, const BitconvTile &t, uint64_t *lds, int tid)
{
    const int rows = a.cfg.rows, cols = a.cfg.cols;
    const int units = t.nrows * t.nwords;
    for (int u = tid; u < units; u += BC_THREADS) {
        const int r = u / t.nwords, j = u - r * t.nwords;
        const int gr = t.r0 + r, gw = t.wbase + j;
        uint64_t v = 0;
        if (t.src >= 0 && gr < rows && gw < a.W) {
            if (!U8) v = a.frames[((size_t)t.src * (size_t)rows + (size_t)gr) * (size_t)a.W + (size_t)gw];
            else {
                const uint8_t *p = a.images + ((size_t)t.src * (size_t)rows + (size_t)gr) * (size_t)cols;
                for (int q = 0; q < 4; q++) {
                    const int c0 = 64 * gw + 16 * q;
                    unsigned bits = 0;
                    if (c0 + 16 <= cols) {
                        uint4 x;
                        __builtin_memcpy(&x, p + c0, 16);
                        bits = replay_bits16(x);
                    } else {
                        for (int k = 0; k < 16 && c0 + k < cols; k++) bits |= (unsigned)(p[c0 + k] == 255) << k;
                    }
                    v |= (uint64_t)bits << (16 * q);
                }
            }
        }
        lds[r * BC_LWORDS + j] = v;
    }
}

// The mask of the window of output (ty, tx) of the tile: bit ky * K + kx = pixel (row + ky, col + kx).  Two words per row only
// where the window crosses a word boundary.
template <int K>
__device__ inline uint64_t bitconv_mask(const uint64_t *lds, const BitconvTile &t, int stride, int ty, int tx)
{
    const int pos = t.off + tx * stride, lw = pos >> 6, sh = pos & 63;
    const uint64_t keep = K == 8 ? 0xffull : ((1ull << K) - 1ull);
    uint64_t m = 0;
#pragma unroll
    for (int ky = 0; ky < K; ky++) {
        const uint64_t *row = lds + (ty * stride + ky) * BC_LWORDS + lw;
        uint64_t v = row[0] >> sh;
        if (sh + K > 64) v |= row[1] << (64 - sh);
        m |= (v & keep) << (ky * K);
    }
    return m;
}

// grid: (images of this launch) * tiles_y * tiles_x; weight [C, K, K], bias [C] or NULL, out [n, C, OH, OW]
template <int K, bool U8>
static __global__ __launch_bounds__(BC_THREADS) void bitconv_forward_kernel(BitconvArgs a, const float *__restrict__ weight, const float *__restrict__ bias,
                                                                           float *__restrict__ out)
{
    __shared__ uint64_t lds[BC_LROWS * BC_LWORDS];
    const f110_bitconv_config &c = a.cfg;
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    const BitconvTile t = bitconv_tile(a, a.first * ((long long)a.tiles_x * a.tiles_y) + (long long)blockIdx.x);
    bitconv_stage<U8>(a, t, lds, tid);
    __syncthreads();
    const int oy = t.oy0 + ty, ox = t.ox0 + tx;
    if (oy >= a.OH || ox >= a.OW) return;
    const uint64_t m = bitconv_mask<K>(lds, t, c.stride, ty, tx);
    float bit[K * K];
#pragma unroll
    for (int k = 0; k < K * K; k++) bit[k] = (m >> k) & 1ull ? 1.0f : 0.0f;
    const size_t plane = (size_t)a.OH * (size_t)a.OW;
    float *o = out + (size_t)t.i * (size_t)c.channels * plane + (size_t)oy * (size_t)a.OW + (size_t)ox;
    for (int ch = 0; ch < c.channels; ch++) {
        const float *w = weight + ch * (K * K);        // wave-uniform, and `out` is no alias: scalar loads
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < K * K; k++) acc = __builtin_fmaf(w[k], bit[k], acc);
        float v = acc * c.on;
        v = v + (bias ? bias[ch] : 0.0f);
        if (c.relu) v = v < 0.0f ? 0.0f : v;
        o[(size_t)ch * plane] = v;
    }
}

// grid: (G, ceil(C / BC_CHUNK)).  Workgroup g sums tiles g, g + G, ... of all n samples for BC_CHUNK channels: lane = tap, wave =
// row of the tile; grad_out of the tile goes through LDS, where a wave reads four pixels of a channel at once (the same address
// in every lane).  The order of every sum is fixed by the shape, so two calls give the same bits.
template <int K>
static __global__ __launch_bounds__(BC_THREADS) void bitconv_backward_kernel(BitconvArgs a)
{
    __shared__ uint64_t lds[BC_LROWS * BC_LWORDS];
    __shared__ uint64_t masks[BC_THREADS];
    __shared__ float4 gl4[BC_CHUNK * BC_THREADS / 4];          // [BC_CHUNK][BC_THREADS] grad_out, later [4][BC_CHUNK][64] partials
    __shared__ float bred[4 * BC_CHUNK];
    float *gl = reinterpret_cast<float *>(gl4);
    const f110_bitconv_config &c = a.cfg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = c.channels, c0 = blockIdx.y * BC_CHUNK;
    const size_t plane = (size_t)a.OH * (size_t)a.OW;
    const long long tiles = a.n * (long long)a.tiles_x * a.tiles_y;
    float acc[BC_CHUNK], bsum[BC_CHUNK];
#pragma unroll
    for (int j = 0; j < BC_CHUNK; j++) { acc[j] = 0.0f; bsum[j] = 0.0f; }
    for (long long tile = blockIdx.x; tile < tiles; tile += a.G) {
        const BitconvTile t = bitconv_tile(a, tile);
        bitconv_stage<false>(a, t, lds, tid);
        __syncthreads();
        {   // lane = pixel: its window's mask and its grad_out of the chunk's channels
            const int oy = t.oy0 + wave, ox = t.ox0 + lane;
            const bool in = oy < a.OH && ox < a.OW;
            masks[tid] = in ? bitconv_mask<K>(lds, t, c.stride, wave, lane) : 0ull;
            const float *g = a.grad_out + (size_t)t.i * (size_t)C * plane + (size_t)oy * (size_t)a.OW + (size_t)ox;
#pragma unroll
            for (int j = 0; j < BC_CHUNK; j++) {
                const int ch = min(c0 + j, C - 1);             // (a channel beyond C repeats the last one; it is not written)
                const float v = in ? g[(size_t)ch * plane] : 0.0f;
                gl[j * BC_THREADS + tid] = v;
                bsum[j] = bsum[j] + v;
            }
        }
        __syncthreads();
        if (t.oy0 + wave < a.OH) {  // lane = tap over the 64 pixels of the wave's row
            for (int p = 0; p < 64; p += 4) {
                float b[4];
#pragma unroll
                for (int q = 0; q < 4; q++) b[q] = (masks[wave * 64 + p + q] >> lane) & 1ull ? 1.0f : 0.0f;
#pragma unroll
                for (int j = 0; j < BC_CHUNK; j++) {
                    const float4 g = gl4[(j * BC_THREADS + wave * 64 + p) >> 2];
                    acc[j] = __builtin_fmaf(g.x, b[0], acc[j]);
                    acc[j] = __builtin_fmaf(g.y, b[1], acc[j]);
                    acc[j] = __builtin_fmaf(g.z, b[2], acc[j]);
                    acc[j] = __builtin_fmaf(g.w, b[3], acc[j]);
                }
            }
        }
        __syncthreads();
    }
    // the four waves' sums, wave 0 first
#pragma unroll
    for (int j = 0; j < BC_CHUNK; j++) gl[(wave * BC_CHUNK + j) * 64 + lane] = acc[j];
#pragma unroll
    for (int j = 0; j < BC_CHUNK; j++) {
        float v = bsum[j];
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
        if (lane == 0) bred[wave * BC_CHUNK + j] = v;
    }
    __syncthreads();
    float *wsw = a.ws + (size_t)blockIdx.x * (size_t)C * (size_t)(K * K);
    float *wsb = a.ws + (size_t)a.G * (size_t)C * (size_t)(K * K) + (size_t)blockIdx.x * (size_t)C;
    for (int o = tid; o < BC_CHUNK * 64; o += BC_THREADS) {
        const int j = o >> 6, k = o & 63;
        if (c0 + j < C && k < K * K)
            wsw[(size_t)(c0 + j) * (size_t)(K * K) + (size_t)k] =
                ((gl[(0 * BC_CHUNK + j) * 64 + k] + gl[(1 * BC_CHUNK + j) * 64 + k]) + gl[(2 * BC_CHUNK + j) * 64 + k]) + gl[(3 * BC_CHUNK + j) * 64 + k];
    }
    if (tid < BC_CHUNK && c0 + tid < C)
        wsb[c0 + tid] = ((bred[tid] + bred[BC_CHUNK + tid]) + bred[2 * BC_CHUNK + tid]) + bred[3 * BC_CHUNK + tid];
}

// one lane per element of grad_weight (nw = C * kernel^2 of them) and of grad_bias (C): the G partials as four interleaved sums.
// <false>: grad_weight [C, kk] (kk, stack and j are not read).  <true>: the same sums into column j of grad_weight [C, stack, kk];
// the bias (the same for every column: it does not depend on the frames) where the caller passes it.
template <bool STACK>
static __global__ __launch_bounds__(BC_THREADS) void bitconv_reduce_kernel(const float *ws, int G, int nw, int C, float on,
                                                                          float *grad_weight, float *grad_bias, int kk, int stack, int j)
{
    const int o = blockIdx.x * BC_THREADS + threadIdx.x;
    if (o >= nw + C) return;
    const bool is_w = o < nw;
    const float *p = is_w ? ws + o : ws + (size_t)G * (size_t)nw + (size_t)(o - nw);
    const size_t step = is_w ? (size_t)nw : (size_t)C;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int g = 0; g < G; g += 4) {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (g + q < G) s[q] = s[q] + p[(size_t)(g + q) * step];
    }
    const float v = (s[0] + s[1]) + (s[2] + s[3]);
    if (is_w) {
        size_t at = (size_t)o;
        if constexpr (STACK) {
            const int ch = o / kk, k = o - ch * kk;
            at = ((size_t)ch * (size_t)stack + (size_t)j) * (size_t)kk + (size_t)k;
        }
        grad_weight[at] = v * on;
    } else if (grad_bias) grad_bias[o - nw] = v;
}

// ---------------------------------------------------------------- the same layer on a stack of frames
// grid as bitconv_forward_kernel; weight [C, stack, K, K], index [n, stack].  Pass 1: for every frame of the stack the tile is staged
// and each lane keeps its window's mask in LDS (masks[j][tid]: its own entry, so pass 2 needs no barrier).  Pass 2: per chunk of
// BCS_CHUNK channels one accumulator per channel in registers; for the frames in order the mask is expanded once to bit[K * K]
// (constant indices only) and every channel of the chunk adds its K * K taps, the weights wave-uniform.  Per channel that is the
// contract's order -- j major, ky, kx minor -- and with stack = 1 the one-frame kernel's chain of fmas.
template <int K>
static __global__ __launch_bounds__(BC_THREADS) void bitconv_forward_stack_kernel(BitconvStackArgs s, const float *__restrict__ weight,
                                                                                 const float *__restrict__ bias, float *__restrict__ out)
{
    __shared__ uint64_t lds[BC_LROWS * BC_LWORDS];
    __shared__ uint64_t masks[F110_BITCONV_MAX_STACK * BC_THREADS];
    const BitconvArgs &a = s.a;
    const f110_bitconv_config &c = a.cfg;
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    BitconvTile t = bitconv_tile(a, a.first * ((long long)a.tiles_x * a.tiles_y) + (long long)blockIdx.x);
    const int oy = t.oy0 + ty, ox = t.ox0 + tx;
    const bool in = oy < a.OH && ox < a.OW;
    for (int j = 0; j < s.stack; j++) {
        const long long src = s.index[(size_t)t.i * (size_t)s.stack + (size_t)j];
        t.src = src >= 0 && src < a.n_frames ? src : -1;
        bitconv_stage<false>(a, t, lds, tid);
        __syncthreads();
        masks[j * BC_THREADS + tid] = in ? bitconv_mask<K>(lds, t, c.stride, ty, tx) : 0ull;
        __syncthreads();
    }
    if (!in) return;
    const size_t plane = (size_t)a.OH * (size_t)a.OW;
    float *o = out + (size_t)t.i * (size_t)c.channels * plane + (size_t)oy * (size_t)a.OW + (size_t)ox;
    for (int c0 = 0; c0 < c.channels; c0 += BCS_CHUNK) {
        float acc[BCS_CHUNK];
#pragma unroll
        for (int q = 0; q < BCS_CHUNK; q++) acc[q] = 0.0f;
        for (int j = 0; j < s.stack; j++) {
            const uint64_t m = masks[j * BC_THREADS + tid];
            float bit[K * K];
#pragma unroll
            for (int k = 0; k < K * K; k++) bit[k] = (m >> k) & 1ull ? 1.0f : 0.0f;
#pragma unroll
            for (int q = 0; q < BCS_CHUNK; q++) {
                const int ch = min(c0 + q, c.channels - 1);    // (a channel beyond C repeats the last one; it is not written)
                const float *w = weight + ((size_t)ch * (size_t)s.stack + (size_t)j) * (size_t)(K * K);   // wave-uniform: scalar loads
#pragma unroll
                for (int k = 0; k < K * K; k++) acc[q] = __builtin_fmaf(w[k], bit[k], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < BCS_CHUNK; q++) {
            const int ch = c0 + q;
            if (ch < c.channels) {
                float v = acc[q] * c.on;
                v = v + (bias ? bias[ch] : 0.0f);
                if (c.relu) v = v < 0.0f ? 0.0f : v;
                o[(size_t)ch * plane] = v;
            }
        }
    }
}

// one lane per entry: index [n, stack] -> columns [stack, n], so that f110_bitconv_backward's kernels read column j as their index
static __global__ __launch_bounds__(BC_THREADS) void bitconv_index_columns_kernel(const long long *__restrict__ index, long long n, int stack,
                                                                                 long long *__restrict__ columns)
{
    const long long o = (long long)blockIdx.x * BC_THREADS + threadIdx.x;
    if (o >= n * stack) return;
    const long long j = o / n, i = o - j * n;
    columns[o] = index[i * stack + j];
}

} // namespace f110
