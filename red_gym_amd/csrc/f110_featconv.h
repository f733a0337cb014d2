// f110_featconv.h -- a dense convolution of fp32 feature maps, forward and backward: conv2 = nn.Conv2d(16, 32, 4, 2) and conv3 =
// nn.Conv2d(32, 32, 3, 1) of the reference's Actor and Critic (src/SAL.py:398-399, 430-431) with their ReLU, under the numerics
// contract of the stem's second layer (f110_bitconv2.h; include/f110_hip.h): an implicit GEMM over LDS-resident planes on
// v_mfma_f32_16x16x4_f32, K fed through the accumulator, which on gfx950 is bit for bit a k-ordered fmaf chain.
//   featconv_gemm_kernel<false>  forward.  A workgroup walks work items (sample, band of BR output rows), item = blockIdx.x,
//                                + gridDim.x, ...  Per item the band's input rows of every channel go to LDS, planes[Ci][NR][XW];
//                                M = the band's output pixels, N = co, K = (ci, ky, kx); out = acc + bias, relu.
//   featconv_gemm_kernel<true>   grad_x: the same GEMM on g = grad_out (masked by out > 0 under relu) staged zero-padded by
//                                k - 1 and zero-dilated by the stride, planes[Co][BR + k - 1][W + k - 1], with a koff table that
//                                walks ky, kx downward: M = the band's input pixels, N = ci, K = (co, ky, kx).  A term without an
//                                output pixel is fma(w, 0, acc), which leaves acc (never -0) as it is.
//   featconv_gradw_kernel        stage 1 of grad_weight / grad_bias: P[n][co][(ci, ky, kx)] with M = co, N = (ci, ky, kx) and
//                                K = the sample's output pixels, oy major, ox minor.  A workgroup owns a sample (blockIdx.x,
//                                + gridDim.x, ...) and FCW_TILES N-tiles (blockIdx.y), restages g and x band by band and keeps its
//                                accumulators across the sample's bands; a band's pixels are padded to a multiple of 4 with
//                                fma(0, 0, acc).  The bias partial is the chain acc = acc + g over the same pixels: one wave, lane =
//                                co, walks gs[co][p] pixel by pixel (a stride of wGP floats between lanes: LDS bank conflicts) while
//                                the other waves wait at the band's barrier -- in the contract's order, and not tuned.
//   featconv_reduce_kernel       stage 2: grad = ((P[0] + P[1]) + P[2]) + ..., samples ascending, one thread per element.
// K of the two GEMMs over planes goes in chunks of FC_CHUNK steps of 4 whose weights a lane loads into registers
// (b[j] = w[n = 16 nt + (lane & 15)][k = 4 (FC_CHUNK c + j) + (lane >> 4)]); K is padded to a whole chunk with terms fma(0, 0, acc).
// koff[k]: where in the planes the k-th term of a window lies relative to the window's first element, -1 for the padding, whose
// operand is read from FC_ZERO_BYTES of zeros that lie in front of the planes: every LDS read is unconditional (a select on
// the address, no branch), so the reads of a chunk run ahead of its multiplies.
// (The stem's bitconv2_mma holds a whole N-tile's weights, at most 64 steps, in registers; K reaches 128 steps here, so the
// multiply is restated per chunk with the same operand layout and the same koff idea.)
// A wave takes jobs (N-tile, run of FC_ACCS M-tiles) wave, wave + 4, ...: the independent accumulators are different output
// tiles, never a split of K.  The order of every sum depends on the shape and n alone, never on the grid, the band or timing.
// The limits (f110_featconv_validate: k, stride 1..4, Ci <= 32, Co <= 64, Ci k^2 <= 512, Co k^2 <= 512, W <= 64) keep a band of
// one output row inside FC_LDS_BYTES in all three kernels; the host sizes bands of whole rows to that budget (featconv_geometry).
// Workspace: P is n Co (Ci k^2 + 1) floats -- 2.4 MB for conv3 at the update's batch of 64, 151 MB at 4 096 rows.
#pragma once
#include "f110_bounds.h" // F110_BOUNDS_ONLY
#include "f110_featconv_plan.h" // limits, FeatconvGemm, FeatconvArgs; the host's checks and launch plans

#pragma clang fp contract(off)

namespace f110 {

typedef float fc_f32x4 __attribute__((ext_vector_type(4)));

// FC_CHUNK steps of K for FC_ACCS M-tiles against one N-tile: acc[j] = mfma(planes at fm[j] + koff[k], b[i], acc[j]), k ascending.
// A padding term (koff < 0; b is 0 there) multiplies the 0 at planes[-1] by 0.
__device__ inline void featconv_mma(const float *planes, const int *koff, const float (&b)[FC_CHUNK], const int (&fm)[FC_ACCS],
                                    fc_f32x4 (&acc)[FC_ACCS], int quad, int planes_len)
{
    // all of the chunk's operands first (its koff entries, then FC_CHUNK x FC_ACCS elements of the planes), then its multiplies: two
    // LDS latencies per chunk instead of two per step
    int ko[FC_CHUNK];
    float av[FC_CHUNK][FC_ACCS];
#pragma unroll
    for (int i = 0; i < FC_CHUNK; i++) ko[i] = koff[4 * i + quad];
#pragma unroll
    for (int i = 0; i < FC_CHUNK; i++) {
#pragma unroll
        for (int j = 0; j < FC_ACCS; j++) {
            int at = ko[i] >= 0 ? fm[j] + ko[i] : -1;
            F110_BOUNDS_ONLY(if (at < -1 || at >= planes_len) at = -1;)
            av[i][j] = planes[at];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < FC_CHUNK; i++) {
#pragma unroll
        for (int j = 0; j < FC_ACCS; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][j], b[i], acc[j], 0, 0, 0);
    }
}

// Element `to` of each of C planes in LDS (dst_stride apart) from element `from` of each of C planes in memory (src_stride apart),
// FC_STAGE planes at a time; with `mask` (the forward's out under relu) an element is kept where mask > 0 and 0 elsewhere.
__device__ inline void featconv_stage(float *dst, int dst_stride, const float *__restrict__ src, const float *__restrict__ mask, size_t src_stride,
                                      int C, int to, size_t from)
{
    for (int c0 = 0; c0 < C; c0 += FC_STAGE) {
        float v[FC_STAGE], m[FC_STAGE];
#pragma unroll
        for (int u = 0; u < FC_STAGE; u++) {
            const size_t at = (size_t)min(c0 + u, C - 1) * src_stride + from;
            v[u] = src[at];
            m[u] = mask ? mask[at] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < FC_STAGE; u++)
            if (c0 + u < C) dst[(c0 + u) * dst_stride + to] = m[u] > 0.0f ? v[u] : 0.0f;
    }
}

// the weight of output channel nidx at term k of the GEMM's K: forward w[co = nidx][k]; grad_x w[co][ci = nidx][ky][kx], k = (co, ky, kx)
template <bool BWD>
__device__ inline float featconv_weight(const FeatconvArgs &a, const float *__restrict__ w, int nidx, int k)
{
    const FeatconvGemm &g = a.g;
    if (k >= g.ktot || nidx >= g.N) return 0.0f;
    if (!BWD) return w[(size_t)nidx * (size_t)g.ktot + (size_t)k];
    const int kk = a.k * a.k, co = k / kk, r = k - co * kk;
    return w[((size_t)co * (size_t)a.Ci + (size_t)nidx) * (size_t)kk + (size_t)r];
}

// grid: min(items, FC_MAX_GRID); dynamic LDS of planes_off + 4 C NR XW bytes
template <bool BWD>
static __global__ __launch_bounds__(FC_THREADS) void featconv_gemm_kernel(FeatconvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    int *koff = reinterpret_cast<int *>(fc_lds);
    const FeatconvGemm &g = a.g;
    float *planes = reinterpret_cast<float *>(fc_lds + g.planes_off);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int kk = a.k * a.k;
    for (int k = tid; k < g.chunks * 4 * FC_CHUNK; k += FC_THREADS) {
        const int c = k / kk, rem = k - c * kk, ky = rem / a.k, kx = rem - ky * a.k;
        koff[k] = k >= g.ktot ? -1 : BWD ? (c * g.NR + (a.k - 1 - ky)) * g.XW + (a.k - 1 - kx) : (c * g.NR + ky) * g.XW + kx;
    }
    if (tid < FC_ZERO_BYTES / 4) planes[-1 - tid] = 0.0f;
    const int NT = (g.N + 15) >> 4;
    const size_t plane_out = (size_t)g.PH * (size_t)g.PW, plane_o = (size_t)a.OH * (size_t)a.OW;
    const int planes_len = g.C * g.NR * g.XW;

    for (long long item = blockIdx.x; item < g.items; item += gridDim.x) {
        const long long sample = item / g.bands;
        const int band = (int)(item - sample * g.bands);
        const int y0 = band * g.BR, nyb = min(g.BR, g.PH - y0);
        // the band's planes
        if (!BWD) {
            const int nr = (nyb - 1) * a.s + a.k, per = nr * g.XW;
            const float *xs = a.x + (size_t)sample * (size_t)a.Ci * (size_t)a.H * (size_t)a.W + (size_t)(y0 * a.s) * (size_t)a.W;
            for (int e = tid; e < per; e += FC_THREADS) {
                const int r = e / g.XW, xcol = e - r * g.XW;
                featconv_stage(planes, g.NR * g.XW, xs, nullptr, (size_t)a.H * (size_t)a.W, g.C, e, (size_t)(r * a.W + xcol));
            }
        } else {
            // row r of the band is row y0 + r of g padded by k - 1 and dilated by s: output row (y0 + r - (k - 1)) / s where that exists
            const int nr = nyb + a.k - 1, per = nr * g.XW;
            const size_t base = (size_t)sample * (size_t)a.Co * plane_o;
            for (int e = tid; e < per; e += FC_THREADS) {
                const int r = e / g.XW, xcol = e - r * g.XW;
                const int py = y0 + r - (a.k - 1), px = xcol - (a.k - 1);
                const int oy = py / a.s, ox = px / a.s;
                const bool live = py >= 0 && px >= 0 && oy * a.s == py && ox * a.s == px && oy < a.OH && ox < a.OW;
                if (live) {
                    featconv_stage(planes, g.NR * g.XW, a.grad_out + base, a.relu ? a.out + base : nullptr, plane_o, g.C, e, (size_t)(oy * a.OW + ox));
                } else {
                    for (int c = 0; c < g.C; c++) planes[c * g.NR * g.XW + e] = 0.0f;
                }
            }
        }
        __syncthreads();

        const int mband = nyb * g.PW, MT = (mband + 15) >> 4, runs = (MT + FC_ACCS - 1) / FC_ACCS;
        for (int job = wave; job < NT * runs; job += FC_THREADS / 64) {
            const int nt = job / runs, mt0 = (job - nt * runs) * FC_ACCS;
            const int nj = min(FC_ACCS, MT - mt0);
            const int nidx = nt * 16 + col;
            int fm[FC_ACCS];
            fc_f32x4 acc[FC_ACCS];
#pragma unroll
            for (int j = 0; j < FC_ACCS; j++) {
                const int m = (mt0 + j) * 16 + col, mm = m < mband ? m : 0;           // (a pixel beyond the band repeats pixel 0; it is not written)
                const int yl = mm / g.PW, xo = mm - yl * g.PW;
                fm[j] = g.ms * (yl * g.XW + xo);
                acc[j] = fc_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            float b[FC_CHUNK], bn[FC_CHUNK];
#pragma unroll
            for (int i = 0; i < FC_CHUNK; i++) bn[i] = featconv_weight<BWD>(a, a.w, nidx, 4 * i + quad);
            for (int c = 0; c < g.chunks; c++) {
#pragma unroll
                for (int i = 0; i < FC_CHUNK; i++) b[i] = bn[i];
                if (c + 1 < g.chunks) {
#pragma unroll
                    for (int i = 0; i < FC_CHUNK; i++) bn[i] = featconv_weight<BWD>(a, a.w, nidx, 4 * ((c + 1) * FC_CHUNK + i) + quad);
                }
                featconv_mma(planes, koff + c * 4 * FC_CHUNK, b, fm, acc, quad, planes_len);
            }
            // lane: channel nidx, pixels m0 .. m0 + 3 of the band, which are neighbours in memory
            if (nidx < g.N) {
                const float bias = !BWD && a.bias ? a.bias[nidx] : 0.0f;
                float *o = a.dst + ((size_t)sample * (size_t)g.N + (size_t)nidx) * plane_out + (size_t)y0 * (size_t)g.PW;
#pragma unroll
                for (int j = 0; j < FC_ACCS; j++) {
                    if (j < nj) {
                        const int m0 = (mt0 + j) * 16 + quad * 4;
                        float v[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            v[q] = acc[j][q];
                            if (!BWD) {
                                v[q] = v[q] + bias;
                                if (a.relu) v[q] = v[q] < 0.0f ? 0.0f : v[q];
                            }
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
        __syncthreads();            // (the next item's planes replace these)
    }
}

// grid: (min(n, FC_MAX_GRID), ceil(wNT / FCW_TILES)); dynamic LDS of 4 (xs_at + Ci wNR wXW) bytes: zeros, gs[Co][wGP], xs[Ci][wNR][wXW].
// Wave w of workgroup y owns N-tiles FCW_TILES y + 2 w and + 1 against all MT M-tiles.
template <int MT>
static __global__ __launch_bounds__(FC_THREADS) void featconv_gradw_kernel(FeatconvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    float *lds = reinterpret_cast<float *>(fc_lds);                 // lds[0] is 0: what a term beyond the band, Co or Ci k k reads
    float *gs = lds + FC_ZERO_BYTES / 4, *xs = lds + a.xs_at;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int kk = a.k * a.k;
    const size_t plane_o = (size_t)a.OH * (size_t)a.OW;
    const int xs_len = a.Ci * a.wNR * a.wXW;
    // the lane's columns of B: where in xs the window term n = (ci, ky, kx) of output pixel 0 lies, -1 beyond Ci k k
    int noff[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int nidx = ((int)blockIdx.y * FCW_TILES + 2 * wave + t) * 16 + col;
        const int ci = nidx / kk, rem = nidx - ci * kk, ky = rem / a.k, kx = rem - ky * a.k;
        noff[t] = nidx < a.wktot ? (ci * a.wNR + ky) * a.wXW + kx : -1;
    }
    if (tid < FC_ZERO_BYTES / 4) lds[tid] = 0.0f;
    const int step_y = 4 / a.OW, step_x = 4 - step_y * a.OW;         // four pixels on
    const bool bias_wave = blockIdx.y == 0 && wave == FC_THREADS / 64 - 1 && lane < a.Co;
    const size_t prow = (size_t)a.Co * (size_t)(a.wktot + 1);

    for (long long sample = blockIdx.x; sample < a.n; sample += gridDim.x) {
        fc_f32x4 acc[MT][2];
#pragma unroll
        for (int m = 0; m < MT; m++) { acc[m][0] = fc_f32x4{0.0f, 0.0f, 0.0f, 0.0f}; acc[m][1] = fc_f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
        float bsum = 0.0f;
        for (int band = 0; band < a.wbands; band++) {
            const int oy0 = band * a.wBR, nyb = min(a.wBR, a.OH - oy0);
            const int npix = nyb * a.OW, nr = (nyb - 1) * a.s + a.k, per = nr * a.wXW;
            const size_t gbase = (size_t)sample * (size_t)a.Co * plane_o + (size_t)oy0 * (size_t)a.OW;
            for (int p = tid; p < npix; p += FC_THREADS)
                featconv_stage(gs, a.wGP, a.grad_out + gbase, a.relu ? a.out + gbase : nullptr, plane_o, a.Co, p, (size_t)p);
            const float *xg = a.x + (size_t)sample * (size_t)a.Ci * (size_t)a.H * (size_t)a.W + (size_t)(oy0 * a.s) * (size_t)a.W;
            for (int e = tid; e < per; e += FC_THREADS) {
                const int r = e / a.wXW, xcol = e - r * a.wXW;
                featconv_stage(xs, a.wNR * a.wXW, xg, nullptr, (size_t)a.H * (size_t)a.W, a.Ci, e, (size_t)(r * a.W + xcol));
            }
            __syncthreads();
            // K: the band's pixels in steps of 4, pixel 4 step + quad; beyond the band both operands are 0
            int oyl = quad / a.OW, ox = quad - oyl * a.OW;
            // the operands of pixel p (the 0 at lds[0] beyond the band, Co or Ci k k); the next step's are read before this step's multiplies
            auto fetch = [&](int p, int oyl, int ox, float (&av)[MT], float (&bv)[2]) {
                const bool live = p < npix;
                const int poff = a.s * (oyl * a.wXW + ox);
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    int at = live && noff[t] >= 0 ? a.xs_at + noff[t] + poff : 0;
                    F110_BOUNDS_ONLY(if (at < 0 || at >= a.xs_at + xs_len) at = 0;)
                    bv[t] = lds[at];
                }
#pragma unroll
                for (int m = 0; m < MT; m++) {
                    const int co = m * 16 + col;
                    av[m] = lds[live && co < a.Co ? FC_ZERO_BYTES / 4 + co * a.wGP + p : 0];
                }
            };
            float av[MT], bv[2];
            fetch(quad, oyl, ox, av, bv);
            for (int p = quad; p < ((npix + 3) & ~3); p += 4) {
                ox += step_x; oyl += step_y;
                if (ox >= a.OW) { ox -= a.OW; oyl++; }
                float nav[MT], nbv[2];
                fetch(p + 4, oyl, ox, nav, nbv);
#pragma unroll
                for (int m = 0; m < MT; m++) {
                    acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[0], acc[m][0], 0, 0, 0);
                    acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[1], acc[m][1], 0, 0, 0);
                }
#pragma unroll
                for (int m = 0; m < MT; m++) av[m] = nav[m];
                bv[0] = nbv[0]; bv[1] = nbv[1];
            }
            if (bias_wave)
                for (int p = 0; p < npix; p++) bsum = bsum + gs[lane * a.wGP + p];
            __syncthreads();        // (the next band replaces gs and xs)
        }
        // lane: rows co = 16 m + 4 quad + q of P, column n = (tile, lane & 15)
        float *P = a.P + (size_t)sample * prow;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int nidx = ((int)blockIdx.y * FCW_TILES + 2 * wave + t) * 16 + col;
            if (nidx < a.wktot) {
#pragma unroll
                for (int m = 0; m < MT; m++) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int co = m * 16 + quad * 4 + q;
                        if (co < a.Co) P[(size_t)co * (size_t)a.wktot + (size_t)nidx] = acc[m][t][q];
                    }
                }
            }
        }
        if (bias_wave) P[(size_t)a.Co * (size_t)a.wktot + (size_t)lane] = bsum;
    }
}

// grid: ceil(Co (ktot + 1) / FC_THREADS).  Element e < Co ktot -> grad_weight[e], the rest -> grad_bias; either may be NULL.
static __global__ __launch_bounds__(FC_THREADS) void featconv_reduce_kernel(const float *__restrict__ P, long long n, int nw, int nb,
                                                                           float *__restrict__ grad_weight, float *__restrict__ grad_bias)
{
    const int e = blockIdx.x * FC_THREADS + threadIdx.x;
    if (e >= nw + nb) return;
    float *dst = e < nw ? (grad_weight ? grad_weight + e : nullptr) : (grad_bias ? grad_bias + (e - nw) : nullptr);
    if (!dst) return;
    const size_t row = (size_t)(nw + nb);
    float acc = P[e];
    long long i = 1;
    for (; i + 16 <= n; i += 16) {      // sixteen loads in flight, added in the same ascending order
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = P[(size_t)(i + u) * row + (size_t)e];
#pragma unroll
        for (int u = 0; u < 16; u++) acc = acc + v[u];
    }
    for (; i < n; i++) acc = acc + P[(size_t)i * row + (size_t)e];
    *dst = acc;
}

} // namespace f110
