// f110_policyhead.h -- the head of the reference's policy (src/SAL.py:410-421: fc_mean and fc_log_std on the features of fc1, clamp,
// exp, rsample, tanh and the squashed-Gaussian log_prob summed over the action), forward in one kernel and a backward without atomics.
//   policyhead_forward_kernel  a workgroup walks tiles of PH_ROWS rows, tile = blockIdx.x, + gridDim.x, ...; a wave owns 16 rows.  The
//                              2A rows of weights lie in LDS as N-tiles of 16: tiles 0 .. T - 1 hold w_mean (T = ceil(A / 16)), tiles
//                              T .. 2T - 1 w_log_std, so that the lane that ends with mean[j] also holds log_std[j]; rows past A are
//                              zeros.  Per 16 columns of K: one 16-byte LDS read per N-tile, four v_mfma_f32_16x16x4_f32 per N-tile
//                              (A operand: h[row = lane & 15][k = 4 s + (lane >> 4)], straight from memory, 64 columns ahead).
//                              Then the tail in fp64 on the lane that holds (row 4 (lane >> 4) + q, j = 16 t + (lane & 15)), and the
//                              row's log_prob as a sum over j ascending, the terms fetched lane by lane.
//   policyhead_gpre_kernel     backward, one lane per (row, j): the tail again from pre and eps, g_pre [n, 2A] fp32 into the workspace
//   policyhead_gradh_kernel    grad_h: lane = column k, PH_GH_ROWS rows per workgroup, the fmaf chain over j
//   policyhead_gradw_kernel    stage 1 of grad_w / grad_b: one wave per (slice of F110_POLICYHEAD_SLICE_ROWS rows, 64 columns of K),
//                              lane = column, 2A chains over the slice's rows in ascending order; the last block row sums g_pre itself
//   policyhead_reduce_kernel   stage 2: the slices of every element summed in ascending order
// LDS of the forward kernel: [32 T][kc] fp32, kc = min(PH_LDS_BYTES / (128 T), K rounded up to 64) columns of K at a time (512 for
// A <= 16, 256 above): one chunk when K <= kc, staged once per workgroup; else every tile stages its chunks in turn.  Within a row the
// 16 columns of a block lie transposed (column 4 s + q at 4 q + s), so that a lane's four steps are one read, and the block's place is
// XORed with 4 (row & 15), which spreads the 16 rows a read touches over all banks.  Columns past K are zeros: fma(0, 0, acc).
// Numerics (the contract of include/f110_hip.h): the MFMA is a k-ordered fmaf chain through C.
#pragma once
#include "f110_policyhead_plan.h" // limits, PolicyheadArgs; the host's checks and launch plans

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#pragma clang fp contract(off)

namespace f110 {

typedef float ph_f32x4 __attribute__((ext_vector_type(4)));

// What the tail makes of one element, in fp64 (forward and backward agree on it by construction).
struct PolicyheadTail {
    double ls, sd, y, om;           // clamped log_std, exp(ls), tanh(x), 1 - y y
    bool inside;                    // -20 <= pre_ls <= 2
};

__device__ inline PolicyheadTail policyhead_tail(float pre_mean, float pre_ls, float eps, bool sampling)
{
    PolicyheadTail t;
    const double pl = (double)pre_ls;
    t.inside = pl >= -20.0 && pl <= 2.0;
    t.ls = pl < -20.0 ? -20.0 : pl > 2.0 ? 2.0 : pl;
    t.sd = exp(t.ls);
    const double x = sampling ? (double)pre_mean + t.sd * (double)eps : (double)pre_mean;
    t.y = tanh(x);
    t.om = 1.0 - t.y * t.y;
    return t;
}

// Rows 16 tile + c of the weights in LDS for columns k0 .. k0 + kc - 1, transposed and swizzled as the header of this file says.
template <int T>
__device__ inline void policyhead_stage(const PolicyheadArgs &a, float *lw, int k0, int tid)
{
    const int blocks = a.kc >> 4;
    for (int it = tid; it < 32 * T * blocks; it += PH_THREADS) {
        const int r = it / blocks, blk = it - r * blocks;
        const int tile = r >> 4, c = r & 15;
        const int j = 16 * (tile < T ? tile : tile - T) + c;
        const float *src = j < a.A ? (tile < T ? a.w_mean : a.w_log_std) + (size_t)j * (size_t)a.K : nullptr;
        const int kb = k0 + 16 * blk;
        float v[16];
        if (src && kb + 16 <= a.K && ((uintptr_t)(src + kb) & 15) == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float4 x = *reinterpret_cast<const float4 *>(src + kb + 4 * i);
                v[4 * i] = x.x; v[4 * i + 1] = x.y; v[4 * i + 2] = x.z; v[4 * i + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) v[i] = src && kb + i < a.K ? src[kb + i] : 0.0f;
        }
        float *dst = lw + (size_t)r * a.kc;
#pragma unroll
        for (int q = 0; q < 4; q++)
            *reinterpret_cast<float4 *>(dst + ((16 * blk + 4 * q) ^ (c << 2))) = make_float4(v[q], v[4 + q], v[8 + q], v[12 + q]);
    }
}

// grid: min(tiles, PH_MAX_GRID); dynamic LDS of 128 T kc bytes
template <int T, bool F64>
static __global__ __launch_bounds__(PH_THREADS) void policyhead_forward_kernel(PolicyheadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ph_lds[];
    float *lw = reinterpret_cast<float *>(ph_lds);
    typedef typename std::conditional<F64, double, float>::type out_t;
    out_t *action = reinterpret_cast<out_t *>(a.action), *log_prob = reinterpret_cast<out_t *>(a.log_prob);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const bool sampling = a.eps != nullptr;
    if (a.chunks == 1) {
        policyhead_stage<T>(a, lw, 0, tid);
        __syncthreads();
    }
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long row0 = tile * PH_ROWS + 16 * wave;
        const bool arow_ok = row0 + col < a.n;
        const float *hp = a.h + (size_t)(arow_ok ? row0 + col : 0) * (size_t)a.K;
        ph_f32x4 acc[2 * T];
#pragma unroll
        for (int t = 0; t < 2 * T; t++) acc[t] = ph_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = 0; c < a.chunks; c++) {
            const int k0 = c * a.kc, len = min(a.kc, a.K - k0), batches = (len + PH_PREFETCH - 1) / PH_PREFETCH;
            if (a.chunks > 1) {
                __syncthreads();                      // (the waves have finished with the chunk before)
                policyhead_stage<T>(a, lw, k0, tid);
                __syncthreads();
            }
            // a lane's A operands of 16 steps: columns k0 + 64 b + 4 s + quad
            float av[16], an[16];
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const int k = k0 + 4 * s + quad;
                av[s] = arow_ok && k < a.K ? hp[k] : 0.0f;
            }
            for (int b = 0; b < batches; b++) {
                if (b + 1 < batches) {
#pragma unroll
                    for (int s = 0; s < 16; s++) {
                        const int k = k0 + PH_PREFETCH * (b + 1) + 4 * s + quad;
                        an[s] = arow_ok && k < a.K ? hp[k] : 0.0f;
                    }
                }
#pragma unroll
                for (int blk = 0; blk < 4; blk++) {
                    const int at = (PH_PREFETCH * b + 16 * blk + 4 * quad) ^ (col << 2);
                    ph_f32x4 w[2 * T];
#pragma unroll
                    for (int t = 0; t < 2 * T; t++) w[t] = *reinterpret_cast<const ph_f32x4 *>(lw + (size_t)(16 * t + col) * a.kc + at);
#pragma unroll
                    for (int s = 0; s < 4; s++) {
#pragma unroll
                        for (int t = 0; t < 2 * T; t++)
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[4 * blk + s], w[t][s], acc[t], 0, 0, 0);
                    }
                }
                if (b + 1 < batches) {
#pragma unroll
                    for (int s = 0; s < 16; s++) av[s] = an[s];
                }
            }
        }

        // the tail: lane = (rows row0 + 4 quad + q, j = 16 t + col)
        double term[T][4];
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int j = 16 * t + col;
            const bool jok = j < a.A;
            const float bm = jok && a.b_mean ? a.b_mean[j] : 0.0f, bl = jok && a.b_log_std ? a.b_log_std[j] : 0.0f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const long long row = row0 + 4 * quad + q;
                const bool ok = jok && row < a.n;
                const float pm = acc[t][q] + bm, pl = acc[T + t][q] + bl;
                term[t][q] = 0.0;
                if (ok) {
                    float *p = a.pre + (size_t)row * (size_t)(2 * a.A);
                    p[j] = pm;
                    p[a.A + j] = pl;
                    const size_t e = (size_t)row * (size_t)a.A + (size_t)j;
                    const float ev = sampling ? a.eps[e] : 0.0f;
                    const PolicyheadTail r = policyhead_tail(pm, pl, ev, sampling);
                    action[e] = (out_t)r.y;
                    if (sampling) {
                        const double ed = (double)ev;
                        term[t][q] = ((-(ed * ed) / 2.0 - r.ls) - PH_HALF_LOG_2PI) - log(r.om + 1e-6);
                    }
                }
            }
        }
        if (sampling) {
            // row (quad, q): its terms lie on the 16 lanes of the quad, j ascending = t major, lane minor
            double lp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < T; t++) {
                for (int c = 0; c < 16 && 16 * t + c < a.A; c++) {
#pragma unroll
                    for (int q = 0; q < 4; q++) lp[q] += __shfl(term[t][q], (lane & 48) | c);
                }
            }
            const long long row = row0 + 4 * quad + col;
            if (col < 4 && row < a.n) log_prob[row] = (out_t)(col == 0 ? lp[0] : col == 1 ? lp[1] : col == 2 ? lp[2] : lp[3]);
        }
    }
}

// grid: ceil(n A / PH_THREADS).  g_pre of (row, j): [row][j] the mean's, [row][A + j] the log_std's
template <bool F64>
static __global__ __launch_bounds__(PH_THREADS) void policyhead_gpre_kernel(PolicyheadArgs a)
{
    typedef typename std::conditional<F64, double, float>::type out_t;
    const long long e = (long long)blockIdx.x * PH_THREADS + threadIdx.x;
    if (e >= a.n * a.A) return;
    const long long row = e / a.A;
    const int j = (int)(e - row * a.A);
    const bool sampling = a.eps != nullptr;
    const float *p = a.pre + (size_t)row * (size_t)(2 * a.A);
    const float ev = sampling ? a.eps[e] : 0.0f;
    const PolicyheadTail r = policyhead_tail(p[j], p[a.A + j], ev, sampling);
    const double gy = (double)reinterpret_cast<const out_t *>(a.grad_action)[e];
    const double glp = a.grad_log_prob ? (double)reinterpret_cast<const out_t *>(a.grad_log_prob)[row] : 0.0;
    const double gx = gy * r.om + glp * (2.0 * r.y * r.om / (r.om + 1e-6));
    const double gl = sampling && r.inside ? gx * r.sd * (double)ev - glp : 0.0;
    const float *gp = a.grad_pre ? a.grad_pre + (size_t)row * (size_t)(2 * a.A) : nullptr;
    float *g = a.gpre + (size_t)row * (size_t)(2 * a.A);
    g[j] = (float)(gp ? gx + (double)gp[j] : gx);
    g[a.A + j] = (float)(gp ? gl + (double)gp[a.A + j] : gl);
}

// grid: (ceil(n / PH_GH_ROWS), ceil(K / PH_THREADS)).  grad_h[b][k]: acc = fmaf(w[j][k], g_pre[b][j], acc), j ascending over 2A
static __global__ __launch_bounds__(PH_THREADS) void policyhead_gradh_kernel(PolicyheadArgs a)
{
    __shared__ float g[PH_GH_ROWS][2 * PH_MAX_A];
    const int tid = threadIdx.x, J = 2 * a.A;
    const long long r0 = (long long)blockIdx.x * PH_GH_ROWS;
    const int nr = (int)min((long long)PH_GH_ROWS, a.n - r0);
    for (int i = tid; i < PH_GH_ROWS * J; i += PH_THREADS) {
        const int r = i / J, j = i - r * J;
        g[r][j] = r < nr ? a.gpre[(size_t)(r0 + r) * (size_t)J + (size_t)j] : 0.0f;
    }
    __syncthreads();
    const int k = blockIdx.y * PH_THREADS + tid;
    if (k >= a.K) return;
    float acc[PH_GH_ROWS];
#pragma unroll
    for (int r = 0; r < PH_GH_ROWS; r++) acc[r] = 0.0f;
    for (int j = 0; j < J; j++) {
        const float w = j < a.A ? a.w_mean[(size_t)j * (size_t)a.K + (size_t)k] : a.w_log_std[(size_t)(j - a.A) * (size_t)a.K + (size_t)k];
#pragma unroll
        for (int r = 0; r < PH_GH_ROWS; r++) acc[r] = __builtin_fmaf(w, g[r][j], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < PH_GH_ROWS; r++)
        if (r < nr) a.grad_h[(size_t)(r0 + r) * (size_t)a.K + (size_t)k] = acc[r];
}

// grid: (slices, ceil(K / 64) + 1), one wave.  partial[s][j][k] = the chain acc = fmaf(g_pre[b][j], h[b][k], acc) over the slice's rows
// b ascending; block row ceil(K / 64): partial[s][j][K] = the sum of g_pre[b][j], b ascending
static __global__ __launch_bounds__(64) void policyhead_gradw_kernel(PolicyheadArgs a)
{
    const int lane = threadIdx.x, J = 2 * a.A, kt = blockIdx.y, ktiles = (a.K + 63) >> 6;
    const long long b0 = (long long)blockIdx.x * PH_SLICE, b1 = min(a.n, b0 + PH_SLICE);
    const float *__restrict__ g = a.gpre;
    float *out = a.partial + (size_t)blockIdx.x * (size_t)J * (size_t)(a.K + 1);
    if (kt == ktiles) {
        if (lane >= J) return;
        float acc = 0.0f;
        for (long long b = b0; b < b1; b++) acc = acc + g[(size_t)b * (size_t)J + (size_t)lane];
        out[(size_t)lane * (size_t)(a.K + 1) + (size_t)a.K] = acc;
        return;
    }
    const int k = kt * 64 + lane;
    const bool kok = k < a.K;
    const float *__restrict__ hp = a.h + (kok ? k : 0);
    float acc[2 * PH_MAX_A];
#pragma unroll
    for (int j = 0; j < 2 * PH_MAX_A; j++) acc[j] = 0.0f;
    for (long long b = b0; b < b1; b += 4) {
        float hv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) hv[u] = kok && b + u < b1 ? hp[(size_t)(b + u) * (size_t)a.K] : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (b + u < b1) {
                const float *gr = g + (size_t)(b + u) * (size_t)J;
#pragma unroll
                for (int j = 0; j < 2 * PH_MAX_A; j++)
                    if (j < J) acc[j] = __builtin_fmaf(gr[j], hv[u], acc[j]);
            }
        }
    }
    if (!kok) return;
#pragma unroll
    for (int j = 0; j < 2 * PH_MAX_A; j++)
        if (j < J) out[(size_t)j * (size_t)(a.K + 1) + (size_t)k] = acc[j];
}

// grid: ceil(2A (K + 1) / PH_THREADS).  The slices of an element added in ascending order; outputs that are NULL are skipped
static __global__ __launch_bounds__(PH_THREADS) void policyhead_reduce_kernel(PolicyheadArgs a)
{
    const int J = 2 * a.A, K1 = a.K + 1;
    const int e = blockIdx.x * PH_THREADS + threadIdx.x;
    if (e >= J * K1) return;
    const int j = e / K1, k = e - j * K1;
    float acc = 0.0f;
    for (int s = 0; s < a.slices; s++) acc = acc + a.partial[(size_t)s * (size_t)J * (size_t)K1 + (size_t)e];
    const bool mean = j < a.A;
    const int jj = mean ? j : j - a.A;
    if (k < a.K) {
        float *gw = mean ? a.grad_w_mean : a.grad_w_log_std;
        if (gw) gw[(size_t)jj * (size_t)a.K + (size_t)k] = acc;
    } else {
        float *gb = mean ? a.grad_b_mean : a.grad_b_log_std;
        if (gb) gb[jj] = acc;
    }
}

} // namespace f110
