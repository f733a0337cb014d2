// f110_qhead.h -- the tail of the reference's critics (src/SAL.py:440-442 behind the feature part of fc1, and :546-549: the 16-wide
// action part of fc1, bias, ReLU, fc2, the min over the twin critics and the TD target), forward in one kernel and a backward without
// atomics, for C = 1 or 2 critics at once.
//   qhead_forward_kernel   a workgroup walks tiles of QH_ROWS rows, tile = blockIdx.x, + gridDim.x, ...; a wave owns QH_RPW rows and
//                          lane l the hidden units l, l + 64, ..., so that a wave's loads of pre are whole 256-byte lines.  Critic by
//                          critic: its w_act, b1 and w2 are staged in LDS, then the tiles are walked; the second critic's pass reads
//                          the first one's q back (the lane that wrote it) and finishes qmin and the target.
//   qhead_rows_kernel      backward, the same walk with one row per wave: z again, g_z = [z > 0] G w2, grad_pre, and grad_action's
//                          64 partial chains per action column, the tree, and the critics added through grad_action itself
//   qhead_gradw_kernel     stage 1 of the parameter gradients: a workgroup per (slice of F110_QHEAD_SLICE_ROWS rows, 256 hidden
//                          units, critic), lane = unit, the chains over the slice's rows in ascending order
//   qhead_reduce_kernel    stage 2: the slices of every element summed in ascending order, written with the row stride ld
// LDS of the two row kernels, for one critic: w_act transposed [A][hc + 1] (lane = unit reads consecutive words; the pad spreads the
// staging writes), b1 [hc], w2 [hc]; hc = the hidden units held at a time, a multiple of 64: all of H when (A (H64 + 1) + 2 H64) * 4
// <= QH_LDS_BYTES (SAL: 36.1 KB), staged once per critic and workgroup; else every tile stages its chunks in turn.
// Numerics: the contract of include/f110_hip.h; every fused step is an explicit fmaf, every other one a separately rounded operation.
#pragma once
#include "f110_qhead_plan.h" // limits, QheadArgs, qhead_partial_floats; the host's checks and launch plans

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace f110 {

// Units j0 .. j0 + hc - 1 of critic c in LDS; units past H are zeros.
__device__ inline void qhead_stage(const QheadArgs &a, float *lw, int c, int j0, int tid)
{
    const int hcp = a.hc + 1;
    float *lb = lw + a.A * hcp, *l2 = lb + a.hc;
    const float *__restrict__ w = a.w_act[c];
    for (int it = tid; it < a.hc * a.A; it += QH_THREADS) {
        const int jj = it / a.A, k = it - jj * a.A, j = j0 + jj;
        lw[k * hcp + jj] = j < a.H ? w[(size_t)j * (size_t)a.ld + (size_t)k] : 0.0f;
    }
    for (int jj = tid; jj < a.hc; jj += QH_THREADS) {
        const int j = j0 + jj;
        lb[jj] = j < a.H && a.b1[c] ? a.b1[c][j] : 0.0f;
        l2[jj] = j < a.H ? a.w2[c][j] : 0.0f;
    }
}

// lane k < A: action[row][k] rounded once to fp32 (0 on the other lanes and for a row past n)
__device__ inline float qhead_action(const QheadArgs &a, long long row, int lane)
{
    if (row >= a.n || lane >= a.A) return 0.0f;
    const size_t e = (size_t)row * (size_t)a.A + (size_t)lane;
    return a.act_fp64 ? (float)reinterpret_cast<const double *>(a.action)[e] : reinterpret_cast<const float *>(a.action)[e];
}

__device__ inline float qhead_lane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// s_l = s_l + s_{l + m} for m = 32 .. 1: lane 0 ends with the tree's sum
__device__ inline float qhead_tree(float s)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_down(s, m, 64);
    return s;
}

// grid: min(tiles, QH_MAX_GRID); dynamic LDS of (A (hc + 1) + 2 hc) * 4 bytes
static __global__ __launch_bounds__(QH_THREADS) void qhead_forward_kernel(QheadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qh_lds[];
    float *lw = reinterpret_cast<float *>(qh_lds);
    const int hcp = a.hc + 1;
    const float *lb = lw + a.A * hcp, *l2 = lb + a.hc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = 0; c < a.C; c++) {
        if (c > 0) __syncthreads();                   // (the waves have finished with the critic before)
        if (a.chunks == 1) {
            qhead_stage(a, lw, c, 0, tid);
            __syncthreads();
        }
        const float *__restrict__ pre = a.pre[c];
        for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
            const long long row0 = tile * QH_ROWS + QH_RPW * wave;
            bool rok[QH_RPW];
            float av[QH_RPW], s[QH_RPW];
            const float *pr[QH_RPW];
#pragma unroll
            for (int r = 0; r < QH_RPW; r++) {
                rok[r] = row0 + r < a.n;
                av[r] = qhead_action(a, row0 + r, lane);
                s[r] = 0.0f;
                pr[r] = pre + (size_t)(rok[r] ? row0 + r : 0) * (size_t)a.H;
            }
            for (int ch = 0; ch < a.chunks; ch++) {
                const int j0 = ch * a.hc;
                if (a.chunks > 1) {
                    __syncthreads();                  // (the waves have finished with the chunk before)
                    qhead_stage(a, lw, c, j0, tid);
                    __syncthreads();
                }
                if (!rok[0]) continue;                // (uniform in the wave; the barriers above are passed by every wave)
                for (int i0 = 0; i0 < a.hc; i0 += 128) {
                    // two units of the lane, two rows: four chains
                    int jj[2];
                    bool ok[2];
                    float p[2][QH_RPW], acc[2][QH_RPW];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        jj[u] = i0 + 64 * u + lane;
                        ok[u] = jj[u] < a.hc && j0 + jj[u] < a.H;
                        if (!ok[u]) jj[u] = lane;
#pragma unroll
                        for (int r = 0; r < QH_RPW; r++) {
                            p[u][r] = ok[u] && rok[r] ? pr[r][j0 + jj[u]] : 0.0f;
                            acc[u][r] = 0.0f;
                        }
                    }
                    for (int k = 0; k < a.A; k++) {
                        float x[QH_RPW];
#pragma unroll
                        for (int r = 0; r < QH_RPW; r++) x[r] = qhead_lane(av[r], k);
#pragma unroll
                        for (int u = 0; u < 2; u++) {
                            const float w = lw[k * hcp + jj[u]];
#pragma unroll
                            for (int r = 0; r < QH_RPW; r++) acc[u][r] = __builtin_fmaf(w, x[r], acc[u][r]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        if (!ok[u]) continue;
                        const float b = lb[jj[u]], w2 = l2[jj[u]];
#pragma unroll
                        for (int r = 0; r < QH_RPW; r++) {
                            const float z = (p[u][r] + acc[u][r]) + b;
                            const float h = z > 0.0f ? z : 0.0f;
                            s[r] = __builtin_fmaf(w2, h, s[r]);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < QH_RPW; r++) {
                if (!rok[r]) continue;                // (uniform in the wave)
                const float sum = qhead_tree(s[r]);
                if (lane != 0) continue;
                const long long row = row0 + r;
                const float q = sum + (a.b2[c] ? a.b2[c][0] : 0.0f);
                a.q[(size_t)c * (size_t)a.n + (size_t)row] = q;
                if (c != a.C - 1) continue;
                float qm = q;
                if (a.C == 2) {
                    const float q0 = a.q[row];       // (this lane wrote it in the first critic's pass)
                    qm = q0 < q ? q0 : q;
                }
                if (a.qmin) a.qmin[row] = qm;
                if (a.target) {
                    const double lp = a.act_fp64 ? reinterpret_cast<const double *>(a.nlp)[row] : (double)reinterpret_cast<const float *>(a.nlp)[row];
                    const double alpha = a.alpha_dev ? *a.alpha_dev : a.alpha;      // (uniform in the launch)
                    const double tq = (double)qm - alpha * lp;
                    const double gamma = a.discount_dev ? a.discount_dev[row] : a.gamma;  // (the branch is uniform in the launch)
                    const double keep = (1.0 - (double)a.done[row]) * gamma;
                    a.target[row] = (float)(a.reward[row] + keep * tq);
                }
            }
        }
    }
}

// G_c[b] = grad_q[c][b] + grad_qmin[b] * m_c[b]; m_c = 1, 0.5, 0 where q_c <, ==, > the other critic's (C = 1: 1)
__device__ inline float qhead_G(const QheadArgs &a, int c, long long b)
{
    float m = 1.0f;
    if (a.C == 2) {
        const float mine = a.q_in[(size_t)c * (size_t)a.n + (size_t)b], other = a.q_in[(size_t)(1 - c) * (size_t)a.n + (size_t)b];
        m = mine < other ? 1.0f : mine == other ? 0.5f : 0.0f;
    }
    const float gq = a.grad_q ? a.grad_q[(size_t)c * (size_t)a.n + (size_t)b] : 0.0f;
    const float gm = a.grad_qmin ? a.grad_qmin[b] : 0.0f;
    return gq + gm * m;
}

// grid: min(tiles, QH_MAX_GRID), tiles of QH_BROWS rows; dynamic LDS as the forward kernel's.  AMAX: 16 or 32, the accumulators held
template <int AMAX>
static __global__ __launch_bounds__(QH_THREADS) void qhead_rows_kernel(QheadArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qh_lds[];
    float *lw = reinterpret_cast<float *>(qh_lds);
    const int hcp = a.hc + 1;
    const float *lb = lw + a.A * hcp, *l2 = lb + a.hc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool want_ga = a.grad_action != nullptr;
    for (int c = 0; c < a.C; c++) {
        if (c > 0) __syncthreads();
        if (a.chunks == 1) {
            qhead_stage(a, lw, c, 0, tid);
            __syncthreads();
        }
        const float *__restrict__ pre = a.pre[c];
        float *gpre = a.grad_pre[c];
        for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
            const long long row = tile * QH_BROWS + wave;
            const bool rok = row < a.n;
            const float av = qhead_action(a, row, lane);
            const float G = rok ? qhead_G(a, c, row) : 0.0f;
            const size_t base = (size_t)(rok ? row : 0) * (size_t)a.H;
            float ga[AMAX];
#pragma unroll
            for (int k = 0; k < AMAX; k++) ga[k] = 0.0f;
            for (int ch = 0; ch < a.chunks; ch++) {
                const int j0 = ch * a.hc;
                if (a.chunks > 1) {
                    __syncthreads();
                    qhead_stage(a, lw, c, j0, tid);
                    __syncthreads();
                }
                if (!rok) continue;
                for (int i0 = 0; i0 < a.hc; i0 += 128) {
                    int jj[2];
                    bool ok[2];
                    float p[2], acc[2], w[2][AMAX];
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        jj[u] = i0 + 64 * u + lane;
                        ok[u] = jj[u] < a.hc && j0 + jj[u] < a.H;
                        if (!ok[u]) jj[u] = lane;
                        p[u] = ok[u] ? pre[base + (size_t)(j0 + jj[u])] : 0.0f;
                        acc[u] = 0.0f;
                    }
#pragma unroll
                    for (int k = 0; k < AMAX; k++) {
                        if (k < a.A) {
                            const float x = qhead_lane(av, k);
#pragma unroll
                            for (int u = 0; u < 2; u++) {
                                w[u][k] = lw[k * hcp + jj[u]];
                                acc[u] = __builtin_fmaf(w[u][k], x, acc[u]);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        if (!ok[u]) continue;
                        const float z = (p[u] + acc[u]) + lb[jj[u]];
                        const float gz = z > 0.0f ? G * l2[jj[u]] : 0.0f;
                        if (gpre) gpre[base + (size_t)(j0 + jj[u])] = gz;
                        if (want_ga) {
#pragma unroll
                            for (int k = 0; k < AMAX; k++)
                                if (k < a.A) ga[k] = __builtin_fmaf(gz, w[u][k], ga[k]);
                        }
                    }
                }
            }
            if (!rok || !want_ga) continue;           // (uniform in the wave)
#pragma unroll
            for (int k = 0; k < AMAX; k++) {
                if (k < a.A) {
                    const float t = qhead_tree(ga[k]);
                    if (lane == 0) {
                        // the critics added in ascending order from 0: the first pass's sum comes back from grad_action itself
                        // (this lane wrote it; a float survives the way through a double unchanged)
                        const size_t e = (size_t)row * (size_t)a.A + (size_t)k;
                        if (a.act_fp64) {
                            double *o = reinterpret_cast<double *>(a.grad_action);
                            o[e] = (double)((c == 0 ? 0.0f : (float)o[e]) + t);
                        } else {
                            float *o = reinterpret_cast<float *>(a.grad_action);
                            o[e] = (c == 0 ? 0.0f : o[e]) + t;
                        }
                    }
                }
            }
        }
    }
}

// grid: (slices, ceil(H / QH_THREADS), C).  partial[c][slice]: for unit j = lane: grad_w_act[j][k]: acc = fmaf(g_z[b][j], action[b][k],
// acc); grad_b1[j]: acc = acc + g_z[b][j]; grad_w2[j]: acc = fmaf(G[b], h[b][j], acc); grad_b2: acc = acc + G[b]; b ascending
template <int AMAX>
static __global__ __launch_bounds__(QH_THREADS) void qhead_gradw_kernel(QheadArgs a)
{
    __shared__ float sa[QH_SLICE * AMAX];
    __shared__ float sG[QH_SLICE];
    const int tid = threadIdx.x, c = blockIdx.z;
    const long long b0 = (long long)blockIdx.x * QH_SLICE;
    const int rows = (int)min((long long)QH_SLICE, a.n - b0);
    for (int it = tid; it < rows * a.A; it += QH_THREADS) {
        const size_t e = (size_t)b0 * (size_t)a.A + (size_t)it;
        sa[it] = a.act_fp64 ? (float)reinterpret_cast<const double *>(a.action)[e] : reinterpret_cast<const float *>(a.action)[e];
    }
    for (int r = tid; r < rows; r += QH_THREADS) sG[r] = qhead_G(a, c, b0 + r);
    __syncthreads();
    const int j = blockIdx.y * QH_THREADS + tid;
    const bool jok = j < a.H;
    float w[AMAX], gw[AMAX];
#pragma unroll
    for (int k = 0; k < AMAX; k++) {
        w[k] = jok && k < a.A ? a.w_act[c][(size_t)j * (size_t)a.ld + (size_t)k] : 0.0f;
        gw[k] = 0.0f;
    }
    const float b1 = jok && a.b1[c] ? a.b1[c][j] : 0.0f, w2 = jok ? a.w2[c][j] : 0.0f;
    const float *__restrict__ pre = a.pre[c] + (size_t)b0 * (size_t)a.H + (size_t)(jok ? j : 0);
    float gb1 = 0.0f, gw2 = 0.0f, gb2 = 0.0f;
    for (int r0 = 0; r0 < rows; r0 += 4) {
        float p[4];
#pragma unroll
        for (int u = 0; u < 4; u++) p[u] = jok && r0 + u < rows ? pre[(size_t)(r0 + u) * (size_t)a.H] : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + u;
            if (r >= rows) break;
            const float *x = sa + r * a.A;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < AMAX; k++)
                if (k < a.A) acc = __builtin_fmaf(w[k], x[k], acc);
            const float z = (p[u] + acc) + b1;
            const float G = sG[r];
            const float h = z > 0.0f ? z : 0.0f, gz = z > 0.0f ? G * w2 : 0.0f;
#pragma unroll
            for (int k = 0; k < AMAX; k++)
                if (k < a.A) gw[k] = __builtin_fmaf(gz, x[k], gw[k]);
            gb1 = gb1 + gz;
            gw2 = __builtin_fmaf(G, h, gw2);
            gb2 = gb2 + G;
        }
    }
    float *out = a.partial + ((size_t)c * (size_t)a.slices + (size_t)blockIdx.x) * qhead_partial_floats(a.H, a.A);
    if (jok) {
#pragma unroll
        for (int k = 0; k < AMAX; k++)
            if (k < a.A) out[(size_t)j * (size_t)a.A + (size_t)k] = gw[k];
        out[(size_t)a.H * (size_t)a.A + (size_t)j] = gb1;
        out[(size_t)a.H * (size_t)(a.A + 1) + (size_t)j] = gw2;
    }
    if (j == 0) out[(size_t)a.H * (size_t)(a.A + 2)] = gb2;
}

// grid: (ceil((H (A + 2) + 1) / QH_THREADS), C).  The slices of an element added in ascending order from 0; NULL outputs are skipped
static __global__ __launch_bounds__(QH_THREADS) void qhead_reduce_kernel(QheadArgs a)
{
    const size_t P = qhead_partial_floats(a.H, a.A), e = (size_t)blockIdx.x * QH_THREADS + threadIdx.x;
    const int c = blockIdx.y;
    if (e >= P) return;
    const float *p = a.partial + (size_t)c * (size_t)a.slices * P + e;
    float acc = 0.0f;
    for (int s = 0; s < a.slices; s++) acc = acc + p[(size_t)s * P];
    const size_t HA = (size_t)a.H * (size_t)a.A, H = (size_t)a.H;
    if (e < HA) {
        const size_t j = e / (size_t)a.A, k = e - j * (size_t)a.A;
        if (a.grad_w_act[c]) a.grad_w_act[c][j * (size_t)a.ld + k] = acc;
    } else if (e < HA + H) {
        if (a.grad_b1[c]) a.grad_b1[c][e - HA] = acc;
    } else if (e < HA + 2 * H) {
        if (a.grad_w2[c]) a.grad_w2[c][e - HA - H] = acc;
    } else if (a.grad_b2[c]) {
        a.grad_b2[c][0] = acc;
    }
}

} // namespace f110
