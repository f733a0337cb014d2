// f110_dense.h -- a dense layer of fp32 features, forward and backward: fc1 = nn.Linear(32 * 28 * 28, 512) of the reference's Actor
// and the feature columns of nn.Linear(32 * 28 * 28 + 16, 512) of its Critic (src/SAL.py:400, 432) with their ReLU, under the
// numerics contract of include/f110_hip.h: three GEMMs on v_mfma_f32_16x16x4_f32, K fed through the accumulator, which on gfx950
// is bit for bit a k-ordered fmaf chain (as f110_featconv.h relies on).
//   dense_forward_kernel<false>  M = rows, N = h, K = k.  A workgroup owns a block of DN_BM rows x DN_BN outputs and walks the
//                                segments of K: per segment a chain from 0, then sum = acc_0, sum = sum + acc_j in registers;
//                                out = sum + bias, relu.
//   dense_forward_kernel<true>   the same block and ONE segment (blockIdx.x) per workgroup: the chain goes to P[segment][row][h].
//   dense_sum_kernel             out = (((P[0] + P[1]) + P[2]) + ...) + bias, relu: the adds of the kernel above, a thread per output.
//   dense_gradx_kernel           M = rows, N = k, K = h: one chain over all of H.  g = grad_out masked by out > 0 under relu.
//   dense_gradw_kernel           M = h, N = k, K = rows: one chain over all n rows.  Writes rows of grad_weight ld apart.
//   dense_gradb_kernel           acc = acc + g[r][h], rows ascending, a thread per h.
// Operands.  MFMA step m of a chunk takes from lane (col = lane & 15, quad = lane >> 4) the term 4 m + quad of row col of both tiles,
// so the four terms of a step are consecutive and the steps ascend.  A lane never feeds the four components of one 16-byte load to
// four steps (that would interleave k); instead the workgroup stages DN_KC terms of both tiles in LDS with 16-byte loads along
// whichever index memory runs (k for x and weight, h for grad_out, k for the rows of grad_weight's operands) and every lane reads
// its one float per step back: tiles staged [row][term] lie DN_LDK floats apart, tiles staged [term][column] DN_LDM / DN_LDN, so the
// 64 addresses of a read fall into 64 different banks.  The next chunk's global loads are issued before the current chunk's
// multiplies.  A term beyond the end of a segment, of K, of H or of n, and a row or column beyond the matrix, is staged as 0: the
// step computes fma(0, 0, acc), which leaves acc (never -0) as it is.
// A wave holds two accumulators, the block's two M-tiles against its own N-tile: independent output tiles, never a split of a chain.
// 16-byte global loads need a 16-byte aligned base and a row stride that is a multiple of 4 floats (DenseArgs vec_*); a view such
// as fc1.weight[:, :F] of the critics' [H, F + A] matrix, or its gradient, is read and written with 4-byte accesses where it is not.
// Not tuned: the block is small (x is re-read once per DN_BN outputs, weight once per DN_BM rows), there is no direct-to-LDS load,
// and dense_gradb_kernel is one thread per output.
#pragma once
#include "f110_bounds.h"
#include "f110_dense_plan.h" // limits, DenseArgs; the host's checks and launch plans

#pragma clang fp contract(off)

namespace f110 {

typedef float dn_f32x4 __attribute__((ext_vector_type(4)));

// elements k .. k + 3 of a row (nullptr: a row beyond the matrix), 0 from `end` on; one 16-byte load where vec allows
__device__ inline float4 dense_load4(const float *__restrict__ row, int k, int end, bool vec)
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!row) return v;
    if (vec && k + 4 <= end) return *reinterpret_cast<const float4 *>(row + k);
    if (k < end) v.x = row[k];
    if (k + 1 < end) v.y = row[k + 1];
    if (k + 2 < end) v.z = row[k + 2];
    if (k + 3 < end) v.w = row[k + 3];
    return v;
}

// g of the backward at elements h .. h + 3 of a row: grad_out, and 0 where out is not positive under relu (mask = out's row)
__device__ inline float4 dense_load_g(const float *__restrict__ go, const float *__restrict__ mask, int h, int end, bool vec)
{
    float4 g = dense_load4(go, h, end, vec);
    if (mask && go) {
        const float4 o = dense_load4(mask, h, end, vec);
        g.x = o.x > 0.0f ? g.x : 0.0f; g.y = o.y > 0.0f ? g.y : 0.0f; g.z = o.z > 0.0f ? g.z : 0.0f; g.w = o.w > 0.0f ? g.w : 0.0f;
    }
    return g;
}

__device__ inline void dense_put4(float *lds, int at, float4 v) { *reinterpret_cast<float4 *>(lds + at) = v; }

// the eight steps of a staged chunk: A tiles [row][term] or [term][row] (stride given per term and per row), B likewise
template <int A_ROW, int A_TERM, int B_ROW, int B_TERM>
__device__ inline void dense_mma(const float *as, const float *bs, int wave, int col, int quad, dn_f32x4 (&acc)[2])
{
    float a0[DN_KC / 4], a1[DN_KC / 4], b[DN_KC / 4];
#pragma unroll
    for (int m = 0; m < DN_KC / 4; m++) {
        const int t = 4 * m + quad;
        a0[m] = as[col * A_ROW + t * A_TERM];
        a1[m] = as[(16 + col) * A_ROW + t * A_TERM];
        b[m] = bs[(16 * wave + col) * B_ROW + t * B_TERM];
    }
#pragma unroll
    for (int m = 0; m < DN_KC / 4; m++) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[m], b[m], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[m], b[m], acc[1], 0, 0, 0);
    }
}

// grid: SPLIT (segs, mblocks nblocks), else (mblocks, nblocks); static LDS DN_FORWARD_LDS
template <bool SPLIT>
static __global__ __launch_bounds__(DN_THREADS) void dense_forward_kernel(DenseArgs a)
{
    __shared__ __attribute__((aligned(16))) float xs[DN_BM * DN_LDK];
    __shared__ __attribute__((aligned(16))) float ws[DN_BN * DN_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
    const int mb = SPLIT ? (int)blockIdx.y / a.nblocks : (int)blockIdx.x, nb = SPLIT ? (int)blockIdx.y % a.nblocks : (int)blockIdx.y;
    const long long r0 = (long long)mb * DN_BM;
    const int h0 = nb * DN_BN;
    // what this thread stages: terms sk .. sk + 3 of row srow of x, and of rows srow and DN_BM + srow of the weight block
    const int srow = tid >> 3, sk = (tid & 7) * 4;
    const float *xrow = r0 + srow < a.n ? a.x + (size_t)(r0 + srow) * (size_t)a.K : nullptr;
    const float *wrow0 = h0 + srow < a.H ? a.w + (size_t)(h0 + srow) * (size_t)a.ld : nullptr;
    const float *wrow1 = h0 + DN_BM + srow < a.H ? a.w + (size_t)(h0 + DN_BM + srow) * (size_t)a.ld : nullptr;
    const bool vx = a.vec_x != 0, vw = a.vec_w != 0;

    dn_f32x4 sum[2];
    const int j0 = SPLIT ? (int)blockIdx.x : 0, j1 = SPLIT ? j0 + 1 : a.segs;
    for (int j = j0; j < j1; j++) {
        const int kb = j * a.S, ke = min(a.K, kb + a.S);
        const int chunks = (ke - kb + DN_KC - 1) / DN_KC;
        dn_f32x4 acc[2] = {dn_f32x4{0.0f, 0.0f, 0.0f, 0.0f}, dn_f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
        float4 px = dense_load4(xrow, kb + sk, ke, vx), pw0 = dense_load4(wrow0, kb + sk, ke, vw), pw1 = dense_load4(wrow1, kb + sk, ke, vw);
        for (int c = 0; c < chunks; c++) {
            dense_put4(xs, srow * DN_LDK + sk, px);
            dense_put4(ws, srow * DN_LDK + sk, pw0);
            dense_put4(ws, (DN_BM + srow) * DN_LDK + sk, pw1);
            __syncthreads();
            if (c + 1 < chunks) {
                const int k = kb + (c + 1) * DN_KC + sk;
                px = dense_load4(xrow, k, ke, vx); pw0 = dense_load4(wrow0, k, ke, vw); pw1 = dense_load4(wrow1, k, ke, vw);
            }
            dense_mma<DN_LDK, 1, DN_LDK, 1>(xs, ws, wave, col, quad, acc);
            __syncthreads();            // (the next chunk replaces the tiles)
        }
        if (SPLIT) {
            // lane: rows 16 t + 4 quad + q of the block, output h0 + 16 wave + col
            const int h = h0 + 16 * wave + col;
#pragma unroll
            for (int t = 0; t < 2; t++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const long long r = r0 + 16 * t + 4 * quad + q;
                    if (r < a.n && h < a.H) a.P[((size_t)j * (size_t)a.n + (size_t)r) * (size_t)a.H + (size_t)h] = acc[t][q];
                }
            }
        } else if (j == 0) {
            sum[0] = acc[0]; sum[1] = acc[1];
        } else {
            sum[0] = sum[0] + acc[0]; sum[1] = sum[1] + acc[1];
        }
    }
    if (!SPLIT) {
        const int h = h0 + 16 * wave + col;
        if (h < a.H) {
            const float bias = a.bias ? a.bias[h] : 0.0f;
#pragma unroll
            for (int t = 0; t < 2; t++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const long long r = r0 + 16 * t + 4 * quad + q;
                    float v = sum[t][q] + bias;
                    if (a.relu) v = v < 0.0f ? 0.0f : v;
                    if (r < a.n) a.dst[(size_t)r * (size_t)a.H + (size_t)h] = v;
                }
            }
        }
    }
}

// grid: ceil(n H / DN_THREADS)
static __global__ __launch_bounds__(DN_THREADS) void dense_sum_kernel(DenseArgs a)
{
    const size_t total = (size_t)a.n * (size_t)a.H;
    const size_t e = (size_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= total) return;
    const float *__restrict__ P = a.P;
    float sum = P[e];
    int j = 1;
    for (; j + 16 <= a.segs; j += 16) {      // sixteen loads in flight, added in the same ascending order
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = P[(size_t)(j + u) * total + e];
#pragma unroll
        for (int u = 0; u < 16; u++) sum = sum + v[u];
    }
    for (; j < a.segs; j++) sum = sum + P[(size_t)j * total + e];
    float v = sum + (a.bias ? a.bias[e % (size_t)a.H] : 0.0f);
    if (a.relu) v = v < 0.0f ? 0.0f : v;
    a.dst[e] = v;
}

// grid: (ceil(n / DN_BM), ceil(K / DN_BN)); static LDS DN_GRADX_LDS.  a.dst = grad_x.
static __global__ __launch_bounds__(DN_THREADS) void dense_gradx_kernel(DenseArgs a)
{
    __shared__ __attribute__((aligned(16))) float gs[DN_BM * DN_LDK];      // g [row][h of the chunk]
    __shared__ __attribute__((aligned(16))) float ws[DN_KC * DN_LDN];      // weight [h of the chunk][k of the block]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
    const long long r0 = (long long)blockIdx.x * DN_BM;
    const int k0 = (int)blockIdx.y * DN_BN;
    const int grow = tid >> 3, gh = (tid & 7) * 4;          // g: elements gh .. gh + 3 of the chunk in row grow
    const int wh = tid >> 4, wk = (tid & 15) * 4;           // weight: columns k0 + wk .. + 3 of rows wh and 16 + wh of the chunk
    const bool live = r0 + grow < a.n;
    const float *gorow = live ? a.grad_out + (size_t)(r0 + grow) * (size_t)a.H : nullptr;
    const float *mrow = live && a.relu ? a.out + (size_t)(r0 + grow) * (size_t)a.H : nullptr;
    const bool vg = a.vec_g != 0, vw = a.vec_w != 0;
    auto wload = [&](int h) { return dense_load4(h < a.H ? a.w + (size_t)h * (size_t)a.ld : nullptr, k0 + wk, a.K, vw); };

    const int chunks = (a.H + DN_KC - 1) / DN_KC;
    dn_f32x4 acc[2] = {dn_f32x4{0.0f, 0.0f, 0.0f, 0.0f}, dn_f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
    float4 pg = dense_load_g(gorow, mrow, gh, a.H, vg), pw0 = wload(wh), pw1 = wload(16 + wh);
    for (int c = 0; c < chunks; c++) {
        dense_put4(gs, grow * DN_LDK + gh, pg);
        dense_put4(ws, wh * DN_LDN + wk, pw0);
        dense_put4(ws, (16 + wh) * DN_LDN + wk, pw1);
        __syncthreads();
        if (c + 1 < chunks) {
            const int hc = (c + 1) * DN_KC;
            pg = dense_load_g(gorow, mrow, hc + gh, a.H, vg); pw0 = wload(hc + wh); pw1 = wload(hc + 16 + wh);
        }
        dense_mma<DN_LDK, 1, 1, DN_LDN>(gs, ws, wave, col, quad, acc);
        __syncthreads();
    }
    const int k = k0 + 16 * wave + col;
    if (k < a.K) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const long long r = r0 + 16 * t + 4 * quad + q;
                if (r < a.n) a.dst[(size_t)r * (size_t)a.K + (size_t)k] = acc[t][q];
            }
        }
    }
}

// grid: (ceil(H / DN_BM), ceil(K / DN_BN)); static LDS DN_GRADW_LDS.  a.dst = grad_weight, rows ld apart.
static __global__ __launch_bounds__(DN_THREADS) void dense_gradw_kernel(DenseArgs a)
{
    __shared__ __attribute__((aligned(16))) float gs[DN_KC * DN_LDM];      // g [row of the chunk][h of the block]
    __shared__ __attribute__((aligned(16))) float xs[DN_KC * DN_LDN];      // x [row of the chunk][k of the block]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
    const int h0 = (int)blockIdx.x * DN_BM, k0 = (int)blockIdx.y * DN_BN;
    const int gr = tid >> 3, gh = (tid & 7) * 4;            // g: columns h0 + gh .. + 3 of row gr of the chunk
    const int xr = tid >> 4, xk = (tid & 15) * 4;           // x: columns k0 + xk .. + 3 of rows xr and 16 + xr of the chunk
    const bool vg = a.vec_g != 0, vx = a.vec_x != 0;
    auto gload = [&](long long r) {
        const bool live = r < a.n;
        return dense_load_g(live ? a.grad_out + (size_t)r * (size_t)a.H : nullptr, live && a.relu ? a.out + (size_t)r * (size_t)a.H : nullptr, h0 + gh, a.H, vg);
    };
    auto xload = [&](long long r) { return dense_load4(r < a.n ? a.x + (size_t)r * (size_t)a.K : nullptr, k0 + xk, a.K, vx); };

    const long long chunks = (a.n + DN_KC - 1) / DN_KC;
    dn_f32x4 acc[2] = {dn_f32x4{0.0f, 0.0f, 0.0f, 0.0f}, dn_f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
    float4 pg = gload(gr), px0 = xload(xr), px1 = xload(16 + xr);
    for (long long c = 0; c < chunks; c++) {
        dense_put4(gs, gr * DN_LDM + gh, pg);
        dense_put4(xs, xr * DN_LDN + xk, px0);
        dense_put4(xs, (16 + xr) * DN_LDN + xk, px1);
        __syncthreads();
        if (c + 1 < chunks) {
            const long long rc = (c + 1) * DN_KC;
            pg = gload(rc + gr); px0 = xload(rc + xr); px1 = xload(rc + 16 + xr);
        }
        dense_mma<1, DN_LDM, 1, DN_LDN>(gs, xs, wave, col, quad, acc);
        __syncthreads();
    }
    const int k = k0 + 16 * wave + col;
    if (k < a.K) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int h = h0 + 16 * t + 4 * quad + q;
                if (h < a.H) a.dst[(size_t)h * (size_t)a.ld + (size_t)k] = acc[t][q];
            }
        }
    }
}

// grid: ceil(H / 64) workgroups of one wave
static __global__ __launch_bounds__(64) void dense_gradb_kernel(DenseArgs a)
{
    const int h = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (h >= a.H) return;
    const float *__restrict__ go = a.grad_out + h;
    const float *__restrict__ o = a.relu ? a.out + h : nullptr;
    const size_t H = (size_t)a.H;
    float acc = 0.0f;
    long long r = 0;
    for (; r + 16 <= a.n; r += 16) {        // sixteen rows in flight, added in the same ascending order
        float g[16], m[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { g[u] = go[(size_t)(r + u) * H]; m[u] = o ? o[(size_t)(r + u) * H] : 1.0f; }
#pragma unroll
        for (int u = 0; u < 16; u++) acc = acc + (m[u] > 0.0f ? g[u] : 0.0f);
    }
    for (; r < a.n; r++) acc = acc + ((o ? o[(size_t)r * H] : 1.0f) > 0.0f ? go[(size_t)r * H] : 0.0f);
    a.grad_bias[h] = acc;
}

} // namespace f110
