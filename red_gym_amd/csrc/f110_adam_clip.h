// f110_adam_clip.h -- gradient clipping for the parameter update (f110_adam.h): the global norm of a step's gradients, the clip
// coefficient and the non-finite guard on the device, and the Adam pass that consumes them.  Kernels of their own beside adam_kernel and
// adam_advance_kernel, which keep their code, registers and bits.
//   adam_gradnorm_kernel      a workgroup owns one chunk, found as adam_kernel finds it.  Lane l is chain l of the chunk's sum: it holds
//                             the quads l, l + 256, l + 512, l + 768 of the chunk (adam_clip_chain, f110_adam_plan.h) -- on the 16-byte
//                             path one float4 each, the loads adam_kernel makes of g -- and adds their squares in fp64 in element
//                             order; the up to three elements behind a tensor's last whole quad belong to the last quad's chain and are
//                             loaded one by one by that lane.  A tensor whose g is not 16-byte aligned goes element by element with the
//                             same membership.  Then the losses' tree over 2 KiB of LDS; lane 0 stores the partial.
//   adam_clip_kernel          one workgroup: 256 chains over the partials, the tree, and lane 0 forms norm, coef and skip, advances
//                             the counters and writes the 64-byte state with plain stores.
//   adam_advance_clip_kernel  adam_advance_kernel behind a test of clip->skip.
//   adam_clipped_kernel<TARGET>  adam_kernel<true, TARGET> with gc = g * coef in g's place and the Adam half inside `if (!skip)`: skip is
//                             one scalar load, the branch wave-uniform; on a skip g, m and v are not even loaded.
// Sizing: the norm pass reads 4 bytes per parameter with four independent 16-byte loads in flight per lane, behind them 16 dependent
// fp64 additions per lane and 8 tree levels; the partials of SAL's critic are 3 143 doubles, which the one-workgroup second stage walks
// in 13 additions per lane.  Numerics: the contract of include/f110_hip.h ("Gradient clipping"); nothing contracted.
#pragma once
#include <hip/hip_runtime.h>
#include "f110_adam.h"
#include "f110_adam_plan.h"
#include "f110_sacloss.h"

#pragma clang fp contract(off)

namespace f110 {

static_assert(AC_THREADS == AD_THREADS && AC_THREADS == SL_THREADS && AC_QUADS == AD_VPL, "the chains are the update's lanes and the tree's");

using AdamClipState = f110_adam_clip_state;

// grid: the chunks of every tensor of the table; partials: the step's array behind chunk_base.  Of the table g, n, vec and chunk_end.
static __global__ __launch_bounds__(AC_THREADS) void adam_gradnorm_kernel(const AdamTable tab, double *partials)
{
    __shared__ double s[AC_THREADS];
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = tab.n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab.chunk_end[mid] > b) hi = mid; else lo = mid + 1;
    }
    const uint32_t first = lo > 0 ? tab.chunk_end[lo - 1] : 0u;
    const float *const G = tab.t[lo].g;
    const uint32_t n = tab.t[lo].n;
    const bool vec = tab.t[lo].vec != 0;
    const size_t base = (size_t)(b - first) * (size_t)AC_CHUNK;
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (base < (size_t)n) {                             // (always: the host sized the grid from the same counts)
        const uint32_t cnt = (uint32_t)((size_t)n - base < (size_t)AC_CHUNK ? (size_t)n - base : (size_t)AC_CHUNK);
        if (vec) {
            const uint32_t nv = cnt / 4;                // whole quads of the chunk
            float4 g[AC_QUADS];
#pragma unroll
            for (int k = 0; k < AC_QUADS; k++) {
                const uint32_t i = (uint32_t)tid + (uint32_t)k * AC_THREADS;
                g[k] = i < nv ? *reinterpret_cast<const float4 *>(G + base + 4 * (size_t)i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int k = 0; k < AC_QUADS; k++) {
                const uint32_t i = (uint32_t)tid + (uint32_t)k * AC_THREADS;
                if (i < nv) {
                    acc = acc + (double)g[k].x * (double)g[k].x;
                    acc = acc + (double)g[k].y * (double)g[k].y;
                    acc = acc + (double)g[k].z * (double)g[k].z;
                    acc = acc + (double)g[k].w * (double)g[k].w;
                }
            }
            if (adam_clip_chain(4 * nv) == tid) {       // the elements behind the last whole quad: that quad's chain, behind all others
                for (uint32_t j = 4 * nv; j < cnt; j++) {
                    const float x = G[base + (size_t)j];
                    acc = acc + (double)x * (double)x;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4 * AC_QUADS; k++) {
                const uint32_t j = adam_clip_element(tid, k);
                if (j < cnt) {
                    const float x = G[base + (size_t)j];
                    acc = acc + (double)x * (double)x;
                }
            }
        }
    }
    s[tid] = acc;
    sacloss_tree(s, tid);
    if (tid == 0) partials[b] = s[0];
}

// grid 1, block 256
static __global__ __launch_bounds__(AC_THREADS) void adam_clip_kernel(const double *partials, long long n_chunks, double max_norm, AdamClipState *clip)
{
    __shared__ double s[AC_THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long c = tid; c < n_chunks; c += AC_THREADS) acc = acc + partials[c];
    s[tid] = acc;
    sacloss_tree(s, tid);
    if (tid != 0) return;
    const double S = s[0];
    const bool finite = S < __builtin_inf();
    const double inf = __builtin_inf();
    double norm = inf;
    float coef = 1.0f;
    if (finite) {
        norm = S == 0.0 ? 0.0 : adam_sqrt_rn(S);
        const double den = norm + 1e-6;
        const double c = max_norm / den;
        coef = c < 1.0 ? (float)c : 1.0f;
    }
    const bool clipped = finite && coef < 1.0f;
    clip->sumsq = finite ? S : inf;
    clip->norm = norm;
    clip->coef = coef;
    clip->skip = finite ? 0 : 1;
    clip->steps_clipped = clip->steps_clipped + (clipped ? 1 : 0);
    clip->steps_skipped = clip->steps_skipped + (finite ? 0 : 1);
}

// grid 1, block 64
static __global__ void adam_advance_clip_kernel(AdamState *s, const AdamClipState *clip, double beta1, double beta2, double lr)
{
    if (threadIdx.x != 0 || clip->skip != 0) return;
    adam_advance(s, beta1, beta2, lr);
}

// grid: the chunks of every tensor of the table, as adam_kernel's
template <bool TARGET>
static __global__ __launch_bounds__(AD_THREADS) void adam_clipped_kernel(const AdamTable tab, const AdamState *state, const AdamClipState *clip)
{
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = tab.n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab.chunk_end[mid] > b) hi = mid; else lo = mid + 1;
    }
    const bool skip = clip->skip != 0;                  // one scalar load: uniform in the launch
    if (skip && !TARGET) return;
    const uint32_t first = lo > 0 ? tab.chunk_end[lo - 1] : 0u;
    float *const P = tab.t[lo].p;
    const float *const G = tab.t[lo].g;
    float *const M = tab.t[lo].m;
    float *const V = tab.t[lo].v;
    float *const T = tab.t[lo].target;
    const uint32_t n = tab.t[lo].n;
    const bool vec = tab.t[lo].vec != 0;
    const size_t base = (size_t)(b - first) * (size_t)AD_CHUNK;
    if (base >= (size_t)n) return;
    const uint32_t cnt = (uint32_t)((size_t)n - base < (size_t)AD_CHUNK ? (size_t)n - base : (size_t)AD_CHUNK);
    AdamConsts c;
    c.c1 = tab.c1; c.c2 = tab.c2; c.b2 = tab.b2; c.eps = tab.eps; c.tau = tab.tau;
    c.k2 = state->k2;
    c.a = state->a;
    const float coef = clip->coef;
    const uint32_t tid = threadIdx.x;
    float unused = 0.0f;
    if (vec) {
        const uint32_t nv = cnt / 4;
        float4 p[AD_VPL], g[AD_VPL], m[AD_VPL], v[AD_VPL], tp[AD_VPL];
#pragma unroll
        for (int k = 0; k < AD_VPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < nv) {
                const size_t e = base + 4 * (size_t)i;
                p[k] = *reinterpret_cast<const float4 *>(P + e);
                if (!skip) {
                    g[k] = *reinterpret_cast<const float4 *>(G + e);
                    m[k] = *reinterpret_cast<const float4 *>(M + e);
                    v[k] = *reinterpret_cast<const float4 *>(V + e);
                }
                if (TARGET) tp[k] = *reinterpret_cast<const float4 *>(T + e);
            }
        }
#pragma unroll
        for (int k = 0; k < AD_VPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < nv) {
                const size_t e = base + 4 * (size_t)i;
                if (!skip) {
                    adam_element<true, false>(c, p[k].x, g[k].x * coef, m[k].x, v[k].x, unused);
                    adam_element<true, false>(c, p[k].y, g[k].y * coef, m[k].y, v[k].y, unused);
                    adam_element<true, false>(c, p[k].z, g[k].z * coef, m[k].z, v[k].z, unused);
                    adam_element<true, false>(c, p[k].w, g[k].w * coef, m[k].w, v[k].w, unused);
                    *reinterpret_cast<float4 *>(P + e) = p[k];
                    *reinterpret_cast<float4 *>(M + e) = m[k];
                    *reinterpret_cast<float4 *>(V + e) = v[k];
                }
                if (TARGET) {
                    adam_element<false, true>(c, p[k].x, unused, unused, unused, tp[k].x);
                    adam_element<false, true>(c, p[k].y, unused, unused, unused, tp[k].y);
                    adam_element<false, true>(c, p[k].z, unused, unused, unused, tp[k].z);
                    adam_element<false, true>(c, p[k].w, unused, unused, unused, tp[k].w);
                    *reinterpret_cast<float4 *>(T + e) = tp[k];
                }
            }
        }
        const uint32_t i = 4 * nv + tid;                // the elements behind the last whole vector: lanes 0 .. 2
        if (tid < 4 && i < cnt) {
            const size_t e = base + (size_t)i;
            float p1 = P[e];
            if (!skip) {
                float m1 = M[e], v1 = V[e];
                adam_element<true, false>(c, p1, G[e] * coef, m1, v1, unused);
                P[e] = p1; M[e] = m1; V[e] = v1;
            }
            if (TARGET) {
                float t1 = T[e];
                adam_element<false, true>(c, p1, unused, unused, unused, t1);
                T[e] = t1;
            }
        }
    } else {
        float p[AD_EPL], g[AD_EPL], m[AD_EPL], v[AD_EPL], tp[AD_EPL];
#pragma unroll
        for (int k = 0; k < AD_EPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < cnt) {
                const size_t e = base + (size_t)i;
                p[k] = P[e];
                if (!skip) { g[k] = G[e]; m[k] = M[e]; v[k] = V[e]; }
                if (TARGET) tp[k] = T[e];
            }
        }
#pragma unroll
        for (int k = 0; k < AD_EPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < cnt) {
                const size_t e = base + (size_t)i;
                if (!skip) {
                    adam_element<true, false>(c, p[k], g[k] * coef, m[k], v[k], unused);
                    P[e] = p[k]; M[e] = m[k]; V[e] = v[k];
                }
                if (TARGET) {
                    adam_element<false, true>(c, p[k], unused, unused, unused, tp[k]);
                    T[e] = tp[k];
                }
            }
        }
    }
}

} // namespace f110
