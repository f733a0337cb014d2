// f110_adam.h -- the parameter update of the reference's SACAgent.update (src/SAL.py:556-578): Adam with the reference's defaults
// (:487-492: no weight decay, no amsgrad, no maximize) and the soft update of a target network, over a list of tensors in ONE pass:
// p, g, m and v are read once, p, m and v written once, and the target is moved from the new p while it is still in a register
// (28 bytes per parameter, 36 with a target; the framework's foreach form makes about ten passes and lerps the targets in one more).
//   adam_advance_kernel  one wave, in front of a step's first update launch: t += 1, the two running powers advance by one fp64
//                        multiplication, and k2 and a (below) are formed in fp64 and rounded once.  The step state lives on the
//                        device, so a step passes no host value that changes from step to step and a captured step replays; every
//                        workgroup of the step, and every further launch of a step with more than AD_MAX_T tensors, reads the same
//                        two floats.  Cost: one dependent kernel boundary per step, measured at 2.8 us on an MI355X
//                        (tools/time_optim.py, profiles/r16_optim.txt); lr enters here as a launch argument and is frozen
//                        under capture.
//   adam_kernel<ADAM, TARGET>  Adam, Adam plus target, target only.  A workgroup owns one chunk of AD_CHUNK consecutive elements of
//                        one tensor.  The table of tensors (AdamTable) travels in the kernel arguments BY VALUE, with the prefix sums
//                        of the tensors' chunk counts: the workgroup finds its (tensor, chunk) by a binary search of blockIdx.x in the
//                        prefix sums, which is wave-uniform (scalar loads of the argument block); no table lives in device memory, so
//                        an eager call follows .grad wherever autograd has put it and a captured one bakes its own pool's addresses.
//                        A tensor whose pointers are all 16-byte aligned is read and written as float4 (lane l holds the vectors l, l
//                        + 256, ... of the chunk: whole 4 KiB runs per wave instruction, AD_VPL independent vectors of each array
//                        in flight per lane), the up to three elements behind its last whole vector one by one; any other tensor (a view
//                        at an odd element offset) goes one element per lane and access.  No LDS, no atomics, no element is touched
//                        by two lanes.
// Sizing: the pass is pure streaming, so what matters is bytes in flight: a 256-thread workgroup asks for 4 (5) arrays x AD_VPL x 4 KiB
// = 64 (80) KiB before its first store; 96 VGPRs (112 with a target, 52 for the target alone), no scratch, so five (four, eight)
// workgroups fit a CU; SAL's critic is 3 143 chunks on 256 CUs.  Measured: one update's worth for SAL's three networks, 1.29 GB, takes
// 250 us, where a device copy of the same bytes takes 239 us (profiles/r16_optim.txt).
// AD_MAX_T: 64 entries of 48 bytes and 64 prefix sums are 3 328 bytes of the 4 KiB a kernel's arguments may take.
// Numerics: the contract of include/f110_hip.h; every fused step is an explicit fmaf, every other one a separately rounded operation,
// the division and the square root are the correctly rounded ones, denormals are kept.
#pragma once
#include "../../include/f110_hip.h" // F110_ADAM_CHUNK, F110_ADAM_MAX_TENSORS, f110_adam_state

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace f110 {

constexpr int AD_THREADS = 256;
constexpr int AD_CHUNK = F110_ADAM_CHUNK;               // elements of a workgroup
constexpr int AD_MAX_T = F110_ADAM_MAX_TENSORS;         // tensors of a launch
constexpr int AD_VPL = AD_CHUNK / (4 * AD_THREADS);     // float4 per lane and array
constexpr int AD_EPL = AD_CHUNK / AD_THREADS;           // elements per lane on the 4-byte path
static_assert(AD_VPL * 4 * AD_THREADS == AD_CHUNK, "a chunk is whole float4 rounds of the workgroup");

struct AdamEntry {
    float *p;
    const float *g;
    float *m, *v, *target;
    uint32_t n;                     // elements, <= 2^31
    uint32_t vec;                   // nonzero: every pointer the mode uses is 16-byte aligned
};

struct AdamTable {
    AdamEntry t[AD_MAX_T];
    uint32_t chunk_end[AD_MAX_T];   // chunks of the tensors 0 .. i: tensor i owns the workgroups chunk_end[i - 1] .. chunk_end[i] - 1
    int n_tensors;
    float c1, c2, b2, eps, tau;     // float(1 - beta1), float(1 - beta2), float(beta2), float(eps), float(tau)
};
static_assert(sizeof(AdamEntry) == 48 && sizeof(AdamTable) + sizeof(void *) <= 4096, "the table must fit the kernel arguments");

using AdamState = f110_adam_state;

// sqrt of a normal positive x (the step's 1 - pow2 in (0, 1]; the sum of squares of f110_adam_clip.h, at least 2^-298 and 2^287 a tensor),
// correctly rounded whatever the library's own last bit: Tuckerman's test (y is the rounded root exactly when y * pred(y) < x <= y *
// succ(y)), each product's sign taken from one fma, which is exact in sign while y * y stays clear of the overflow and denormal ranges.
__device__ inline double adam_sqrt_rn(double x)
{
    double y = sqrt(x);
    for (int k = 0; k < 2; k++) {
        const double lo = __longlong_as_double(__double_as_longlong(y) - 1), hi = __longlong_as_double(__double_as_longlong(y) + 1);
        if (fma(y, lo, -x) >= 0.0) y = lo;
        else if (fma(y, hi, -x) < 0.0) y = hi;
        else break;
    }
    return y;
}

// one lane: the state of step t -> that of step t + 1 (adam_advance_kernel, and the temperature step of f110_temperature.h)
__device__ inline void adam_advance(AdamState *s, double beta1, double beta2, double lr)
{
    const double p1 = s->pow1 * beta1, p2 = s->pow2 * beta2;
    const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
    s->t = s->t + 1;
    s->pow1 = p1;
    s->pow2 = p2;
    s->k2 = (float)adam_sqrt_rn(bc2);
    s->a = (float)(lr / bc1);
}

// grid 1, block 64
static __global__ void adam_advance_kernel(AdamState *s, double beta1, double beta2, double lr)
{
    if (threadIdx.x != 0) return;
    adam_advance(s, beta1, beta2, lr);
}

struct AdamConsts { float c1, c2, b2, eps, tau, k2, a; };

// one element: the table of include/f110_hip.h, line by line
template <bool ADAM, bool TARGET>
__device__ inline void adam_element(const AdamConsts &c, float &p, const float &g, float &m, float &v, float &tp)
{
    if (ADAM) {
        const float d = g - m;
        m = __builtin_fmaf(c.c1, d, m);
        const float t1 = g * g;
        const float t2 = t1 * c.c2;
        v = __builtin_fmaf(c.b2, v, t2);
        const float s = __builtin_sqrtf(v);
        const float r = s / c.k2;
        const float den = r + c.eps;
        const float q = m / den;
        p = __builtin_fmaf(-c.a, q, p);
    }
    if (TARGET) {
        const float u = p - tp;
        tp = __builtin_fmaf(c.tau, u, tp);
    }
}

// grid: the chunks of every tensor of the table, chunk_end[n_tensors - 1]
template <bool ADAM, bool TARGET>
static __global__ __launch_bounds__(AD_THREADS) void adam_kernel(const AdamTable tab, const AdamState *state)
{
    const uint32_t b = blockIdx.x;
    int lo = 0, hi = tab.n_tensors - 1;                 // the first tensor whose chunks end behind b (an empty tensor never is)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab.chunk_end[mid] > b) hi = mid; else lo = mid + 1;
    }
    const uint32_t first = lo > 0 ? tab.chunk_end[lo - 1] : 0u;
    float *const P = tab.t[lo].p;
    const float *const G = tab.t[lo].g;
    float *const M = tab.t[lo].m;
    float *const V = tab.t[lo].v;
    float *const T = tab.t[lo].target;
    const uint32_t n = tab.t[lo].n;
    const bool vec = tab.t[lo].vec != 0;
    const size_t base = (size_t)(b - first) * (size_t)AD_CHUNK;
    if (base >= (size_t)n) return;                      // (never: the host sized the grid from the same counts)
    const uint32_t cnt = (uint32_t)((size_t)n - base < (size_t)AD_CHUNK ? (size_t)n - base : (size_t)AD_CHUNK);
    AdamConsts c;
    c.c1 = tab.c1; c.c2 = tab.c2; c.b2 = tab.b2; c.eps = tab.eps; c.tau = tab.tau;
    c.k2 = ADAM ? state->k2 : 1.0f;
    c.a = ADAM ? state->a : 0.0f;
    const uint32_t tid = threadIdx.x;
    if (vec) {
        const uint32_t nv = cnt / 4;                    // whole vectors of the chunk (base is a multiple of 4)
        float4 p[AD_VPL], g[AD_VPL], m[AD_VPL], v[AD_VPL], tp[AD_VPL];
#pragma unroll
        for (int k = 0; k < AD_VPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < nv) {
                const size_t e = base + 4 * (size_t)i;
                p[k] = *reinterpret_cast<const float4 *>(P + e);
                if (ADAM) {
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
                adam_element<ADAM, TARGET>(c, p[k].x, g[k].x, m[k].x, v[k].x, tp[k].x);
                adam_element<ADAM, TARGET>(c, p[k].y, g[k].y, m[k].y, v[k].y, tp[k].y);
                adam_element<ADAM, TARGET>(c, p[k].z, g[k].z, m[k].z, v[k].z, tp[k].z);
                adam_element<ADAM, TARGET>(c, p[k].w, g[k].w, m[k].w, v[k].w, tp[k].w);
                if (ADAM) {
                    *reinterpret_cast<float4 *>(P + e) = p[k];
                    *reinterpret_cast<float4 *>(M + e) = m[k];
                    *reinterpret_cast<float4 *>(V + e) = v[k];
                }
                if (TARGET) *reinterpret_cast<float4 *>(T + e) = tp[k];
            }
        }
        const uint32_t i = 4 * nv + tid;                // the elements behind the last whole vector: lanes 0 .. 2
        if (tid < 4 && i < cnt) {
            const size_t e = base + (size_t)i;
            float p1 = P[e], g1 = ADAM ? G[e] : 0.0f, m1 = ADAM ? M[e] : 0.0f, v1 = ADAM ? V[e] : 0.0f, t1 = TARGET ? T[e] : 0.0f;
            adam_element<ADAM, TARGET>(c, p1, g1, m1, v1, t1);
            if (ADAM) { P[e] = p1; M[e] = m1; V[e] = v1; }
            if (TARGET) T[e] = t1;
        }
    } else {
        float p[AD_EPL], g[AD_EPL], m[AD_EPL], v[AD_EPL], tp[AD_EPL];
#pragma unroll
        for (int k = 0; k < AD_EPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < cnt) {
                const size_t e = base + (size_t)i;
                p[k] = P[e];
                if (ADAM) { g[k] = G[e]; m[k] = M[e]; v[k] = V[e]; }
                if (TARGET) tp[k] = T[e];
            }
        }
#pragma unroll
        for (int k = 0; k < AD_EPL; k++) {
            const uint32_t i = tid + (uint32_t)k * AD_THREADS;
            if (i < cnt) {
                const size_t e = base + (size_t)i;
                adam_element<ADAM, TARGET>(c, p[k], g[k], m[k], v[k], tp[k]);
                if (ADAM) { P[e] = p[k]; M[e] = m[k]; V[e] = v[k]; }
                if (TARGET) T[e] = tp[k];
            }
        }
    }
}

} // namespace f110
