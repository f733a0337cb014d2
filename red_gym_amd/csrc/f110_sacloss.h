// f110_sacloss.h -- the two losses of the reference's SACAgent.update (src/SAL.py:553-554 F.mse_loss of each critic against the TD
// target, :568 (alpha * log_prob - min_q).mean()) and their gradients with respect to the kernels' inputs, one launch each, in place
// of a dozen element-wise and reduction launches of the framework whose summation order is not ours.
// The sum, the same for every loss: term t_i in fp64 (below), i = 0 .. n - 1;
//   chain l (0 <= l < 256):  S_l = (((0.0 + t_l) + t_{l + 256}) + t_{l + 512}) + ...    over i = l (mod 256), i ascending
//                            (a chain without a term is 0.0)
//   tree:                    for s = 128, 64, .., 1:  S_l = S_l + S_{l + s}  for every l < s
//   loss = float(S_0 / double(n))                      one fp64 division, rounded to fp32 once
// every + one fp64 addition, nothing contracted.  n alone fixes the order: the 256 chains are the lanes of workgroup 0, which forms the
// sums of any launch; the other workgroups only write gradients.  No atomics, so the same inputs give the same bits.
//   critic c:  e = double(q_c[i]) - double(tv[i]);  t_i = e * e
//              grad_q_c[i] = (q_c[i] - tv[i]) * k2n            fp32: one subtraction, one multiplication, k2n = float(2.0 / double(n))
//   actor:     m = alpha * double(logp[i]);  t_i = m - double(qn[i])
//              grad_logp[i] = alpha / double(n)                (logp fp64), float(alpha / double(n)) (logp fp32)
//              grad_qn[i] = float(-1.0 / double(n))
//              alpha: a launch argument, or (alpha_dev, the learnt temperature of f110_temperature.h) one fp64 load, with alpha / double(n)
//              then divided on the device: IEEE division, the host's bits
// Where n is a power of two each gradient is what autograd gives for the framework's expression, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "f110_sacloss_plan.h"

#pragma clang fp contract(off)

namespace f110 {

// the tree over the chains of workgroup 0 -> S_0 in s[0] (every lane calls it)
__device__ inline void sacloss_tree(double *s, int tid)
{
    __syncthreads();
    for (int w = SL_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) s[tid] = s[tid] + s[tid + w];
        __syncthreads();
    }
}

static __global__ __launch_bounds__(SL_THREADS) void sac_critic_loss_kernel(SaclossArgs a)
{
    __shared__ double s1[SL_THREADS], s2[SL_THREADS];
    const int tid = threadIdx.x;
    for (long long i = (long long)blockIdx.x * SL_THREADS + tid; i < a.n; i += (long long)gridDim.x * SL_THREADS) {
        const float tv = a.tv[i];
        if (a.grad_q1) { const float d = a.q1[i] - tv; a.grad_q1[i] = d * a.k2n; }
        if (a.grad_q2) { const float d = a.q2[i] - tv; a.grad_q2[i] = d * a.k2n; }
    }
    if (blockIdx.x != 0) return;
    double c1 = 0.0, c2 = 0.0;
    for (long long i = tid; i < a.n; i += SL_THREADS) {
        const double tv = (double)a.tv[i];
        const double e1 = (double)a.q1[i] - tv, e2 = (double)a.q2[i] - tv;
        const double t1 = e1 * e1, t2 = e2 * e2;
        c1 = c1 + t1;
        c2 = c2 + t2;
    }
    s1[tid] = c1;
    s2[tid] = c2;
    sacloss_tree(s1, tid);
    sacloss_tree(s2, tid);
    if (tid == 0) {
        a.loss[0] = (float)(s1[0] / (double)a.n);
        a.loss[1] = (float)(s2[0] / (double)a.n);
    }
}

// The critic loss under importance weights (prioritized replay): t_i = double(w[i]) * (e * e), grad_q_c[i] = ((q_c[i] - tv[i]) * k2n) * w[i],
// td_out[i] = max |q_c[i] - tv[i]| in fp32.  The same chains, tree and division; a kernel of its own beside the unweighted one.
static __global__ __launch_bounds__(SL_THREADS) void sac_critic_loss_weighted_kernel(SaclossArgs a)
{
    __shared__ double s1[SL_THREADS], s2[SL_THREADS];
    const int tid = threadIdx.x;
    for (long long i = (long long)blockIdx.x * SL_THREADS + tid; i < a.n; i += (long long)gridDim.x * SL_THREADS) {
        const float tv = a.tv[i], w = a.w[i];
        const float d1 = a.q1[i] - tv, d2 = a.q2[i] - tv;
        if (a.grad_q1) { const float g = d1 * a.k2n; a.grad_q1[i] = g * w; }
        if (a.grad_q2) { const float g = d2 * a.k2n; a.grad_q2[i] = g * w; }
        if (a.td_out) a.td_out[i] = fmaxf(fabsf(d1), fabsf(d2));
    }
    if (blockIdx.x != 0) return;
    double c1 = 0.0, c2 = 0.0;
    for (long long i = tid; i < a.n; i += SL_THREADS) {
        const double tv = (double)a.tv[i], w = (double)a.w[i];
        const double e1 = (double)a.q1[i] - tv, e2 = (double)a.q2[i] - tv;
        const double x1 = e1 * e1, x2 = e2 * e2;
        const double t1 = w * x1, t2 = w * x2;
        c1 = c1 + t1;
        c2 = c2 + t2;
    }
    s1[tid] = c1;
    s2[tid] = c2;
    sacloss_tree(s1, tid);
    sacloss_tree(s2, tid);
    if (tid == 0) {
        a.loss[0] = (float)(s1[0] / (double)a.n);
        a.loss[1] = (float)(s2[0] / (double)a.n);
    }
}

template <bool F64> static __global__ __launch_bounds__(SL_THREADS) void sac_actor_loss_kernel(SaclossArgs a)
{
    __shared__ double s[SL_THREADS];
    const int tid = threadIdx.x;
    double alpha = a.alpha, glp64 = a.glp64;
    float glp32 = a.glp32;
    if (a.alpha_dev) {                                // (uniform in the launch) the host's three lines, on the device's alpha
        alpha = *a.alpha_dev;
        glp64 = alpha / (double)a.n;
        glp32 = (float)glp64;
    }
    for (long long i = (long long)blockIdx.x * SL_THREADS + tid; i < a.n; i += (long long)gridDim.x * SL_THREADS) {
        if (a.grad_logp) {
            if (F64) static_cast<double *>(a.grad_logp)[i] = glp64;
            else static_cast<float *>(a.grad_logp)[i] = glp32;
        }
        if (a.grad_qn) a.grad_qn[i] = a.gqn;
    }
    if (blockIdx.x != 0) return;
    double c = 0.0;
    for (long long i = tid; i < a.n; i += SL_THREADS) {
        const double lp = F64 ? static_cast<const double *>(a.logp)[i] : (double)static_cast<const float *>(a.logp)[i];
        const double m = alpha * lp;
        const double t = m - (double)a.qn[i];
        c = c + t;
    }
    s[tid] = c;
    sacloss_tree(s, tid);
    if (tid == 0) a.loss[0] = (float)(s[0] / (double)a.n);
}

} // namespace f110
