// f110_temperature.h -- SAC's entropy temperature learnt on the device: loss = -(log_alpha * mean(logp + target_entropy)), one Adam
// step on the one parameter log_alpha and alpha = exp(log_alpha), in ONE launch of ONE workgroup, in place of the four a framework
// takes (the loss, its backward, Adam on one element, exp).  alpha stays in device memory, where qhead_forward_kernel and
// sac_actor_loss_kernel read it (their alpha_dev argument), so a captured update replays with the temperature of its own step.
// The sum is the losses' (f110_sacloss.h): 256 chains over i mod 256 ascending and sacloss_tree; lane 0 then does the tail -- mean,
// loss, gradient, adam_advance and adam_element of f110_adam.h on the one element, the fp64 exp -- and writes the 64-byte state with
// plain stores.  Numerics: the contract of include/f110_hip.h; nothing contracted.
// Sizing: one workgroup so that n alone fixes the order; a lane's chain is n / 256 dependent fp64 additions behind one load each,
// which is the walk workgroup 0 of the actor loss makes over the same array.  An update's batch is 64 .. 4 096 rows (at most 16
// additions a lane); the kernel is not meant to be fast at 2^24.  2 KiB of LDS for the tree, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include "f110_adam.h"
#include "f110_sacloss.h"
#include "f110_temperature_plan.h"

#pragma clang fp contract(off)

namespace f110 {

static_assert(TP_THREADS == SL_THREADS, "the tree is the losses'");

// grid 1, block TP_THREADS
template <bool F64> static __global__ __launch_bounds__(TP_THREADS) void temperature_step_kernel(TemperatureArgs a)
{
    __shared__ double s[TP_THREADS];
    const int tid = threadIdx.x;
    double c = 0.0;
    for (long long i = tid; i < a.n; i += TP_THREADS) {
        const double lp = F64 ? static_cast<const double *>(a.logp)[i] : (double)static_cast<const float *>(a.logp)[i];
        const double t = lp + a.target_entropy;
        c = c + t;
    }
    s[tid] = c;
    sacloss_tree(s, tid);
    if (tid != 0) return;
    f110_temperature_state *st = a.state;
    const double mean = s[0] / (double)a.n;
    float p = st->log_alpha, m = st->m, v = st->v, unused = 0.0f;
    const float loss = (float)(-((double)p * mean));
    const float g = (float)(-mean);
    adam_advance(&st->adam, a.beta1, a.beta2, a.lr);
    AdamConsts k;
    k.c1 = a.c1; k.c2 = a.c2; k.b2 = a.b2; k.eps = a.eps; k.tau = 0.0f;
    k.k2 = st->adam.k2; k.a = st->adam.a;
    adam_element<true, false>(k, p, g, m, v, unused);
    st->alpha = exp((double)p);
    st->log_alpha = p;
    st->m = m;
    st->v = v;
    st->grad = g;
    st->loss = loss;
}

} // namespace f110
