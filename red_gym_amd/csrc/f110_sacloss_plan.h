// f110_sacloss_plan.h -- the host side of the SAC losses (f110_sacloss.h): limits, the kernels' argument struct, the scalars the
// gradients are scaled with and the launch plan of both entry points.
// Plain C++17 without HIP (tests/test_sacloss_cpu.py compiles it for the host); f110_policy_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h"
#include "f110_launch.h"

#include <algorithm>
#include <cstring>

namespace f110 {

constexpr int SL_THREADS = 256;               // lanes of a workgroup = chains of the sum
constexpr int SL_MAX_GRID = 64;               // workgroups of a launch; each walks its share of the rows for the gradients
constexpr long long SL_MAX_ROWS = 1ll << 24;

struct SaclossArgs {
    long long n;
    const float *q1, *q2, *tv;      // critic loss: [n]
    const void *logp;               // actor loss: [n] double (logp_fp64) or float
    const float *qn;                // actor loss: [n]
    int logp_fp64;
    double alpha;
    float k2n;                      // float(2 / n): the critics' gradient is (q - tv) * k2n
    double glp64;                   // alpha / n
    float glp32, gqn;               // float(alpha / n), float(-1 / n)
    float *loss;                    // [2] (critic) or [1] (actor)
    float *grad_q1, *grad_q2;       // [n] or NULL
    void *grad_logp;                // [n] of logp's type, or NULL
    float *grad_qn;                 // [n] or NULL
    const double *alpha_dev;        // actor loss, f110_sac_actor_loss_alpha_dev: alpha is read here and alpha / n formed on the device;
                                    // NULL (every other entry): alpha, glp64 and glp32 above
    const float *w;                 // f110_sac_critic_loss_weighted: [n] the rows' importance weights
    float *td_out;                  // the same entry: [n] max |q_c - tv| or NULL
};

// One launch of sac_critic_loss_kernel (inst 0) or sac_actor_loss_kernel (inst 1 + logp_fp64) on 1 <= n <= SL_MAX_ROWS rows.  The
// grid only shares out the gradients' rows; workgroup 0 alone forms the sums, in an order that n fixes.
struct SaclossPlan { SaclossArgs a; Launch l; };

inline SaclossPlan sacloss_plan(int64_t n, bool actor, bool logp_fp64, double alpha)
{
    SaclossPlan p;
    memset(&p.a, 0, sizeof(p.a));
    p.a.n = n;
    p.a.logp_fp64 = logp_fp64 ? 1 : 0;
    p.a.alpha = alpha;
    p.a.k2n = (float)(2.0 / (double)n);
    p.a.glp64 = alpha / (double)n;
    p.a.glp32 = (float)p.a.glp64;
    p.a.gqn = (float)(-1.0 / (double)n);
    const long long groups = (n + SL_THREADS - 1) / SL_THREADS;
    p.l = {(unsigned)std::min<long long>(groups, SL_MAX_GRID), 1, 1, (unsigned)SL_THREADS, 0, actor ? 1 + p.a.logp_fp64 : 0};
    return p;
}

} // namespace f110
