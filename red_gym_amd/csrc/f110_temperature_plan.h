// f110_temperature_plan.h -- the host side of the temperature step (f110_temperature.h): the kernel's argument struct, the checks of
// f110_temperature_validate and f110_temperature_step that need no device, and the launch plan.
// Plain C++17 without HIP (tests/test_temperature_cpu.py compiles it for the host); f110_policy_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h"
#include "f110_launch.h"

#include <cmath>
#include <cstring>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int TP_THREADS = 256;               // lanes of the one workgroup = chains of the sum (SL_THREADS: the tree is the losses')
constexpr long long TP_MAX_ROWS = 1ll << 24;
static_assert(sizeof(f110_temperature_state) == 64 && sizeof(f110_adam_state) == 32, "the device state is 64 bytes, the Adam state its first 32");

struct TemperatureArgs {
    long long n;
    const void *logp;               // [n] double (logp_fp64) or float
    int logp_fp64;
    double target_entropy;
    double beta1, beta2, lr;        // of the state's advance
    float c1, c2, b2, eps;          // float(1 - beta1), float(1 - beta2), float(beta2), float(eps): the Adam contract's constants
    f110_temperature_state *state;
};

inline int temperature_check(const f110_temperature_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return fail(F110_E_INVALID, "%s: beta1 %g (0 <= beta1 < 1)", who, cfg->beta1);
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return fail(F110_E_INVALID, "%s: beta2 %g (0 <= beta2 < 1)", who, cfg->beta2);
    if (!std::isfinite(cfg->eps) || !(cfg->eps > 0.0)) return fail(F110_E_INVALID, "%s: eps %g (finite and > 0)", who, cfg->eps);
    if (!std::isfinite(cfg->target_entropy)) return fail(F110_E_INVALID, "%s: target_entropy is not finite", who);
    return F110_OK;
}

// what f110_temperature_step refuses before it asks the runtime where the pointers live
inline int temperature_step_check(const char *who, const f110_temperature_config *cfg, const void *logp, int32_t logp_fp64, int64_t n,
                                  const f110_temperature_state *state, double lr)
{
    if (int rc = temperature_check(cfg, who)) return rc;
    if (!logp) return fail(F110_E_INVALID, "%s: null logp", who);
    if (!state) return fail(F110_E_INVALID, "%s: null state", who);
    if (n < 1 || n > TP_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (1..%lld)", who, (long long)n, (long long)TP_MAX_ROWS);
    if (!std::isfinite(lr)) return fail(F110_E_INVALID, "%s: lr is not finite", who);
    if ((uintptr_t)logp % (logp_fp64 ? 8 : 4)) return fail(F110_E_INVALID, "%s: logp is not aligned to its type", who);
    if ((uintptr_t)state % 8) return fail(F110_E_INVALID, "%s: the state is not 8-byte aligned", who);
    return F110_OK;
}

// One launch of temperature_step_kernel<logp_fp64> (inst = logp_fp64): one workgroup whatever n, so that n alone fixes the sum's order.
struct TemperaturePlan { TemperatureArgs a; Launch l; };

inline TemperaturePlan temperature_plan(const f110_temperature_config &c, int64_t n, bool logp_fp64, double lr)
{
    TemperaturePlan p;
    memset(&p.a, 0, sizeof(p.a));
    p.a.n = n;
    p.a.logp_fp64 = logp_fp64 ? 1 : 0;
    p.a.target_entropy = c.target_entropy;
    p.a.beta1 = c.beta1; p.a.beta2 = c.beta2; p.a.lr = lr;
    p.a.c1 = (float)(1.0 - c.beta1); p.a.c2 = (float)(1.0 - c.beta2); p.a.b2 = (float)c.beta2; p.a.eps = (float)c.eps;
    p.l = {1u, 1u, 1u, (unsigned)TP_THREADS, 0, p.a.logp_fp64};
    return p;
}

} // namespace f110
