// f110_policyhead_plan.h -- the host side of the policy head (f110_policyhead.h): limits, the kernels' argument struct, the checks
// of f110_policyhead_validate, the workspace layout and the launch plan of both entry points.
// Plain C++17 without HIP (tests/test_launch_plans_cpu.py compiles it for the host); f110_policy_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h" // f110_policyhead_config, F110_POLICYHEAD_SLICE_ROWS
#include "f110_launch.h"

#include <algorithm>
#include <cstring>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int PH_THREADS = 256;
constexpr int PH_ROWS = 64;                   // rows of a forward tile: 16 per wave
constexpr int PH_MAX_K = 4096, PH_MAX_A = 32;
constexpr long long PH_MAX_ROWS = 1ll << 24;      // of a call: every launch stays below 2^31 workgroups and 2^32 threads
constexpr int PH_LDS_BYTES = 64 * 1024;       // of a workgroup: what a kernel may ask for without an attribute
constexpr int PH_MAX_GRID = 512;              // workgroups of the forward launch; each walks its share of the tiles
constexpr int PH_PREFETCH = 64;               // columns of h a lane's loads run ahead of the multiply
constexpr int PH_GH_ROWS = 16;                // rows of a grad_h workgroup
constexpr int PH_SLICE = F110_POLICYHEAD_SLICE_ROWS;
constexpr double PH_HALF_LOG_2PI = 0.91893853320467274178;

struct PolicyheadArgs {
    int K, A, T;                    // in_features, action_dim, N-tiles per half
    int kc, chunks;                 // columns of K in LDS at a time, ceil(K / kc)
    int out_fp64;
    long long n, tiles;             // rows, ceil(n / PH_ROWS)
    const float *h, *w_mean, *b_mean, *w_log_std, *b_log_std, *eps;
    float *pre;                     // [n, 2A]
    void *action, *log_prob;        // [n, A], [n]: double or float
    // backward
    const void *grad_action, *grad_log_prob;
    const float *grad_pre;          // [n, 2A] or NULL: a gradient that arrives at pre itself
    float *gpre;                    // workspace [n, 2A]
    float *partial;                 // workspace [slices, 2A, K + 1]
    int slices;
    float *grad_h, *grad_w_mean, *grad_b_mean, *grad_w_log_std, *grad_b_log_std;
};

inline int policyhead_check(const f110_policyhead_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->in_features < 1 || cfg->in_features > PH_MAX_K) return fail(F110_E_INVALID, "%s: in_features %d (1..%d)", who, cfg->in_features, PH_MAX_K);
    if (cfg->action_dim < 1 || cfg->action_dim > PH_MAX_A) return fail(F110_E_INVALID, "%s: action_dim %d (1..%d)", who, cfg->action_dim, PH_MAX_A);
    return F110_OK;
}

// the launch geometry of a validated configuration (restated by tests/policyhead_cases.py paths)
inline void policyhead_geometry(const f110_policyhead_config &c, int64_t n, PolicyheadArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.K = c.in_features; a.A = c.action_dim; a.T = (a.A + 15) / 16; a.out_fp64 = c.out_fp64 ? 1 : 0;
    a.kc = std::min(PH_LDS_BYTES / (128 * a.T), (a.K + 63) / 64 * 64);
    a.chunks = (a.K + a.kc - 1) / a.kc;
    a.n = n; a.tiles = (n + PH_ROWS - 1) / PH_ROWS;
    a.slices = (int)((n + PH_SLICE - 1) / PH_SLICE);
}

// floats of g_pre in the workspace: [n, 2A], rounded up so that the partial sums behind it start 16-byte aligned
inline int64_t policyhead_gpre_floats(const f110_policyhead_config &c, int64_t n) { return (n * 2 * c.action_dim + 3) / 4 * 4; }

// bytes of f110_policyhead_backward's workspace for 1 <= n <= PH_MAX_ROWS rows: g_pre, then [slices, 2A, K + 1] floats
inline int64_t policyhead_workspace_bytes(const f110_policyhead_config &c, int64_t n)
{
    const int64_t slices = (n + PH_SLICE - 1) / PH_SLICE;
    return (policyhead_gpre_floats(c, n) + slices * 2 * c.action_dim * (c.in_features + 1)) * (int64_t)sizeof(float);
}

// f110_policyhead_forward on n >= 1 rows: one launch of policyhead_forward_kernel<T, out_fp64>, l.inst = 2 T + out_fp64 (a workgroup
// walks tiles grid apart, so one launch serves any n; its LDS stays within the 64 KiB every kernel may ask for)
struct PolicyheadForwardPlan { PolicyheadArgs a; Launch l; };

inline PolicyheadForwardPlan policyhead_forward_plan(const f110_policyhead_config &c, int64_t n)
{
    PolicyheadForwardPlan p;
    policyhead_geometry(c, n, p.a);
    p.l = {(unsigned)std::min<long long>(p.a.tiles, PH_MAX_GRID), 1, 1, (unsigned)PH_THREADS, (size_t)128 * p.a.T * p.a.kc, 2 * p.a.T + p.a.out_fp64};
    return p;
}

// f110_policyhead_backward: policyhead_gpre_kernel<out_fp64> (inst = out_fp64); policyhead_gradh_kernel where grad_h is wanted;
// policyhead_gradw_kernel and policyhead_reduce_kernel where a parameter gradient is.  gpre_at, partial_at: where in the
// workspace, in floats, a.gpre and a.partial lie.
struct PolicyheadBackwardPlan { PolicyheadArgs a; Launch gpre, gradh, gradw, reduce; int64_t gpre_at, partial_at; };

inline PolicyheadBackwardPlan policyhead_backward_plan(const f110_policyhead_config &c, int64_t n)
{
    PolicyheadBackwardPlan p;
    PolicyheadArgs &a = p.a;
    policyhead_geometry(c, n, a);
    p.gpre_at = 0; p.partial_at = policyhead_gpre_floats(c, n);
    p.gpre = {(unsigned)((n * a.A + PH_THREADS - 1) / PH_THREADS), 1, 1, (unsigned)PH_THREADS, 0, a.out_fp64};
    p.gradh = {(unsigned)((n + PH_GH_ROWS - 1) / PH_GH_ROWS), (unsigned)((a.K + PH_THREADS - 1) / PH_THREADS), 1, (unsigned)PH_THREADS, 0, 0};
    p.gradw = {(unsigned)a.slices, (unsigned)((a.K + 63) / 64 + 1), 1, 64, 0, 0};
    p.reduce = {(unsigned)((2 * a.A * (a.K + 1) + PH_THREADS - 1) / PH_THREADS), 1, 1, (unsigned)PH_THREADS, 0, 0};
    return p;
}

} // namespace f110
