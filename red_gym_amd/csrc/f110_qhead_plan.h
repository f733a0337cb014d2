// f110_qhead_plan.h -- the host side of the critic head (f110_qhead.h): limits, the kernels' argument struct, the checks of
// f110_qhead_validate, the workspace layout and the launch plan of both entry points.
// Plain C++17 without HIP (tests/test_launch_plans_cpu.py compiles it for the host); f110_policy_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h" // f110_qhead_config, F110_QHEAD_SLICE_ROWS
#include "f110_launch.h"

#include <algorithm>
#include <cstring>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int QH_THREADS = 256;
constexpr int QH_RPW = 2;                     // rows of a wave in the forward kernel: an LDS read of w_act feeds two chains
constexpr int QH_ROWS = 4 * QH_RPW;           // rows of a forward tile
constexpr int QH_BROWS = 4;                   // rows of a backward tile: one per wave
constexpr int QH_MAX_H = 4096, QH_MAX_A = 32, QH_MAX_C = 2;
constexpr long long QH_MAX_ROWS = 1ll << 24;
constexpr int QH_LDS_BYTES = 64 * 1024;       // of a workgroup: what a kernel may ask for without an attribute
constexpr int QH_MAX_GRID = 1024;             // workgroups of a row kernel; each walks its share of the tiles
constexpr int QH_SLICE = F110_QHEAD_SLICE_ROWS;

struct QheadArgs {
    int H, A, C, ld, act_fp64;
    int hc, chunks;                 // hidden units in LDS at a time (a multiple of 64), ceil(H / hc)
    long long n, tiles;             // rows, tiles of the launch
    int slices;
    const float *pre[QH_MAX_C], *w_act[QH_MAX_C], *b1[QH_MAX_C], *w2[QH_MAX_C], *b2[QH_MAX_C];
    const void *action, *nlp;       // [n, A], [n]: double or float
    const double *reward;
    const uint8_t *done;
    double gamma, alpha;
    float *q, *qmin, *target;       // forward outputs
    // backward
    const float *q_in, *grad_q, *grad_qmin;
    float *grad_pre[QH_MAX_C], *grad_w_act[QH_MAX_C], *grad_b1[QH_MAX_C], *grad_w2[QH_MAX_C], *grad_b2[QH_MAX_C];
    void *grad_action;
    float *partial;                 // workspace [C][slices][H (A + 2) + 1]
    const double *alpha_dev;        // forward, f110_qhead_forward_alpha_dev: the target's alpha is read here; NULL: `alpha` above
    const double *discount_dev;     // forward, f110_qhead_forward_rows: [n], row b's discount in gamma's place; NULL: `gamma` above
};

// floats of one (critic, slice) in the workspace: grad_w_act [H][A], grad_b1 [H], grad_w2 [H], grad_b2
F110_HD inline size_t qhead_partial_floats(int H, int A) { return (size_t)H * (size_t)(A + 2) + 1; }

inline int qhead_check(const f110_qhead_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->hidden < 1 || cfg->hidden > QH_MAX_H) return fail(F110_E_INVALID, "%s: hidden %d (1..%d)", who, cfg->hidden, QH_MAX_H);
    if (cfg->action_dim < 1 || cfg->action_dim > QH_MAX_A) return fail(F110_E_INVALID, "%s: action_dim %d (1..%d)", who, cfg->action_dim, QH_MAX_A);
    if (cfg->critics < 1 || cfg->critics > QH_MAX_C) return fail(F110_E_INVALID, "%s: %d critics (1..%d)", who, cfg->critics, QH_MAX_C);
    if (cfg->ld < cfg->action_dim) return fail(F110_E_INVALID, "%s: ld %d is below action_dim %d", who, cfg->ld, cfg->action_dim);
    return F110_OK;
}

// the launch geometry of a validated configuration (restated by tests/qhead_cases.py paths) -> LDS bytes of a row kernel
inline size_t qhead_geometry(const f110_qhead_config &c, int64_t n, int rows_per_tile, QheadArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.H = c.hidden; a.A = c.action_dim; a.C = c.critics; a.ld = c.ld; a.act_fp64 = c.action_fp64 ? 1 : 0;
    a.hc = std::min((QH_LDS_BYTES / 4 - a.A) / (a.A + 2) / 64 * 64, (a.H + 63) / 64 * 64);
    a.chunks = (a.H + a.hc - 1) / a.hc;
    a.n = n; a.tiles = (n + rows_per_tile - 1) / rows_per_tile;
    a.slices = (int)((n + QH_SLICE - 1) / QH_SLICE);
    return ((size_t)a.A * (a.hc + 1) + 2 * (size_t)a.hc) * sizeof(float);
}

// bytes of f110_qhead_backward's workspace for 1 <= n <= QH_MAX_ROWS rows: [C][slices] partials, rounded up to 4 floats
inline int64_t qhead_workspace_bytes(const f110_qhead_config &c, int64_t n)
{
    const int64_t slices = (n + QH_SLICE - 1) / QH_SLICE;
    const int64_t floats = c.critics * slices * (int64_t)qhead_partial_floats(c.hidden, c.action_dim);
    return (floats + 3) / 4 * 4 * (int64_t)sizeof(float);
}

// f110_qhead_forward on n >= 1 rows: one launch of qhead_forward_kernel (a workgroup walks tiles grid apart, so one launch serves
// any n; its LDS stays within the 64 KiB every kernel may ask for)
struct QheadForwardPlan { QheadArgs a; Launch l; };

inline QheadForwardPlan qhead_forward_plan(const f110_qhead_config &c, int64_t n)
{
    QheadForwardPlan p;
    const size_t lds = qhead_geometry(c, n, QH_ROWS, p.a);
    p.l = {(unsigned)std::min<long long>(p.a.tiles, QH_MAX_GRID), 1, 1, (unsigned)QH_THREADS, lds, 0};
    return p;
}

// f110_qhead_backward: qhead_rows_kernel<inst> where a gradient per row is wanted; qhead_gradw_kernel<inst> and qhead_reduce_kernel
// where a parameter gradient is; inst = 16 for A <= 16, else 32.  partial_at: where in the workspace, in floats, a.partial lies.
struct QheadBackwardPlan { QheadArgs a; Launch rows, gradw, reduce; int64_t partial_at; };

inline QheadBackwardPlan qhead_backward_plan(const f110_qhead_config &c, int64_t n)
{
    QheadBackwardPlan p;
    QheadArgs &a = p.a;
    const size_t lds = qhead_geometry(c, n, QH_BROWS, a);
    const int inst = a.A <= 16 ? 16 : 32;
    p.partial_at = 0;
    p.rows = {(unsigned)std::min<long long>(a.tiles, QH_MAX_GRID), 1, 1, (unsigned)QH_THREADS, lds, inst};
    p.gradw = {(unsigned)a.slices, (unsigned)((a.H + QH_THREADS - 1) / QH_THREADS), (unsigned)a.C, (unsigned)QH_THREADS, 0, inst};
    p.reduce = {(unsigned)((qhead_partial_floats(a.H, a.A) + QH_THREADS - 1) / QH_THREADS), (unsigned)a.C, 1, (unsigned)QH_THREADS, 0, 0};
    return p;
}

} // namespace f110
