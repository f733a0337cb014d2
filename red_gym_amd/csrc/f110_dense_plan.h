// f110_dense_plan.h -- the host side of the dense layer (f110_dense.h): limits, the kernels' argument struct, the checks of
// f110_dense_validate, the workspace size and the launch plans of both entry points.
// Plain C++17 without HIP (tests/test_dense_cpu.py compiles it for the host); f110_dense_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h" // f110_dense_config
#include "f110_launch.h"

#include <cstring>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int DN_MAX_K = 1 << 20, DN_MAX_H = 4096, DN_MAX_S = 4096;
constexpr long long DN_MAX_ROWS = 1LL << 24;
constexpr int DN_THREADS = 256;                 // four waves: wave w owns N-tile w of the workgroup's block against both M-tiles
constexpr int DN_BM = 32;                       // rows of the M side of a block: two M-tiles, the wave's two independent accumulators
constexpr int DN_BN = 64;                       // columns of the N side of a block: four N-tiles, one per wave
constexpr int DN_KC = 32;                       // terms of a chain staged at once: eight steps of 4
constexpr int DN_LDK = DN_KC + 4;               // floats between the rows of a tile staged [row][term]: the 16 rows x 4 terms a step reads lie in 64 banks
constexpr int DN_LDM = DN_BM + 16;              // floats between the terms of a tile staged [term][row of the M side]
constexpr int DN_LDN = DN_BN + 16;              // floats between the terms of a tile staged [term][column of the N side]
constexpr int DN_SPLIT_BELOW = 256;             // the forward with fewer blocks than this gives every segment a workgroup of its own
constexpr long long DN_MAX_GRID_X = 1LL << 28, DN_MAX_GRID_Y = 65535;   // workgroups of a launch: no kernel walks, the limits keep every grid inside these
// static LDS of the three GEMM kernels, bytes
constexpr int DN_FORWARD_LDS = (DN_BM + DN_BN) * DN_LDK * 4;
constexpr int DN_GRADX_LDS = (DN_BM * DN_LDK + DN_KC * DN_LDN) * 4;
constexpr int DN_GRADW_LDS = (DN_KC * DN_LDM + DN_KC * DN_LDN) * 4;
constexpr int DN_LDS_BYTES = 64 * 1024;         // of a workgroup: what a kernel may ask for without an attribute

struct DenseArgs {
    int K, H, ld, S, relu;
    int segs;                       // ceil(K / S)
    int chunks;                     // ceil(S / DN_KC): staged chunks of a full segment
    int mblocks, nblocks;           // blocks of the launch's GEMM along M and N
    int split;                      // forward: 1 = a workgroup per (block, segment), partials to P; 0 = a workgroup walks the segments
    int vec_x, vec_w, vec_g;        // 16-byte loads along a row of x / weight / grad_out and out: base and row stride allow them
    long long n;
    const float *x, *w, *bias, *out, *grad_out;
    float *dst;                     // out (forward), grad_x, or grad_weight
    float *P;                       // [segs][n][H]: the chains of the split forward
    float *grad_bias;
};

// What the entry points refuse, on the struct alone (no device).
inline int dense_check(const f110_dense_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->in_features < 1 || cfg->in_features > DN_MAX_K) return fail(F110_E_INVALID, "%s: in_features %d (1..%d)", who, cfg->in_features, DN_MAX_K);
    if (cfg->out_features < 1 || cfg->out_features > DN_MAX_H) return fail(F110_E_INVALID, "%s: out_features %d (1..%d)", who, cfg->out_features, DN_MAX_H);
    if (cfg->ld < cfg->in_features) return fail(F110_E_INVALID, "%s: ld %d below in_features %d", who, cfg->ld, cfg->in_features);
    if (cfg->segment < 4 || cfg->segment > DN_MAX_S || cfg->segment % 4) return fail(F110_E_INVALID, "%s: segment %d (a multiple of 4 in 4..%d)", who, cfg->segment, DN_MAX_S);
    if (cfg->reserved != 0) return fail(F110_E_INVALID, "%s: reserved %d (0)", who, cfg->reserved);
    return F110_OK;
}

inline bool dense_rows_ok(int64_t n) { return n >= 0 && n <= DN_MAX_ROWS; }

inline int dense_segments(const f110_dense_config &c) { return (c.in_features + c.segment - 1) / c.segment; }
inline long long dense_blocks(long long m, int per) { return (m + per - 1) / per; }

// the forward on n >= 1 rows gives every segment a workgroup of its own where the blocks alone would leave the device idle
inline bool dense_split(const f110_dense_config &c, int64_t n)
{
    return dense_segments(c) > 1 && dense_blocks(n, DN_BM) * dense_blocks(c.out_features, DN_BN) < DN_SPLIT_BELOW;
}

// bytes of the forward's workspace for n rows: P [segs][n][H] floats on the split path, 0 on the other
inline int64_t dense_workspace_bytes(const f110_dense_config &c, int64_t n)
{
    if (n < 1 || !dense_rows_ok(n) || !dense_split(c, n)) return 0;
    return (int64_t)dense_segments(c) * n * c.out_features * (int64_t)sizeof(float);
}

inline void dense_geometry(const f110_dense_config &c, int64_t n, DenseArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.K = c.in_features; a.H = c.out_features; a.ld = c.ld; a.S = c.segment; a.relu = c.relu ? 1 : 0;
    a.segs = dense_segments(c); a.chunks = (c.segment + DN_KC - 1) / DN_KC;
    a.n = n;
}

// f110_dense_forward on n >= 1 rows.  M = rows, N = h.  Split (gemm.inst = 1): dense_forward_kernel<true> on a grid of (segs, mblocks
// nblocks), then dense_sum_kernel over the n H outputs; else dense_forward_kernel<false> on (mblocks, nblocks) alone.
struct DenseForwardPlan { DenseArgs a; Launch gemm, sum; };

inline DenseForwardPlan dense_forward_plan(const f110_dense_config &c, int64_t n)
{
    DenseForwardPlan p;
    DenseArgs &a = p.a;
    dense_geometry(c, n, a);
    a.mblocks = (int)dense_blocks(n, DN_BM); a.nblocks = (int)dense_blocks(a.H, DN_BN);
    a.split = dense_split(c, n) ? 1 : 0;
    if (a.split) p.gemm = {(unsigned)a.segs, (unsigned)(a.mblocks * a.nblocks), 1, (unsigned)DN_THREADS, 0, 1};
    else p.gemm = {(unsigned)a.mblocks, (unsigned)a.nblocks, 1, (unsigned)DN_THREADS, 0, 0};
    p.sum = {a.split ? (unsigned)dense_blocks(n * a.H, DN_THREADS) : 0u, 1, 1, (unsigned)DN_THREADS, 0, 0};
    return p;
}

// f110_dense_backward on n >= 1 rows: dense_gradx_kernel (M = rows, N = k, the chain over h), dense_gradw_kernel (M = h, N = k, the
// chain over the rows) on grids of (mblocks, nblocks), and dense_gradb_kernel (a thread per h), each where its output is wanted.
struct DenseBackwardPlan { DenseArgs a; Launch gradx, gradw, gradb; int gx_mblocks, gx_nblocks, gw_mblocks, gw_nblocks; };

inline DenseBackwardPlan dense_backward_plan(const f110_dense_config &c, int64_t n)
{
    DenseBackwardPlan p;
    dense_geometry(c, n, p.a);
    p.gx_mblocks = (int)dense_blocks(n, DN_BM); p.gx_nblocks = (int)dense_blocks(p.a.K, DN_BN);
    p.gw_mblocks = (int)dense_blocks(p.a.H, DN_BM); p.gw_nblocks = p.gx_nblocks;
    p.gradx = {(unsigned)p.gx_mblocks, (unsigned)p.gx_nblocks, 1, (unsigned)DN_THREADS, 0, 0};
    p.gradw = {(unsigned)p.gw_mblocks, (unsigned)p.gw_nblocks, 1, (unsigned)DN_THREADS, 0, 0};
    p.gradb = {(unsigned)dense_blocks(p.a.H, 64), 1, 1, 64u, 0, 0};
    return p;
}

} // namespace f110
