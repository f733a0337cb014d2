// f110_bitconv_plan.h -- the host side of the bit convolution (f110_bitconv.h) and of the fused stem (f110_bitconv2.h): limits, the
// kernels' argument structs, the checks of f110_bitconv_validate / f110_bitconv2_validate, and the launch plan of every entry point.
// Plain C++17 without HIP (tests/test_launch_plans_cpu.py compiles it for the host); f110_bitconv_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h" // f110_bitconv_config, f110_bitconv2_config
#include "f110_launch.h"
#include "f110_replay_bits.h"       // REPLAY_MAX_DIM, replay_words

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int BC_THREADS = 256;
constexpr int BC_TX = 64, BC_TY = 4;          // outputs of a tile: one wave per row
constexpr int BC_MAX_K = 8;                   // kernel * kernel taps fit one 64-bit mask
constexpr int BC_LROWS = (BC_TY - 1) * BC_MAX_K + BC_MAX_K;   // 32 image rows under a tile at most (stride <= kernel <= 8)
constexpr int BC_LWORDS = 9;                  // (63 + 63 * 8 + 8) bits from the first word's bit 0: 575 <= 9 * 64
constexpr int BC_CHUNK = 16;                  // channels one workgroup of the backward pass accumulates
constexpr int BC_MAX_PARTIALS = 1024;         // G at most
constexpr long long BC_FORWARD_GROUP = 1ll << 23; // workgroups of one forward launch at most: a launch has fewer than 2^32 threads

// STEP(K) for a kernel size K in 1..BC_MAX_K that is known when the code runs: the kernels are instantiated per size
#define BITCONV_BY_KERNEL(K, STEP) \
    switch (K) { case 1: STEP(1); break; case 2: STEP(2); break; case 3: STEP(3); break; case 4: STEP(4); break; \
                 case 5: STEP(5); break; case 6: STEP(6); break; case 7: STEP(7); break; default: STEP(8); break; }

struct BitconvArgs {
    f110_bitconv_config cfg;
    const uint64_t *frames;         // [n_frames, rows, W], or
    const uint8_t *images;          // [n_frames, rows, cols]
    long long n_frames;
    const long long *index;         // [n] or NULL
    long long first, n;             // forward: this launch computes images first .. first + gridDim.x / tiles - 1
    const float *grad_out;          // backward [n, C, OH, OW]
    float *ws;                      // backward [G, C, kernel^2] then [G, C]
    int OH, OW, W, tiles_x, tiles_y, G;
};

// What the entry points refuse, on the struct alone (no device).
inline int bitconv_check(const f110_bitconv_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->kernel < 1 || cfg->kernel > BC_MAX_K) return fail(F110_E_INVALID, "%s: kernel %d (1..%d: a window is one 64-bit mask)", who, cfg->kernel, BC_MAX_K);
    if (cfg->stride < 1 || cfg->stride > cfg->kernel) return fail(F110_E_INVALID, "%s: stride %d (1..kernel = %d)", who, cfg->stride, cfg->kernel);
    if (cfg->channels < 1 || cfg->channels > 64) return fail(F110_E_INVALID, "%s: %d channels (1..64)", who, cfg->channels);
    if (cfg->rows < cfg->kernel || cfg->cols < cfg->kernel || cfg->rows > REPLAY_MAX_DIM || cfg->cols > REPLAY_MAX_DIM)
        return fail(F110_E_INVALID, "%s: image of %d x %d pixels (kernel = %d .. %d)", who, cfg->rows, cfg->cols, cfg->kernel, REPLAY_MAX_DIM);
    if (!std::isfinite(cfg->on)) return fail(F110_E_INVALID, "%s: `on` is not finite", who);
    return F110_OK;
}

// the launch geometry of a validated configuration (restated by tests/bitconv_cases.py paths)
inline void bitconv_geometry(const f110_bitconv_config &c, BitconvArgs &a)
{
    a.cfg = c;
    a.OH = (c.rows - c.kernel) / c.stride + 1; a.OW = (c.cols - c.kernel) / c.stride + 1;
    a.W = replay_words(c.cols);
    a.tiles_x = (a.OW + BC_TX - 1) / BC_TX; a.tiles_y = (a.OH + BC_TY - 1) / BC_TY;
}

inline int bitconv_partials(const BitconvArgs &a, int64_t n)
{
    const int64_t tiles = n * a.tiles_x * a.tiles_y;
    return (int)std::min<int64_t>(tiles, BC_MAX_PARTIALS);
}

// bytes of f110_bitconv_backward's workspace for n >= 1 samples: [G, C, kernel^2] then [G, C] floats
inline int64_t bitconv_workspace_bytes(const f110_bitconv_config &c, int64_t n)
{
    BitconvArgs a;
    bitconv_geometry(c, a);
    return (int64_t)bitconv_partials(a, n) * c.channels * (c.kernel * c.kernel + 1) * (int64_t)sizeof(float);
}

// f110_bitconv_forward[_u8] on n >= 1 samples: bitconv_forward_kernel<K, U8>, l.inst = 2 K + U8, once per group with a.first = first
// and l.gx = grid (images go in groups of at most BC_FORWARD_GROUP workgroups)
struct BitconvGroup { long long first; unsigned grid; };
struct BitconvForwardPlan { BitconvArgs a; Launch l; std::vector<BitconvGroup> groups; };

inline BitconvForwardPlan bitconv_forward_plan(const f110_bitconv_config &c, bool u8, int64_t n)
{
    BitconvForwardPlan p;
    memset(&p.a, 0, sizeof(p.a));
    bitconv_geometry(c, p.a);
    p.a.n = n;
    p.l = {0, 1, 1, (unsigned)BC_THREADS, 0, 2 * c.kernel + (u8 ? 1 : 0)};
    const int64_t per = (int64_t)p.a.tiles_x * p.a.tiles_y, group = std::max<int64_t>(1, BC_FORWARD_GROUP / per);
    for (int64_t first = 0; first < n; first += group) p.groups.push_back({first, (unsigned)(std::min(group, n - first) * per)});
    return p;
}

// f110_bitconv_backward: bitconv_backward_kernel<K> (inst = K) on (G, chunks of channels), then bitconv_reduce_kernel<false> over the
// nw weights and C biases
struct BitconvBackwardPlan { BitconvArgs a; Launch partials, reduce; int nw; };

inline BitconvBackwardPlan bitconv_backward_plan(const f110_bitconv_config &c, int64_t n)
{
    BitconvBackwardPlan p;
    memset(&p.a, 0, sizeof(p.a));
    bitconv_geometry(c, p.a);
    p.a.n = n;
    p.a.G = bitconv_partials(p.a, n);
    p.nw = c.channels * c.kernel * c.kernel;
    p.partials = {(unsigned)p.a.G, (unsigned)((c.channels + BC_CHUNK - 1) / BC_CHUNK), 1, (unsigned)BC_THREADS, 0, c.kernel};
    p.reduce = {(unsigned)((p.nw + c.channels + BC_THREADS - 1) / BC_THREADS), 1, 1, (unsigned)BC_THREADS, 0, 0};
    return p;
}

// ---------------------------------------------------------------- the same layer on a stack of frames
constexpr int BCS_CHUNK = 4;                  // channels whose accumulators a lane of the stacked forward keeps at once: their
                                              // K * K weights each are wave-uniform and share the scalar registers (8 or 16 spill)

struct BitconvStackArgs {
    BitconvArgs a;                  // as the one-frame launch, with a.index = NULL: the frames are named by `index` below
    const long long *index;         // [n, stack]: frame of channel j of sample i
    int stack;                      // 1 .. F110_BITCONV_MAX_STACK
};

inline int bitconv_stack_check(int32_t stack, const char *who)
{
    if (stack < 1 || stack > F110_BITCONV_MAX_STACK) return fail(F110_E_INVALID, "%s: stack %d (1..%d)", who, stack, F110_BITCONV_MAX_STACK);
    return F110_OK;
}

// f110_bitconv_forward_stack on n >= 1 samples: bitconv_forward_stack_kernel<K>, l.inst = K, once per group as the one-frame forward
struct BitconvStackForwardPlan { BitconvStackArgs s; Launch l; std::vector<BitconvGroup> groups; };

inline BitconvStackForwardPlan bitconv_forward_stack_plan(const f110_bitconv_config &c, int stack, int64_t n)
{
    const BitconvForwardPlan one = bitconv_forward_plan(c, false, n);
    BitconvStackForwardPlan p;
    p.s.a = one.a; p.s.index = nullptr; p.s.stack = stack;
    p.l = one.l; p.l.inst = c.kernel;
    p.groups = one.groups;
    return p;
}

// f110_bitconv_backward_stack: the workspace is f110_bitconv_backward's partial sums (rounded up to 16 bytes), then the index
// transposed to [stack, n] int64; bitconv_index_columns_kernel fills the latter (one lane per entry), then per column j the one-frame
// plan's partials launch on column j and bitconv_reduce_kernel<true> (the one-frame reduce's grid) into grad_weight[:, j]
inline int64_t bitconv_stack_partial_bytes(const f110_bitconv_config &c, int64_t n) { return (bitconv_workspace_bytes(c, n) + 15) / 16 * 16; }
inline int64_t bitconv_stack_workspace_bytes(const f110_bitconv_config &c, int stack, int64_t n)
{
    return bitconv_stack_partial_bytes(c, n) + (int64_t)stack * n * (int64_t)sizeof(int64_t);
}

struct BitconvStackBackwardPlan { BitconvBackwardPlan one; Launch columns; int64_t index_offset; };

inline BitconvStackBackwardPlan bitconv_backward_stack_plan(const f110_bitconv_config &c, int stack, int64_t n)
{
    BitconvStackBackwardPlan p;
    p.one = bitconv_backward_plan(c, n);
    p.columns = {(unsigned)(((int64_t)stack * n + BC_THREADS - 1) / BC_THREADS), 1, 1, (unsigned)BC_THREADS, 0, 0};
    p.index_offset = bitconv_stack_partial_bytes(c, n);
    return p;
}

// ---------------------------------------------------------------- policy stem: conv1 + relu + conv2 from bits
constexpr int BC2_MAX_K2 = 4, BC2_MAX_C1 = 16, BC2_MAX_C2 = 64, BC2_MAX_OW1 = 64;
constexpr int BC2_KSTEPS = BC2_MAX_C1 * BC2_MAX_K2 * BC2_MAX_K2 / 4;     // 64 steps of 4 at most
constexpr int BC2_ACCS = 6;                    // M-tiles a wave accumulates at once
constexpr int BC2_LDS_BYTES = 64 * 1024;       // of a workgroup: what a kernel may ask for without an attribute; two fit a CU
constexpr int BC2_MAX_GRID = 2048;             // workgroups of a launch; each walks its share of the items

struct Bitconv2Args {
    BitconvArgs l1;                 // the first layer: cfg, frames / images, n_frames, index, n, OH, OW, W
    int u8;                         // images, not frames
    int k2, s2, C2, relu2;
    int OH2, OW2, XW;               // XW: columns of a1 that conv2 reads
    int BR, bands, NR1;             // output rows of a band, bands of a sample, conv1 rows under a full band
    int ktot, ksteps;               // C1 k2 k2 and ceil(ktot / 4)
    int a1_off, koff_off;           // byte offsets into the workgroup's LDS
    long long items;                // n * bands
};

inline f110_bitconv_config bitconv2_layer1_config(const f110_bitconv2_config &c)
{
    f110_bitconv_config l1;
    l1.rows = c.rows; l1.cols = c.cols; l1.kernel = c.kernel; l1.stride = c.stride; l1.channels = c.channels; l1.relu = c.relu; l1.on = c.on;
    return l1;
}

inline int bitconv2_check(const f110_bitconv2_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    const f110_bitconv_config l1 = bitconv2_layer1_config(*cfg);
    if (int rc = bitconv_check(&l1, "f110_bitconv_validate")) return rc;
    if (cfg->channels > BC2_MAX_C1) return fail(F110_E_INVALID, "%s: %d channels in the first layer (1..%d)", who, cfg->channels, BC2_MAX_C1);
    if (cfg->kernel2 < 1 || cfg->kernel2 > BC2_MAX_K2) return fail(F110_E_INVALID, "%s: kernel2 %d (1..%d)", who, cfg->kernel2, BC2_MAX_K2);
    if (cfg->stride2 < 1 || cfg->stride2 > cfg->kernel2) return fail(F110_E_INVALID, "%s: stride2 %d (1..kernel2 = %d)", who, cfg->stride2, cfg->kernel2);
    if (cfg->channels2 < 1 || cfg->channels2 > BC2_MAX_C2) return fail(F110_E_INVALID, "%s: %d channels in the second layer (1..%d)", who, cfg->channels2, BC2_MAX_C2);
    const int oh1 = (cfg->rows - cfg->kernel) / cfg->stride + 1, ow1 = (cfg->cols - cfg->kernel) / cfg->stride + 1;
    if (ow1 > BC2_MAX_OW1) return fail(F110_E_INVALID, "%s: the first layer's output is %d wide (at most %d: a band is whole rows)", who, ow1, BC2_MAX_OW1);
    if (oh1 < cfg->kernel2 || ow1 < cfg->kernel2)
        return fail(F110_E_INVALID, "%s: the first layer's output of %d x %d is smaller than kernel2 = %d", who, oh1, ow1, cfg->kernel2);
    return F110_OK;
}

// LDS bytes of a workgroup whose bands have `br` output rows; the offsets of koff and a1 in it
inline size_t bitconv2_lds(const f110_bitconv2_config &c, int br, int xw, int ksteps, int *koff_off, int *a1_off)
{
    const int nr1 = (br - 1) * c.stride2 + c.kernel2, img_rows = (nr1 - 1) * c.stride + c.kernel;
    const size_t words = (size_t)img_rows * BC_LWORDS * sizeof(uint64_t), koff = (size_t)BC2_KSTEPS * 4 * sizeof(int);
    if (koff_off) *koff_off = (int)words;
    if (a1_off) *a1_off = (int)(words + koff);
    return words + koff + (size_t)c.channels * nr1 * xw * sizeof(float);
}

// the launch geometry of a validated configuration (restated by tests/bitconv2_cases.py paths2)
inline size_t bitconv2_geometry(const f110_bitconv2_config &c, Bitconv2Args &a)
{
    memset(&a, 0, sizeof(a));
    bitconv_geometry(bitconv2_layer1_config(c), a.l1);
    a.k2 = c.kernel2; a.s2 = c.stride2; a.C2 = c.channels2; a.relu2 = c.relu2;
    a.OH2 = (a.l1.OH - a.k2) / a.s2 + 1; a.OW2 = (a.l1.OW - a.k2) / a.s2 + 1;
    a.XW = (a.OW2 - 1) * a.s2 + a.k2;
    a.ktot = c.channels * a.k2 * a.k2; a.ksteps = (a.ktot + 3) / 4;
    a.BR = 1;
    while (a.BR < a.OH2 && bitconv2_lds(c, a.BR + 1, a.XW, a.ksteps, nullptr, nullptr) <= (size_t)BC2_LDS_BYTES) a.BR++;
    a.bands = (a.OH2 + a.BR - 1) / a.BR;
    a.NR1 = (a.BR - 1) * a.s2 + a.k2;
    return bitconv2_lds(c, a.BR, a.XW, a.ksteps, &a.koff_off, &a.a1_off);
}

// f110_bitconv2_forward[_u8] on n >= 1 samples: one launch of bitconv2_forward_kernel<false> (a workgroup walks items grid apart, so one
// launch serves any n; its LDS stays below the 64 KiB every kernel may ask for)
struct Bitconv2Plan { Bitconv2Args a; Launch l; };

inline Bitconv2Plan bitconv2_forward_plan(const f110_bitconv2_config &c, bool u8, int64_t n)
{
    Bitconv2Plan p;
    const size_t lds = bitconv2_geometry(c, p.a);
    p.a.u8 = u8 ? 1 : 0;
    p.a.l1.n = n;
    p.a.items = (long long)n * p.a.bands;
    p.l = {(unsigned)std::min<long long>(p.a.items, BC2_MAX_GRID), 1, 1, (unsigned)BC_THREADS, lds, 0};
    return p;
}

// ---------------------------------------------------------------- the stem on a stack of frames
struct Bitconv2StackArgs {
    Bitconv2Args a;                 // as the one-frame launch, with a.l1.index = NULL and a.u8 = 0: the frames are named by `index` below
    const long long *index;         // [n, stack]: frame of channel j of sample i
    int stack;                      // 1 .. F110_BITCONV_MAX_STACK
};

// f110_bitconv2_forward_stack on n >= 1 samples: one launch of bitconv2_forward_kernel<true>.  The frames of a stack pass through the
// one-frame kernel's `words` one after the other and the running sums live in a1 itself, so the LDS, and with it the bands, are the
// one-frame plan's at every stack: nothing that plan accepts is refused here.
struct Bitconv2StackPlan { Bitconv2StackArgs s; Launch l; };

inline Bitconv2StackPlan bitconv2_forward_stack_plan(const f110_bitconv2_config &c, int stack, int64_t n)
{
    const Bitconv2Plan one = bitconv2_forward_plan(c, false, n);
    Bitconv2StackPlan p;
    p.s.a = one.a; p.s.index = nullptr; p.s.stack = stack;
    p.l = one.l;
    return p;
}

} // namespace f110
