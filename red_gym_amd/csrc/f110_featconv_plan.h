// f110_featconv_plan.h -- the host side of the dense convolution (f110_featconv.h): limits, the kernels' argument structs, the
// checks of f110_featconv_validate, the workspace size and the launch plan of both entry points.
// Plain C++17 without HIP (tests/test_launch_plans_cpu.py compiles it for the host); f110_featconv_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h" // f110_featconv_config
#include "f110_launch.h"

#include <algorithm>
#include <cstring>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int FC_MAX_K = 4, FC_MAX_S = 4, FC_MAX_CI = 32, FC_MAX_CO = 64, FC_MAX_KTOT = 512, FC_MAX_W = 64;
constexpr int FC_THREADS = 256;
constexpr int FC_CHUNK = 8;                    // steps of 4 in a chunk of K
constexpr int FC_ACCS = 4;                     // M-tiles a wave accumulates at once
constexpr int FC_STAGE = 8;                    // planes a lane stages at once: that many loads in flight
constexpr int FC_ZERO_BYTES = 16;              // zeros in front of the staged data: what a padding term reads (index -1)
constexpr int FC_LDS_BYTES = 64 * 1024;        // of a workgroup: what a kernel may ask for without an attribute
constexpr int FC_MAX_GRID = 2048;              // workgroups of a launch in x; each walks its share of the items
constexpr int FCW_TILES = 8;                   // N-tiles of a workgroup of featconv_gradw_kernel, two per wave
constexpr int FCW_MAX_MT = FC_MAX_CO / 16;

// One GEMM over planes: the forward (C = Ci planes of x, N = Co) or grad_x (C = Co planes of g, N = Ci).
struct FeatconvGemm {
    int C, N;                       // staged planes, output channels
    int ktot, chunks;               // C k k and ceil(ktot / (4 FC_CHUNK))
    int PH, PW;                     // the output plane
    int ms;                         // distance in the planes between the windows of neighbouring output pixels
    int XW;                         // columns of a staged plane
    int BR, bands, NR;              // output rows of a band, bands of a sample, staged rows under a full band
    int planes_off;                 // byte offset of the planes in the workgroup's LDS: koff[32 chunks], FC_ZERO_BYTES of zeros, the planes
    long long items;                // n * bands
};

struct FeatconvArgs {
    int Ci, H, W, Co, k, s, relu, OH, OW;
    FeatconvGemm g;
    // stage 1 of grad_weight
    int wBR, wbands, wNR, wXW, wGP; // output rows of a band, bands, staged rows and columns of x, pixels of a full band
    int wktot, wNT, wMT;            // Ci k k, its N-tiles, the M-tiles of Co
    int xs_at;                      // float index of the x planes in the workgroup's LDS: FC_ZERO_BYTES of zeros, g, x
    long long n;
    const float *x, *out, *grad_out, *w, *bias;
    float *dst;                     // out (forward) or grad_x
    float *P;                       // [n][Co ktot + Co]
};

// What the entry points refuse, on the struct alone (no device).
inline int featconv_check(const f110_featconv_config *cfg, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->kernel < 1 || cfg->kernel > FC_MAX_K) return fail(F110_E_INVALID, "%s: kernel %d (1..%d)", who, cfg->kernel, FC_MAX_K);
    if (cfg->stride < 1 || cfg->stride > FC_MAX_S) return fail(F110_E_INVALID, "%s: stride %d (1..%d)", who, cfg->stride, FC_MAX_S);
    if (cfg->in_channels < 1 || cfg->in_channels > FC_MAX_CI) return fail(F110_E_INVALID, "%s: %d input channels (1..%d)", who, cfg->in_channels, FC_MAX_CI);
    if (cfg->out_channels < 1 || cfg->out_channels > FC_MAX_CO) return fail(F110_E_INVALID, "%s: %d output channels (1..%d)", who, cfg->out_channels, FC_MAX_CO);
    const int kk = cfg->kernel * cfg->kernel;
    if (cfg->in_channels * kk > FC_MAX_KTOT) return fail(F110_E_INVALID, "%s: in_channels * kernel^2 = %d (at most %d)", who, cfg->in_channels * kk, FC_MAX_KTOT);
    if (cfg->out_channels * kk > FC_MAX_KTOT) return fail(F110_E_INVALID, "%s: out_channels * kernel^2 = %d (at most %d)", who, cfg->out_channels * kk, FC_MAX_KTOT);
    if (cfg->rows < cfg->kernel) return fail(F110_E_INVALID, "%s: %d rows (at least kernel = %d)", who, cfg->rows, cfg->kernel);
    if (cfg->cols < cfg->kernel || cfg->cols > FC_MAX_W)
        return fail(F110_E_INVALID, "%s: %d columns (kernel = %d .. %d: a band is whole rows)", who, cfg->cols, cfg->kernel, FC_MAX_W);
    return F110_OK;
}

// bytes of f110_featconv_backward's workspace for n >= 1 samples: P is [n][Co ktot + Co] floats (0 where the count does not fit)
inline int64_t featconv_workspace_bytes(const f110_featconv_config &c, int64_t n)
{
    const int64_t row = c.out_channels * (int64_t)(c.in_channels * c.kernel * c.kernel + 1) * (int64_t)sizeof(float);
    return n > INT64_MAX / row ? 0 : n * row;
}

// bytes in front of the planes of a GEMM: koff for whole chunks of K, then the zeros a padding term reads
inline size_t featconv_planes_off(int chunks) { return (size_t)chunks * 4 * FC_CHUNK * sizeof(int) + FC_ZERO_BYTES; }
inline size_t featconv_gemm_lds(int chunks, int planes, int nr, int xw) { return featconv_planes_off(chunks) + (size_t)planes * nr * xw * sizeof(float); }

// bytes of the zeros and g [Co][br OW] in front of the x planes of stage 1, rounded up to 16
inline size_t featconv_gradw_gs(const f110_featconv_config &c, int br, int ow) { return FC_ZERO_BYTES + ((size_t)c.out_channels * br * ow * sizeof(float) + 15) / 16 * 16; }

// the launch geometry of a validated configuration (restated by tests/featconv_cases.py paths)
inline void featconv_geometry(const f110_featconv_config &c, FeatconvArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.Ci = c.in_channels; a.H = c.rows; a.W = c.cols; a.Co = c.out_channels; a.k = c.kernel; a.s = c.stride; a.relu = c.relu ? 1 : 0;
    a.OH = (a.H - a.k) / a.s + 1; a.OW = (a.W - a.k) / a.s + 1;
}

// the forward's bands -> LDS bytes
inline size_t featconv_forward_geometry(FeatconvArgs &a, int64_t n)
{
    FeatconvGemm &g = a.g;
    g.C = a.Ci; g.N = a.Co; g.ktot = a.Ci * a.k * a.k; g.chunks = (g.ktot + 4 * FC_CHUNK - 1) / (4 * FC_CHUNK);
    g.PH = a.OH; g.PW = a.OW; g.ms = a.s; g.XW = (a.OW - 1) * a.s + a.k;
    g.BR = 1;
    while (g.BR < g.PH && featconv_gemm_lds(g.chunks, g.C, g.BR * a.s + a.k, g.XW) <= (size_t)FC_LDS_BYTES) g.BR++;
    g.bands = (g.PH + g.BR - 1) / g.BR; g.NR = (g.BR - 1) * a.s + a.k;
    g.items = (long long)n * g.bands; g.planes_off = (int)featconv_planes_off(g.chunks);
    return featconv_gemm_lds(g.chunks, g.C, g.NR, g.XW);
}

// grad_x's bands (rows of the input) -> LDS bytes
inline size_t featconv_gradx_geometry(FeatconvArgs &a, int64_t n)
{
    FeatconvGemm &g = a.g;
    g.C = a.Co; g.N = a.Ci; g.ktot = a.Co * a.k * a.k; g.chunks = (g.ktot + 4 * FC_CHUNK - 1) / (4 * FC_CHUNK);
    g.PH = a.H; g.PW = a.W; g.ms = 1; g.XW = a.W + a.k - 1;
    g.BR = 1;
    while (g.BR < g.PH && featconv_gemm_lds(g.chunks, g.C, g.BR + a.k, g.XW) <= (size_t)FC_LDS_BYTES) g.BR++;
    g.bands = (g.PH + g.BR - 1) / g.BR; g.NR = g.BR + a.k - 1;
    g.items = (long long)n * g.bands; g.planes_off = (int)featconv_planes_off(g.chunks);
    return featconv_gemm_lds(g.chunks, g.C, g.NR, g.XW);
}

// stage 1 of grad_weight: bands of output rows -> LDS bytes
inline size_t featconv_gradw_geometry(const f110_featconv_config &c, FeatconvArgs &a)
{
    a.wXW = (a.OW - 1) * a.s + a.k;
    a.wktot = a.Ci * a.k * a.k; a.wNT = (a.wktot + 15) / 16; a.wMT = (a.Co + 15) / 16;
    auto lds = [&](int br) { return featconv_gradw_gs(c, br, a.OW) + (size_t)a.Ci * ((br - 1) * a.s + a.k) * a.wXW * sizeof(float); };
    a.wBR = 1;
    while (a.wBR < a.OH && lds(a.wBR + 1) <= (size_t)FC_LDS_BYTES) a.wBR++;
    a.wbands = (a.OH + a.wBR - 1) / a.wBR; a.wNR = (a.wBR - 1) * a.s + a.k; a.wGP = a.wBR * a.OW;
    a.xs_at = (int)(featconv_gradw_gs(c, a.wBR, a.OW) / sizeof(float));
    return lds(a.wBR);
}

// f110_featconv_forward on n >= 1 samples: one launch of featconv_gemm_kernel<false> (a workgroup walks items grid apart, so one
// launch serves any n; its LDS stays within the 64 KiB every kernel may ask for)
struct FeatconvForwardPlan { FeatconvArgs a; Launch l; };

inline FeatconvForwardPlan featconv_forward_plan(const f110_featconv_config &c, int64_t n)
{
    FeatconvForwardPlan p;
    featconv_geometry(c, p.a);
    const size_t lds = featconv_forward_geometry(p.a, n);
    p.a.n = n;
    p.l = {(unsigned)std::min<long long>(p.a.g.items, FC_MAX_GRID), 1, 1, (unsigned)FC_THREADS, lds, 0};
    return p;
}

// f110_featconv_backward: featconv_gemm_kernel<true> where grad_x is wanted (a.g is its GEMM); featconv_gradw_kernel<MT>
// (inst = MT = a.wMT) and featconv_reduce_kernel over the nw weights and Co biases where a parameter gradient is
struct FeatconvBackwardPlan { FeatconvArgs a; Launch gradx, partials, reduce; int nw; };

inline FeatconvBackwardPlan featconv_backward_plan(const f110_featconv_config &c, int64_t n)
{
    FeatconvBackwardPlan p;
    FeatconvArgs &a = p.a;
    featconv_geometry(c, a);
    a.n = n;
    const size_t gx_lds = featconv_gradx_geometry(a, n), gw_lds = featconv_gradw_geometry(c, a);
    p.nw = a.Co * a.wktot;
    p.gradx = {(unsigned)std::min<long long>(a.g.items, FC_MAX_GRID), 1, 1, (unsigned)FC_THREADS, gx_lds, 0};
    p.partials = {(unsigned)std::min<long long>(n, FC_MAX_GRID), (unsigned)((a.wNT + FCW_TILES - 1) / FCW_TILES), 1, (unsigned)FC_THREADS, gw_lds, a.wMT};
    p.reduce = {(unsigned)((p.nw + a.Co + FC_THREADS - 1) / FC_THREADS), 1, 1, (unsigned)FC_THREADS, 0, 0};
    return p;
}

} // namespace f110
