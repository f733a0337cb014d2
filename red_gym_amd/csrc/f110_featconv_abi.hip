// f110_featconv_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_featconv.h"

// ---------------------------------------------------------------- dense convolution of feature maps, forward and backward
// What the entry points refuse, on the struct alone (no device).
extern "C" int f110_featconv_validate(const f110_featconv_config *cfg)
{
    const char *who = "f110_featconv_validate";
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

extern "C" int64_t f110_featconv_workspace(const f110_featconv_config *cfg, int64_t n)
{
    if (n < 1 || f110_featconv_validate(cfg) != F110_OK) return 0;
    const int64_t row = cfg->out_channels * (int64_t)(cfg->in_channels * cfg->kernel * cfg->kernel + 1) * (int64_t)sizeof(float);
    return n > INT64_MAX / row ? 0 : n * row;      // (0 as well where the count does not fit)
}

// bytes in front of the planes of a GEMM: koff for whole chunks of K, then the zeros a padding term reads
static size_t featconv_planes_off(int chunks) { return (size_t)chunks * 4 * FC_CHUNK * sizeof(int) + FC_ZERO_BYTES; }
static size_t featconv_gemm_lds(int chunks, int planes, int nr, int xw) { return featconv_planes_off(chunks) + (size_t)planes * nr * xw * sizeof(float); }

// bytes of the zeros and g [Co][br OW] in front of the x planes of stage 1, rounded up to 16
static size_t featconv_gradw_gs(const f110_featconv_config &c, int br, int ow) { return FC_ZERO_BYTES + ((size_t)c.out_channels * br * ow * sizeof(float) + 15) / 16 * 16; }

// the launch geometry of a validated configuration (restated by tests/featconv_cases.py paths)
static void featconv_geometry(const f110_featconv_config &c, FeatconvArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.Ci = c.in_channels; a.H = c.rows; a.W = c.cols; a.Co = c.out_channels; a.k = c.kernel; a.s = c.stride; a.relu = c.relu ? 1 : 0;
    a.OH = (a.H - a.k) / a.s + 1; a.OW = (a.W - a.k) / a.s + 1;
}

// the forward's bands -> LDS bytes
static size_t featconv_forward_geometry(FeatconvArgs &a, int64_t n)
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
static size_t featconv_gradx_geometry(FeatconvArgs &a, int64_t n)
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
static size_t featconv_gradw_geometry(const f110_featconv_config &c, FeatconvArgs &a)
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

extern "C" int f110_featconv_forward(const f110_featconv_config *cfg, const float *x, int64_t n, const float *weight, const float *bias, float *out,
                                     void *stream)
{
    const char *who = "f110_featconv_forward";
    if (int rc = f110_featconv_validate(cfg)) return rc;
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%lld samples", who, (long long)n);
    if (n == 0) return F110_OK;
    if (!x || !weight || !out) return fail(F110_E_INVALID, "%s: null pointer", who);
    std::vector<DevicePtr> ptrs = {{"x", x}, {"weight", weight}, {"out", out}};
    if (bias) ptrs.push_back({"bias", bias});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    FeatconvArgs a;
    featconv_geometry(*cfg, a);
    const size_t lds = featconv_forward_geometry(a, n);
    a.n = n; a.x = x; a.w = weight; a.bias = bias; a.dst = out;
    // (a workgroup walks items grid apart, so one launch serves any n; its LDS stays within the 64 KiB every kernel may ask for)
    const unsigned grid = (unsigned)std::min<long long>(a.g.items, FC_MAX_GRID);
    hipLaunchKernelGGL(featconv_gemm_kernel<false>, dim3(grid), dim3(FC_THREADS), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_featconv_backward(const f110_featconv_config *cfg, const float *x, const float *out, const float *grad_out, int64_t n,
                                      const float *weight, float *grad_x, float *grad_weight, float *grad_bias, float *workspace, void *stream)
{
    const char *who = "f110_featconv_backward";
    if (int rc = f110_featconv_validate(cfg)) return rc;
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%lld samples", who, (long long)n);
    if (n == 0) return F110_OK;
    const bool params = grad_weight || grad_bias;
    if (!grad_out || (cfg->relu && !out) || (grad_x && !weight) || (params && !x)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (params && !workspace) return fail(F110_E_INVALID, "%s: parameter gradients need the workspace", who);
    if ((uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
    std::vector<DevicePtr> ptrs = {{"grad_out", grad_out}};
    if (cfg->relu) ptrs.push_back({"out", out});
    if (grad_x) { ptrs.push_back({"weight", weight}); ptrs.push_back({"grad_x", grad_x}); }
    if (params) { ptrs.push_back({"x", x}); ptrs.push_back({"workspace", workspace}); }
    if (grad_weight) ptrs.push_back({"grad_weight", grad_weight});
    if (grad_bias) ptrs.push_back({"grad_bias", grad_bias});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    hipStream_t s = (hipStream_t)stream;
    FeatconvArgs a;
    featconv_geometry(*cfg, a);
    a.n = n; a.x = x; a.out = out; a.grad_out = grad_out; a.w = weight;
    if (grad_x) {
        const size_t lds = featconv_gradx_geometry(a, n);
        a.dst = grad_x;
        const unsigned grid = (unsigned)std::min<long long>(a.g.items, FC_MAX_GRID);
        hipLaunchKernelGGL(featconv_gemm_kernel<true>, dim3(grid), dim3(FC_THREADS), lds, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (params) {
        const size_t lds = featconv_gradw_geometry(*cfg, a);
        a.P = workspace;
        const dim3 grid((unsigned)std::min<long long>(n, FC_MAX_GRID), (unsigned)((a.wNT + FCW_TILES - 1) / FCW_TILES));
#define FEATCONV_GRADW(MT) hipLaunchKernelGGL(featconv_gradw_kernel<MT>, grid, dim3(FC_THREADS), lds, s, a)
        switch (a.wMT) { case 1: FEATCONV_GRADW(1); break; case 2: FEATCONV_GRADW(2); break; case 3: FEATCONV_GRADW(3); break; default: FEATCONV_GRADW(4); break; }
#undef FEATCONV_GRADW
        HIP_TRY(hipGetLastError());
        const int nw = a.Co * a.wktot;
        hipLaunchKernelGGL(featconv_reduce_kernel, dim3((unsigned)((nw + a.Co + FC_THREADS - 1) / FC_THREADS)), dim3(FC_THREADS), 0, s,
                           (const float *)workspace, (long long)n, nw, a.Co, grad_weight, grad_bias);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}
