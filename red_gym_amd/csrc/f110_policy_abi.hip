// f110_policy_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_bitconv.h"
#include "f110_bitconv2.h"
#include "f110_policyhead.h"
#include "f110_qhead.h"
#include "f110_adam.h"

// ---------------------------------------------------------------- first convolution from bits
// What the entry points refuse, on the struct alone (no device).
extern "C" int f110_bitconv_validate(const f110_bitconv_config *cfg)
{
    const char *who = "f110_bitconv_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->kernel < 1 || cfg->kernel > BC_MAX_K) return fail(F110_E_INVALID, "%s: kernel %d (1..%d: a window is one 64-bit mask)", who, cfg->kernel, BC_MAX_K);
    if (cfg->stride < 1 || cfg->stride > cfg->kernel) return fail(F110_E_INVALID, "%s: stride %d (1..kernel = %d)", who, cfg->stride, cfg->kernel);
    if (cfg->channels < 1 || cfg->channels > 64) return fail(F110_E_INVALID, "%s: %d channels (1..64)", who, cfg->channels);
    if (cfg->rows < cfg->kernel || cfg->cols < cfg->kernel || cfg->rows > REPLAY_MAX_DIM || cfg->cols > REPLAY_MAX_DIM)
        return fail(F110_E_INVALID, "%s: image of %d x %d pixels (kernel = %d .. %d)", who, cfg->rows, cfg->cols, cfg->kernel, REPLAY_MAX_DIM);
    if (!std::isfinite(cfg->on)) return fail(F110_E_INVALID, "%s: `on` is not finite", who);
    return F110_OK;
}

// the launch geometry of a validated configuration
static void bitconv_geometry(const f110_bitconv_config &c, BitconvArgs &a)
{
    a.cfg = c;
    a.OH = (c.rows - c.kernel) / c.stride + 1; a.OW = (c.cols - c.kernel) / c.stride + 1;
    a.W = replay_words(c.cols);
    a.tiles_x = (a.OW + BC_TX - 1) / BC_TX; a.tiles_y = (a.OH + BC_TY - 1) / BC_TY;
}

static int bitconv_partials(const BitconvArgs &a, int64_t n)
{
    const int64_t tiles = n * a.tiles_x * a.tiles_y;
    return (int)std::min<int64_t>(tiles, BC_MAX_PARTIALS);
}

extern "C" int64_t f110_bitconv_workspace(const f110_bitconv_config *cfg, int64_t n)
{
    if (n < 1 || f110_bitconv_validate(cfg) != F110_OK) return 0;
    BitconvArgs a;
    bitconv_geometry(*cfg, a);
    return (int64_t)bitconv_partials(a, n) * cfg->channels * (cfg->kernel * cfg->kernel + 1) * (int64_t)sizeof(float);
}

#define BITCONV_BY_KERNEL(K, LAUNCH) \
    switch (K) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; \
                 case 5: LAUNCH(5); break; case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(8); break; }

static int bitconv_forward(const char *who, const f110_bitconv_config *cfg, const void *src, bool u8, int64_t n_frames, const int64_t *index,
                           int64_t n, const float *weight, const float *bias, float *out, hipStream_t stream)
{
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    if (n < 0 || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (n == 0) return F110_OK;
    if (!weight || !out || (n_frames > 0 && !src)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!index && n > n_frames) return fail(F110_E_INVALID, "%s: %lld samples of %lld frames without an index", who, (long long)n, (long long)n_frames);
    if (!u8 && (uintptr_t)src % 8) return fail(F110_E_INVALID, "%s: frames must be 8-byte aligned", who);
    BitconvArgs a;
    memset(&a, 0, sizeof(a));
    bitconv_geometry(*cfg, a);
    if (u8) a.images = (const uint8_t *)src; else a.frames = (const uint64_t *)src;
    a.n_frames = n_frames; a.index = (const long long *)index; a.n = n;
    // a launch has fewer than 2^32 threads: images go in groups of at most 2^23 workgroups
    const int64_t per = (int64_t)a.tiles_x * a.tiles_y, group = std::max<int64_t>(1, ((int64_t)1 << 23) / per);
    for (int64_t first = 0; first < n; first += group) {
        a.first = first;
        const unsigned grid = (unsigned)(std::min(group, n - first) * per);
#define BITCONV_FWD(K) do { if (u8) hipLaunchKernelGGL((bitconv_forward_kernel<K, true>), dim3(grid), dim3(BC_THREADS), 0, stream, a, weight, bias, out); \
                            else hipLaunchKernelGGL((bitconv_forward_kernel<K, false>), dim3(grid), dim3(BC_THREADS), 0, stream, a, weight, bias, out); } while (0)
        BITCONV_BY_KERNEL(cfg->kernel, BITCONV_FWD)
#undef BITCONV_FWD
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

extern "C" int f110_bitconv_forward(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                                    const float *weight, const float *bias, float *out, void *stream)
{
    return bitconv_forward("f110_bitconv_forward", cfg, frames, false, n_frames, index, n, weight, bias, out, (hipStream_t)stream);
}

extern "C" int f110_bitconv_forward_u8(const f110_bitconv_config *cfg, const uint8_t *images, int64_t n_frames, const int64_t *index, int64_t n,
                                       const float *weight, const float *bias, float *out, void *stream)
{
    return bitconv_forward("f110_bitconv_forward_u8", cfg, images, true, n_frames, index, n, weight, bias, out, (hipStream_t)stream);
}

extern "C" int f110_bitconv_backward(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                                     const float *grad_out, float *grad_weight, float *grad_bias, float *workspace, void *stream)
{
    const char *who = "f110_bitconv_backward";
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    if (n < 1 || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (!grad_out || !grad_weight || !workspace || (n_frames > 0 && !frames)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!index && n > n_frames) return fail(F110_E_INVALID, "%s: %lld samples of %lld frames without an index", who, (long long)n, (long long)n_frames);
    if ((uintptr_t)frames % 8 || (uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: frames must be 8-byte and the workspace 16-byte aligned", who);
    BitconvArgs a;
    memset(&a, 0, sizeof(a));
    bitconv_geometry(*cfg, a);
    a.frames = frames; a.n_frames = n_frames; a.index = (const long long *)index; a.n = n; a.grad_out = grad_out; a.ws = workspace;
    a.G = bitconv_partials(a, n);
    const dim3 grid((unsigned)a.G, (unsigned)((cfg->channels + BC_CHUNK - 1) / BC_CHUNK));
#define BITCONV_BWD(K) hipLaunchKernelGGL((bitconv_backward_kernel<K>), grid, dim3(BC_THREADS), 0, (hipStream_t)stream, a)
    BITCONV_BY_KERNEL(cfg->kernel, BITCONV_BWD)
#undef BITCONV_BWD
    HIP_TRY(hipGetLastError());
    const int nw = cfg->channels * cfg->kernel * cfg->kernel;
    hipLaunchKernelGGL(bitconv_reduce_kernel, dim3((unsigned)((nw + cfg->channels + BC_THREADS - 1) / BC_THREADS)), dim3(BC_THREADS), 0, (hipStream_t)stream,
                       (const float *)workspace, a.G, nw, cfg->channels, cfg->on, grad_weight, grad_bias);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- policy stem: conv1 + relu + conv2 from bits
static f110_bitconv_config bitconv2_layer1_config(const f110_bitconv2_config &c)
{
    f110_bitconv_config l1;
    l1.rows = c.rows; l1.cols = c.cols; l1.kernel = c.kernel; l1.stride = c.stride; l1.channels = c.channels; l1.relu = c.relu; l1.on = c.on;
    return l1;
}

extern "C" int f110_bitconv2_validate(const f110_bitconv2_config *cfg)
{
    const char *who = "f110_bitconv2_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    const f110_bitconv_config l1 = bitconv2_layer1_config(*cfg);
    if (int rc = f110_bitconv_validate(&l1)) return rc;
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
static size_t bitconv2_lds(const f110_bitconv2_config &c, int br, int xw, int ksteps, int *koff_off, int *a1_off)
{
    const int nr1 = (br - 1) * c.stride2 + c.kernel2, img_rows = (nr1 - 1) * c.stride + c.kernel;
    const size_t words = (size_t)img_rows * BC_LWORDS * sizeof(uint64_t), koff = (size_t)BC2_KSTEPS * 4 * sizeof(int);
    if (koff_off) *koff_off = (int)words;
    if (a1_off) *a1_off = (int)(words + koff);
    return words + koff + (size_t)c.channels * nr1 * xw * sizeof(float);
}

// the launch geometry of a validated configuration (restated by tests/bitconv2_cases.py paths2)
static size_t bitconv2_geometry(const f110_bitconv2_config &c, Bitconv2Args &a)
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

static int bitconv2_forward(const char *who, const f110_bitconv2_config *cfg, const void *src, bool u8, int64_t n_frames, const int64_t *index,
                            int64_t n, const float *w1, const float *b1, const float *w2, const float *b2, float *out, hipStream_t stream)
{
    if (int rc = f110_bitconv2_validate(cfg)) return rc;
    if (n < 0 || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (n == 0) return F110_OK;
    if (!w1 || !w2 || !out || !src) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!index && n > n_frames) return fail(F110_E_INVALID, "%s: %lld samples of %lld frames without an index", who, (long long)n, (long long)n_frames);
    if (!u8 && (uintptr_t)src % 8) return fail(F110_E_INVALID, "%s: frames must be 8-byte aligned", who);
    Bitconv2Args a;
    const size_t lds = bitconv2_geometry(*cfg, a);
    if (u8) a.l1.images = (const uint8_t *)src; else a.l1.frames = (const uint64_t *)src;
    a.u8 = u8 ? 1 : 0;
    a.l1.n_frames = n_frames; a.l1.index = (const long long *)index; a.l1.n = n;
    a.items = (long long)n * a.bands;
    // (a workgroup walks items grid apart, so one launch serves any n; its LDS stays below the 64 KiB every kernel may ask for)
    const unsigned grid = (unsigned)std::min<long long>(a.items, BC2_MAX_GRID);
    hipLaunchKernelGGL(bitconv2_forward_kernel, dim3(grid), dim3(BC_THREADS), lds, stream, a, w1, b1, w2, b2, out);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_bitconv2_forward(const f110_bitconv2_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                                     const float *w1, const float *b1, const float *w2, const float *b2, float *out, void *stream)
{
    return bitconv2_forward("f110_bitconv2_forward", cfg, frames, false, n_frames, index, n, w1, b1, w2, b2, out, (hipStream_t)stream);
}

extern "C" int f110_bitconv2_forward_u8(const f110_bitconv2_config *cfg, const uint8_t *images, int64_t n_frames, const int64_t *index, int64_t n,
                                        const float *w1, const float *b1, const float *w2, const float *b2, float *out, void *stream)
{
    return bitconv2_forward("f110_bitconv2_forward_u8", cfg, images, true, n_frames, index, n, w1, b1, w2, b2, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------- policy head: fc_mean, fc_log_std and the sampling tail
extern "C" int f110_policyhead_validate(const f110_policyhead_config *cfg)
{
    const char *who = "f110_policyhead_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->in_features < 1 || cfg->in_features > PH_MAX_K) return fail(F110_E_INVALID, "%s: in_features %d (1..%d)", who, cfg->in_features, PH_MAX_K);
    if (cfg->action_dim < 1 || cfg->action_dim > PH_MAX_A) return fail(F110_E_INVALID, "%s: action_dim %d (1..%d)", who, cfg->action_dim, PH_MAX_A);
    return F110_OK;
}

// the launch geometry of a validated configuration (restated by tests/policyhead_cases.py paths)
static void policyhead_geometry(const f110_policyhead_config &c, int64_t n, PolicyheadArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.K = c.in_features; a.A = c.action_dim; a.T = (a.A + 15) / 16; a.out_fp64 = c.out_fp64 ? 1 : 0;
    a.kc = std::min(PH_LDS_BYTES / (128 * a.T), (a.K + 63) / 64 * 64);
    a.chunks = (a.K + a.kc - 1) / a.kc;
    a.n = n; a.tiles = (n + PH_ROWS - 1) / PH_ROWS;
    a.slices = (int)((n + PH_SLICE - 1) / PH_SLICE);
}

// floats of g_pre in the workspace: [n, 2A], rounded up so that the partial sums behind it start 16-byte aligned
static int64_t policyhead_gpre_floats(const f110_policyhead_config &c, int64_t n) { return (n * 2 * c.action_dim + 3) / 4 * 4; }

extern "C" int64_t f110_policyhead_workspace(const f110_policyhead_config *cfg, int64_t n)
{
    if (n < 1 || n > PH_MAX_ROWS || f110_policyhead_validate(cfg) != F110_OK) return 0;
    const int64_t slices = (n + PH_SLICE - 1) / PH_SLICE;
    return (policyhead_gpre_floats(*cfg, n) + slices * 2 * cfg->action_dim * (cfg->in_features + 1)) * (int64_t)sizeof(float);
}

extern "C" int f110_policyhead_forward(const f110_policyhead_config *cfg, const float *h, int64_t n, const float *w_mean, const float *b_mean,
                                       const float *w_log_std, const float *b_log_std, const float *eps, float *pre, void *action, void *log_prob,
                                       void *stream)
{
    const char *who = "f110_policyhead_forward";
    if (int rc = f110_policyhead_validate(cfg)) return rc;
    if (n < 0 || n > PH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)PH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!h || !w_mean || !w_log_std || !pre || !action) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((eps == nullptr) != (log_prob == nullptr)) return fail(F110_E_INVALID, "%s: log_prob must be NULL exactly when eps is NULL", who);
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"h", h}, {"w_mean", w_mean}, {"w_log_std", w_log_std}, {"pre", pre}, {"action", action}})) return rc;
    PolicyheadArgs a;
    policyhead_geometry(*cfg, n, a);
    a.h = h; a.w_mean = w_mean; a.b_mean = b_mean; a.w_log_std = w_log_std; a.b_log_std = b_log_std; a.eps = eps;
    a.pre = pre; a.action = action; a.log_prob = log_prob;
    // (a workgroup walks tiles grid apart, so one launch serves any n; its LDS stays within the 64 KiB every kernel may ask for)
    const unsigned grid = (unsigned)std::min<long long>(a.tiles, PH_MAX_GRID);
    const size_t lds = (size_t)128 * a.T * a.kc;
#define POLICYHEAD_FWD(T, F64) hipLaunchKernelGGL((policyhead_forward_kernel<T, F64>), dim3(grid), dim3(PH_THREADS), lds, (hipStream_t)stream, a)
    if (a.T == 1) { if (a.out_fp64) POLICYHEAD_FWD(1, true); else POLICYHEAD_FWD(1, false); }
    else { if (a.out_fp64) POLICYHEAD_FWD(2, true); else POLICYHEAD_FWD(2, false); }
#undef POLICYHEAD_FWD
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_policyhead_backward(const f110_policyhead_config *cfg, const float *h, int64_t n, const float *w_mean, const float *w_log_std,
                                        const float *pre, const float *eps, const void *grad_action, const void *grad_log_prob, const float *grad_pre,
                                        float *grad_h, float *grad_w_mean, float *grad_b_mean, float *grad_w_log_std, float *grad_b_log_std, float *workspace,
                                        void *stream)
{
    const char *who = "f110_policyhead_backward";
    if (int rc = f110_policyhead_validate(cfg)) return rc;
    if (n < 0 || n > PH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)PH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!h || !w_mean || !w_log_std || !pre || !grad_action || !workspace) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!eps && grad_log_prob) return fail(F110_E_INVALID, "%s: grad_log_prob without eps (no log_prob was produced)", who);
    if ((uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"h", h}, {"w_mean", w_mean}, {"w_log_std", w_log_std}, {"pre", pre},
                                                                    {"grad_action", grad_action}, {"workspace", workspace}})) return rc;
    PolicyheadArgs a;
    policyhead_geometry(*cfg, n, a);
    a.h = h; a.w_mean = w_mean; a.w_log_std = w_log_std; a.eps = eps; a.pre = const_cast<float *>(pre);
    a.grad_action = grad_action; a.grad_log_prob = grad_log_prob; a.grad_pre = grad_pre;
    a.gpre = workspace; a.partial = workspace + policyhead_gpre_floats(*cfg, n);
    a.grad_h = grad_h; a.grad_w_mean = grad_w_mean; a.grad_b_mean = grad_b_mean; a.grad_w_log_std = grad_w_log_std; a.grad_b_log_std = grad_b_log_std;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n * a.A + PH_THREADS - 1) / PH_THREADS);
    if (a.out_fp64) hipLaunchKernelGGL(policyhead_gpre_kernel<true>, dim3(blocks), dim3(PH_THREADS), 0, s, a);
    else hipLaunchKernelGGL(policyhead_gpre_kernel<false>, dim3(blocks), dim3(PH_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    if (grad_h) {
        hipLaunchKernelGGL(policyhead_gradh_kernel, dim3((unsigned)((n + PH_GH_ROWS - 1) / PH_GH_ROWS), (unsigned)((a.K + PH_THREADS - 1) / PH_THREADS)),
                           dim3(PH_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (grad_w_mean || grad_b_mean || grad_w_log_std || grad_b_log_std) {
        hipLaunchKernelGGL(policyhead_gradw_kernel, dim3((unsigned)a.slices, (unsigned)((a.K + 63) / 64 + 1)), dim3(64), 0, s, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(policyhead_reduce_kernel, dim3((unsigned)((2 * a.A * (a.K + 1) + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

// ---------------------------------------------------------------- critic head: the twin Q tail and the TD target
extern "C" int f110_qhead_validate(const f110_qhead_config *cfg)
{
    const char *who = "f110_qhead_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->hidden < 1 || cfg->hidden > QH_MAX_H) return fail(F110_E_INVALID, "%s: hidden %d (1..%d)", who, cfg->hidden, QH_MAX_H);
    if (cfg->action_dim < 1 || cfg->action_dim > QH_MAX_A) return fail(F110_E_INVALID, "%s: action_dim %d (1..%d)", who, cfg->action_dim, QH_MAX_A);
    if (cfg->critics < 1 || cfg->critics > QH_MAX_C) return fail(F110_E_INVALID, "%s: %d critics (1..%d)", who, cfg->critics, QH_MAX_C);
    if (cfg->ld < cfg->action_dim) return fail(F110_E_INVALID, "%s: ld %d is below action_dim %d", who, cfg->ld, cfg->action_dim);
    return F110_OK;
}

// the launch geometry of a validated configuration (restated by tests/qhead_cases.py paths)
static size_t qhead_geometry(const f110_qhead_config &c, int64_t n, int rows_per_tile, QheadArgs &a)
{
    memset(&a, 0, sizeof(a));
    a.H = c.hidden; a.A = c.action_dim; a.C = c.critics; a.ld = c.ld; a.act_fp64 = c.action_fp64 ? 1 : 0;
    a.hc = std::min((QH_LDS_BYTES / 4 - a.A) / (a.A + 2) / 64 * 64, (a.H + 63) / 64 * 64);
    a.chunks = (a.H + a.hc - 1) / a.hc;
    a.n = n; a.tiles = (n + rows_per_tile - 1) / rows_per_tile;
    a.slices = (int)((n + QH_SLICE - 1) / QH_SLICE);
    return ((size_t)a.A * (a.hc + 1) + 2 * (size_t)a.hc) * sizeof(float);
}

extern "C" int64_t f110_qhead_workspace(const f110_qhead_config *cfg, int64_t n)
{
    if (n < 1 || n > QH_MAX_ROWS || f110_qhead_validate(cfg) != F110_OK) return 0;
    const int64_t slices = (n + QH_SLICE - 1) / QH_SLICE;
    const int64_t floats = cfg->critics * slices * (int64_t)qhead_partial_floats(cfg->hidden, cfg->action_dim);
    return (floats + 3) / 4 * 4 * (int64_t)sizeof(float);
}

// what both entry points ask of the critics' arrays; the pointers that must be device memory are appended to `ptrs`
static int qhead_critics(const char *who, const f110_qhead_config *cfg, const f110_qhead_critics *p, QheadArgs &a, std::vector<DevicePtr> &ptrs)
{
    static const char *names[3][QH_MAX_C] = {{"pre[0]", "pre[1]"}, {"w_act[0]", "w_act[1]"}, {"w2[0]", "w2[1]"}};
    for (int c = 0; c < cfg->critics; c++) {
        if (!p->pre[c] || !p->w_act[c] || !p->w2[c]) return fail(F110_E_INVALID, "%s: null pre, w_act or w2 of critic %d", who, c);
        a.pre[c] = p->pre[c]; a.w_act[c] = p->w_act[c]; a.b1[c] = p->b1[c]; a.w2[c] = p->w2[c]; a.b2[c] = p->b2[c];
        ptrs.push_back({names[0][c], p->pre[c]}); ptrs.push_back({names[1][c], p->w_act[c]}); ptrs.push_back({names[2][c], p->w2[c]});
    }
    return F110_OK;
}

extern "C" int f110_qhead_forward(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const double *reward,
                                  const uint8_t *done, const void *next_log_prob, double gamma, double alpha, float *q, float *qmin, float *target,
                                  void *stream)
{
    const char *who = "f110_qhead_forward";
    if (int rc = f110_qhead_validate(cfg)) return rc;
    if (n < 0 || n > QH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)QH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!p || !action || !q) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (target && (!reward || !done || !next_log_prob)) return fail(F110_E_INVALID, "%s: a target needs reward, done and next_log_prob", who);
    if (target && (!std::isfinite(gamma) || !std::isfinite(alpha))) return fail(F110_E_INVALID, "%s: gamma or alpha is not finite", who);
    QheadArgs a;
    const size_t lds = qhead_geometry(*cfg, n, QH_ROWS, a);
    std::vector<DevicePtr> ptrs = {{"action", action}, {"q", q}};
    if (int rc = qhead_critics(who, cfg, p, a, ptrs)) return rc;
    if (target) { ptrs.push_back({"reward", reward}); ptrs.push_back({"done", done}); ptrs.push_back({"next_log_prob", next_log_prob}); ptrs.push_back({"target", target}); }
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    a.action = action; a.q = q; a.qmin = qmin; a.target = target;
    if (target) { a.reward = reward; a.done = done; a.nlp = next_log_prob; a.gamma = gamma; a.alpha = alpha; }
    // (a workgroup walks tiles grid apart, so one launch serves any n; its LDS stays within the 64 KiB every kernel may ask for)
    const unsigned grid = (unsigned)std::min<long long>(a.tiles, QH_MAX_GRID);
    hipLaunchKernelGGL(qhead_forward_kernel, dim3(grid), dim3(QH_THREADS), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_qhead_backward(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const float *q,
                                   const float *grad_q, const float *grad_qmin, const f110_qhead_grads *g, void *grad_action, float *workspace,
                                   void *stream)
{
    const char *who = "f110_qhead_backward";
    if (int rc = f110_qhead_validate(cfg)) return rc;
    if (n < 0 || n > QH_MAX_ROWS) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, (long long)QH_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!p || !action || !q || !g) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
    QheadArgs a;
    const size_t lds = qhead_geometry(*cfg, n, QH_BROWS, a);
    std::vector<DevicePtr> ptrs = {{"action", action}, {"q", q}};
    if (int rc = qhead_critics(who, cfg, p, a, ptrs)) return rc;
    bool rows = grad_action != nullptr, params = false;
    for (int c = 0; c < a.C; c++) {
        a.grad_pre[c] = g->grad_pre[c]; a.grad_w_act[c] = g->grad_w_act[c]; a.grad_b1[c] = g->grad_b1[c]; a.grad_w2[c] = g->grad_w2[c]; a.grad_b2[c] = g->grad_b2[c];
        rows = rows || a.grad_pre[c];
        params = params || a.grad_w_act[c] || a.grad_b1[c] || a.grad_w2[c] || a.grad_b2[c];
    }
    if (params && !workspace) return fail(F110_E_INVALID, "%s: parameter gradients need the workspace", who);
    if (params) ptrs.push_back({"workspace", workspace});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    a.action = action; a.q_in = q; a.grad_q = grad_q; a.grad_qmin = grad_qmin; a.grad_action = grad_action; a.partial = workspace;
    hipStream_t s = (hipStream_t)stream;
    if (rows) {
        const unsigned grid = (unsigned)std::min<long long>(a.tiles, QH_MAX_GRID);
        if (a.A <= 16) hipLaunchKernelGGL(qhead_rows_kernel<16>, dim3(grid), dim3(QH_THREADS), lds, s, a);
        else hipLaunchKernelGGL(qhead_rows_kernel<32>, dim3(grid), dim3(QH_THREADS), lds, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (params) {
        const dim3 grid((unsigned)a.slices, (unsigned)((a.H + QH_THREADS - 1) / QH_THREADS), (unsigned)a.C);
        if (a.A <= 16) hipLaunchKernelGGL(qhead_gradw_kernel<16>, grid, dim3(QH_THREADS), 0, s, a);
        else hipLaunchKernelGGL(qhead_gradw_kernel<32>, grid, dim3(QH_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
        const unsigned blocks = (unsigned)((qhead_partial_floats(a.H, a.A) + QH_THREADS - 1) / QH_THREADS);
        hipLaunchKernelGGL(qhead_reduce_kernel, dim3(blocks, (unsigned)a.C), dim3(QH_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

// ---------------------------------------------------------------- parameter update: Adam and the soft update of the targets
static int adam_scalar_checks(const char *who, const f110_adam_config *cfg, bool target)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0)) return fail(F110_E_INVALID, "%s: beta1 %g (0 <= beta1 < 1)", who, cfg->beta1);
    if (!(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0)) return fail(F110_E_INVALID, "%s: beta2 %g (0 <= beta2 < 1)", who, cfg->beta2);
    if (!std::isfinite(cfg->eps) || !(cfg->eps > 0.0)) return fail(F110_E_INVALID, "%s: eps %g (finite and > 0)", who, cfg->eps);
    if (target && (!std::isfinite(cfg->tau) || cfg->tau < 0.0 || cfg->tau > 1.0)) return fail(F110_E_INVALID, "%s: tau %g (0 <= tau <= 1)", who, cfg->tau);
    return F110_OK;
}

extern "C" int f110_adam_validate(const f110_adam_config *cfg)
{
    return adam_scalar_checks("f110_adam_validate", cfg, cfg && cfg->with_target);
}

extern "C" int64_t f110_adam_state_bytes(void) { return (int64_t)sizeof(f110_adam_state); }

// the checks on the table and the kernel's copy of it -> chunks of the launch in *grid
static int adam_table(const char *who, const f110_adam_tensor *table, int n_tensors, bool adam, bool target, AdamTable &tab, uint32_t *grid,
                      std::vector<DevicePtr> &ptrs)
{
    if (n_tensors < 0 || n_tensors > AD_MAX_T) return fail(F110_E_INVALID, "%s: n_tensors %d (0..%d a call)", who, n_tensors, AD_MAX_T);
    if (n_tensors > 0 && !table) return fail(F110_E_INVALID, "%s: null table", who);
    memset(&tab, 0, sizeof(tab));
    tab.n_tensors = n_tensors;
    uint32_t chunks = 0;
    for (int i = 0; i < n_tensors; i++) {
        const f110_adam_tensor &t = table[i];
        if (t.n < 0 || t.n > ((int64_t)1 << 31)) return fail(F110_E_INVALID, "%s: tensor %d: n %lld (0..2^31)", who, i, (long long)t.n);
        if (t.n > 0) {
            if (!t.p) return fail(F110_E_INVALID, "%s: tensor %d: null p", who, i);
            if (adam && !t.m) return fail(F110_E_INVALID, "%s: tensor %d: null m", who, i);
            if (adam && !t.v) return fail(F110_E_INVALID, "%s: tensor %d: null v", who, i);
            if (adam && !t.g) return fail(F110_E_INVALID, "%s: tensor %d: null g", who, i);
            if (target && !t.target) return fail(F110_E_INVALID, "%s: tensor %d: null target", who, i);
            if (target && t.target == t.p) return fail(F110_E_INVALID, "%s: tensor %d: target == p", who, i);
            uintptr_t bits = (uintptr_t)t.p;
            if (adam) bits |= (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v;
            if (target) bits |= (uintptr_t)t.target;
            if (bits % 4) return fail(F110_E_INVALID, "%s: tensor %d: a pointer is not 4-byte aligned", who, i);
            AdamEntry &e = tab.t[i];
            e.p = t.p; e.n = (uint32_t)t.n; e.vec = bits % 16 == 0;
            if (adam) { e.g = t.g; e.m = t.m; e.v = t.v; }
            if (target) e.target = t.target;
            chunks += (uint32_t)((t.n + AD_CHUNK - 1) / AD_CHUNK);
            ptrs.push_back({"p", t.p});
            if (target) ptrs.push_back({"target", t.target});
        }
        tab.chunk_end[i] = chunks;      // (at most 64 * 2^19)
    }
    *grid = chunks;
    return F110_OK;
}

extern "C" int f110_adam_step(const f110_adam_config *cfg, const f110_adam_tensor *table, int32_t n_tensors, f110_adam_state *state, double lr,
                              void *stream)
{
    const char *who = "f110_adam_step";
    if (int rc = adam_scalar_checks(who, cfg, cfg && cfg->with_target)) return rc;
    if (!state) return fail(F110_E_INVALID, "%s: null state", who);
    if ((uintptr_t)state % 8) return fail(F110_E_INVALID, "%s: the state is not 8-byte aligned", who);
    if (!std::isfinite(lr)) return fail(F110_E_INVALID, "%s: lr is not finite", who);
    const bool target = cfg->with_target != 0;
    AdamTable tab;
    uint32_t grid = 0;
    std::vector<DevicePtr> ptrs = {{"state", state}};
    if (int rc = adam_table(who, table, n_tensors, true, target, tab, &grid, ptrs)) return rc;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    tab.c1 = (float)(1.0 - cfg->beta1); tab.c2 = (float)(1.0 - cfg->beta2); tab.b2 = (float)cfg->beta2; tab.eps = (float)cfg->eps;
    tab.tau = target ? (float)cfg->tau : 0.0f;
    hipStream_t s = (hipStream_t)stream;
    if (cfg->advance) {
        hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, s, state, cfg->beta1, cfg->beta2, lr);
        HIP_TRY(hipGetLastError());
    }
    if (grid == 0) return F110_OK;
    if (target) hipLaunchKernelGGL((adam_kernel<true, true>), dim3(grid), dim3(AD_THREADS), 0, s, tab, (const AdamState *)state);
    else hipLaunchKernelGGL((adam_kernel<true, false>), dim3(grid), dim3(AD_THREADS), 0, s, tab, (const AdamState *)state);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_soft_update(const f110_adam_tensor *table, int32_t n_tensors, double tau, void *stream)
{
    const char *who = "f110_soft_update";
    if (!std::isfinite(tau) || tau < 0.0 || tau > 1.0) return fail(F110_E_INVALID, "%s: tau %g (0 <= tau <= 1)", who, tau);
    AdamTable tab;
    uint32_t grid = 0;
    std::vector<DevicePtr> ptrs;
    if (int rc = adam_table(who, table, n_tensors, false, true, tab, &grid, ptrs)) return rc;
    if (grid == 0) return F110_OK;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    tab.tau = (float)tau;
    hipLaunchKernelGGL((adam_kernel<false, true>), dim3(grid), dim3(AD_THREADS), 0, (hipStream_t)stream, tab, (const AdamState *)nullptr);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
