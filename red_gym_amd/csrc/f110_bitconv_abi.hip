// f110_bitconv_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_bitconv.h"
#include "f110_bitconv2.h"

// ---------------------------------------------------------------- first convolution from bits
extern "C" int f110_bitconv_validate(const f110_bitconv_config *cfg) { return bitconv_check(cfg, "f110_bitconv_validate"); }

extern "C" int64_t f110_bitconv_workspace(const f110_bitconv_config *cfg, int64_t n)
{
    if (n < 1 || f110_bitconv_validate(cfg) != F110_OK) return 0;
    return bitconv_workspace_bytes(*cfg, n);
}

// LAUNCH(K) for the kernel size a plan's instantiation number names
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
    BitconvForwardPlan p = bitconv_forward_plan(*cfg, u8, n);
    BitconvArgs &a = p.a;
    if (u8) a.images = (const uint8_t *)src; else a.frames = (const uint64_t *)src;
    a.n_frames = n_frames; a.index = (const long long *)index;
    for (const BitconvGroup &g : p.groups) {
        a.first = g.first; p.l.gx = g.grid;
#define BITCONV_FWD(K) do { if (p.l.inst & 1) F110_LAUNCH((bitconv_forward_kernel<K, true>), p.l, stream, a, weight, bias, out); \
                            else F110_LAUNCH((bitconv_forward_kernel<K, false>), p.l, stream, a, weight, bias, out); } while (0)
        BITCONV_BY_KERNEL(p.l.inst >> 1, BITCONV_FWD)
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
    BitconvBackwardPlan p = bitconv_backward_plan(*cfg, n);
    BitconvArgs &a = p.a;
    a.frames = frames; a.n_frames = n_frames; a.index = (const long long *)index; a.grad_out = grad_out; a.ws = workspace;
#define BITCONV_BWD(K) F110_LAUNCH((bitconv_backward_kernel<K>), p.partials, (hipStream_t)stream, a)
    BITCONV_BY_KERNEL(p.partials.inst, BITCONV_BWD)
#undef BITCONV_BWD
    HIP_TRY(hipGetLastError());
    F110_LAUNCH(bitconv_reduce_kernel, p.reduce, (hipStream_t)stream, (const float *)workspace, a.G, p.nw, cfg->channels, cfg->on, grad_weight, grad_bias);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- the same layer on a stack of frames
extern "C" int f110_bitconv_forward_stack(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                                          int64_t n, const float *weight, const float *bias, float *out, void *stream)
{
    const char *who = "f110_bitconv_forward_stack";
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    if (int rc = bitconv_stack_check(stack, who)) return rc;
    if (n < 0 || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (!index) return fail(F110_E_INVALID, "%s: null index (a stack names its frames)", who);
    if (n == 0) return F110_OK;
    if (!weight || !out || (n_frames > 0 && !frames)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((uintptr_t)frames % 8) return fail(F110_E_INVALID, "%s: frames must be 8-byte aligned", who);
    BitconvStackForwardPlan p = bitconv_forward_stack_plan(*cfg, stack, n);
    BitconvStackArgs &s = p.s;
    s.a.frames = frames; s.a.n_frames = n_frames; s.index = (const long long *)index;
    for (const BitconvGroup &g : p.groups) {
        s.a.first = g.first; p.l.gx = g.grid;
#define BITCONV_FWDS(K) F110_LAUNCH((bitconv_forward_stack_kernel<K>), p.l, (hipStream_t)stream, s, weight, bias, out)
        BITCONV_BY_KERNEL(p.l.inst, BITCONV_FWDS)
#undef BITCONV_FWDS
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

extern "C" int64_t f110_bitconv_workspace_stack(const f110_bitconv_config *cfg, int32_t stack, int64_t n)
{
    if (n < 1 || stack < 1 || stack > F110_BITCONV_MAX_STACK || f110_bitconv_validate(cfg) != F110_OK) return 0;
    return bitconv_stack_workspace_bytes(*cfg, stack, n);
}

extern "C" int f110_bitconv_backward_stack(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                                           int64_t n, const float *grad_out, float *grad_weight, float *grad_bias, float *workspace, void *stream)
{
    const char *who = "f110_bitconv_backward_stack";
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    if (int rc = bitconv_stack_check(stack, who)) return rc;
    if (n < 1 || n > (1ll << 31) || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (!index) return fail(F110_E_INVALID, "%s: null index (a stack names its frames)", who);
    if (!grad_out || !grad_weight || !workspace || (n_frames > 0 && !frames)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((uintptr_t)frames % 8 || (uintptr_t)workspace % 16) return fail(F110_E_INVALID, "%s: frames must be 8-byte and the workspace 16-byte aligned", who);
    BitconvStackBackwardPlan p = bitconv_backward_stack_plan(*cfg, stack, n);
    long long *columns = reinterpret_cast<long long *>(reinterpret_cast<char *>(workspace) + p.index_offset);
    F110_LAUNCH(bitconv_index_columns_kernel, p.columns, (hipStream_t)stream, (const long long *)index, (long long)n, (int)stack, columns);
    HIP_TRY(hipGetLastError());
    BitconvArgs &a = p.one.a;
    a.frames = frames; a.n_frames = n_frames; a.grad_out = grad_out; a.ws = workspace;
    for (int j = 0; j < stack; j++) {
        a.index = columns + (size_t)j * (size_t)n;
#define BITCONV_BWD(K) F110_LAUNCH((bitconv_backward_kernel<K>), p.one.partials, (hipStream_t)stream, a)
        BITCONV_BY_KERNEL(p.one.partials.inst, BITCONV_BWD)
#undef BITCONV_BWD
        HIP_TRY(hipGetLastError());
        F110_LAUNCH(bitconv_reduce_stack_kernel, p.one.reduce, (hipStream_t)stream, (const float *)workspace, a.G, p.one.nw, cfg->channels, cfg->on,
                    cfg->kernel * cfg->kernel, (int)stack, j, grad_weight, j == 0 ? grad_bias : (float *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

// ---------------------------------------------------------------- policy stem: conv1 + relu + conv2 from bits
extern "C" int f110_bitconv2_validate(const f110_bitconv2_config *cfg) { return bitconv2_check(cfg, "f110_bitconv2_validate"); }

static int bitconv2_forward(const char *who, const f110_bitconv2_config *cfg, const void *src, bool u8, int64_t n_frames, const int64_t *index,
                            int64_t n, const float *w1, const float *b1, const float *w2, const float *b2, float *out, hipStream_t stream)
{
    if (int rc = f110_bitconv2_validate(cfg)) return rc;
    if (n < 0 || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (n == 0) return F110_OK;
    if (!w1 || !w2 || !out || !src) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!index && n > n_frames) return fail(F110_E_INVALID, "%s: %lld samples of %lld frames without an index", who, (long long)n, (long long)n_frames);
    if (!u8 && (uintptr_t)src % 8) return fail(F110_E_INVALID, "%s: frames must be 8-byte aligned", who);
    Bitconv2Plan p = bitconv2_forward_plan(*cfg, u8, n);
    Bitconv2Args &a = p.a;
    if (u8) a.l1.images = (const uint8_t *)src; else a.l1.frames = (const uint64_t *)src;
    a.l1.n_frames = n_frames; a.l1.index = (const long long *)index;
    F110_LAUNCH(bitconv2_forward_kernel, p.l, stream, a, w1, b1, w2, b2, out);
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

extern "C" int f110_bitconv2_forward_stack(const f110_bitconv2_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                                           int64_t n, const float *w1, const float *b1, const float *w2, const float *b2, float *out, void *stream)
{
    const char *who = "f110_bitconv2_forward_stack";
    if (int rc = f110_bitconv2_validate(cfg)) return rc;
    if (int rc = bitconv_stack_check(stack, who)) return rc;
    if (n < 1 || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (!index) return fail(F110_E_INVALID, "%s: null index (a stack names its frames)", who);
    if (!w1 || !w2 || !out || !frames) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((uintptr_t)frames % 8) return fail(F110_E_INVALID, "%s: frames must be 8-byte aligned", who);
    Bitconv2StackPlan p = bitconv2_forward_stack_plan(*cfg, stack, n);
    Bitconv2StackArgs &s = p.s;
    s.a.l1.frames = frames; s.a.l1.n_frames = n_frames; s.index = (const long long *)index;
    F110_LAUNCH(bitconv2_forward_stack_kernel, p.l, (hipStream_t)stream, s, w1, b1, w2, b2, out);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
