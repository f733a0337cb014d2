// f110_bitconv_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_bitconv.h"
#include "f110_bitconv2.h"

#include <initializer_list>

// ---------------------------------------------------------------- first convolution from bits
extern "C" int f110_bitconv_validate(const f110_bitconv_config *cfg) { return bitconv_check(cfg, "f110_bitconv_validate"); }

extern "C" int64_t f110_bitconv_workspace(const f110_bitconv_config *cfg, int64_t n)
{
    if (n < 1 || f110_bitconv_validate(cfg) != F110_OK) return 0;
    return bitconv_workspace_bytes(*cfg, n);
}

// What every launching entry point checks once its config has passed, in this order (it decides which message a call that breaks
// several rules gets): the stack, the counts, the index a stack needs; then, unless n = 0 (nothing to do: the caller returns F110_OK
// without looking at a pointer), the pointers, the samples without an index, the alignments.
//   stack: NULL for one frame per sample (index [n] or NULL), else the frames of a stack (index [n, stack] required)
//   n_min .. n_max: the samples accepted;  src_always: src is needed even while n_frames = 0;  packed: src holds 64-bit words
//   tensors: what else must not be NULL;  has_ws: a workspace, 16-byte aligned, comes with the call
static int bitconv_call_check(const char *who, const int32_t *stack, int64_t n_min, int64_t n_max, bool src_always, bool packed, bool has_ws,
                              const void *src, int64_t n_frames, const int64_t *index, int64_t n, std::initializer_list<const void *> tensors,
                              const void *ws = nullptr)
{
    if (stack)
        if (int rc = bitconv_stack_check(*stack, who)) return rc;
    if (n < n_min || n > n_max || n_frames < 0) return fail(F110_E_INVALID, "%s: n=%lld samples of %lld frames", who, (long long)n, (long long)n_frames);
    if (stack && !index) return fail(F110_E_INVALID, "%s: null index (a stack names its frames)", who);
    if (n == 0) return F110_OK;
    bool null = ((src_always || n_frames > 0) && !src) || (has_ws && !ws);
    for (const void *t : tensors) null = null || !t;
    if (null) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (!index && n > n_frames) return fail(F110_E_INVALID, "%s: %lld samples of %lld frames without an index", who, (long long)n, (long long)n_frames);
    if ((packed && (uintptr_t)src % 8) || (has_ws && (uintptr_t)ws % 16))
        return fail(F110_E_INVALID, has_ws ? "%s: frames must be 8-byte and the workspace 16-byte aligned" : "%s: frames must be 8-byte aligned", who);
    return F110_OK;
}

static int bitconv_forward(const char *who, const f110_bitconv_config *cfg, const void *src, bool u8, int64_t n_frames, const int64_t *index,
                           int64_t n, const float *weight, const float *bias, float *out, hipStream_t stream)
{
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    const int rc = bitconv_call_check(who, nullptr, 0, INT64_MAX, false, !u8, false, src, n_frames, index, n, {weight, out});
    if (rc || n == 0) return rc;
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

// The partial sums over the frames that p.a.index names (into p.a.ws), then their reduction into column j of grad_weight [C, stack, kk]
// and, where given, into grad_bias.  <false>: grad_weight [C, kk], the one column there is.
template <bool STACK>
static int bitconv_backward_column(const BitconvBackwardPlan &p, int stack, int j, float *grad_weight, float *grad_bias, hipStream_t stream)
{
    const BitconvArgs &a = p.a;
    const f110_bitconv_config &c = a.cfg;
#define BITCONV_BWD(K) F110_LAUNCH((bitconv_backward_kernel<K>), p.partials, stream, a)
    BITCONV_BY_KERNEL(p.partials.inst, BITCONV_BWD)
#undef BITCONV_BWD
    HIP_TRY(hipGetLastError());
    F110_LAUNCH(bitconv_reduce_kernel<STACK>, p.reduce, stream, (const float *)a.ws, a.G, p.nw, c.channels, c.on, grad_weight, grad_bias,
                c.kernel * c.kernel, stack, j);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_bitconv_backward(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                                     const float *grad_out, float *grad_weight, float *grad_bias, float *workspace, void *stream)
{
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    if (int rc = bitconv_call_check("f110_bitconv_backward", nullptr, 1, INT64_MAX, false, true, true, frames, n_frames, index, n,
                                    {grad_out, grad_weight}, workspace))
        return rc;
    BitconvBackwardPlan p = bitconv_backward_plan(*cfg, n);
    BitconvArgs &a = p.a;
    a.frames = frames; a.n_frames = n_frames; a.index = (const long long *)index; a.grad_out = grad_out; a.ws = workspace;
    return bitconv_backward_column<false>(p, 1, 0, grad_weight, grad_bias, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the same layer on a stack of frames
extern "C" int f110_bitconv_forward_stack(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                                          int64_t n, const float *weight, const float *bias, float *out, void *stream)
{
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    const int rc = bitconv_call_check("f110_bitconv_forward_stack", &stack, 0, INT64_MAX, false, true, false, frames, n_frames, index, n, {weight, out});
    if (rc || n == 0) return rc;
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
    if (int rc = f110_bitconv_validate(cfg)) return rc;
    if (int rc = bitconv_call_check("f110_bitconv_backward_stack", &stack, 1, 1ll << 31, false, true, true, frames, n_frames, index, n,
                                    {grad_out, grad_weight}, workspace))
        return rc;
    BitconvStackBackwardPlan p = bitconv_backward_stack_plan(*cfg, stack, n);
    long long *columns = reinterpret_cast<long long *>(reinterpret_cast<char *>(workspace) + p.index_offset);
    F110_LAUNCH(bitconv_index_columns_kernel, p.columns, (hipStream_t)stream, (const long long *)index, (long long)n, (int)stack, columns);
    HIP_TRY(hipGetLastError());
    BitconvArgs &a = p.one.a;
    a.frames = frames; a.n_frames = n_frames; a.grad_out = grad_out; a.ws = workspace;
    for (int j = 0; j < stack; j++) {
        a.index = columns + (size_t)j * (size_t)n;
        if (int rc = bitconv_backward_column<true>(p.one, stack, j, grad_weight, j == 0 ? grad_bias : nullptr, (hipStream_t)stream)) return rc;
    }
    return F110_OK;
}

// ---------------------------------------------------------------- policy stem: conv1 + relu + conv2 from bits
extern "C" int f110_bitconv2_validate(const f110_bitconv2_config *cfg) { return bitconv2_check(cfg, "f110_bitconv2_validate"); }

static int bitconv2_forward(const char *who, const f110_bitconv2_config *cfg, const void *src, bool u8, int64_t n_frames, const int64_t *index,
                            int64_t n, const float *w1, const float *b1, const float *w2, const float *b2, float *out, hipStream_t stream)
{
    if (int rc = f110_bitconv2_validate(cfg)) return rc;
    const int rc = bitconv_call_check(who, nullptr, 0, INT64_MAX, true, !u8, false, src, n_frames, index, n, {w1, w2, out});
    if (rc || n == 0) return rc;
    Bitconv2Plan p = bitconv2_forward_plan(*cfg, u8, n);
    Bitconv2Args &a = p.a;
    if (u8) a.l1.images = (const uint8_t *)src; else a.l1.frames = (const uint64_t *)src;
    a.l1.n_frames = n_frames; a.l1.index = (const long long *)index;
    F110_LAUNCH(bitconv2_forward_kernel<false>, p.l, stream, a, w1, b1, w2, b2, out);
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
    if (int rc = f110_bitconv2_validate(cfg)) return rc;
    if (int rc = bitconv_call_check("f110_bitconv2_forward_stack", &stack, 1, INT64_MAX, true, true, false, frames, n_frames, index, n, {w1, w2, out}))
        return rc;
    Bitconv2StackPlan p = bitconv2_forward_stack_plan(*cfg, stack, n);
    Bitconv2StackArgs &s = p.s;
    s.a.l1.frames = frames; s.a.l1.n_frames = n_frames; s.index = (const long long *)index;
    F110_LAUNCH(bitconv2_forward_kernel<true>, p.l, (hipStream_t)stream, s, w1, b1, w2, b2, out);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
