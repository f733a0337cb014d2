// f110_featconv_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_featconv.h"

// ---------------------------------------------------------------- dense convolution of feature maps, forward and backward
extern "C" int f110_featconv_validate(const f110_featconv_config *cfg) { return featconv_check(cfg, "f110_featconv_validate"); }

extern "C" int64_t f110_featconv_workspace(const f110_featconv_config *cfg, int64_t n)
{
    if (n < 1 || f110_featconv_validate(cfg) != F110_OK) return 0;
    return featconv_workspace_bytes(*cfg, n);
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
    FeatconvForwardPlan p = featconv_forward_plan(*cfg, n);
    FeatconvArgs &a = p.a;
    a.x = x; a.w = weight; a.bias = bias; a.dst = out;
    F110_LAUNCH(featconv_gemm_kernel<false>, p.l, (hipStream_t)stream, a);
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
    FeatconvBackwardPlan p = featconv_backward_plan(*cfg, n);
    FeatconvArgs &a = p.a;
    a.x = x; a.out = out; a.grad_out = grad_out; a.w = weight;
    if (grad_x) {
        a.dst = grad_x;
        F110_LAUNCH(featconv_gemm_kernel<true>, p.gradx, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (params) {
        a.P = workspace;
#define FEATCONV_GRADW(MT) F110_LAUNCH(featconv_gradw_kernel<MT>, p.partials, s, a)
        switch (p.partials.inst) { case 1: FEATCONV_GRADW(1); break; case 2: FEATCONV_GRADW(2); break; case 3: FEATCONV_GRADW(3); break; default: FEATCONV_GRADW(4); break; }
#undef FEATCONV_GRADW
        HIP_TRY(hipGetLastError());
        F110_LAUNCH(featconv_reduce_kernel, p.reduce, s, (const float *)workspace, (long long)n, p.nw, a.Co, grad_weight, grad_bias);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}
