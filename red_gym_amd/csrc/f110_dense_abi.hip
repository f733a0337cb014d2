// f110_dense_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_dense.h"

// ---------------------------------------------------------------- dense layer (fc1), forward and backward
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int f110_dense_validate(const f110_dense_config *cfg) { return dense_check(cfg, "f110_dense_validate"); }

extern "C" int64_t f110_dense_workspace(const f110_dense_config *cfg, int64_t n)
{
    if (n < 1 || f110_dense_validate(cfg) != F110_OK) return 0;
    return dense_workspace_bytes(*cfg, n);
}

extern "C" int f110_dense_forward(const f110_dense_config *cfg, const float *x, int64_t n, const float *weight, const float *bias, float *out,
                                  float *workspace, void *stream)
{
    const char *who = "f110_dense_forward";
    if (int rc = f110_dense_validate(cfg)) return rc;
    if (!dense_rows_ok(n)) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, DN_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!x || !weight || !out) return fail(F110_E_INVALID, "%s: null pointer", who);
    DenseForwardPlan p = dense_forward_plan(*cfg, n);
    DenseArgs &a = p.a;
    if (a.split && !workspace) return fail(F110_E_INVALID, "%s: this shape needs the workspace (f110_dense_workspace)", who);
    std::vector<DevicePtr> ptrs = {{"x", x}, {"weight", weight}, {"out", out}};
    if (bias) ptrs.push_back({"bias", bias});
    if (a.split) ptrs.push_back({"workspace", workspace});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    hipStream_t s = (hipStream_t)stream;
    a.x = x; a.w = weight; a.bias = bias; a.dst = out; a.P = workspace;
    a.vec_x = aligned16(x) && a.K % 4 == 0; a.vec_w = aligned16(weight) && a.ld % 4 == 0;
    if (a.split) {
        F110_LAUNCH(dense_forward_kernel<true>, p.gemm, s, a);
        HIP_TRY(hipGetLastError());
        F110_LAUNCH(dense_sum_kernel, p.sum, s, a);
    } else {
        F110_LAUNCH(dense_forward_kernel<false>, p.gemm, s, a);
    }
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_dense_backward(const f110_dense_config *cfg, const float *x, const float *out, const float *grad_out, int64_t n,
                                   const float *weight, float *grad_x, float *grad_weight, float *grad_bias, void *stream)
{
    const char *who = "f110_dense_backward";
    if (int rc = f110_dense_validate(cfg)) return rc;
    if (!dense_rows_ok(n)) return fail(F110_E_INVALID, "%s: n=%lld rows (0..%lld)", who, (long long)n, DN_MAX_ROWS);
    if (n == 0) return F110_OK;
    if (!grad_out || (cfg->relu && !out) || (grad_x && !weight) || (grad_weight && !x)) return fail(F110_E_INVALID, "%s: null pointer", who);
    std::vector<DevicePtr> ptrs = {{"grad_out", grad_out}};
    if (cfg->relu) ptrs.push_back({"out", out});
    if (grad_x) { ptrs.push_back({"weight", weight}); ptrs.push_back({"grad_x", grad_x}); }
    if (grad_weight) { ptrs.push_back({"x", x}); ptrs.push_back({"grad_weight", grad_weight}); }
    if (grad_bias) ptrs.push_back({"grad_bias", grad_bias});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DenseBackwardPlan p = dense_backward_plan(*cfg, n);
    DenseArgs &a = p.a;
    a.x = x; a.out = out; a.grad_out = grad_out; a.w = weight; a.grad_bias = grad_bias;
    a.vec_x = aligned16(x) && a.K % 4 == 0; a.vec_w = aligned16(weight) && a.ld % 4 == 0;
    a.vec_g = aligned16(grad_out) && (!cfg->relu || aligned16(out)) && a.H % 4 == 0;
    if (grad_x) {
        a.dst = grad_x;
        F110_LAUNCH(dense_gradx_kernel, p.gradx, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (grad_weight) {
        a.dst = grad_weight;
        F110_LAUNCH(dense_gradw_kernel, p.gradw, s, a);
        HIP_TRY(hipGetLastError());
    }
    if (grad_bias) {
        F110_LAUNCH(dense_gradb_kernel, p.gradb, s, a);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}
