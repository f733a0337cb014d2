// f110_gauss_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_gauss.h"

// ---------------------------------------------------------------- the policy's Gaussian draws
// both entry points; state: where seed and t are read on the device, NULL: `seed` and `t`
static int gauss_fill(const char *who, const f110_gauss_state *state, uint64_t seed, int32_t stream, uint64_t t, int64_t n, int32_t A,
                      const int64_t *rows, float *out, bool by_state, bool advance, void *hip_stream)
{
    if (int rc = gauss_check(who, by_state, state, stream, n, A, out)) return rc;
    if (int rc = gauss_rows_check(who, rows)) return rc;
    std::vector<DevicePtr> ptrs = {{"out", out}};
    if (by_state) ptrs.push_back({"state", state});
    if (rows) ptrs.push_back({"rows", rows});
    if (int rc = check_device_pointers(who, (hipStream_t)hip_stream, ptrs)) return rc;
    GaussPlan p = gauss_plan(n, A, out);
    p.a.state = by_state ? state : nullptr;
    p.a.seed = seed; p.a.stream = (uint64_t)stream; p.a.t = t;
    p.a.rows = rows;
    F110_LAUNCH(gauss_fill_kernel, p.l, (hipStream_t)hip_stream, p.a);
    HIP_TRY(hipGetLastError());
    if (advance) {
        hipLaunchKernelGGL(gauss_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, const_cast<f110_gauss_state *>(state), (int)stream);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

extern "C" int64_t f110_gauss_state_bytes(void) { return (int64_t)sizeof(f110_gauss_state); }

extern "C" int f110_gauss_fill(f110_gauss_state *state, int32_t stream, int64_t n, int32_t A, const int64_t *rows, float *out, int32_t advance,
                               void *hip_stream)
{
    return gauss_fill("f110_gauss_fill", state, 0, stream, 0, n, A, rows, out, true, advance != 0, hip_stream);
}

extern "C" int f110_gauss_fill_at(uint64_t seed, int32_t stream, uint64_t t, int64_t n, int32_t A, const int64_t *rows, float *out, void *hip_stream)
{
    return gauss_fill("f110_gauss_fill_at", nullptr, seed, stream, t, n, A, rows, out, false, false, hip_stream);
}
