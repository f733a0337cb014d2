// f110_common.h -- what every translation unit of libf110_hip.so needs: the C ABI, the error plumbing, the device scope and the
// owners of HIP resources.  The kernels live in headers; a header that defines a non-template __global__ function is included,
// directly or through another header, ONLY by the units that launch it: every unit that sees such a definition emits the kernel.
// Units (red_gym_amd/build.py compiles them in parallel and links them into the one library):
//   f110_handle.hip     handle life cycle, host tables, vehicle parameters, buffers, device error word, host EDT
//   f110_maps.hip       map installation (host table / occupancy mask -> cell codes, LUTs), device EDT, track mask
//   f110_noise_abi.hip  lidar noise: slots, ring, generators, per-env mode
//   f110_step.hip       launch policy of the scan, the step, hipGraphs, measurement aid, function-level entry points
//   f110_consumers.hip  the callers either side of the step, on the handle: pure-pursuit planner, progress tracker, reward shaper,
//                       path follower, replay buffer and its priority tree, episode tracker
//   f110_bitconv_abi.hip the policy's first layers from bits, stateless: bit convolution, policy stem
//   f110_policy_abi.hip the policy's and the critics' tails, stateless: policy head, critic head, the parameter update (Adam and
//                       the soft update of the targets), the two losses of a SAC update and the learnt entropy temperature
//   f110_gauss_abi.hip  the policy's Gaussian draws, stateless but for the caller's 64-byte state: NumPy's Philox normals per element
//   f110_featconv_abi.hip the trunk's dense convolutions (conv2, conv3), stateless: forward, grad_x, grad_weight / grad_bias
//   f110_dense_abi.hip  the dense layer fc1, stateless: forward, grad_x, grad_weight, grad_bias
//   f110_bitmap_abi.hip the scan's consumers with no handle: scan -> bitmap (its own f110_bitmap object), occupancy grid
#pragma once
#include "../../include/f110_hip.h"
#include "f110_launch.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

namespace f110 {} // (the kernel headers fill it)
using namespace f110;

int fail(int code, const char *fmt, ...);                 // f110_handle.hip
int check_current_device(int dev, const char *who);       // f110_handle.hip

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(F110_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// One launch as a plan (f110_*_plan.h) describes it; `kernel` in parentheses where its template arguments hold a comma.
#define F110_LAUNCH(kernel, L, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3((L).gx, (L).gy, (L).gz), dim3((L).block), (L).lds, stream, __VA_ARGS__)

// Makes `dev` the calling thread's current device for the scope of one library call and restores the caller's own
// afterwards: a process that drives several GPUs (or several handles on different GPUs) keeps ITS current device across
// every call.  f110_step / f110_reset and the function-level entry points do not switch -- they launch on the caller's
// stream, which belongs to the caller's current device -- they check (check_device) and refuse a mismatch.
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};
#define ON_DEVICE(dev)            \
    DeviceScope dev_scope_(dev);  \
    HIP_TRY(dev_scope_.err)


// Owners of what the library allocates.  Every device buffer, event, stream and graph lives in one of these and is released by
// its destructor; a table is replaced by building the new one in a local owner and moving it in, which frees the old one.
template <typename T> class DevBuf { // device memory of size() elements of T
    T *p_ = nullptr;
    size_t n_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf &operator=(DevBuf o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; } // (o takes the old memory along)
    ~DevBuf() { if (p_) (void)hipFree(p_); }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    hipError_t alloc(size_t n) // new memory first: a failure leaves what is held
    {
        T *p = nullptr;
        const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) { std::swap(p_, p); n_ = n; if (p) (void)hipFree(p); }
        return e;
    }
    hipError_t upload(const T *src, size_t n) // (re)allocates when n differs from size()
    {
        const hipError_t e = n == n_ && p_ ? hipSuccess : alloc(n);
        return e == hipSuccess ? hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice) : e;
    }
};

template <typename H, hipError_t (*Destroy)(H)> class HipOwner { // an event, stream or graph
    H h_ = nullptr;
public:
    HipOwner() = default;
    HipOwner(HipOwner &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    HipOwner &operator=(HipOwner o) noexcept { std::swap(h_, o.h_); return *this; }
    ~HipOwner() { if (h_) (void)Destroy(h_); }
    H get() const { return h_; }
    H *put() { *this = HipOwner(); return &h_; } // for the call that creates it: what was held is released first
};
using Event = HipOwner<hipEvent_t, hipEventDestroy>;
using Stream = HipOwner<hipStream_t, hipStreamDestroy>;
using Graph = HipOwner<hipGraph_t, hipGraphDestroy>;
using GraphExec = HipOwner<hipGraphExec_t, hipGraphExecDestroy>;

// The stateless entry points launch on the calling thread's current device: every required pointer must be memory of that device
// and a stream given must belong to it.  A mismatch is refused here, before any launch (host-side queries only, no synchronisation).
struct DevicePtr { const char *name; const void *p; };
inline int check_device_pointers(const char *who, hipStream_t stream, const std::vector<DevicePtr> &ptrs)
{
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (stream) {
        hipDevice_t sdev = -1;
        if (hipStreamGetDevice(stream, &sdev) != hipSuccess) {
            (void)hipGetLastError();
            return fail(F110_E_INVALID, "%s: `stream` is not a stream of this process", who);
        }
        if ((int)sdev != cur) return fail(F110_E_INVALID, "%s: `stream` belongs to device %d but the calling thread's current device is %d", who, (int)sdev, cur);
    }
    for (const DevicePtr &q : ptrs) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof(at));
        const hipError_t e = hipPointerGetAttributes(&at, q.p);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged))
            return fail(F110_E_INVALID, "%s: `%s` is not device memory", who, q.name);
        if (at.device != cur) return fail(F110_E_INVALID, "%s: `%s` lives on device %d but the calling thread's current device is %d", who, q.name, at.device, cur);
    }
    return F110_OK;
}
