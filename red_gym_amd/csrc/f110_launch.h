// f110_launch.h -- what a launch plan says of one kernel launch, and F110_HD for the few functions host and device share.
// Plain C++17 without HIP: the plan headers (f110_*_plan.h) include it, and tests/test_launch_plans_cpu.py compiles them for the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define F110_HD __host__ __device__
#else
#define F110_HD
#endif

namespace f110 {

struct Launch {
    unsigned gx, gy, gz, block;     // grid and workgroup size
    size_t lds;                     // dynamic LDS bytes
    int inst;                       // which instantiation of the kernel (0 where there is one); each plan says how it counts
};

} // namespace f110
