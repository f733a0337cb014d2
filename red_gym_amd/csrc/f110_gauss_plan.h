// f110_gauss_plan.h -- the host side of the policy's Gaussian draws (f110_gauss.h): the kernel's argument struct, the checks of
// f110_gauss_fill and f110_gauss_fill_at that need no device, and the launch plan.
// Plain C++17 without HIP (tests/test_gauss_cpu.py compiles it for the host); f110_gauss_abi.hip launches what it plans.
#pragma once
#include "../../include/f110_hip.h"
#include "f110_launch.h"

#include <cstring>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int GS_THREADS = 256;                   // one lane per element
constexpr unsigned GS_MAX_BLOCKS = 2048;          // 8 workgroups a CU on 256 CUs; beyond GS_MAX_BLOCKS * GS_THREADS elements the lanes stride
constexpr long long GS_MAX_ELEMENTS = 1ll << 31;  // n * A of one call: an element's index and the stride behind it fit 32 bits
static_assert(sizeof(f110_gauss_state) == 64, "the device state is 64 bytes");
static_assert((unsigned long long)GS_MAX_ELEMENTS + (unsigned long long)GS_MAX_BLOCKS * GS_THREADS <= 1ull << 32, "32-bit element index");

struct GaussArgs {
    const f110_gauss_state *state;  // where seed and t = calls[stream] are read on the device, or NULL: `seed` and `t` below
    uint64_t seed, stream, t;
    const int64_t *rows;            // [n] row ids, or NULL: row i is i
    float *out;                     // [n, A]
    uint32_t total, A;              // n * A (2^31 at most) and A
    int vec;                        // 16-byte stores: out is 16-byte aligned
};

// what both entry points refuse before they ask the runtime where the pointers live (by_state: f110_gauss_fill)
inline int gauss_check(const char *who, bool by_state, const f110_gauss_state *state, int32_t stream, int64_t n, int32_t A, const float *out)
{
    if (by_state && !state) return fail(F110_E_INVALID, "%s: null state", who);
    if (by_state && (uintptr_t)state % 8) return fail(F110_E_INVALID, "%s: the state is not 8-byte aligned", who);
    if (stream < 0 || stream >= F110_GAUSS_STREAMS) return fail(F110_E_INVALID, "%s: stream %d (0..%d)", who, stream, F110_GAUSS_STREAMS - 1);
    if (n < 1) return fail(F110_E_INVALID, "%s: n=%lld rows (at least 1)", who, (long long)n);
    if (A < 1 || A > F110_GAUSS_MAX_COLUMNS) return fail(F110_E_INVALID, "%s: A=%d columns (1..%d)", who, A, F110_GAUSS_MAX_COLUMNS);
    if (n > GS_MAX_ELEMENTS / A) return fail(F110_E_INVALID, "%s: n * A = %lld * %d elements (2^31 at most)", who, (long long)n, A);
    if (!out) return fail(F110_E_INVALID, "%s: null out", who);
    if ((uintptr_t)out % 4) return fail(F110_E_INVALID, "%s: out is not 4-byte aligned", who);
    return F110_OK;
}

inline int gauss_rows_check(const char *who, const int64_t *rows)
{
    if ((uintptr_t)rows % 8) return fail(F110_E_INVALID, "%s: rows is not 8-byte aligned", who);
    return F110_OK;
}

// One launch of gauss_fill_kernel: a lane per element up to GS_MAX_BLOCKS workgroups, a grid-stride walk beyond.
struct GaussPlan { GaussArgs a; Launch l; };

inline GaussPlan gauss_plan(int64_t n, int32_t A, const float *out)
{
    GaussPlan p;
    memset(&p.a, 0, sizeof(p.a));
    const long long total = (long long)n * A;
    p.a.total = (uint32_t)total; p.a.A = (uint32_t)A;
    p.a.out = const_cast<float *>(out);
    p.a.vec = (uintptr_t)out % 16 == 0;
    const long long blocks = (total + GS_THREADS - 1) / GS_THREADS;
    p.l = {(unsigned)(blocks < (long long)GS_MAX_BLOCKS ? blocks : (long long)GS_MAX_BLOCKS), 1u, 1u, (unsigned)GS_THREADS, 0, 0};
    return p;
}

} // namespace f110
