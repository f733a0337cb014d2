// f110_adam_plan.h -- the host side of gradient clipping (f110_adam_clip.h): how a step's tensors are cut into chunks and numbered, which
// chain of a chunk's sum an element belongs to, which chain of the step's sum a chunk's partial belongs to, and the checks of the three
// entry points that need no device.
// Plain C++17 without HIP (tests/test_clip_cpu.py compiles it for the host); the kernels and f110_policy_abi.hip include it.
#pragma once
#include "../../include/f110_hip.h"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define F110_ADAM_HD __host__ __device__
#else
#define F110_ADAM_HD
#endif

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int AC_THREADS = 256;               // lanes of a workgroup = chains of both sums (SL_THREADS: the tree is the losses')
constexpr int AC_CHUNK = F110_ADAM_CHUNK;     // elements of a chunk: adam_kernel's
constexpr int AC_QUADS = AC_CHUNK / (4 * AC_THREADS);   // quads of a chunk per chain
static_assert(AC_QUADS * 4 * AC_THREADS == AC_CHUNK, "a chunk is whole rounds of quads over the chains");
static_assert(sizeof(f110_adam_clip_state) == F110_ADAM_CLIP_STATE_BYTES, "the clip state is 64 bytes");

// chunks of a tensor of n elements: what adam_table counts for it
F110_ADAM_HD inline int64_t adam_chunks(int64_t n) { return (n + AC_CHUNK - 1) / AC_CHUNK; }

// the chain of the chunk partial that takes element j of a chunk (0 <= j < AC_CHUNK): by element index, whatever the access width
F110_ADAM_HD inline int adam_clip_chain(uint32_t j) { return (int)((j >> 2) & (uint32_t)(AC_THREADS - 1)); }

// element number `k` (0 <= k < 4 * AC_QUADS) of chain l, ascending in j
F110_ADAM_HD inline uint32_t adam_clip_element(int l, int k) { return 4u * ((uint32_t)l + (uint32_t)(k >> 2) * AC_THREADS) + (uint32_t)(k & 3); }

// the chain of the step sum that takes the partial of chunk c
F110_ADAM_HD inline int adam_clip_partial_chain(int64_t c) { return (int)(c & (AC_THREADS - 1)); }

// The chunk numbers of one call's tensors: first[i] = the number of tensor i's first chunk (chunk_base + the chunks of the tensors in
// front of it; an empty tensor owns none and gets the next tensor's) -> the chunks of the call.
inline int64_t adam_clip_number(const int64_t *n, int n_tensors, int64_t chunk_base, int64_t *first)
{
    int64_t chunks = 0;
    for (int i = 0; i < n_tensors; i++) {
        if (first) first[i] = chunk_base + chunks;
        chunks += n[i] > 0 ? adam_chunks(n[i]) : 0;
    }
    return chunks;
}

// what f110_adam_gradnorm refuses on its scalars before it looks at the table (chunks: the table's, once counted: pass -1 before)
inline int adam_gradnorm_check(const char *who, int64_t chunk_base, const double *partials, int64_t partials_len, int64_t chunks)
{
    if (!partials) return fail(F110_E_INVALID, "%s: null partials", who);
    if ((uintptr_t)partials % 8) return fail(F110_E_INVALID, "%s: partials is not 8-byte aligned", who);
    if (chunk_base < 0) return fail(F110_E_INVALID, "%s: chunk_base %lld (>= 0)", who, (long long)chunk_base);
    if (partials_len < 0) return fail(F110_E_INVALID, "%s: partials_len %lld (>= 0)", who, (long long)partials_len);
    if (chunks >= 0 && (chunk_base > partials_len || chunks > partials_len - chunk_base))
        return fail(F110_E_INVALID, "%s: the table's %lld chunks behind chunk_base %lld do not fit partials_len %lld", who, (long long)chunks,
                    (long long)chunk_base, (long long)partials_len);
    return F110_OK;
}

inline int adam_clip_check(const char *who, const double *partials, int64_t n_chunks, double max_norm, const f110_adam_clip_state *clip)
{
    if (!partials) return fail(F110_E_INVALID, "%s: null partials", who);
    if (!clip) return fail(F110_E_INVALID, "%s: null clip", who);
    if ((uintptr_t)partials % 8) return fail(F110_E_INVALID, "%s: partials is not 8-byte aligned", who);
    if ((uintptr_t)clip % 8) return fail(F110_E_INVALID, "%s: clip is not 8-byte aligned", who);
    if (n_chunks < 0) return fail(F110_E_INVALID, "%s: n_chunks %lld (>= 0)", who, (long long)n_chunks);
    if (std::isnan(max_norm) || !(max_norm > 0.0)) return fail(F110_E_INVALID, "%s: max_norm %g (> 0; +inf: the guard alone)", who, max_norm);
    return F110_OK;
}

} // namespace f110
