// f110_replay.h -- the replay buffer of the reference's RL consumer (src/SAL.py:447-463 ReplayBuffer, pushed at :1000) on the
// device: a ring of T step slots behind the shaper.  A FILL image has two values, so a frame is kept as bits -- a row of
// `cols` pixels is ceil(cols / 64) 64-bit words, bit k of word w = (pixel[64 w + k] == 255), np.packbits(bitorder='little') --
// and once: next_obs of step t is obs of step t + 1, so T step slots own T + 1 frame slots.  Push number c (the device-side
// counter `count`) writes frame slot c % (T + 1) and step slot c % T; its transition is (frame c - 1, action, reward, frame c,
// done).  Nothing here takes a slot by value from the host: every kernel reads `count`, so a captured push replays correctly.
//   replay_push_kernel     one workgroup per env: 16 pixels per lane in one 16-byte load, reduced to 16 bits in registers, one
//                          2-byte store per lane -- a wave reads 1 KiB and writes 128 B, both contiguous; behind a shaper that
//                          holds its image as bits already (f110_bitmap_render_bits) the frame is copied, 16 bytes per lane
//   replay_advance_kernel  one lane: count += 1, behind the push
//   replay_draw_kernel     one lane per draw: splitmix64 candidates over the stored transitions, the first valid one wins
//   replay_gather_kernel   one wave per (sample, frame, 4 rows): bits back to uint8 (4 pixels = one 4-byte store per lane) or fp32
//   replay_locate_kernel   one lane per index: where the gather would read, for consumers that read the bits themselves (f110_bitconv.h)
//   replay_sample_kernel   one lane per draw: the draw, the locate and the gather's tail in one, from a draw counter that lives on the
//                          device (the caller's), so that a captured sample replays with fresh draws
//   replay_counter_advance_kernel  one lane: counter += n, behind the sample
//   replay_nstep_kernel    one lane per index: the truncated n-step return of the transition (replay_walk: up to nstep - 1 dependent
//                          loads of valid, reward and done, one step slot = n_envs cells apart), for indices the caller names
//   replay_sample_nstep_kernel  one lane per draw: replay_sample_kernel with the walk behind the locate; both are kernels of their
//                          own beside the one-step ones, which keep their code
//   replay_stack_kernel    one lane per frame row: the rows of the env's previous stack - 1 frames, walked backwards while the pushes
//                          between them link (up to stack - 1 loads of valid); the oldest row reached fills the rest
#pragma once
#include "../../include/f110_hip.h" // F110_REPLAY_TRIES
#include "f110_bounds.h"
#include "f110_replay_bits.h"

#pragma clang fp contract(off)

namespace f110 {

constexpr int REPLAY_THREADS = 256;
constexpr int REPLAY_ROWS = 16;              // rows of a frame one workgroup of the gather unpacks (4 per wave)

// One image [rows, cols] -> [rows, words] as 16-bit pieces, by the `nthr` threads of a workgroup.  Piece u = row * ch + c holds
// pixels 16 c .. 16 c + 15 of its row (ch = 4 * words; pieces beyond the row are the zero padding).  `img` is 16-byte aligned.
__device__ inline void replay_pack_image(const uint8_t *__restrict__ img, int rows, int cols, uint16_t *__restrict__ out, int tid, int nthr)
{
    const int ch = 4 * replay_words(cols);
    const int units = rows * ch;
    if ((cols & 15) == 0) {
        // rows are whole 16-byte pieces: four independent aligned loads in flight per lane
        const int full = cols >> 4;
        const bool dense = full == ch;            // cols a multiple of 64: piece u is bytes 16 u .. of the image
        for (int u0 = tid; u0 < units; u0 += 4 * nthr) {
            uint4 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = u0 + j * nthr;
                v[j] = make_uint4(0u, 0u, 0u, 0u);
                if (u < units) {
                    if (dense) v[j] = *reinterpret_cast<const uint4 *>(img + 16 * (size_t)u);
                    else {
                        const int r = u / ch, c = u - r * ch;
                        if (c < full) v[j] = *reinterpret_cast<const uint4 *>(img + (size_t)r * (size_t)cols + 16 * (size_t)c);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int u = u0 + j * nthr;
                if (u < units) out[u] = (uint16_t)replay_bits16(v[j]);
            }
        }
        return;
    }
    // a row's byte length is no multiple of 16: its rows start anywhere, whole pieces are read as 16 bytes of alignment 1 and
    // the row's last piece byte by byte under a mask
    for (int u = tid; u < units; u += nthr) {
        const int r = u / ch, c = u - r * ch, col0 = 16 * c;
        const uint8_t *p = img + (size_t)r * (size_t)cols + (size_t)col0;
        unsigned bits = 0;
        if (col0 + 16 <= cols) {
            uint4 v;
            __builtin_memcpy(&v, p, 16);
            bits = replay_bits16(v);
        } else {
            for (int k = 0; k < 16 && col0 + k < cols; k++) bits |= (unsigned)(p[k] == 255) << k;
        }
        out[u] = (uint16_t)bits;
    }
}

// One packed row (NULL: a row of zeros) -> cols pixels of 0 / 255 (uint8) or 0 / `on` (fp32), by the 64 lanes of a wave.  With
// cols a multiple of 4 a lane writes 4 pixels at once (their bits share a word): 4 bytes, or 16 as fp32.
__device__ inline void replay_unpack_row(const uint64_t *__restrict__ prow, int cols, uint8_t *__restrict__ orow, int lane)
{
    if ((cols & 3) == 0) {
        for (int c0 = 4 * lane; c0 < cols; c0 += 256) {
            const unsigned b = prow ? (unsigned)(prow[c0 >> 6] >> (c0 & 63)) & 15u : 0u;
            // bit i -> byte i (exponents i + 7 j are pairwise distinct: no carries), times 255
            *reinterpret_cast<unsigned *>(orow + c0) = ((b * 0x00204081u) & 0x01010101u) * 255u;
        }
        return;
    }
    for (int c = lane; c < cols; c += 64)
        orow[c] = prow && ((prow[c >> 6] >> (c & 63)) & 1ull) ? (uint8_t)255 : (uint8_t)0;
}
__device__ inline void replay_unpack_row(const uint64_t *__restrict__ prow, int cols, float *__restrict__ orow, int lane, float on)
{
    if ((cols & 3) == 0) {
        for (int c0 = 4 * lane; c0 < cols; c0 += 256) {
            const unsigned b = prow ? (unsigned)(prow[c0 >> 6] >> (c0 & 63)) & 15u : 0u;
            *reinterpret_cast<float4 *>(orow + c0) = make_float4(b & 1u ? on : 0.0f, b & 2u ? on : 0.0f, b & 4u ? on : 0.0f, b & 8u ? on : 0.0f);
        }
        return;
    }
    for (int c = lane; c < cols; c += 64)
        orow[c] = prow && ((prow[c >> 6] >> (c & 63)) & 1ull) ? on : 0.0f;
}

__device__ inline unsigned long long replay_splitmix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct ReplayRing {                 // what the three kernels share
    uint64_t *frames;               // [steps + 1, n_envs, rows, words]
    float *actions;                 // [steps, n_envs, action_dim]
    double *rewards;                // [steps, n_envs]
    uint8_t *dones, *valid;         // [steps, n_envs]
    long long *count;               // [1] pushes made
    long long steps;
    int n_envs, rows, cols, action_dim;
    uint32_t *dev_err;
    __device__ size_t frame_words() const { return (size_t)rows * (size_t)replay_words(cols); }
    __device__ uint64_t *frame(long long fs, int env) const { return frames + ((size_t)fs * (size_t)n_envs + (size_t)env) * frame_words(); }
};

// Transition `id` (step slot * n_envs + env) of the ring as `count` stands: false for an index outside the ring, a slot no push
// has reached or an invalid transition; else `c` = the newest push that went to its step slot (its frames are c - 1 and c) and
// `env`.  The addressing the gather and the locate share.
__device__ inline bool replay_resolve(const ReplayRing &g, long long id, long long &c, int &env)
{
    const long long count = *g.count;
    bool ok = id >= 0 && id < g.steps * g.n_envs && count >= 1;
    c = 0;
    env = 0;
    if (ok) {
        const long long slot = id / g.n_envs;
        env = (int)(id - slot * g.n_envs);
        ok = slot <= count - 1 && g.valid[id] != 0;
        if (ok) {
            c = count - 1 - (count - 1 - slot) % g.steps;   // the newest push that went to this step slot
            F110_BCHK(c >= 1 && c % g.steps == slot, BT_REPLAY, g.dev_err);
            ok = c >= 1;                                    // (push 0 has no previous frame and is never valid)
        }
    }
    return ok;
}

// One frame in the ring's format [rows * words] copied as it is, by the `nthr` threads of a workgroup: 16 bytes per access where
// both frames start on a 16-byte boundary (`pairs`: an even word count, the arrays themselves are aligned), else 8.
__device__ inline void replay_copy_frame(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, size_t n_words, int tid, int nthr)
{
    if ((n_words & 1) == 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        const size_t n4 = n_words >> 1;
#pragma unroll 4
        for (size_t i = (size_t)tid; i < n4; i += (size_t)nthr) d4[i] = s4[i];   // (restrict: the unrolled loads go out together)
        return;
    }
    for (size_t i = (size_t)tid; i < n_words; i += (size_t)nthr) dst[i] = src[i];
}

struct ReplayPushArgs {
    ReplayRing ring;
    const uint8_t *bitmap;          // [n_envs, rows, cols] the shaper's image of the scan the step returned, or (exactly one of the two)
    const uint64_t *bitmap_bits;    // [n_envs, rows, words] the same image in the ring's own format
    const float *action_in;         // [n_envs, action_dim]
    const double *total;            // [n_envs] the shaper's reward
    const uint8_t *done;            // [n_envs]
    const double *current_time;     // [n_envs]
    double timestep;
    const long long *chain_start;   // [1] the push number that has no previous frame (install, load_state_dict)
    double *t_seen;                 // [n_envs] clock at the env's previous push (< 0: none)
    uint8_t *last_valid;            // [n_envs] valid as this push decided it
};

struct ReplayDrawArgs {
    ReplayRing ring;
    unsigned long long seed, first; // draw j of this launch is draw number first + j of the stream `seed`
    int n;
    long long *idx;                 // [n] step slot * n_envs + env, or -1
    uint8_t *ok;                    // [n]
};

struct ReplaySampleArgs {
    ReplayRing ring;
    unsigned long long seed;
    const unsigned long long *counter; // [1] draws made so far, on the device: draw i of this launch is draw number *counter + i
    int n;
    long long *idx, *s_frame, *ns_frame; // [n]
    float *a;                       // [n, action_dim]
    double *r;                      // [n]
    uint8_t *d, *ok;                // [n]
};

struct ReplayNstepArgs {
    ReplayRing ring;
    unsigned long long seed;           // the sample form: as ReplaySampleArgs
    const unsigned long long *counter; // [1]
    const long long *idx_in;           // [n] the form that takes its indices from the caller
    int n, nstep;                      // 1 <= nstep <= F110_REPLAY_MAX_NSTEP
    double gamma;
    long long *idx, *s_frame, *ns_frame; // [n]; idx and s_frame: the sample form only
    float *a;                          // [n, action_dim], the sample form only
    double *ret, *discount;            // [n]
    uint8_t *d, *ok;                   // [n]; ok: the sample form only
    int *span;                         // [n]
};

struct ReplayGatherArgs {
    ReplayRing ring;
    const long long *idx;           // [n]
    int n;
    uint8_t *s8, *ns8;              // [n, rows, cols], or
    float *s32, *ns32;              // [n, 1, rows, cols] = pixel * scale
    float on;                       // 255.0f * scale
    float *a;                       // [n, action_dim]
    double *r;                      // [n]
    uint8_t *d, *ok;                // [n]
};

struct ReplayPackArgs {
    const uint8_t *bitmaps;         // [n, rows, cols]
    uint64_t *packed;               // [n, rows, words]
    int rows, cols;
};

static __global__ __launch_bounds__(REPLAY_THREADS) void replay_push_kernel(ReplayPushArgs a)
{
    const ReplayRing &g = a.ring;
    const int env = blockIdx.x, tid = threadIdx.x;
    const long long count = *g.count;
    F110_BCHK(count >= 0, BT_REPLAY, g.dev_err);
    if (count < 0) return;
    const long long fs = count % (g.steps + 1), ss = count % g.steps;
    F110_BCHK(fs >= 0 && fs <= g.steps && ss >= 0 && ss < g.steps, BT_REPLAY, g.dev_err);
    if (a.bitmap_bits)
        replay_copy_frame(a.bitmap_bits + (size_t)env * g.frame_words(), g.frame(fs, env), g.frame_words(), tid, REPLAY_THREADS);
    else
        replay_pack_image(a.bitmap + (size_t)env * (size_t)g.rows * (size_t)g.cols, g.rows, g.cols,
                          reinterpret_cast<uint16_t *>(g.frame(fs, env)), tid, REPLAY_THREADS);
    const size_t cell = (size_t)ss * (size_t)g.n_envs + (size_t)env;
    for (int k = tid; k < g.action_dim; k += REPLAY_THREADS)
        g.actions[cell * (size_t)g.action_dim + (size_t)k] = a.action_in[(size_t)env * (size_t)g.action_dim + (size_t)k];
    if (tid == 0) {
        // the clock idiom of f110_shaping.h: an env's clock reads exactly `timestep` iff the last step that touched it was
        // its reset (terminal frame -> spawn frame is no transition); a clock that stands still was not stepped by the call
        const double now = a.current_time[env], seen = a.t_seen[env];
        const uint8_t v = count > *a.chain_start && now != a.timestep && now != seen ? 1 : 0;
        g.rewards[cell] = a.total[env];
        g.dones[cell] = a.done[env] != 0 ? 1 : 0;
        g.valid[cell] = v;
        a.last_valid[env] = v;
        a.t_seen[env] = now;
    }
}

static __global__ void replay_advance_kernel(long long *count)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *count += 1;
}

// Draw number j of the stream `seed` over the ring as `count` stands: the first of F110_REPLAY_TRIES splitmix64 candidates whose
// transition is valid, or -1.  What the draw and the sample share.
__device__ inline long long replay_pick(const ReplayRing &g, unsigned long long seed, unsigned long long j)
{
    const long long count = *g.count;
    const long long stored = count < 0 ? 0 : (count < g.steps ? count : g.steps);
    const unsigned long long total = (unsigned long long)stored * (unsigned long long)g.n_envs;
    if (total == 0) return -1;
    for (int k = 0; k < F110_REPLAY_TRIES; k++) {
        const unsigned long long z = replay_splitmix64(seed + 0x9E3779B97F4A7C15ull * (1ull + j * (unsigned long long)F110_REPLAY_TRIES + (unsigned long long)k));
        const unsigned long long cand = __umul64hi(z, total);
        const long long age = (long long)(cand / (unsigned long long)g.n_envs), env = (long long)(cand % (unsigned long long)g.n_envs);
        const long long slot = (count - 1 - age) % g.steps;
        F110_BCHK(age < stored && slot >= 0 && slot < g.steps, BT_REPLAY, g.dev_err);
        const long long id = slot * g.n_envs + env;
        if (g.valid[id]) return id;
    }
    return -1;
}

static __global__ __launch_bounds__(REPLAY_THREADS) void replay_draw_kernel(ReplayDrawArgs a)
{
    const int i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const long long pick = replay_pick(a.ring, a.seed, a.first + (unsigned long long)i);
    a.idx[i] = pick;
    a.ok[i] = pick >= 0 ? 1 : 0;
}

// grid (n, ceil(rows / REPLAY_ROWS), 2): z = 0 the transition's frame before (s), z = 1 its frame after (ns)
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_gather_kernel(ReplayGatherArgs a)
{
    const ReplayRing &g = a.ring;
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long id = a.idx[i];
    long long c = 0;
    int env = 0;
    const bool ok = replay_resolve(g, id, c, env);
    const uint64_t *frame = nullptr;
    if (ok) {
        const long long fs = (blockIdx.z ? c : c - 1) % (g.steps + 1);
        F110_BCHK(fs >= 0 && fs <= g.steps, BT_REPLAY, g.dev_err);
        frame = g.frame(fs, env);
    }
    const int W = replay_words(g.cols);
    const size_t img = (size_t)i * (size_t)g.rows * (size_t)g.cols;
    uint8_t *o8 = blockIdx.z ? a.ns8 : a.s8;
    float *o32 = blockIdx.z ? a.ns32 : a.s32;
    for (int rr = 0; rr < REPLAY_ROWS / 4; rr++) {
        const int row = blockIdx.y * REPLAY_ROWS + wave * (REPLAY_ROWS / 4) + rr;
        if (row >= g.rows) break;
        const uint64_t *prow = frame ? frame + (size_t)row * (size_t)W : nullptr;
        if (o8) replay_unpack_row(prow, g.cols, o8 + img + (size_t)row * (size_t)g.cols, lane);
        else replay_unpack_row(prow, g.cols, o32 + img + (size_t)row * (size_t)g.cols, lane, a.on);
    }
    if (blockIdx.y == 0 && blockIdx.z == 0) {
        for (int k = tid; k < g.action_dim; k += REPLAY_THREADS)
            a.a[(size_t)i * (size_t)g.action_dim + (size_t)k] = ok ? g.actions[(size_t)id * (size_t)g.action_dim + (size_t)k] : 0.0f;
        if (tid == 0) {
            a.r[i] = ok ? g.rewards[id] : 0.0;
            a.d[i] = ok ? g.dones[id] : (uint8_t)0;
            a.ok[i] = ok ? 1 : 0;
        }
    }
}

// The row of the frame tensor viewed as [(steps + 1) * n_envs, rows, words] that holds the frame before push `c` of `env`, as
// replay_resolve gave them; -1 for a refused transition.
__device__ inline long long replay_frame_before(const ReplayRing &g, bool ok, long long c, int env)
{
    return ok ? ((c - 1) % (g.steps + 1)) * g.n_envs + env : -1;
}

// one lane per index: the rows of the frame tensor viewed as [(steps + 1) * n_envs, rows, words] that hold the transition's frame
// before and its frame after, -1 for both where the gather would write zeros
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_locate_kernel(ReplayRing g, const long long *idx, int n, long long *s_frame, long long *ns_frame)
{
    const int i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i >= n) return;
    long long c = 0;
    int env = 0;
    const bool ok = replay_resolve(g, idx[i], c, env);
    s_frame[i] = replay_frame_before(g, ok, c, env);
    ns_frame[i] = ok ? (c % (g.steps + 1)) * g.n_envs + env : -1;
}

// one lane per draw: draw number *counter + i (replay_pick), where its two frames lie (the locate) and its action, reward and done
// (the gather's tail); -1, -1 and zeros with ok = 0 where no valid transition was found.  Every lane reads the counter; nothing in
// this launch writes it (replay_counter_advance_kernel behind it does).
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_sample_kernel(ReplaySampleArgs a)
{
    const ReplayRing &g = a.ring;
    const int i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long first = *a.counter;
    const long long id = replay_pick(g, a.seed, first + (unsigned long long)i);
    long long c = 0;
    int env = 0;
    const bool ok = replay_resolve(g, id, c, env);
    F110_BCHK(!ok || (id >= 0 && id < g.steps * g.n_envs), BT_REPLAY, g.dev_err);
    a.idx[i] = id;
    a.s_frame[i] = replay_frame_before(g, ok, c, env);
    a.ns_frame[i] = ok ? (c % (g.steps + 1)) * g.n_envs + env : -1;
    for (int k = 0; k < g.action_dim; k++)
        a.a[(size_t)i * (size_t)g.action_dim + (size_t)k] = ok ? g.actions[(size_t)id * (size_t)g.action_dim + (size_t)k] : 0.0f;
    a.r[i] = ok ? g.rewards[id] : 0.0;
    a.d[i] = ok ? g.dones[id] : (uint8_t)0;
    a.ok[i] = ok ? 1 : 0;
}

// The truncated n-step return of the transition replay_resolve gave as (ok, push c0, env); the contract is include/f110_hip.h's.
// span m = the pushes c0 .. c0 + m - 1 walked: the walk goes on to push c = c0 + m while m < nstep, push c - 1 was not done, c is
// stored (c <= count - 1: it is then still in the ring, because c0 is the newest push of its slot and so is every later one) and
// valid.  ret = r_0 + g r_1 + ..., g the running product of gamma, every product and sum rounded on its own in fp64 (this file
// compiles with contraction off); discount = g behind the last step (gamma for m = 1); d = done of push c0 + m - 1, and ns_frame
// the row of its frame after in the frame tensor viewed as [(steps + 1) * n_envs, rows, words].  A refused row is the zero transition
// with discount = gamma.  The two moduli differ: step slots wrap at `steps`, frame slots at `steps + 1`.
__device__ inline void replay_walk(const ReplayRing &g, bool ok, long long c0, int env, int nstep, double gamma, long long &ns_frame, double &ret,
                                   double &discount, uint8_t &d, int &span)
{
    ns_frame = -1;
    ret = 0.0;
    discount = gamma;
    d = 0;
    span = 0;
    if (!ok) return;
    const long long count = *g.count;
    const long long s0 = c0 % g.steps;
    F110_BCHK(c0 >= 1 && c0 <= count - 1 && s0 >= 0 && s0 < g.steps && env >= 0 && env < g.n_envs, BT_REPLAY, g.dev_err);
    const size_t cell0 = (size_t)s0 * (size_t)g.n_envs + (size_t)env;
    double R = g.rewards[cell0], gk = gamma;
    uint8_t dn = g.dones[cell0];
    int m = 1;
    while (m < nstep && dn == 0) {
        const long long c = c0 + m;
        if (c > count - 1) break;                       // the newest push ends the span
        const long long ss = c % g.steps;
        F110_BCHK(ss >= 0 && ss < g.steps, BT_REPLAY, g.dev_err);
        const size_t cell = (size_t)ss * (size_t)g.n_envs + (size_t)env;
        if (g.valid[cell] == 0) break;                  // a reset, an env not stepped, a chain break: the span ends in front of it
        R = R + gk * g.rewards[cell];
        gk = gk * gamma;
        dn = g.dones[cell];
        m++;
    }
    const long long fs = (c0 + m - 1) % (g.steps + 1);
    F110_BCHK(fs >= 0 && fs <= g.steps, BT_REPLAY, g.dev_err);
    ns_frame = fs * g.n_envs + env;
    ret = R;
    discount = gk;
    d = dn;
    span = m;
}

// The walk from (ok, push c, env), stored as row i: what every kernel with the walk ends in.
__device__ inline void replay_walk_store(const ReplayNstepArgs &a, int i, bool ok, long long c, int env)
{
    long long ns_frame;
    double ret, discount;
    uint8_t d;
    int span;
    replay_walk(a.ring, ok, c, env, a.nstep, a.gamma, ns_frame, ret, discount, d, span);
    a.ns_frame[i] = ns_frame;
    a.ret[i] = ret;
    a.discount[i] = discount;
    a.d[i] = d;
    a.span[i] = span;
}

// one lane per index: the walk from the transition the caller names
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_nstep_kernel(ReplayNstepArgs a)
{
    const ReplayRing &g = a.ring;
    const int i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i >= a.n) return;
    long long c = 0;
    int env = 0;
    const bool ok = replay_resolve(g, a.idx_in[i], c, env);
    replay_walk_store(a, i, ok, c, env);
}

// one lane per draw: replay_sample_kernel's draw, frame before and action, then the walk for the frame after, the return, done, the
// discount and the span.  Every lane reads the counter; nothing in this launch writes it.
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_sample_nstep_kernel(ReplayNstepArgs a)
{
    const ReplayRing &g = a.ring;
    const int i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long first = *a.counter;
    const long long id = replay_pick(g, a.seed, first + (unsigned long long)i);
    long long c = 0;
    int env = 0;
    const bool ok = replay_resolve(g, id, c, env);
    F110_BCHK(!ok || (id >= 0 && id < g.steps * g.n_envs), BT_REPLAY, g.dev_err);
    a.idx[i] = id;
    a.s_frame[i] = replay_frame_before(g, ok, c, env);
    for (int k = 0; k < g.action_dim; k++)
        a.a[(size_t)i * (size_t)g.action_dim + (size_t)k] = ok ? g.actions[(size_t)id * (size_t)g.action_dim + (size_t)k] : 0.0f;
    a.ok[i] = ok ? 1 : 0;
    replay_walk_store(a, i, ok, c, env);
}

struct ReplayStackArgs {
    ReplayRing ring;
    const long long *rows_in;       // [n] rows of the frame tensor, or NULL: row i = env i's newest frame (n = n_envs)
    int n, stack;                   // 1 <= stack <= F110_REPLAY_MAX_STACK
    long long *rows_out;            // [n, stack]
    int *depth;                     // [n]
};

// one lane per row: the backward walk, the mirror of replay_walk (the contract is include/f110_hip.h's "Frame stacks").  Frame row
// -> the push c that wrote it (the newest one of its frame slot), then the frames c - 1, c - 2, ... of the same env while push c - j
// + 1 links: it is still in the ring (>= count - steps; >= 1, because push 0 has no frame before it) and valid.  The loads of valid
// do not depend on one another; frame slots wrap at steps + 1, step slots at steps.
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_stack_kernel(ReplayStackArgs a)
{
    const ReplayRing &g = a.ring;
    const int i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const long long count = *g.count, F = g.steps + 1;
    long long c = 0;
    int env = 0;
    bool ok = count >= 1;
    if (a.rows_in) {
        const long long row = a.rows_in[i];
        ok = ok && row >= 0 && row < F * g.n_envs;
        if (ok) {
            const long long slot = row / g.n_envs;
            env = (int)(row - slot * g.n_envs);
            ok = slot <= count - 1;                       // a slot no push has written
            c = count - 1 - (count - 1 - slot) % F;       // the newest push that went to this frame slot
        }
    } else {
        env = i;
        c = count - 1;
        ok = ok && env < g.n_envs;
    }
    long long *o = a.rows_out + (size_t)i * (size_t)a.stack;
    if (!ok) {
        for (int j = 0; j < a.stack; j++) o[j] = -1;
        a.depth[i] = 0;
        return;
    }
    F110_BCHK(c >= 0 && c <= count - 1 && c >= count - F && env >= 0 && env < g.n_envs, BT_REPLAY, g.dev_err);
    const long long oldest = count - g.steps;             // the oldest push whose step slot is still the ring's
    long long row = (c % F) * g.n_envs + env;
    int depth = 1;
    bool linked = true;
    o[0] = row;
    for (int j = 1; j < a.stack; j++) {
        const long long p = c - j + 1;                    // the push that links frame c - j + 1 to frame c - j
        linked = linked && p >= 1 && p >= oldest;
        if (linked) {
            const long long ss = p % g.steps;
            F110_BCHK(ss >= 0 && ss < g.steps, BT_REPLAY, g.dev_err);
            linked = g.valid[(size_t)ss * (size_t)g.n_envs + (size_t)env] != 0;
        }
        if (linked) {
            const long long fs = (p - 1) % F;
            F110_BCHK(fs >= 0 && fs <= g.steps, BT_REPLAY, g.dev_err);
            row = fs * g.n_envs + env;
            depth++;
        }
        o[j] = row;
    }
    a.depth[i] = depth;
}

static __global__ void replay_counter_advance_kernel(unsigned long long *counter, unsigned long long n)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *counter += n;
}

static __global__ __launch_bounds__(REPLAY_THREADS) void replay_pack_kernel(ReplayPackArgs a)
{
    const size_t i = blockIdx.x;
    replay_pack_image(a.bitmaps + i * (size_t)a.rows * (size_t)a.cols, a.rows, a.cols,
                      reinterpret_cast<uint16_t *>(a.packed + i * (size_t)a.rows * (size_t)replay_words(a.cols)), threadIdx.x, REPLAY_THREADS);
}

// grid (n, ceil(rows / REPLAY_ROWS))
static __global__ __launch_bounds__(REPLAY_THREADS) void replay_unpack_kernel(ReplayPackArgs a, uint8_t *out)
{
    const size_t i = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = replay_words(a.cols);
    for (int rr = 0; rr < REPLAY_ROWS / 4; rr++) {
        const int row = blockIdx.y * REPLAY_ROWS + wave * (REPLAY_ROWS / 4) + rr;
        if (row >= a.rows) break;
        replay_unpack_row(a.packed + (i * (size_t)a.rows + (size_t)row) * (size_t)W, a.cols,
                          out + (i * (size_t)a.rows + (size_t)row) * (size_t)a.cols, lane);
    }
}

} // namespace f110
