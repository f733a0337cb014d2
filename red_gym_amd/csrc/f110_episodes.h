// f110_episodes.h -- the episode of the reference's training loop (src/SAL.py:986-1015: `ep_reward = 0; for st in range(max_steps):
// ... ep_reward += reward; if done: break`) for every env, behind the step: the return and the length of the running episode, a step
// limit per env that ends an episode the env itself would never end, and a log of the finished ones.  One lane per env.  An
// episode's end appends one record to a ring of L records; within one update the records stand in ascending env order, record k of
// the run in slot k % L -- a stream compaction in a fixed order, without atomics (a slot taken by an atomic would depend on
// scheduling, and this project's replays are `==`):
//   episodes_count_kernel    decides for every env whether this update closes its episode (episode_rule: it reads, it writes no
//                            state) and stores the number of closing envs of each workgroup in block_counts
//   episodes_update_kernel   decides again -- nothing the rule reads has changed -- and ranks the closing envs: inside a wave by a
//                            ballot and the popcount of the lower lanes, across the waves of a workgroup through 4 LDS words, across
//                            workgroups by summing block_counts below its own (every workgroup sums the whole list: at most
//                            ceil(B / 256) ints, L2-resident).  Rank g of `total` goes to slot (count + g) % L if g >= total - L (of
//                            more than L closing envs only the last L are written, each to its own slot); then the env's state is
//                            updated.  `count` is read by every lane and written by none.
//   episodes_advance_kernel  one wave: count += sum(block_counts), behind the writes, so that a captured update replays with fresh
//                            slots (the idiom of replay_advance_kernel, f110_replay.h)
// gfx950, hipcc -O3: count 12 VGPRs / 28 SGPRs, update 37 VGPRs / 68 SGPRs, advance 9 VGPRs / 15 SGPRs; LDS 16 / 80 / 0 bytes; no
// scratch, no spills (tools/kernel_resources.py).  fp64 adds in step order, no contraction.
#pragma once
#include "../../include/f110_hip.h" // F110_EPISODE_*, F110_EPISODES_BLOCK
#include "f110_bounds.h"
#include "f110_device.h"

#pragma clang fp contract(off)

namespace f110 {

constexpr int EPISODES_THREADS = F110_EPISODES_BLOCK; // one entry of the caller's block_counts per workgroup
constexpr int EPISODES_WAVES = EPISODES_THREADS / 64;

struct EpisodesArgs {
    int n;                          // envs
    int log;                        // L: records the ring holds
    int limit_all;                  // the step limit of every env while `limit` is NULL
    double timestep;
    const double *reward;           // [n] the reward of the step just made, or NULL: `timestep`, the constant the env pays
    const uint8_t *done;            // [n]
    const double *current_time;     // [n] the envs' clocks
    const int32_t *laps;            // laps of env e: laps[e * laps_stride], or NULL: 0 is logged
    long long laps_stride;
    uint8_t *pending_reset;         // [n] raised with a LIMIT, or NULL: autoreset is off
    double *ep_return;              // [n] state
    int32_t *ep_length;             // [n]
    uint8_t *ep_open;               // [n]
    double *t_seen;                 // [n]
    uint8_t *truncated;             // [n]
    const int32_t *limit;           // [n] or NULL
    int32_t *log_env, *log_length, *log_laps; // [L]
    double *log_return, *log_time;  // [L]
    uint8_t *log_reason;            // [L]
    const long long *count;         // [1] episodes closed before this update
    int32_t *block_counts;          // [ceil(n / EPISODES_THREADS)] scratch
    uint32_t *dev_err;
};

enum { EP_IDLE, EP_RESET, EP_STEP, EP_CLOSED };  // what the last step was to the env: nothing, its reset, a step, a step of a closed episode

// What this update is to env `env`, from what the step left and the state of the previous update; `reason` = the record it appends
// (0: none).  Reads only; both kernels call it on the same values.
__device__ inline int episode_rule(const EpisodesArgs &a, int env, int &reason)
{
    reason = 0;
    const double now = a.current_time[env], seen = a.t_seen[env];
    const bool open = a.ep_open[env] != 0;
    if (now == seen) return EP_IDLE;                       // not stepped since its previous update (a masked reset left it alone)
    if (now == a.timestep) {                               // reset by its last step (f110_shaping.h): the reference's env.reset()
        if (open && a.ep_length[env] > 0) reason = F110_EPISODE_RESET;   // a masked reset by the user cut a running episode
        return EP_RESET;
    }
    if (!open) return EP_CLOSED;                           // closed and stepping on (autoreset off): frozen until the reset
    const int lim = a.limit ? a.limit[env] : a.limit_all;
    if (a.done[env] != 0) reason = F110_EPISODE_DONE;
    else if (lim > 0 && a.ep_length[env] + 1 >= lim) reason = F110_EPISODE_LIMIT;
    return EP_STEP;
}

// The closing lanes of a workgroup in thread order: this lane's rank among them and their number.  Every thread of the workgroup
// calls it (two barriers).
__device__ inline void episodes_block_rank(bool closes, int *wave_counts, int &rank, int &block_total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = vote(closes);
    if (lane == 0) wave_counts[wave] = __popcll(m);
    __syncthreads();
    rank = __popcll(m & ((1ull << lane) - 1ull));
    block_total = 0;
#pragma unroll
    for (int w = 0; w < EPISODES_WAVES; w++) {
        const int c = wave_counts[w];
        if (w < wave) rank += c;
        block_total += c;
    }
    __syncthreads();                                       // (wave_counts may be written again)
}

static __global__ __launch_bounds__(EPISODES_THREADS) void episodes_count_kernel(EpisodesArgs a)
{
    __shared__ int wave_counts[EPISODES_WAVES];
    const int env = blockIdx.x * EPISODES_THREADS + threadIdx.x;
    int reason = 0;
    if (env < a.n) episode_rule(a, env, reason);
    int rank, total;
    episodes_block_rank(reason != 0, wave_counts, rank, total);
    if (threadIdx.x == 0) a.block_counts[blockIdx.x] = total;
}

static __global__ __launch_bounds__(EPISODES_THREADS) void episodes_update_kernel(EpisodesArgs a)
{
    __shared__ int wave_counts[EPISODES_WAVES];
    __shared__ long long sums[2 * EPISODES_WAVES];
    const int env = blockIdx.x * EPISODES_THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int reason = 0, what = EP_IDLE;
    if (env < a.n) what = episode_rule(a, env, reason);
    int rank, block_total;
    episodes_block_rank(reason != 0, wave_counts, rank, block_total);
    // closing envs of the workgroups below this one, and of all: integer sums, any order gives the same
    long long below = 0, all = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += EPISODES_THREADS) {
        const long long c = a.block_counts[b];
        all += c;
        if (b < (int)blockIdx.x) below += c;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { below += __shfl_xor(below, s, 64); all += __shfl_xor(all, s, 64); }
    if (lane == 0) { sums[wave] = below; sums[EPISODES_WAVES + wave] = all; }
    __syncthreads();
    below = 0; all = 0;
#pragma unroll
    for (int w = 0; w < EPISODES_WAVES; w++) { below += sums[w]; all += sums[EPISODES_WAVES + w]; }
    if (env >= a.n || what == EP_IDLE) return;
    const double now = a.current_time[env];
    if (what == EP_CLOSED) { a.t_seen[env] = now; return; }
    int length = a.ep_length[env];
    double ret = a.ep_return[env];
    if (what == EP_STEP) {
        ret = ret + (a.reward ? a.reward[env] : a.timestep);  // ep_reward += reward
        length += 1;
    }
    if (reason) {
        const long long g = below + rank, count = *a.count;
        F110_BCHK(g >= 0 && g < all && count >= 0, BT_EPISODES, a.dev_err);
        if (g >= all - (long long)a.log && count >= 0) {
            const long long slot = (count + g) % (long long)a.log;
            a.log_env[slot] = env; a.log_length[slot] = length; a.log_return[slot] = ret; a.log_reason[slot] = (uint8_t)reason;
            a.log_time[slot] = now; a.log_laps[slot] = a.laps ? a.laps[(size_t)env * (size_t)a.laps_stride] : 0;
        }
    }
    if (what == EP_RESET) {
        a.ep_return[env] = 0.0; a.ep_length[env] = 0; a.ep_open[env] = 1; a.truncated[env] = 0;
    } else {
        a.ep_return[env] = ret; a.ep_length[env] = length;
        if (reason) {
            a.ep_open[env] = 0;
            if (reason == F110_EPISODE_LIMIT) {
                a.truncated[env] = 1;
                if (a.pending_reset) a.pending_reset[env] = 1;   // what env_kernel raises on `done`: the next step respawns the env
            }
        }
    }
    a.t_seen[env] = now;
}

static __global__ __launch_bounds__(64) void episodes_advance_kernel(long long *count, const int32_t *block_counts, int blocks)
{
    long long sum = 0;
    for (int b = threadIdx.x; b < blocks; b += 64) sum += block_counts[b];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) sum += __shfl_xor(sum, s, 64);
    if (threadIdx.x == 0) *count += sum;
}

} // namespace f110
