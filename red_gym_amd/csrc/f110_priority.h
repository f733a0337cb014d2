// f110_priority.h -- prioritized replay (Schaul et al.) on the device: an exact integer sum tree over the replay ring's transitions.
// A priority is a uint32 word (fixed point, F110_PRIORITY_SHIFT fraction bits), a node the uint64 sum of its up to 64 children
// (f110_priority_plan.h has the layout), so every sum is exact in any order: the integer atomics below give the same bits in every
// run, and the whole structure is `==` a checker in Python ints.  Nothing takes a slot or a draw number by value from the host.
//   ptree_level_kernel       one wave per node of one level: the sum of its children (rebuild: one launch per level, bottom up)
//   ptree_clear_kernel       one lane per row: atomicExch of the row's leaf to 0; whoever takes a word out subtracts it from every ancestor
//   ptree_raise_kernel       one lane per row: atomicMax of the row's word on its leaf; a lane that raised the leaf adds the difference to
//                            every ancestor (the raises of one leaf telescope to its final word).  set = clear, then raise: 2 launches
//   ptree_pick_kernel        one wave per draw: the descent by prefix sums across lanes and a ballot
//   priority_push_kernel     one wave per level-1 node the pushed row touches: the row's leaves = valid ? qmax : 0 and that node's sum
//   priority_upper_kernel    one workgroup: the nodes above level 1 over a range of leaves, level by level
//   priority_fill_kernel     one lane per leaf: valid ? qmax : 0 (reset, before a rebuild)
//   priority_sample_kernel   one wave per draw: the pick, then replay_sample_nstep_kernel's resolve, action gather and walk
//   priority_weight_kernel   one workgroup: the importance weights of a batch, the counter's and beta's advance
#pragma once
#include "f110_replay.h"
#include "f110_priority_plan.h"

#pragma clang fp contract(off)

namespace f110 {

struct PriorityTree {
    uint32_t *leaf;                 // [L]
    unsigned long long *node;       // [lay.words]
    PriorityLayout lay;
    uint32_t *dev_err;
};

// level 0 = the leaves, level k >= 1 = node level k: child c of that level, 0 beyond its end
__device__ inline unsigned long long pt_child(const PriorityTree &t, int lev, long long c)
{
    if (lev == 0) return c < t.lay.leaves ? (unsigned long long)t.leaf[c] : 0ull;
    return c < t.lay.count[lev - 1] ? t.node[t.lay.offset[lev - 1] + c] : 0ull;
}

__device__ inline unsigned long long pt_wave_sum(unsigned long long v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inclusive prefix sum across the lanes of a wave
__device__ inline unsigned long long pt_wave_scan(unsigned long long v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// grid ceil(count[lev - 1] / 4): node level `lev` from its children
static __global__ __launch_bounds__(PT_THREADS) void ptree_level_kernel(PriorityTree t, int lev)
{
    const int lane = threadIdx.x & 63;
    const long long nd = (long long)blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6);
    if (nd >= t.lay.count[lev - 1]) return;                 // (uniform in the wave)
    const unsigned long long s = pt_wave_sum(pt_child(t, lev - 1, nd * PT_FANOUT + lane));
    if (lane == 0) t.node[t.lay.offset[lev - 1] + nd] = s;
}

// p = pow(double(td) + eps, exponent), q = clamp(llrint(p * 2^16), 1, 2^32 - 1); NaN and +inf give 2^32 - 1.  The device library's pow
// is within an ulp but not exact at exponent 1 (a td on a rounding tie, 2.5 * 2^-16, came out a word high): there p is the sum itself.
__device__ inline uint32_t priority_quantise(float td, double exponent, double eps)
{
    if (td != td || td == __builtin_inff()) return 0xFFFFFFFFu;
    const double s = (double)td + eps;
    const double p = exponent == 1.0 ? s : pow(s, exponent);
    const double x = p * 65536.0;
    if (!(x < 4294967295.0)) return 0xFFFFFFFFu;            // (a NaN of the pow as well)
    if (!(x >= 1.0)) return 1u;
    return (uint32_t)(unsigned long long)rint(x);           // to nearest, ties to even
}

struct PrioritySetArgs {
    PriorityTree tree;
    const long long *idx;           // [n]
    const uint8_t *ok;              // [n] or NULL: every row
    const uint32_t *q_in;           // [n] the words, or NULL: quantised from
    const float *td;                // [n]
    const uint8_t *valid;           // the ring's valid [L], or NULL (the stateless entry)
    int n;
    double exponent, eps;
    uint32_t *q_out;                // [n] or NULL
    uint32_t *qmax;                 // the state's, or NULL
};

// a row that is applied: its index inside the tree, its ok set and (on a ring) its transition valid
__device__ inline bool pt_row_live(const PrioritySetArgs &a, int i, long long &id)
{
    id = a.idx[i];
    if (id < 0 || id >= a.tree.lay.leaves) return false;
    if (a.ok && a.ok[i] == 0) return false;
    return !a.valid || a.valid[id] != 0;
}

// delta (mod 2^64) onto every ancestor of leaf `id`
__device__ inline void pt_add_up(const PriorityTree &t, long long id, unsigned long long delta)
{
    long long c = id;
    for (int k = 0; k < t.lay.levels; k++) {
        c >>= 6;
        F110_BCHK(c >= 0 && c < t.lay.count[k], BT_REPLAY, t.dev_err);
        if (c < t.lay.count[k]) atomicAdd(&t.node[t.lay.offset[k] + c], delta);
    }
}

static __global__ __launch_bounds__(PT_THREADS) void ptree_clear_kernel(PrioritySetArgs a)
{
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= a.n) return;
    long long id;
    if (!pt_row_live(a, i, id)) return;
    const uint32_t old = atomicExch(&a.tree.leaf[id], 0u);
    if (old) pt_add_up(a.tree, id, 0ull - (unsigned long long)old);
}

static __global__ __launch_bounds__(PT_THREADS) void ptree_raise_kernel(PrioritySetArgs a)
{
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (i >= a.n) return;
    long long id;
    const bool live = pt_row_live(a, i, id);
    uint32_t q = 0;
    if (live) {
        q = a.q_in ? a.q_in[i] : priority_quantise(a.td[i], a.exponent, a.eps);
        const uint32_t prev = atomicMax(&a.tree.leaf[id], q);
        if (q > prev) pt_add_up(a.tree, id, (unsigned long long)(q - prev));
        if (a.qmax && q) atomicMax(a.qmax, q);
    }
    if (a.q_out) a.q_out[i] = q;
}

// The draw of one wave: z -> u = mulhi64(z, total), then from the top level down the first child whose inclusive prefix exceeds u.
// Returns the leaf (its word in `q`), -1 with q = 0 for an empty tree.  Every lane returns the same.
__device__ inline long long pt_pick(const PriorityTree &t, unsigned long long z, int lane, uint32_t &q)
{
    int lev = t.lay.levels;
    long long nd = 0;
    unsigned long long v = pt_child(t, lev, (long long)lane);
    unsigned long long pre = pt_wave_scan(v, lane);
    const unsigned long long total = __shfl(pre, 63, 64);
    q = 0;
    if (total == 0) return -1;
    unsigned long long u = __umul64hi(z, total);
    for (;;) {
        const unsigned long long m = __ballot(pre > u);
        F110_BCHK(m != 0, BT_REPLAY, t.dev_err);            // (u < the sum of these children while every node is the sum of its own)
        const int ch = m ? __ffsll((long long)m) - 1 : 63;
        u -= __shfl(pre - v, ch, 64);
        nd = nd * PT_FANOUT + ch;
        if (lev == 0) {
            q = (uint32_t)__shfl(v, ch, 64);
            F110_BCHK(nd < t.lay.leaves && q > 0, BT_REPLAY, t.dev_err);
            if (nd >= t.lay.leaves) { q = 0; return -1; }
            return nd;
        }
        lev--;
        v = pt_child(t, lev, nd * PT_FANOUT + lane);
        pre = pt_wave_scan(v, lane);
    }
}

__device__ inline unsigned long long pt_draw_bits(unsigned long long seed, unsigned long long j)
{
    return replay_splitmix64(seed + 0x9E3779B97F4A7C15ull * (1ull + j * (unsigned long long)F110_REPLAY_TRIES));
}

static __global__ __launch_bounds__(PT_THREADS) void ptree_pick_kernel(PriorityTree t, unsigned long long seed, unsigned long long first, int n,
                                                                       long long *idx_out, uint32_t *q_out)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;                                     // (uniform in the wave)
    uint32_t q;
    const long long id = pt_pick(t, pt_draw_bits(seed, first + (unsigned long long)i), lane, q);
    if (lane == 0) {
        idx_out[i] = id;
        q_out[i] = q;
    }
}

struct PriorityPushArgs {
    PriorityTree tree;
    const uint8_t *valid;           // the ring's [steps, n_envs]
    const long long *count;         // [1] the push just made is number *count (the advance runs behind this)
    long long steps;
    int n_envs;
    const uint32_t *qmax;
};

// grid ceil((n_envs / 64 + 2) / 4): wave w takes level-1 node first + w of the row of step slot count % steps
static __global__ __launch_bounds__(PT_THREADS) void priority_push_kernel(PriorityPushArgs a)
{
    const PriorityTree &t = a.tree;
    const int lane = threadIdx.x & 63;
    const long long count = *a.count;
    F110_BCHK(count >= 0, BT_REPLAY, t.dev_err);
    if (count < 0) return;
    const long long lo = (count % a.steps) * a.n_envs, hi = lo + a.n_envs - 1;
    F110_BCHK(lo >= 0 && hi < t.lay.leaves, BT_REPLAY, t.dev_err);
    if (lo < 0 || hi >= t.lay.leaves) return;
    const long long nd = (lo >> 6) + (long long)blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6);
    if (nd > (hi >> 6)) return;                             // (uniform in the wave)
    const long long p = nd * PT_FANOUT + lane;
    unsigned long long v = 0;
    if (p >= lo && p <= hi) {
        const uint32_t w = a.valid[p] ? *a.qmax : 0u;
        t.leaf[p] = w;
        v = w;
    } else if (p < t.lay.leaves) {
        v = t.leaf[p];                                      // (a neighbouring row's leaves under the same node)
    }
    if (t.lay.levels == 0) return;
    const unsigned long long s = pt_wave_sum(v);
    if (lane == 0) t.node[nd] = s;
}

// one workgroup: every node above level 1 over the leaves lo .. hi (the pushed row: from count), a level at a time
static __global__ __launch_bounds__(PT_THREADS) void priority_upper_kernel(PriorityPushArgs a)
{
    const PriorityTree &t = a.tree;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long count = *a.count;
    if (count < 0) return;
    const long long lo = (count % a.steps) * a.n_envs, hi = lo + a.n_envs - 1;
    if (lo < 0 || hi >= t.lay.leaves) return;
    for (int lev = 2; lev <= t.lay.levels; lev++) {
        const long long first = lo >> (6 * lev), last = hi >> (6 * lev);
        for (long long nd = first + wave; nd <= last; nd += PT_THREADS / 64) {
            F110_BCHK(nd < t.lay.count[lev - 1], BT_REPLAY, t.dev_err);
            if (nd >= t.lay.count[lev - 1]) break;
            const unsigned long long s = pt_wave_sum(pt_child(t, lev - 1, nd * PT_FANOUT + lane));
            if (lane == 0) t.node[t.lay.offset[lev - 1] + nd] = s;
        }
        __threadfence();
        __syncthreads();                                    // the next level reads what the four waves wrote
    }
}

static __global__ __launch_bounds__(PT_THREADS) void priority_fill_kernel(PriorityTree t, const uint8_t *valid, const uint32_t *qmax)
{
    const long long p = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (p < t.lay.leaves) t.leaf[p] = valid[p] ? *qmax : 0u;
}

struct PrioritySampleArgs {
    PriorityTree tree;
    ReplayNstepArgs s;              // the sample form, as replay_sample_nstep_kernel takes it
    uint32_t *prio;                 // [n] the drawn leaf's word
};

// grid ceil(n / 4): one wave per draw.  Every lane reads the counter; nothing in this launch writes it.
static __global__ __launch_bounds__(PT_THREADS) void priority_sample_kernel(PrioritySampleArgs p)
{
    const ReplayNstepArgs &a = p.s;
    const ReplayRing &g = a.ring;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;                                   // (uniform in the wave)
    const unsigned long long first = *a.counter;
    uint32_t q;
    const long long id = pt_pick(p.tree, pt_draw_bits(a.seed, first + (unsigned long long)i), lane, q);
    long long c = 0;
    int env = 0;
    const bool ok = replay_resolve(g, id, c, env);
    F110_BCHK(!ok || (id >= 0 && id < g.steps * g.n_envs), BT_REPLAY, g.dev_err);
    for (int k = lane; k < g.action_dim; k += 64)
        a.a[(size_t)i * (size_t)g.action_dim + (size_t)k] = ok ? g.actions[(size_t)id * (size_t)g.action_dim + (size_t)k] : 0.0f;
    if (lane != 0) return;
    a.idx[i] = id;
    a.s_frame[i] = replay_frame_before(g, ok, c, env);
    a.ok[i] = ok ? 1 : 0;
    p.prio[i] = q;
    replay_walk_store(a, i, ok, c, env);
}

struct PriorityWeightArgs {
    const uint32_t *prio;           // [n]
    const uint8_t *ok;              // [n]
    float *weight;                  // [n]
    int n;
    unsigned long long *counter;    // [1] += n
    f110_priority_state *state;     // beta is read, then advanced
};

// one workgroup: qmin over the rows with ok, weight = (qmin / prio)^beta with the beta read before its advance
static __global__ __launch_bounds__(PT_THREADS) void priority_weight_kernel(PriorityWeightArgs a)
{
    __shared__ uint32_t m[PT_THREADS];
    const int tid = threadIdx.x;
    const double beta = a.state->beta;
    uint32_t mn = 0xFFFFFFFFu;
    for (int i = tid; i < a.n; i += PT_THREADS)
        if (a.ok[i] && a.prio[i] && a.prio[i] < mn) mn = a.prio[i];
    m[tid] = mn;
    __syncthreads();
    for (int w = PT_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w && m[tid + w] < m[tid]) m[tid] = m[tid + w];
        __syncthreads();
    }
    const double qmin = (double)m[0];
    for (int i = tid; i < a.n; i += PT_THREADS) {
        const uint32_t q = a.prio[i];
        a.weight[i] = a.ok[i] && q ? (float)pow(qmin / (double)q, beta) : 0.0f;
    }
    __syncthreads();                                        // every lane has read beta
    if (tid == 0) {
        *a.counter += (unsigned long long)a.n;
        const double next = beta + a.state->beta_step;
        a.state->beta = next < a.state->beta_end ? next : a.state->beta_end;
    }
}

} // namespace f110
