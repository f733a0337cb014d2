// f110_env.h -- the step either side of the scan: dynamics_kernel (lane per car), env_kernel (lane per env) or, when A > 1,
// post_scan_kernel in its place, check_done_kernel and pack_env_kernel.
#pragma once
#include "f110_bounds.h"
#include "f110_device.h"
#include "f110_noise.h"    // NoiseDesc
#include "f110_opponents.h" // post_scan_kernel calls opp_setup_body

#pragma clang fp contract(off)

namespace f110 {

// ------------------------------------------------------------------ dynamics (lane per car)
struct DynArgs {
    int n_cars, agents;
    double *state;        // [N,7]
    double *steer_buf;    // [N,2]
    int32_t *steer_cnt;   // [N]
    int32_t *noise_step;  // [N] or NULL
    const double *actions;// [N,2] (steer, speed)
    const double *spawn;  // [N,3] or NULL
    const uint8_t *pending_reset; // [B] or NULL
    uint8_t *was_pending; // [B] or NULL: pending_reset as this step found it (env_kernel clears / re-arms the flag itself)
    int reset_only;
    double *pose_snap;    // [N,3] or NULL
    uint8_t *in_collision;// [N] or NULL: cleared here, set by scan_kernel
    // Vehicle parameters: [slots, 1 + agents] -- per params slot (= the `params` one reference env was constructed with,
    // f110_env.py:125-128) entry 0 is Simulator.params (GJK vertices, base_classes.py:542), entry 1 + i RaceCar.params of
    // agent i (:84,169, changed by update_params :507-527)
    const Params *params;
    const int32_t *env_params;  // [B] params slot of every env, or NULL (all envs on slot 0)
    double time_step;
    int integrator;
    int param_slots;            // slots `params` holds (read by the bounds-checked build only)
    uint32_t *dev_err;          // device error word
    const NoiseDesc *noise;     // the rows the noise table holds (or NULL): the scan behind this kernel reads row noise_step[car] unchecked
};

// The single-track model switches to its kinematic form below 0.5 m/s (dynamic_models.py:152): a wavefront that holds
// one slow car among 63 fast ones executes BOTH forms at every RK4 stage (the slow form is a third of the instructions
// of a step, and with autoreset a few per cent of the cars are always just leaving their spawn pose -- enough to put a
// slow car into most wavefronts).  The block therefore deals its cars out so that the slow ones (and the idle lanes)
// share the LAST wavefronts: lane l works on car s_perm[l], the others' waves skip the kinematic code altogether.
// Which lane integrates a car does not change a bit of its result.
static __global__ __launch_bounds__(256) void dynamics_kernel(DynArgs a)
{
    __shared__ int s_perm[256];
    __shared__ int s_cnt[2][4]; // per wave: fast cars, slow cars
    int car;
    {
        const int c0 = blockIdx.x * blockDim.x + threadIdx.x;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        bool work = c0 < a.n_cars, slow = true;
        if (work) {
            const bool pend0 = a.pending_reset && a.pending_reset[c0 / a.agents];
            if (a.reset_only && !pend0) work = false;
            else slow = pend0 || !(fabs(a.state[(size_t)c0 * 7 + 3]) >= 0.5); // a reset car starts at rest
        }
        const unsigned long long mf = __builtin_amdgcn_ballot_w64(work && !slow), ms = __builtin_amdgcn_ballot_w64(work && slow);
        if (lane == 0) { s_cnt[0][wave] = __popcll(mf); s_cnt[1][wave] = __popcll(ms); }
        for (int i = threadIdx.x; i < 256; i += blockDim.x) s_perm[i] = -1;
        __syncthreads();
        int fast_before = 0, slow_before = 0, fast_total = 0, slow_total = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) { fast_before += s_cnt[0][w]; slow_before += s_cnt[1][w]; }
            fast_total += s_cnt[0][w]; slow_total += s_cnt[1][w];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        // fast cars fill the block's lanes from the front, slow cars from the back (idle lanes in between)
        if (work && !slow) s_perm[fast_before + __popcll(mf & below)] = c0;
        if (work && slow) s_perm[255 - (slow_before + __popcll(ms & below))] = c0;
        __syncthreads();
        car = s_perm[threadIdx.x];
        (void)fast_total; (void)slow_total;
    }
    if (car < 0) return;
    const int env = car / a.agents;
    const bool pend = a.pending_reset && a.pending_reset[env];
    if (a.was_pending) a.was_pending[env] = pend ? 1 : 0; // (every car of the env stores the same byte)
    double st[7], sb[2];
    int sc;
    double steer, speed;
    if (pend) {
        // RaceCar.reset (base_classes.py:181-202) followed by the zero-action step of
        // F110Env.reset (f110_env.py:335-336)
#pragma unroll
        for (int i = 0; i < 7; i++) st[i] = 0.;
        st[0] = a.spawn[(size_t)car * 3];
        st[1] = a.spawn[(size_t)car * 3 + 1];
        st[4] = a.spawn[(size_t)car * 3 + 2];
        sb[0] = sb[1] = 0.;
        sc = 0;
        steer = 0.;
        speed = 0.;
        if (a.noise_step) a.noise_step[car] = 0;
    } else {
#pragma unroll
        for (int i = 0; i < 7; i++) st[i] = a.state[(size_t)car * 7 + i];
        sb[0] = a.steer_buf[(size_t)car * 2];
        sb[1] = a.steer_buf[(size_t)car * 2 + 1];
        sc = a.steer_cnt[car];
        steer = a.actions[(size_t)car * 2];
        speed = a.actions[(size_t)car * 2 + 1];
    }
    // (the noise window's bounds and the car's row travel with the loads above: read after the stores below they were one more
    // memory round trip at the end of a kernel that is nothing but latency)
    int nrow = 0, nlo = 0, nhi = 0x7fffffff;
    if (a.noise && a.noise_step) { nrow = pend ? 0 : a.noise_step[car]; nlo = a.noise->lo; nhi = a.noise->hi; }
    const Params P = a.params[(size_t)params_slot_of(a.env_params, env, a.param_slots, a.dev_err) * (a.agents + 1) + 1 + car % a.agents];
    update_pose(st, sb, sc, steer, speed, P, a.time_step, a.integrator);
#pragma unroll
    for (int i = 0; i < 7; i++) a.state[(size_t)car * 7 + i] = st[i];
    a.steer_buf[(size_t)car * 2] = sb[0];
    a.steer_buf[(size_t)car * 2 + 1] = sb[1];
    a.steer_cnt[car] = sc;
    if (a.in_collision) a.in_collision[car] = 0;
    // the host keeps the noise table ahead of every car (Engine.ready_noise); a row outside it is reported, never silent
    if (__builtin_expect(nrow < nlo || nrow >= nhi, 0))
        if (a.dev_err) atomicOr(a.dev_err, DEVERR_NOISE_WINDOW);
    if (a.pose_snap) {
        a.pose_snap[(size_t)car * 3] = st[0];
        a.pose_snap[(size_t)car * 3 + 1] = st[1];
        a.pose_snap[(size_t)car * 3 + 2] = st[4];
    }
}

// ------------------------------------------------------------------ env bookkeeping (lane per env)
struct EnvArgs {
    int n_envs, agents, ego_idx, autoreset, reset_only;
    double *state;            // [N,7]: state[3:] zeroed here on an iTTC hit
    int32_t *noise_step;      // [N]: one noise row consumed per scan
    const double *pose_snap;  // [N,3]
    const double *spawn;      // [N,3]
    const uint8_t *in_collision; // [N]
    uint8_t *collisions;      // [N]
    int32_t *collision_idx;   // [N]
    double *start_rot;        // [B,4]
    uint8_t *near_start;      // [N]
    int32_t *toggles;         // [N]
    int32_t *lap_counts;      // [N]
    double *lap_times;        // [N]
    double *current_time;     // [B]
    uint8_t *pending_reset;   // [B]
    uint8_t *done;            // [B]
    uint8_t *checkpoint_done; // [N] or NULL
    const Params *params;     // [slots, 1 + agents] (see DynArgs): entry 0 of the env's slot sizes the GJK quads
    const int32_t *env_params;// [B] or NULL
    double time_step;
    int param_slots;          // (bounds-checked build only)
    uint32_t *dev_err;
};

// collision_models.py:185-212 on A <= 8 quads held in registers/scratch
__device__ inline void collision_multiple_dev(const double *poses /*[A,3]*/, int A, double L, double W,
                                              uint8_t *col, int32_t *cidx)
{
    for (int i = 0; i < A; i++) { col[i] = 0; cidx[i] = -1; }
    for (int i = 0; i < A - 1; i++) {
        double vi[4][2];
        get_vertices(poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], L, W, vi);
        for (int j = i + 1; j < A; j++) {
            double vj[4][2];
            get_vertices(poses[3 * j], poses[3 * j + 1], poses[3 * j + 2], L, W, vj);
            if (gjk_collision(vi, vj)) {
                col[i] = 1; col[j] = 1;
                cidx[i] = j; cidx[j] = i;
            }
        }
    }
}

// F110Env._check_done (f110_env.py:202-244) for the A cars of one env: every car's offset from its OWN start
// position, rotated by the EGO's start rotation (:219-221, :329), folded onto the 2 m wide start strip (:223-229),
// `closes = dist2 <= 0.1` (:231), toggle on every change of near_start (:232-239), lap_counts = toggles // 2 (:238),
// lap_times follows current_time while toggles < 4 (:239-240).  Returns all(toggles >= 4).
// xy: car i's position at xy[i*stride], xy[i*stride+1]; start: [A,3] (x, y, theta).
__device__ inline bool check_done_dev(const double *xy, int stride, const double *start, int A, double r00, double r01,
                                      double r10, double r11, double current_time, uint8_t *near_start, int32_t *toggles,
                                      int32_t *lap_counts, double *lap_times, uint8_t *checkpoint_done)
{
    const double left_t = 2, right_t = 2;
    bool all_done = true;
    for (int i = 0; i < A; i++) {
        const double px = xy[(size_t)i * stride] - start[(size_t)i * 3];
        const double py = xy[(size_t)i * stride + 1] - start[(size_t)i * 3 + 1];
        const double dx = r00 * px + r01 * py;
        double temp_y = r10 * px + r11 * py;
        if (temp_y > left_t) temp_y -= left_t;
        else if (temp_y < -right_t) temp_y = -right_t - temp_y;
        else temp_y = 0;
        const double dist2 = dx * dx + temp_y * temp_y;
        const bool closes = dist2 <= 0.1;
        bool ns = near_start[i] != 0;
        int tg = toggles[i];
        if (closes && !ns) { ns = true; tg += 1; }
        else if (!closes && ns) { ns = false; tg += 1; }
        near_start[i] = ns ? 1 : 0;
        toggles[i] = tg;
        lap_counts[i] = tg / 2;
        if (tg < 4) lap_times[i] = current_time;
        if (checkpoint_done) checkpoint_done[i] = tg >= 4 ? 1 : 0;
        if (!(tg >= 4)) all_done = false;
    }
    return all_done;
}

// function-level _check_done: lane per env (f110_check_done)
struct CheckDoneArgs {
    int n_envs, agents, ego_idx;
    const double *poses;        // [n,A,3]
    const double *start;        // [n,A,3]
    const double *start_rot;    // [n,4] row-major 2x2
    const double *current_time; // [n]
    const uint8_t *collisions;  // [n,A]
    uint8_t *near_start;        // [n,A] in/out
    int32_t *toggles;           // [n,A] in/out
    int32_t *lap_counts;        // [n,A]
    double *lap_times;          // [n,A] in/out
    uint8_t *done;              // [n]
    uint8_t *checkpoint_done;   // [n,A] or NULL
};

static __global__ __launch_bounds__(128) void check_done_kernel(CheckDoneArgs a)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.n_envs) return;
    const int A = a.agents, c0 = env * A;
    const double *R = a.start_rot + (size_t)env * 4;
    const bool all_done = check_done_dev(a.poses + (size_t)c0 * 3, 3, a.start + (size_t)c0 * 3, A, R[0], R[1], R[2], R[3],
                                         a.current_time[env], a.near_start + c0, a.toggles + c0, a.lap_counts + c0,
                                         a.lap_times + c0, a.checkpoint_done ? a.checkpoint_done + c0 : nullptr);
    a.done[env] = ((a.collisions[c0 + a.ego_idx] != 0) || all_done) ? 1 : 0; // :242
}

// ONE: the env has one agent (no pair to test: the GJK code is not even compiled in, the kernel is a third of the size)
template <bool ONE>
__device__ inline void env_body(const EnvArgs &a, int env)
{
    if (env >= a.n_envs) return;
    const bool pend = a.pending_reset[env] != 0;
    if (a.reset_only && !pend) return;
    const int A = ONE ? 1 : a.agents, c0 = env * A;
    if (ONE) {
        a.collisions[c0] = 0; a.collision_idx[c0] = -1; // collision_multiple (collision_models.py:185-212) on one quad
    } else {
        // Simulator.check_collision (base_classes.py:529-543) on the post-integration poses
        const Params &SP = a.params[(size_t)params_slot_of(a.env_params, env, a.param_slots, a.dev_err) * (A + 1)]; // Simulator.params (:542)
        collision_multiple_dev(a.pose_snap + (size_t)c0 * 3, A, SP.v[P_LENGTH], SP.v[P_WIDTH],
                               a.collisions + c0, a.collision_idx + c0);
    }
    for (int i = 0; i < A; i++) {
        if (a.in_collision[c0 + i]) {
            a.collisions[c0 + i] = 1; // :581-582
            double *st = a.state + (size_t)(c0 + i) * 7; // check_ttc, base_classes.py:244-247
            st[3] = 0.; st[4] = 0.; st[5] = 0.; st[6] = 0.;
        }
        a.noise_step[c0 + i] += 1;
    }
    double ct = a.current_time[env];
    double r00, r01, r10, r11;
    if (pend) {
        // F110Env.reset (f110_env.py:318-329)
        ct = 0.0;
        const double th = -a.spawn[(size_t)(c0 + a.ego_idx) * 3 + 2];
        double sth, cth;
        sincos(th, &sth, &cth);
        r00 = cth; r01 = -sth; r10 = sth; r11 = cth;
        a.start_rot[(size_t)env * 4] = r00; a.start_rot[(size_t)env * 4 + 1] = r01;
        a.start_rot[(size_t)env * 4 + 2] = r10; a.start_rot[(size_t)env * 4 + 3] = r11;
        for (int i = 0; i < A; i++) { a.near_start[c0 + i] = 1; a.toggles[c0 + i] = 0; }
        a.pending_reset[env] = 0;
    } else {
        r00 = a.start_rot[(size_t)env * 4]; r01 = a.start_rot[(size_t)env * 4 + 1];
        r10 = a.start_rot[(size_t)env * 4 + 2]; r11 = a.start_rot[(size_t)env * 4 + 3];
    }
    ct = ct + a.time_step; // f110_env.py:293
    a.current_time[env] = ct;
    const bool all_done = check_done_dev(a.state + (size_t)c0 * 7, 7, a.spawn + (size_t)c0 * 3, A, r00, r01, r10, r11, ct,
                                         a.near_start + c0, a.toggles + c0, a.lap_counts + c0, a.lap_times + c0,
                                         a.checkpoint_done ? a.checkpoint_done + c0 : nullptr);
    const bool dn = (a.collisions[c0 + a.ego_idx] != 0) || all_done;
    a.done[env] = dn ? 1 : 0;
    if (a.autoreset && dn) a.pending_reset[env] = 1;
}

template <bool ONE>
__global__ __launch_bounds__(128) void env_kernel(EnvArgs a) { env_body<ONE>(a, blockIdx.x * blockDim.x + threadIdx.x); }

// A > 1: the env bookkeeping and the opponents' set-up in ONE launch.  Both are small kernels whose time is latency (256 and
// 2 048 waves), and neither reads what the other writes -- except that env_body zeroes the yaw of a car whose iTTC fired, for
// which the set-up uses 0 anyway, and clears pending_reset, of which the set-up reads dynamics_kernel's snapshot
// (OppArgs::pending_reset = was_pending) -- so the first env_blocks workgroups do one and the rest the other, side by side.
struct PostScanArgs {
    EnvArgs e;
    OppArgs o;
    int env_blocks;
};

static __global__ __launch_bounds__(128) void post_scan_kernel(PostScanArgs a)
{
    if ((int)blockIdx.x < a.env_blocks) env_body<false>(a.e, blockIdx.x * blockDim.x + threadIdx.x);
    else opp_setup_body(a.o, (blockIdx.x - a.env_blocks) * blockDim.x + threadIdx.x);
}

// ------------------------------------------------------------------ one env's observation in one buffer
// The single-env facade (red_gym_amd.F110Env = the reference's Gym API on a batch of one) returns NumPy / Python objects
// every step: instead of a device -> host copy per field, one kernel gathers env `env` into one fp64 row
//   [A*7 state | A collisions | A lap_times | A lap_counts | A toggles | current_time | done | A*nb scans]
// (every small field is exactly representable in fp64) and ONE copy takes it to the host.
struct PackArgs {
    int env, agents, nb;
    const double *state; const uint8_t *collisions; const double *lap_times; const int32_t *lap_counts; const int32_t *toggles;
    const double *current_time; const uint8_t *done; const double *scans64; const float *scans32;
    double *out;
};

static __global__ __launch_bounds__(256) void pack_env_kernel(PackArgs a)
{
    const int A = a.agents, c0 = a.env * A;
    const int n_small = 11 * A + 2, n = n_small + A * a.nb;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double v;
        if (i < 7 * A) v = a.state[(size_t)c0 * 7 + i];
        else if (i < 8 * A) v = (double)a.collisions[c0 + i - 7 * A];
        else if (i < 9 * A) v = a.lap_times[c0 + i - 8 * A];
        else if (i < 10 * A) v = (double)a.lap_counts[c0 + i - 9 * A];
        else if (i < 11 * A) v = (double)a.toggles[c0 + i - 10 * A];
        else if (i == 11 * A) v = a.current_time[a.env];
        else if (i == 11 * A + 1) v = (double)a.done[a.env];
        else {
            const size_t k = (size_t)c0 * a.nb + (size_t)(i - n_small);
            v = a.scans64 ? a.scans64[k] : (double)a.scans32[k];
        }
        a.out[i] = v;
    }
}

} // namespace f110
