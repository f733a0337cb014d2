// f110_handle.h -- the handle (f110_handle) with the state of every family that lives on it, and the few helpers that cross a
// unit's border.  It includes the headers whose TYPES the handle stores, none that defines a kernel.
#pragma once
#include "f110_common.h"
#include "f110_device.h"    // Params
#include "f110_map.h"       // MapDev
#include "f110_noise.h"     // NoiseDesc, NoiseGen, NoiseMark, u128
#include "f110_plangrid.h"  // PlanGrid
#include "f110_scan_plan.h" // StageSpec

namespace f110 { struct OppPair; } // f110_opponents.h: the handle only holds the buffer (alloc_opp_pairs, f110_step.hip, sizes it)

// A raceline's grid of candidate lists on the device (f110_plangrid.h PlanGrid; built on the host by build_plan_grid,
// f110_consumers.hip): the geometry, whose count / cand point into the two tables it owns.  The planner's prepared raceline
// and the progress tracker each hold one.
struct PlanGridDev {
    PlanGrid g;
    DevBuf<uint8_t> d_count; DevBuf<uint16_t> d_cand;
    hipError_t upload(const PlanGrid &geometry, const std::vector<uint8_t> &count, const std::vector<uint16_t> &cand)
    {
        hipError_t e = d_count.upload(count.data(), count.size());
        if (e == hipSuccess) e = d_cand.upload(cand.data(), cand.size());
        g = geometry; g.count = d_count.get(); g.cand = d_cand.get();
        return e;
    }
};

// Where the scan finds a car's noise row: row r of the car's slot is base[(slot * cap + (r & mask)) * num_beams], slot =
// env_slot[env] (NULL: slot 0).  ScanArgs and the device-resident NoiseDesc both take it from NoiseState::where.
struct NoiseRows {
    const double *base;
    int cap, mask, slots;
    const int32_t *env_slot;
};

enum class NoiseKind { unset, host_table, generator }; // unset: the row of zeros

// Lidar noise (f110_noise.h, f110_noise_abi.hip).  Ring mode: [slots][cap][num_beams] rows, rows lo .. hi-1 present, every
// env on the slot d_env_slot gives it.  Per-env mode (f110_set_noise_per_env): every env its own generator and ONE row,
// produced in front of every step's scan.
struct NoiseState {
    struct Slot {
        NoiseKind kind = NoiseKind::unset;
        long long T = 0;              // host table: its rows
        NoiseGen seed;                // generator: the stream at row 0
    };
    DevBuf<double> d_rows;            // [slots][cap][num_beams] noise rows (a ring per slot)
    long long cap = 0, lo = 0, hi = 0; // cap: rows per slot (a power of two); noise off: cap 1, hi = "infinity"
    int slots = 1;
    bool on = false;
    Slot slot[F110_MAX_NOISE_SLOTS];
    long long gen_rows = 0;           // rows every generator slot has produced (they all stand at the same row)
    DevBuf<NoiseDesc> d_desc;         // what the kernels read: its address never changes
    DevBuf<NoiseGen> d_gen;           // [F110_MAX_NOISE_SLOTS] device generator states
    DevBuf<int32_t> d_env_slot;       // dev [B] noise slot of every env; passed only when `multi`
    bool multi = false;
    Stream stream;                    // the generator runs here, beside the caller's stream (f110_noise_prefetch)
    Event ev;
    long long pending_hi = 0;         // rows a prefetch in flight on `stream` will have produced (0: none in flight)
    // Ordering of the side stream behind the caller's: recorded on the caller's stream whenever the floor is raised (the steps
    // enqueued so far may still read the rows below it, whose ring places the next prefetch recycles) and whenever a generator
    // kernel is enqueued there (it reads and writes the same generator states); the next prefetch waits for it.
    Event order_ev;
    bool order_ev_set = false;
    DevBuf<NoiseMark> d_marks;        // [marks_slots][marks_cap] generator state at every 64th row (f110_noise.h NoiseMark)
    long long marks_cap = 0;
    int marks_slots = 0;
    DevBuf<u128> d_pcg_tab;           // [2][65] powers and partial sums of the LCG multiplier (f110_noise_kernels.h NoiseGenArgs::pcg_tab)
    bool per_env = false;
    DevBuf<NoiseGen> d_env_gen, d_env_seed;   // [num_envs]
    DevBuf<double> d_env_rows;                // [num_envs][num_beams]
    DevBuf<int32_t> d_env_ident;              // [num_envs] env -> slot = env

    NoiseRows where(int num_envs) const
    {
        if (per_env) return {d_env_rows.get(), 1, 0, num_envs, d_env_ident.get()};
        return {d_rows.get(), (int)cap, (int)(cap - 1), slots, multi ? d_env_slot.get() : nullptr};
    }
};

struct f110_handle {
    f110_config cfg;
    // Vehicle parameters, [slots][1 + A]: per params slot (the `params` one reference env was constructed with) entry 0 =
    // Simulator.params (GJK vertices, base_classes.py:542), entry 1 + i = RaceCar.params of agent i
    std::vector<Params> h_params;
    int param_slots = 1;
    DevBuf<Params> d_params;          // [slots the allocation holds][1 + A]
    DevBuf<int32_t> d_env_params;     // dev [B] params slot of every env; passed to the kernels only when `multi_params`
    bool multi_params = false;
    DevBuf<OppPair> d_opp_pairs;      // [N, A-1] opponent ray-cast scratch (alloc_opp_pairs at f110_create; the entry point f110_step() never allocates)
    DevBuf<uint8_t> d_was_pending;    // [B] pending_reset as the step's first kernel found it
    bool has_map = false, bound = false;
    // Bumped whenever a later f110_step would enqueue different kernels or by-value arguments than an earlier one
    // (a table re-allocated, another scan instantiation selected, buffers re-bound): f110_launch_epoch.
    int64_t epoch = 0;
    std::vector<StageSpec> stages;    // f110_set_scan_stages override, parsed (empty: the built-in choice, f110_scan_plan.h)
    f110_buffers bufs;
    // device tables owned by the handle
    DevBuf<double> d_scan_angles, d_beam_cosines, d_side;
    DevBuf<uint16_t> d_chunk0;
    DevBuf<double2> d_cs;             // interleaved {cos, sin} LUT (repeated, see upload_cs)
    DevBuf<double2> d_beam_cs;        // {cos, sin}(scan_angles) for the opponent ray cast
    std::vector<double> h_sines, h_cosines;
    double side_max = 0.0;            // largest finite side distance (the scan's pre-test for iTTC candidates)
    NoiseState noise;
    // prepared raceline of f110_pure_pursuit (f110_pure_pursuit_prepare) and its grid of candidate lists
    const double *plan_wp = nullptr; int plan_M = 0; bool plan_ok = false;
    PlanGridDev plan;
    // progress tracker (f110_progress_install / _bind / _update, f110_consumers.hip): its own device copy of the racelines and
    // their host-built tables, the grid of candidate lists of a single raceline, and the caller's output buffers
    struct Progress {
        bool on = false, bound = false, use_grid = false;
        int K = 0;
        DevBuf<double> d_xy, d_len, d_cum, d_psi, d_lap;
        DevBuf<int32_t> d_offsets, d_env;   // d_env: [B] raceline of every env (empty: all on raceline 0)
        PlanGridDev grid;
        f110_progress_buffers bufs;
    } progress;
    // reward shaper (f110_shaping_install / _bind / _update, f110_consumers.hip): the configuration and the caller's buffers
    struct Shaping {
        bool on = false, bound = false;
        f110_shaping_config cfg;
        f110_shaping_buffers bufs;
    } shaping;
    // path follower (f110_pathfollow_install / _bind / _act / _update, f110_consumers.hip): the configuration, the QP's host-built
    // tables (f110_pathfollow.h) and the caller's buffers
    struct PathFollow {
        bool on = false, bound = false;
        f110_pathfollow_config cfg;
        DevBuf<double> d_qp;
        f110_pathfollow_buffers bufs;
    } follow;
    // replay buffer (f110_replay_install / _bind / _update / _draw / _gather, f110_consumers.hip): the configuration, the image
    // size of the shaper it was installed behind, and the caller's ring
    struct Replay {
        bool on = false, bound = false;
        f110_replay_config cfg;
        int rows = 0, cols = 0;
        f110_replay_buffers bufs;
    } replay;
    // prioritized replay (f110_priority_install / _bind, f110_consumers.hip) behind the ring above: the configuration and the
    // caller's tree; f110_replay_install switches it off
    struct Priority {
        bool on = false, bound = false;
        f110_priority_config cfg;
        f110_priority_buffers bufs;
    } priority;
    // episode tracker (f110_episodes_install / _bind / _update, f110_consumers.hip): the configuration and the caller's arrays
    struct Episodes {
        bool on = false, bound = false;
        f110_episodes_config cfg;
        f110_episodes_buffers bufs;
    } episodes;
    const int32_t *scan_order = nullptr; // launch order of the step's scan (f110_set_scan_order; caller-owned device array) or NULL
    DevBuf<uint32_t> d_err;           // device error word (f110_device_errors)
    std::vector<double> h_side;       // side distances (host copy of d_side)
    // Side distances per params slot (f110_set_side_distance_slots), while installed: side_n_slots == param_slots at all
    // times, so the slot of every env (d_env_params) has a row.  0: the scan reads d_side for every car.
    DevBuf<double> d_side_slots;      // [side_n_slots][num_beams]
    int side_n_slots = 0;
    std::vector<double> h_side_slot0; // host copy of row 0 (new slots start as copies of it, like their params)
    double side_slots_max = 0.0;      // largest finite value over all installed rows (ScanArgs::side_max while installed)
    // Maps.  Slot 0 is "the" map of the reference's API; further slots let blocks of envs of one shard run on
    // different maps (one handle standing in for many F110Env instances with their own map each).
    struct MapSlot {
        DevBuf<uint16_t> d_cells, d_cells_far;
        DevBuf<double> d_lut, d_lut_lds, d_dt;
        MapDev dev;                   // host copy of d_maps[slot]
        bool used = false, ident = false, pow2 = false;
        // compact forms (f110_map.h LUT_COMPACT), when they were built: their tables and, per form, the share of the map's
        // free cells whose code lies behind its far marker (plan_scan's eligibility rule reads it)
        DevBuf<uint16_t> d_cells_c[N_COMPACT];
        DevBuf<double> d_lut_lds_c[N_COMPACT];
        DevBuf<uint8_t> d_cells_b;    // row-padded byte table of d_cells_c[0] (f110_map.h: cell_elem_bp), built with the
        int pad_rows = 0;             // compact forms where it fits (map_bytes_fit), and its P
        bool compact = false;
        double compact_out[N_COMPACT] = {1.0, 1.0};
        // the same shares over the free cells a car can REACH (8-connected to its spawn cell), averaged over the cars, learnt at
        // the first reset of all envs after the install (learn_reach, f110_step.hip): what the rule reads.  The open ground
        // around a track may be most of the map's free cells and holds next to no car
        bool reach_known = false;
        double reach_out[N_COMPACT] = {1.0, 1.0};
    };
    MapSlot slots[F110_MAX_MAPS];
    DevBuf<MapDev> d_maps;            // dev [F110_MAX_MAPS] descriptors read by scan_kernel
    DevBuf<int32_t> d_env_map;        // dev [B] slot of every env; only passed to the kernel when `multi`
    std::vector<int32_t> h_env_map;   // host copy (all 0 until f110_assign_maps)
    bool multi = false;
    bool wg_single = false;           // some neighbouring cars stand on different maps: the scan runs one wave per workgroup
    bool ident = false, pow2 = false; // AND over the used slots: selects the scan_kernel instantiation
    double theta_inc = 0;
    // measurement aid (f110_profile_begin/end)
    std::vector<Event> prof_ev;      // pairs: [2*i] before, [2*i+1] after the scan launch
    int prof_n = 0, prof_every = 1, prof_seq = 0; // events ride on every prof_every-th step's scan launch (the middle one of
                                                  // each run of prof_every steps: on a clock ramp the samples' mean is then the steps' mean)
    bool prof_on = false;
};

// helpers defined in f110_handle.hip / f110_noise_abi.hip / f110_step.hip and used elsewhere
int check_device(const f110_handle *h, const char *who);
int noise_init(f110_handle *h);
int alloc_opp_pairs(f110_handle *h);
