// f110_step.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
// The kernels of one batched env step on gfx950, in launch order:
//   dynamics_kernel   (lane per car)        RaceCar.update_pose minus the scan (+ reset)
//   scan_kernel       (wave per car)        ScanSimulator2D.scan + noise + iTTC
//   env_kernel        (lane per env)        GJK, collision flags, iTTC state update, lap timing, done, autoreset
// and, when A > 1, in place of env_kernel:
//   post_scan_kernel  (lane per env | 4 lanes per car pair)  env_kernel's work beside opp_setup_body \ RaceCar.ray_cast_agents
//   opp_apply_kernel  (wave per car)                                                                  /
// plus small function-level kernels used by the parity entry points.
#include "f110_handle.h"
#include "f110_scan.h"
#include "f110_env.h"
#include "f110_mirrors.h"
#include "f110_noise_kernels.h" // (the per-env noise rows are produced by a launch of the step)

// scratch of the opponent ray cast: allocated when the handle is created (f110_create, f110_handle.hip), never by the entry point f110_step().  It lives in this
// unit because OppPair does (f110_opponents.h, beside opp_apply_kernel)
int alloc_opp_pairs(f110_handle *h)
{
    if (h->cfg.num_agents < 2) return F110_OK;
    const size_t n = (size_t)h->cfg.num_envs * h->cfg.num_agents * (h->cfg.num_agents - 1);
    DevBuf<OppPair> pairs;
    DevBuf<uint8_t> was_pending;
    HIP_TRY(pairs.alloc(n));
    HIP_TRY(hipMemset(pairs.get(), 0, n * sizeof(OppPair)));
    HIP_TRY(was_pending.alloc((size_t)h->cfg.num_envs));
    HIP_TRY(hipMemset(was_pending.get(), 0, (size_t)h->cfg.num_envs));
    h->d_opp_pairs = std::move(pairs);
    h->d_was_pending = std::move(was_pending);
    return F110_OK;
}

// ---------------------------------------------------------------- launches
// Every kernel of the step path goes through emit(): launched at once on a stream (eager, or inside somebody's stream
// capture), or recorded as a node description for a HIP graph the library builds itself (f110_graph_create).
struct KernelLaunch {
    const void *func;
    dim3 grid, block;
    unsigned shmem;
    std::vector<char> args; // the kernel's single by-value argument block
};

struct Sink {
    hipStream_t st = nullptr;
    std::vector<KernelLaunch> *record = nullptr;
};

template <typename Args>
static int emit(const Sink &k, const void *func, dim3 grid, dim3 block, unsigned shmem, const Args &a, hipEvent_t ev0 = nullptr,
                hipEvent_t ev1 = nullptr)
{
    static_assert(__is_trivially_copyable(Args), "kernel argument blocks are copied byte for byte");
    if (k.record) {
        KernelLaunch l;
        l.func = func; l.grid = grid; l.block = block; l.shmem = shmem;
        l.args.assign((const char *)&a, (const char *)&a + sizeof(Args));
        k.record->push_back(std::move(l));
        return F110_OK;
    }
    void *params[1] = {(void *)&a};
    // plain launches unless the measurement aid attached events (a captured hipGraph then holds ordinary kernel nodes)
    if (ev0 || ev1) HIP_TRY(hipExtLaunchKernel(func, grid, block, params, shmem, k.st, ev0, ev1, 0));
    else HIP_TRY(hipLaunchKernel(func, grid, block, params, shmem, k.st));
    return F110_OK;
}

// The argument block every scan launch starts from: n_cars cars of `agents` agents each at pose_src (x, y at 0 and 1, yaw at
// yaw_off, pose_stride apart) and the outputs.  The step's scan adds its buffers, the plan each launch's cars and stages.
static ScanArgs scan_args(const f110_handle *h, int n_cars, int agents, const double *pose_src, int pose_stride, int yaw_off,
                          float *out_f32, double *out_f64, uint32_t *lookups)
{
    ScanArgs s;
    memset(&s, 0, sizeof(s));
    ScanDev &d = s.scan;
    d.nb = h->cfg.num_beams; d.theta_dis = h->cfg.theta_dis; d.fov = h->cfg.fov; d.eps = h->cfg.eps;
    d.max_range = h->cfg.max_range; d.inc = h->theta_inc; d.inc_fx = (unsigned long long)std::llround(h->theta_inc * 1099511627776.0); d.cs_len = (int)h->d_cs.size(); d.cs = h->d_cs.get();
    s.maps = h->d_maps.get(); s.n_maps = F110_MAX_MAPS; s.n_cars = n_cars; s.agents = agents; s.chunk_beam0 = h->d_chunk0.get();
    s.pose_src = pose_src; s.pose_stride = pose_stride; s.yaw_off = yaw_off; s.out_f32 = out_f32; s.out_f64 = out_f64; s.lookups = lookups;
    return s;
}

// Every pointer a scan launch dereferences without a test of its own, checked on the host: a null here is an error
// code, on the device it is "Memory access fault ... on address (nil)" in every wave (round 2, gpurun_out/r02d).
static int check_scan_args(const ScanArgs &a, const char *who)
{
    if (a.n_cars < 1 || a.agents < 1 || a.scan.nb < 2 || a.scan.nb > MAX_CHUNKS * 64) return fail(F110_E_INVALID, "%s: %d cars, %d agents, %d beams", who, a.n_cars, a.agents, a.scan.nb);
    if (!a.maps || !a.scan.cs || a.scan.cs_len < a.scan.theta_dis || !a.chunk_beam0 || !a.pose_src) return fail(F110_E_INVALID, "%s: a table of the scan is missing (maps / {cos,sin} LUT / chunk order / poses)", who);
    if (!a.out_f32 && !a.out_f64) return fail(F110_E_INVALID, "%s: no output buffer", who);
    if (a.state && (!a.noise_step || !a.noise_base || a.noise_cap < 1 || !a.beam_cosines || !a.in_collision || !a.pending_reset))
        return fail(F110_E_INVALID, "%s: a buffer of the step's scan is missing (noise / beam cosines / in_collision / pending_reset)", who);
    if (!a.state && a.reset_only) return fail(F110_E_INVALID, "%s: reset_only without the step's buffers", who);
    return F110_OK;
}

// scan_kernel<IDENT, POW2, SM> by [SM][IDENT | POW2 << 1]
#define SCAN_KERNELS(SM) {(const void *)&scan_kernel<false, false, SM>, (const void *)&scan_kernel<true, false, SM>, \
                          (const void *)&scan_kernel<false, true, SM>, (const void *)&scan_kernel<true, true, SM>}
static const void *const scan_kernels[3][4] = {SCAN_KERNELS(0), SCAN_KERNELS(1), SCAN_KERNELS(2)};
// the compact forms (kind 3, the step's scan only) by [compact_index(S)][SM - 1]
static const void *const scan_kernels_compact[N_COMPACT][2] = {
    {(const void *)&scan_kernel<true, true, 1, LUT_COMPACT[0]>, (const void *)&scan_kernel<true, true, 2, LUT_COMPACT[0]>},
    {(const void *)&scan_kernel<true, true, 1, LUT_COMPACT[1]>, (const void *)&scan_kernel<true, true, 2, LUT_COMPACT[1]>}};
// the compact form of 256 slots with fp32 rows staged in LDS (ScanLaunch::rowbuf) by [SM - 1]
static const void *const scan_kernels_rowbuf[2] = {(const void *)&scan_kernel<true, true, 1, SCAN_ROWBUF_LUT, true>,
                                                   (const void *)&scan_kernel<true, true, 2, SCAN_ROWBUF_LUT, true>};
// the same reading the byte cell table (ScanLaunch::bytes) by [SM - 1]
static const void *const scan_kernels_bytes[2] = {(const void *)&scan_kernel<true, true, 1, SCAN_ROWBUF_LUT, true, true>,
                                                  (const void *)&scan_kernel<true, true, 2, SCAN_ROWBUF_LUT, true, true>};

// The form of the step's scan on the handle's single map: what F110_SCAN_FORM forces (read once per process; tests and A/B
// runs), else what the eligibility rule picks from the map's recorded shares.  A map without compact tables stays classic
// whatever is asked.  The inputs only change with the map, whose install moves f110_launch_epoch.
static int scan_form_forced() { static const int forced = scan_form_override(getenv("F110_SCAN_FORM")); return forced; }
static int scan_form(const f110_handle *h, int n_cars)
{
    const int forced = scan_form_forced();
    const f110_handle::MapSlot &m = h->slots[0];
    if (!m.compact || h->multi || !(h->ident && h->pow2)) return 0;
    if (forced >= 0) return forced;
    return m.reach_known ? scan_compact_choice(m.reach_out, n_cars, h->cfg.num_agents) : 0;
}

// The shares the rule reads (scan_reach_shares, f110_scan_plan.h), learnt from the spawn poses of a reset of all envs: once per
// map install, and only where the answer is used -- a handle the rule can route, no override.  An explicit call, not a part of
// f110_reset: it synchronises the stream, copies the poses and the cell table to the host and floods the cars' free components
// there (tens of ms on a 1 600 x 1 600 map), none of which f110_reset may do.  Anything that fails here (a stream being
// captured, host memory) leaves the shares unlearnt, i.e. the classic form.
extern "C" int f110_scan_form_learn(f110_handle *h, const double *poses_dev, void *stream)
{
    if (!h || !poses_dev) return fail(F110_E_INVALID, "f110_scan_form_learn: null argument");
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    f110_handle::MapSlot &m = h->slots[0];
    const int N = h->cfg.num_envs * h->cfg.num_agents;
    const double none[N_COMPACT] = {}; // (a handle on which not even a map without a cell behind the markers would be routed: nothing to learn)
    if (!m.compact || m.reach_known || h->multi || !(h->ident && h->pow2) || scan_form_forced() >= 0 ||
        scan_compact_choice(none, N, h->cfg.num_agents) == 0)
        return F110_OK;
    if (int rc = check_device(h, "f110_scan_form_learn")) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); return F110_OK; }
    if (cap != hipStreamCaptureStatusNone) return F110_OK;
    try {
        std::vector<double> poses((size_t)N * 3);
        std::vector<uint16_t> cells(m.d_cells.size());
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(poses.data(), poses_dev, poses.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cells.data(), m.d_cells.get(), cells.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
        const MapDev &d = m.dev;
        const int Hp = map_rows_padded(d.H);
        const unsigned off_far[N_COMPACT] = {compact_off_far(LUT_COMPACT[0]), compact_off_far(LUT_COMPACT[1])};
        scan_reach_shares(d.H, d.W, [&](int r, int c) { return (unsigned)cells[cell_elem(r, c, Hp)]; }, cell_code(0), off_far,
                          poses.data(), 3, N, d.ox, d.oy, d.rinv, m.reach_out);
    } catch (const std::bad_alloc &) {
        return F110_OK;
    }
    m.reach_known = true;
    h->epoch++; // the form of the next launches may differ from the one a captured step froze
    return F110_OK;
}

// F110_SCAN_ROWS = lds | direct (read once per process; tests and A/B runs) over the rule scan_rowbuf_choice
static int scan_rows_forced() { static const int forced = scan_rows_override(getenv("F110_SCAN_ROWS")); return forced; }

extern "C" int f110_scan_rows_info(f110_handle *h, int32_t n_cars, int32_t *lds)
{
    if (!h || !lds || n_cars < 1) return fail(F110_E_INVALID, "f110_scan_rows_info: bad arguments");
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    *lds = scan_rowbuf_choice(scan_form(h, n_cars), true, scan_rows_forced());
    return F110_OK;
}

// F110_SCAN_CODES = byte | word (read once per process; tests and A/B runs) over the rule scan_codes_choice
// ... where slot 0 has its row-padded byte table (scan_codes_available: a map whose padded table did not fit reads word codes)
static int scan_codes_forced() { static const int forced = scan_codes_override(getenv("F110_SCAN_CODES")); return forced; }
static int scan_codes_of(const f110_handle *h) { return scan_codes_available(h->slots[0].dev.cells_b != nullptr, scan_codes_forced()); }

extern "C" int f110_scan_codes_info(f110_handle *h, int32_t n_cars, int32_t *bytes)
{
    if (!h || !bytes || n_cars < 1) return fail(F110_E_INVALID, "f110_scan_codes_info: bad arguments");
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    *bytes = scan_codes_choice(scan_form(h, n_cars), scan_rowbuf_choice(scan_form(h, n_cars), true, scan_rows_forced()), scan_codes_of(h));
    return F110_OK;
}

extern "C" int f110_scan_pad_rows(f110_handle *h, int32_t *rows)
{
    if (!h || !rows) return fail(F110_E_INVALID, "f110_scan_pad_rows: bad arguments");
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    *rows = h->slots[0].dev.cells_b ? (int32_t)h->slots[0].dev.pad_rows : -1;
    return F110_OK;
}

extern "C" int f110_scan_form_info(f110_handle *h, int32_t n_cars, int32_t *form, double *out_share)
{
    if (!h || !form || !out_share || n_cars < 1) return fail(F110_E_INVALID, "f110_scan_form_info: bad arguments");
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    const f110_handle::MapSlot &m = h->slots[0];
    *form = scan_form(h, n_cars);
    for (int i = 0; i < N_COMPACT; i++) {
        out_share[i] = m.compact ? m.compact_out[i] : 1.0;
        out_share[N_COMPACT + i] = m.reach_known ? m.reach_out[i] : -1.0;
    }
    return F110_OK;
}

// The scan of `a` -- the step's when a.state is set, else f110_scan's -- as f110_scan_plan.h plans it.  ev0 / ev1 (measurement
// aid, may be null) ride on the step's first launch: start / stop events attached to the dispatch itself, which costs less than
// bracketing the launch with two hipEventRecord calls (those add two barrier packets to the queue).
static int run_scan(const f110_handle *h, const ScanArgs &a, const Sink &k, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr)
{
    if (int rc = check_scan_args(a, "scan launch")) return rc;
    // F110_SCAN_STORES=plain|stream overrides the plan's choice of stores: test_plain_store_instantiation_matches_streaming
    // reaches scan_kernel<.., 2>, which no test size does otherwise, through it
    static const char *stores_env = getenv("F110_SCAN_STORES");
    ScanPlanIn in;
    in.n_cars = a.n_cars; in.agents = a.agents; in.num_beams = a.scan.nb; in.stages = &h->stages; in.step = a.state != nullptr;
    in.stores = stores_env; in.multi = a.env_map != nullptr; in.wg_single = h->wg_single; in.kind = h->ident | h->pow2 << 1;
    in.compact = in.step && !in.multi ? scan_form(h, a.n_cars) : 0;
    in.out_f32 = a.out_f32 != nullptr; in.rows = scan_rows_forced(); in.codes = scan_codes_of(h);
    std::vector<ScanLaunch> plan;
    if (int rc = plan_scan(in, [h](int env) { const f110_handle::MapSlot &m = h->slots[h->h_env_map[env]]; return m.ident | m.pow2 << 1; }, plan))
        return rc;
    for (const ScanLaunch &l : plan) {
        ScanArgs s = a;
        s.car_base = l.car_base; s.n_cars = l.n_cars; s.wg_single = l.wg_single; s.order = l.order ? h->scan_order : nullptr;
        s.n_stages = l.n_stages; memcpy(s.stage_cars, l.stage_cars, sizeof(s.stage_cars)); memcpy(s.stage_log2w, l.stage_log2w, sizeof(s.stage_log2w));
        const void *func = scan_kernels[l.sm][l.kind];
        if (l.lut) {
            // the compact instantiation dereferences the map's compact tables without a test of its own
            const int ci = compact_index(l.lut);
            const MapDev &m = h->slots[0].dev;
            if (ci < 0 || l.sm < 1 || l.kind != 3 || !m.cells_c[ci] || !m.lut_lds_c[ci])
                return fail(F110_E_INVALID, "scan launch: compact form %d without its tables (kind %d, sm %d)", l.lut, l.kind, l.sm);
            // ... nor the byte instantiation the byte table, whose fast march relies on the table's padding rows
            if (l.bytes && (!l.rowbuf || l.lut != SCAN_ROWBUF_LUT || !m.cells_b || !m.pad_rows ||
                            m.cells_b_bytes != map_cells_bp(m.H, m.W, (int)m.pad_rows) || m.strip_bytes_b != (unsigned)map_rows_b(m.H, (int)m.pad_rows) * 16u))
                return fail(F110_E_INVALID, "scan launch: byte cell codes without their padded table (form %d, rows %d)", l.lut, (int)l.rowbuf);
            func = l.bytes ? scan_kernels_bytes[l.sm - 1] : l.rowbuf ? scan_kernels_rowbuf[l.sm - 1] : scan_kernels_compact[ci][l.sm - 1];
        }
        if (int rc = emit(k, func, dim3(l.grid), dim3(l.block), 0, s, l.events ? ev0 : nullptr,
                          l.events ? ev1 : nullptr))
            return rc;
    }
    return F110_OK;
}

// The step of every env: dynamics_kernel -> scan_kernel -> env_kernel, or for A > 1 -> post_scan_kernel (env bookkeeping and
// the opponents' set-up side by side) -> opp_apply_kernel.  (Two other
// forms -- a scan that also closes the step of a one-agent env, and a workgroup per car with a shared beam queue -- were
// built, held to ==, measured slower at every size and removed: profiles/r03_step_forms.txt.)
static int run_step(f110_handle *h, const double *actions, int reset_only, const Sink &st)
{
    const f110_config &c = h->cfg;
    const f110_buffers &b = h->bufs;
    const int N = c.num_envs * c.num_agents;
    const bool prof = h->prof_on && !st.record && (h->prof_seq++ % h->prof_every) == h->prof_every / 2 && (size_t)(2 * h->prof_n + 1) < h->prof_ev.size();
    hipEvent_t ev0 = prof ? h->prof_ev[2 * h->prof_n].get() : nullptr, ev1 = prof ? h->prof_ev[2 * h->prof_n + 1].get() : nullptr;
    int rc;

    if (h->noise.per_env) {
        // the row every env's scan is about to add (row `pending ? 0 : noise_step`), from the env's own generator
        NoiseGenArgs g;
        memset(&g, 0, sizeof(g));
        g.gen = h->noise.d_env_gen.get(); g.seeds = h->noise.d_env_seed.get(); g.base = h->noise.d_env_rows.get(); g.mask = 0; g.cap = 1; g.nb = c.num_beams;
        g.pcg_tab = h->noise.d_pcg_tab.get(); g.env_row = b.noise_step; g.env_row_stride = c.num_agents; g.n_env = c.num_envs;
        g.reset_only = reset_only; g.env_pending = b.pending_reset;
        if ((rc = emit(st, (const void *)&noise_rows_kernel, dim3((c.num_envs + 3) / 4), dim3(256), 0, g))) return rc;
    }
    {
        DynArgs d;
        d.n_cars = N; d.agents = c.num_agents; d.state = b.state; d.steer_buf = b.steer_buf; d.steer_cnt = b.steer_cnt;
        d.noise_step = b.noise_step; d.actions = actions; d.spawn = b.spawn; d.pending_reset = b.pending_reset;
        d.was_pending = h->d_was_pending.get(); d.reset_only = reset_only; d.pose_snap = b.pose_snap; d.in_collision = b.in_collision; d.params = h->d_params.get(); d.env_params = h->multi_params ? h->d_env_params.get() : nullptr; d.param_slots = h->param_slots; d.dev_err = h->d_err.get(); d.noise = h->noise.d_desc.get();
        d.time_step = c.timestep; d.integrator = c.integrator;
        if ((rc = emit(st, (const void *)&dynamics_kernel, dim3((N + 255) / 256), dim3(256), 0, d))) return rc;
    }

    // the scan (the launch the measurement aid brackets)
    {
        // Instrumentation follows the measurement aid's sampling: while f110_profile_begin is active, the per-car lookup
        // counters are only fed by the steps that also carry the event pair (an atomic per wave costs 2.5 % of a 65 536-env
        // step, profiles/r03_event_cost.txt), so bytes and time of the roofline come from the same launches.
        ScanArgs s = scan_args(h, N, c.num_agents, b.state, 7, 4, b.scans, b.scans_f64, h->prof_on && !prof ? nullptr : b.lookups);
        s.env_map = h->multi ? h->d_env_map.get() : nullptr;
        s.state = b.state; s.noise_step = b.noise_step;
        s.side = h->d_side.get(); s.side_max = h->side_max;
        if (h->side_n_slots) { // every car against its own vehicle's table; the pre-filter's bound then spans all of them
            s.side_slots = h->d_side_slots.get(); s.side_n_slots = h->side_n_slots; s.side_max = h->side_slots_max;
            s.env_params = h->multi_params ? h->d_env_params.get() : nullptr;
        }
        const NoiseRows nr = h->noise.where(c.num_envs);
        s.noise_base = nr.base; s.noise_cap = nr.cap; s.noise_mask = nr.mask; s.noise_slots = nr.slots; s.env_noise = nr.env_slot;
        s.dev_err = h->d_err.get();
        s.beam_cosines = h->d_beam_cosines.get(); s.ttc_thresh = c.ttc_thresh;
        s.in_collision = b.in_collision; s.pending_reset = b.pending_reset; s.reset_only = reset_only;
        rc = run_scan(h, s, st, ev0, ev1);
    }
    if (rc) return rc;
    if (prof) h->prof_n++;

    EnvArgs e;
    e.n_envs = c.num_envs; e.agents = c.num_agents; e.ego_idx = c.ego_idx; e.autoreset = c.autoreset;
    e.reset_only = reset_only; e.state = b.state; e.noise_step = b.noise_step; e.pose_snap = b.pose_snap; e.spawn = b.spawn;
    e.in_collision = b.in_collision; e.collisions = b.collisions; e.collision_idx = b.collision_idx;
    e.start_rot = b.start_rot; e.near_start = b.near_start; e.toggles = b.toggles; e.lap_counts = b.lap_counts;
    e.lap_times = b.lap_times; e.current_time = b.current_time; e.pending_reset = b.pending_reset; e.done = b.done; e.checkpoint_done = b.checkpoint_done;
    e.time_step = c.timestep; e.params = h->d_params.get(); e.env_params = h->multi_params ? h->d_env_params.get() : nullptr; e.param_slots = h->param_slots; e.dev_err = h->d_err.get();
    const int env_blocks = (c.num_envs + 127) / 128;
    if (c.num_agents == 1) return emit(st, (const void *)&env_kernel<true>, dim3(env_blocks), dim3(128), 0, e);

    // A > 1: env bookkeeping and the opponents' set-up side by side in one launch, then the ray cast
    PostScanArgs ps;
    memset(&ps, 0, sizeof(ps));
    ps.e = e; ps.env_blocks = env_blocks;
    OppArgs &o = ps.o;
    o.n_cars = N; o.agents = c.num_agents; o.nb = c.num_beams; o.state = b.state; o.pose_snap = b.pose_snap;
    o.in_collision = b.in_collision; o.scan_angles = h->d_scan_angles.get(); o.beam_cs = h->d_beam_cs.get(); o.params = h->d_params.get(); o.env_params = h->multi_params ? h->d_env_params.get() : nullptr;
    o.pending_reset = h->d_was_pending.get(); o.reset_only = reset_only; o.scans32 = b.scans; o.scans64 = b.scans_f64;
    o.pairs = h->d_opp_pairs.get(); o.param_slots = h->param_slots; o.dev_err = h->d_err.get();
    const int npairs = N * (c.num_agents - 1);
    if ((rc = emit(st, (const void *)&post_scan_kernel, dim3(env_blocks + (4 * npairs + 127) / 128), dim3(128), 0, ps))) return rc; // four lanes per pair
    return emit(st, (const void *)&opp_apply_kernel, dim3((int)(((long long)OPP_GROUP * N + 255) / 256)), dim3(256), 0, ps.o); // OPP_GROUP lanes per car
}

static int check_ready(f110_handle *h, const char *who, bool launches_on_callers_stream = true)
{
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    if (launches_on_callers_stream)
        if (int rc = check_device(h, who)) return rc;
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    if (!h->bound) return fail(F110_E_UNBOUND, "%s: f110_bind has not been called", who);
    return F110_OK;
}

__global__ void arm_reset_kernel(const double *poses, const uint8_t *mask, int n_envs, int agents, double *spawn,
                                 uint8_t *pending)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n_envs) return;
    if (mask && !mask[env]) return;
    for (int i = 0; i < agents * 3; i++) spawn[(size_t)env * agents * 3 + i] = poses[(size_t)env * agents * 3 + i];
    pending[env] = 1;
}

extern "C" int f110_reset(f110_handle *h, const double *poses, const uint8_t *mask, void *stream)
{
    int rc = check_ready(h, "f110_reset");
    if (rc) return rc;
    if (!poses) return fail(F110_E_INVALID, "Number of poses for reset does not match number of agents.");
    hipStream_t st = (hipStream_t)stream;
    const f110_config &c = h->cfg;
    hipLaunchKernelGGL(arm_reset_kernel, dim3((c.num_envs + 255) / 256), dim3(256), 0, st, poses, mask, c.num_envs,
                       c.num_agents, h->bufs.spawn, h->bufs.pending_reset);
    HIP_TRY(hipGetLastError());
    // the zero-action step of F110Env.reset; actions are not read for pending envs
    return run_step(h, nullptr, 1, Sink{st});
}

extern "C" int f110_step(f110_handle *h, const double *actions, void *stream)
{
    int rc = check_ready(h, "f110_step");
    if (rc) return rc;
    if (!actions) return fail(F110_E_INVALID, "f110_step: null actions");
    return run_step(h, actions, 0, Sink{(hipStream_t)stream});
}

// ---------------------------------------------------------------- one env's observation in one buffer
extern "C" int64_t f110_pack_env_size(f110_handle *h)
{
    if (!h) return 0;
    return (int64_t)h->cfg.num_agents * (11 + h->cfg.num_beams) + 2;
}

extern "C" int f110_pack_env(f110_handle *h, int32_t env, double *out_dev, void *stream)
{
    int rc = check_ready(h, "f110_pack_env");
    if (rc) return rc;
    if (!out_dev || env < 0 || env >= h->cfg.num_envs) return fail(env < 0 || env >= h->cfg.num_envs ? F110_E_INDEX : F110_E_INVALID, "f110_pack_env: env %d of %d, out %p", env, h->cfg.num_envs, (void *)out_dev);
    const f110_buffers &b = h->bufs;
    PackArgs a;
    a.env = env; a.agents = h->cfg.num_agents; a.nb = h->cfg.num_beams; a.state = b.state; a.collisions = b.collisions; a.lap_times = b.lap_times;
    a.lap_counts = b.lap_counts; a.toggles = b.toggles; a.current_time = b.current_time; a.done = b.done; a.scans64 = b.scans_f64; a.scans32 = b.scans;
    a.out = out_dev;
    const int n = (int)f110_pack_env_size(h);
    hipLaunchKernelGGL(pack_env_kernel, dim3(std::min((n + 255) / 256, 256)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- the step as a HIP graph built by the library
struct f110_graph {
    f110_handle *h = nullptr;
    Stream cap;                         // (members are destroyed in reverse order: the executable first, this stream last)
    Graph graph;
    GraphExec exec;
    int64_t epoch = 0;
    int nodes = 0;
    std::vector<KernelLaunch> launches; // node argument blocks must outlive hipGraphAddKernelNode only, kept for clarity
};

extern "C" void f110_graph_destroy(f110_graph *g)
{
    if (!g) return;
    DeviceScope on_dev(g->h ? g->h->cfg.device : 0);
    delete g;
}

extern "C" int f110_graph_create(f110_handle *h, const double *actions, int32_t how, f110_graph **out)
{
    int rc = check_ready(h, "f110_graph_create", false); // builds on the handle's device itself (ON_DEVICE below)
    if (rc) return rc;
    if (!actions || !out) return fail(F110_E_INVALID, "f110_graph_create: null argument");
    if (how != F110_GRAPH_NODES && how != F110_GRAPH_CAPTURE) return fail(F110_E_INVALID, "f110_graph_create: how = %d (0 kernel nodes, 1 stream capture)", how);
    ON_DEVICE(h->cfg.device);
    f110_graph *g = new (std::nothrow) f110_graph;
    if (!g) return fail(F110_E_INVALID, "f110_graph_create: out of host memory");
    g->h = h; g->epoch = h->epoch;
    const bool prof = h->prof_on;
    h->prof_on = false; // events cannot ride on graph nodes
    hipError_t e = hipSuccess;
    if (how == F110_GRAPH_NODES) {
        rc = run_step(h, actions, 0, Sink{nullptr, &g->launches});
        if (!rc) {
            e = hipGraphCreate(g->graph.put(), 0);
            hipGraphNode_t prev = nullptr;
            for (size_t i = 0; e == hipSuccess && i < g->launches.size(); i++) {
                KernelLaunch &l = g->launches[i];
                void *params[1] = {(void *)l.args.data()};
                hipKernelNodeParams np;
                memset(&np, 0, sizeof(np));
                np.func = const_cast<void *>(l.func); np.gridDim = l.grid; np.blockDim = l.block; np.sharedMemBytes = l.shmem;
                np.kernelParams = params; np.extra = nullptr;
                hipGraphNode_t node = nullptr;
                e = hipGraphAddKernelNode(&node, g->graph.get(), prev ? &prev : nullptr, prev ? 1 : 0, &np); // a chain: each kernel reads what the one before wrote
                prev = node;
            }
            g->nodes = (int)g->launches.size();
        }
    } else {
        e = hipStreamCreateWithFlags(g->cap.put(), hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamBeginCapture(g->cap.get(), hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            rc = run_step(h, actions, 0, Sink{g->cap.get()});
            e = hipStreamEndCapture(g->cap.get(), g->graph.put());
            size_t n = 0;
            if (e == hipSuccess && hipGraphGetNodes(g->graph.get(), nullptr, &n) == hipSuccess) g->nodes = (int)n;
        }
    }
    h->prof_on = prof;
    if (!rc && e == hipSuccess) e = hipGraphInstantiate(g->exec.put(), g->graph.get(), nullptr, nullptr, 0);
    if (rc || e != hipSuccess) {
        if (!rc) rc = fail(F110_E_HIP, "f110_graph_create: %s", hipGetErrorString(e));
        f110_graph_destroy(g);
        return rc;
    }
    *out = g;
    return F110_OK;
}

extern "C" int f110_graph_launch(f110_graph *g, void *stream)
{
    if (!g || !g->exec.get()) return fail(F110_E_INVALID, "f110_graph_launch: null graph");
    if (g->epoch != g->h->epoch)
        return fail(F110_E_INVALID, "f110_graph_launch: the graph is stale (a table, map, binding or launch setting of the handle "
                                    "changed since f110_graph_create: f110_launch_epoch moved from %lld to %lld); create it again",
                    (long long)g->epoch, (long long)g->h->epoch);
    if (int rc = check_device(g->h, "f110_graph_launch")) return rc;
    HIP_TRY(hipGraphLaunch(g->exec.get(), (hipStream_t)stream));
    return F110_OK;
}

extern "C" int f110_graph_info(f110_graph *g, int32_t *nodes, const char *dot_path)
{
    if (!g) return fail(F110_E_INVALID, "f110_graph_info: null graph");
    if (nodes) *nodes = g->nodes;
    if (dot_path && *dot_path) HIP_TRY(hipGraphDebugDotPrint(g->graph.get(), dot_path, 0));
    return F110_OK;
}

extern "C" int f110_set_scan_stages(f110_handle *h, const char *spec)
{
    if (!h) return fail(F110_E_INVALID, "f110_set_scan_stages: null handle");
    std::vector<StageSpec> parsed;
    if (spec && *spec) {
        const char *why = nullptr;
        if (!parse_stage_spec(spec, parsed, &why)) return fail(F110_E_INVALID, "f110_set_scan_stages: \"%s\": %s", spec, why);
        long long fixed = 0;
        for (const StageSpec &x : parsed) if (x.cars > 0) fixed += x.cars;
        if (fixed > (long long)h->cfg.num_envs * h->cfg.num_agents)
            return fail(F110_E_INVALID, "f110_set_scan_stages: \"%s\" names %lld cars, the handle has %d", spec, fixed, h->cfg.num_envs * h->cfg.num_agents);
    }
    h->stages = std::move(parsed);
    h->epoch++;
    return F110_OK;
}

extern "C" int f110_set_scan_order(f110_handle *h, const int32_t *order_dev)
{
    if (!h) return fail(F110_E_INVALID, "f110_set_scan_order: null handle");
    if (h->scan_order == order_dev) return F110_OK;
    h->scan_order = order_dev;
    h->epoch++; // the scan takes the pointer by value: a captured step is stale (the array's CONTENTS may change under it)
    return F110_OK;
}

extern "C" int f110_launch_epoch(f110_handle *h, int64_t *epoch)
{
    if (!h || !epoch) return fail(F110_E_INVALID, "f110_launch_epoch: null argument");
    *epoch = h->epoch;
    return F110_OK;
}

// ---------------------------------------------------------------- measurement aid
static void prof_clear(f110_handle *h)
{
    h->prof_ev.clear();
    h->prof_n = 0;
    h->prof_on = false;
}

extern "C" int f110_profile_every(f110_handle *h, int32_t every)
{
    if (!h || every < 1) return fail(F110_E_INVALID, "f110_profile_every: bad arguments");
    h->prof_every = every;
    return F110_OK;
}

extern "C" int f110_profile_begin(f110_handle *h, int32_t max_launches)
{
    if (!h || max_launches < 1 || max_launches > (1 << 20)) return fail(F110_E_INVALID, "f110_profile_begin: bad arguments");
    ON_DEVICE(h->cfg.device);
    prof_clear(h);
    h->prof_seq = 0;
    h->prof_ev.resize((size_t)2 * max_launches);
    for (auto &e : h->prof_ev) HIP_TRY(hipEventCreate(e.put()));
    h->prof_on = true;
    return F110_OK;
}

extern "C" int f110_profile_end(f110_handle *h, double *ms_total, int32_t *launches)
{
    if (!h || !ms_total || !launches) return fail(F110_E_INVALID, "f110_profile_end: null argument");
    if (!h->prof_on) return fail(F110_E_INVALID, "f110_profile_end: f110_profile_begin has not been called");
    double tot = 0;
    if (h->prof_n > 0) HIP_TRY(hipEventSynchronize(h->prof_ev[2 * h->prof_n - 1].get()));
    for (int i = 0; i < h->prof_n; i++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->prof_ev[2 * i].get(), h->prof_ev[2 * i + 1].get()));
        tot += ms;
    }
    *ms_total = tot;
    *launches = h->prof_n;
    prof_clear(h);
    return F110_OK;
}

// ---------------------------------------------------------------- function-level entry points
extern "C" int f110_scan(f110_handle *h, const double *poses, int32_t n, double *out64, float *out32,
                         uint32_t *lookups, void *stream)
{
    if (!h || n < 0) return fail(F110_E_INVALID, "f110_scan: bad arguments");
    if (!h->has_map) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    if (n == 0) return F110_OK;
    if (!poses || (!out64 && !out32)) return fail(F110_E_INVALID, "f110_scan: null pose or output pointer");
    if (int rc = check_device(h, "f110_scan")) return rc;
    return run_scan(h, scan_args(h, n, 1, poses, 3, 2, out32, out64, lookups), Sink{(hipStream_t)stream});
}

// The function-level entry points but f110_scan and f110_check_done: n == 0 does nothing, a null pointer or a bad count is
// F110_E_INVALID, the caller's current device must be the handle's; then `launch` enqueues the kernel on the caller's stream.
template <typename Launch>
static int launch_entry_point(f110_handle *h, int n, bool args_ok, const char *who, Launch launch)
{
    if (h && n == 0) return F110_OK;
    if (!h || !args_ok || n < 0) return fail(F110_E_INVALID, "%s: bad arguments", who);
    if (int rc = check_device(h, who)) return rc;
    launch();
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_update_pose(f110_handle *h, double *state, double *steer_buf, int32_t *steer_cnt,
                                const double *actions, int32_t n, void *stream)
{
    return launch_entry_point(h, n, state && steer_buf && steer_cnt && actions, "f110_update_pose", [&] {
        DynArgs d;
        memset(&d, 0, sizeof(d));
        d.n_cars = n; d.agents = 1; d.state = state; d.steer_buf = steer_buf; d.steer_cnt = steer_cnt; d.actions = actions;
        d.params = h->d_params.get(); d.param_slots = h->param_slots; d.dev_err = h->d_err.get(); d.time_step = h->cfg.timestep; d.integrator = h->cfg.integrator;
        hipLaunchKernelGGL(dynamics_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d);
    });
}

extern "C" int f110_vehicle_dynamics(f110_handle *h, const double *x, const double *u, int32_t n, int32_t kinematic,
                                     double *f, void *stream)
{
    return launch_entry_point(h, n, x && u && f, "f110_vehicle_dynamics", [&] {
        hipLaunchKernelGGL(rhs_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, u, n, kinematic,
                           h->d_params.get(), f);
    });
}

extern "C" int f110_get_vertices(f110_handle *h, const double *poses, int32_t n, double *verts, void *stream)
{
    return launch_entry_point(h, n, poses && verts, "f110_get_vertices", [&] {
        hipLaunchKernelGGL(vertices_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, poses, n,
                           h->h_params[0].v[P_LENGTH], h->h_params[0].v[P_WIDTH], verts);
    });
}

extern "C" int f110_gjk_pairs(f110_handle *h, const double *va, const double *vb, int32_t n, uint8_t *hit, void *stream)
{
    return launch_entry_point(h, n, va && vb && hit, "f110_gjk_pairs", [&] {
        hipLaunchKernelGGL(gjk_pairs_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, va, vb, n, hit);
    });
}

extern "C" int f110_collision_multiple(f110_handle *h, const double *verts, int32_t n, int32_t A, uint8_t *col,
                                       int32_t *cidx, void *stream)
{
    return launch_entry_point(h, n, verts && col && cidx && A >= 1, "f110_collision_multiple", [&] {
        hipLaunchKernelGGL(collision_multiple_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, n, A,
                           col, cidx);
    });
}

extern "C" int f110_check_ttc(f110_handle *h, const double *scans, const double *vel, int32_t n, uint8_t *hit,
                              void *stream)
{
    return launch_entry_point(h, n, scans && vel && hit, "f110_check_ttc", [&] {
        hipLaunchKernelGGL(ttc_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, scans, vel, n, h->cfg.num_beams,
                           h->d_beam_cosines.get(), h->d_side.get(), h->cfg.ttc_thresh, hit, (const int32_t *)nullptr, 0,
                           (uint32_t *)nullptr);
    });
}

extern "C" int f110_check_ttc_slots(f110_handle *h, const double *scans, const double *vel, const int32_t *slot_of_row,
                                    int32_t n, uint8_t *hit, void *stream)
{
    if (h && !h->side_n_slots)
        return fail(F110_E_INVALID, "f110_check_ttc_slots: no side-distance tables installed (f110_set_side_distance_slots)");
    return launch_entry_point(h, n, scans && vel && slot_of_row && hit, "f110_check_ttc_slots", [&] {
        hipLaunchKernelGGL(ttc_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, scans, vel, n, h->cfg.num_beams,
                           h->d_beam_cosines.get(), h->d_side_slots.get(), h->cfg.ttc_thresh, hit, slot_of_row,
                           h->side_n_slots, h->d_err.get());
    });
}

extern "C" int f110_ray_cast(f110_handle *h, const double *ego, const double *verts, int32_t n, double *scans,
                             int32_t *span, void *stream)
{
    return launch_entry_point(h, n, ego && verts && scans, "f110_ray_cast", [&] {
        hipLaunchKernelGGL(ray_cast_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, ego, verts, n,
                           h->cfg.num_beams, h->d_scan_angles.get(), h->d_beam_cs.get(), scans, span);
    });
}

extern "C" int f110_check_done(f110_handle *h, const double *poses, const double *start_poses, const double *start_rot,
                               const double *current_time, const uint8_t *collisions, int32_t n, int32_t num_agents,
                               int32_t ego_idx, uint8_t *near_start, int32_t *toggles, int32_t *lap_counts,
                               double *lap_times, uint8_t *done, uint8_t *checkpoint_done, void *stream)
{
    (void)h; // stateless (the strip width and the 0.1 threshold are constants of f110_env.py:216-231)
    if (n < 0 || num_agents < 1 || num_agents > F110_MAX_AGENTS) return fail(F110_E_INVALID, "f110_check_done: bad arguments");
    if (ego_idx < 0 || ego_idx >= num_agents) return fail(F110_E_INDEX, "f110_check_done: ego_idx %d out of range", ego_idx);
    if (n == 0) return F110_OK;
    if (!poses || !start_poses || !start_rot || !current_time || !collisions || !near_start || !toggles || !lap_counts ||
        !lap_times || !done)
        return fail(F110_E_INVALID, "f110_check_done: null pointer (only checkpoint_done is optional)");
    CheckDoneArgs a;
    a.n_envs = n; a.agents = num_agents; a.ego_idx = ego_idx; a.poses = poses; a.start = start_poses; a.start_rot = start_rot;
    a.current_time = current_time; a.collisions = collisions; a.near_start = near_start; a.toggles = toggles;
    a.lap_counts = lap_counts; a.lap_times = lap_times; a.done = done; a.checkpoint_done = checkpoint_done;
    hipLaunchKernelGGL(check_done_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
