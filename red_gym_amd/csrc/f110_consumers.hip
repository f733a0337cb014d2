// f110_consumers.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_handle.h"
#include "f110_planner.h"
#include "f110_progress.h"
#include "f110_shaping.h"
#include "f110_pathfollow.h"
#include "f110_replay.h"
#include "f110_priority.h"
#include "f110_episodes.h"

// ---------------------------------------------------------------- planner
// per device: the LDS a workgroup may use (queried once), the dynamic-LDS attribute already granted to
// pure_pursuit_kernel, and the two-entry raceline header {0, M} of the global-memory fallback of f110_pure_pursuit
struct DevLds { int max_bytes = -1; size_t pp_attr = 0; int32_t *hdr = nullptr; int hdr_m = -1; };
static DevLds &device_lds(int dev)
{
    static DevLds tab[64];
    DevLds &d = tab[dev & 63];
    if (d.max_bytes < 0) {
        int v = 0;
        d.max_bytes = hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess ? v : 0;
        // the attribute may report the 64 KiB every kernel gets without asking; gfx950 grants 160 KiB per workgroup
        // through hipFuncAttributeMaxDynamicSharedMemorySize
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
            d.max_bytes = std::max(d.max_bytes, 160 * 1024);
    }
    return d;
}

// {0, M} on the device for the single-raceline fallback.  Allocated once per device (not inside a stream capture: a
// caller that captures a policy with a long raceline makes one eager call first); the 8-byte upload is synchronous.
static int32_t *single_track_offsets(int dev, int M)
{
    DevLds &d = device_lds(dev);
    if (!d.hdr && hipMalloc((void **)&d.hdr, 2 * sizeof(int32_t)) != hipSuccess) { d.hdr = nullptr; return nullptr; }
    if (d.hdr_m != M) {
        const int32_t off[2] = {0, M};
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(d.hdr, off, sizeof(off), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        d.hdr_m = M;
    }
    return d.hdr;
}

// Host half of a raceline's grid of candidate lists (f110_plangrid.h PlanGrid): the points are (wp[stride * i], wp[stride * i + 1]),
// i < M; `g` gets the geometry and the degenerate flag, `count` / `cand` the tables to upload (g.count / g.cand stay unset).
// cell: edge of a grid cell in metres; margin: how far around the raceline's bounding box the grid reaches.  Shared by the
// planner's prepare and the progress tracker's install, so that both search the same lists.
static int build_plan_grid(const char *who, const double *wp, int stride, int M, double cell, double margin, PlanGrid &g,
                           std::vector<uint8_t> &count, std::vector<uint16_t> &cand)
{
    const size_t st = (size_t)stride;
    const int nseg = M - 1;
    double xl = 1e300, xh = -1e300, yl = 1e300, yh = -1e300;
    bool finite = true, degenerate = false;
    for (int i = 0; i < M; i++) {
        const double x = wp[st * (size_t)i], y = wp[st * (size_t)i + 1];
        finite = finite && std::isfinite(x) && std::isfinite(y);
        xl = std::min(xl, x); xh = std::max(xh, x); yl = std::min(yl, y); yh = std::max(yh, y);
    }
    if (!finite) return fail(F110_E_INVALID, "%s: the raceline has non-finite points", who);
    for (int i = 0; i < nseg; i++) {
        const double dx = wp[st * (size_t)(i + 1)] - wp[st * (size_t)i], dy = wp[st * (size_t)(i + 1) + 1] - wp[st * (size_t)i + 1];
        if (dx * dx + dy * dy == 0.0) degenerate = true;
    }
    memset(&g, 0, sizeof(g));
    g.x0 = xl - margin; g.y0 = yl - margin; g.inv_cell = 1.0 / cell;
    const double gw = std::ceil((xh + margin - g.x0) / cell), gh = std::ceil((yh + margin - g.y0) / cell);
    if (!(gw >= 1 && gh >= 1) || gw * gh > 16.0e6) return fail(F110_E_INVALID, "%s: grid of %.0f x %.0f cells (choose a larger cell)", who, gw, gh);
    g.gw = (int)gw; g.gh = (int)gh; g.degenerate = degenerate ? 1 : 0;
    const size_t cells = (size_t)g.gw * g.gh;
    count.assign(cells, 0);
    cand.assign(cells * PG_CAP, 0);
    if (!degenerate) {
        // segments bucketed by a coarse grid first, so that a cell only looks at the segments that can matter
        const double hd = 0.5 * cell * std::sqrt(2.0);
        auto seg_dist = [&](int i, double px, double py) {
            const double x0 = wp[st * (size_t)i], y0 = wp[st * (size_t)i + 1];
            const double dx = wp[st * (size_t)(i + 1)] - x0, dy = wp[st * (size_t)(i + 1) + 1] - y0;
            const double l2 = dx * dx + dy * dy;
            double t = ((px - x0) * dx + (py - y0) * dy) / l2;
            t = t < 0.0 ? 0.0 : t; t = t > 1.0 ? 1.0 : t;
            const double qx = px - (x0 + t * dx), qy = py - (y0 + t * dy);
            return std::sqrt(qx * qx + qy * qy);
        };
        std::vector<double> dist((size_t)nseg);
        for (int iy = 0; iy < g.gh; iy++)
            for (int ix = 0; ix < g.gw; ix++) {
                const double cx = g.x0 + (ix + 0.5) * cell, cy = g.y0 + (iy + 0.5) * cell;
                double D = 1e300;
                for (int i = 0; i < nseg; i++) { dist[(size_t)i] = seg_dist(i, cx, cy); D = std::min(D, dist[(size_t)i]); }
                const double lim = D + 2.0 * hd + 1e-6;
                unsigned n = 0;
                const size_t c = (size_t)iy * g.gw + ix;
                for (int i = 0; i < nseg && n <= (unsigned)PG_CAP; i++)
                    if (dist[(size_t)i] <= lim) { if (n < (unsigned)PG_CAP) cand[c * PG_CAP + n] = (uint16_t)i; n++; }
                count[c] = n > (unsigned)PG_CAP ? (uint8_t)PG_ALL : (uint8_t)n;
            }
    }
    return F110_OK;
}

// Builds the grid of candidate lists for one raceline (dev [M,3]) in the handle: a cold path (the raceline is copied to the host,
// ~0.1 s for the 783-point example raceline).  The caller promises to call it again when the raceline's values change; the pointer
// and M are what f110_pure_pursuit matches (red_gym_amd.Engine passes the handle only for the very tensor it prepared, unchanged,
// and NULL otherwise).  A successful call replaces the grid's memory and moves the launch epoch; a failed one leaves no grid.
// cell: edge of a grid cell in metres (0: 0.25); margin: how far around the raceline's bounding box the grid reaches (0: 3 m) --
// poses beyond it are planned by the exhaustive search.
extern "C" int f110_pure_pursuit_prepare(f110_handle *h, const double *waypoints, int32_t M, double cell, double margin, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_pure_pursuit_prepare: null argument");
    if (int rc = check_device(h, "f110_pure_pursuit_prepare")) return rc;
    h->plan_ok = false;
    if (!waypoints) return fail(F110_E_INVALID, "f110_pure_pursuit_prepare: null argument");
    if (M < 2 || M > 65535) return fail(F110_E_INVALID, "f110_pure_pursuit_prepare: M=%d waypoints (2..65535)", M);
    if (!(cell >= 0) || !(margin >= 0) || !std::isfinite(cell) || !std::isfinite(margin)) return fail(F110_E_INVALID, "f110_pure_pursuit_prepare: bad cell / margin");
    if (cell == 0) cell = 0.25;
    if (margin == 0) margin = 3.0;
    std::vector<double> wp((size_t)M * 3);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(wp.data(), waypoints, wp.size() * sizeof(double), hipMemcpyDeviceToHost));
    PlanGrid g;
    std::vector<uint8_t> count;
    std::vector<uint16_t> cand;
    if (int rc = build_plan_grid("f110_pure_pursuit_prepare", wp.data(), 3, M, cell, margin, g, count, cand)) return rc;
    ON_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize()); // an enqueued plan may still read the previous grid
    h->epoch++; // a captured launch of the grid kernel takes the grid's pointers by value: they are freed below
    PlanGridDev n;
    HIP_TRY(n.upload(g, count, cand));
    h->plan = std::move(n);
    h->plan_wp = waypoints; h->plan_M = M; h->plan_ok = true;
    return F110_OK;
}

extern "C" int f110_pure_pursuit(f110_handle *h, const double *waypoints, int32_t M, double lookahead, double vgain,
                                 double wheelbase, double max_reacquire, const double *state, int32_t n,
                                 double *actions, void *stream)
{
    // stateless: the handle is optional (NULL: the launch goes to the calling thread's current device)
    if (n < 0) return fail(F110_E_INVALID, "f110_pure_pursuit: bad arguments");
    if (n == 0) return F110_OK;
    if (h) if (int rc = check_device(h, "f110_pure_pursuit")) return rc;
    if (!waypoints || !state || !actions) return fail(F110_E_INVALID, "f110_pure_pursuit: null pointer");
    if (M < 2) return fail(F110_E_INVALID, "f110_pure_pursuit: M=%d waypoints (a raceline has at least 2)", M);
    PlanArgs a;
    a.waypoints = waypoints; a.M = M; a.lookahead = lookahead; a.vgain = vgain; a.wheelbase = wheelbase;
    a.max_reacquire = max_reacquire; a.state = state; a.n = n; a.actions = actions;
    if (h && h->plan_ok && h->plan_wp == waypoints && h->plan_M == M) {
        // a prepared raceline: one lane per car over the grid's candidate lists
        hipLaunchKernelGGL(pure_pursuit_grid_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, h->plan.g);
        HIP_TRY(hipGetLastError());
        return F110_OK;
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const size_t smem = pure_pursuit_lds_bytes(M);
    const DevLds &dl = device_lds(dev);
    if (dl.max_bytes <= 0) return fail(F110_E_HIP, "f110_pure_pursuit: cannot query the LDS size of device %d", dev);
    if (smem + 1024 > (size_t)dl.max_bytes) {
        // The raceline does not fit the LDS of this device (gfx950: 160 KiB, about 6 400 points): the global-memory
        // form, without a workspace for block boxes -- every block is evaluated.  f110_pure_pursuit_tracks with a
        // workspace is the fast way to plan on long or many racelines.
        PlanTracksArgs t;
        memset(&t, 0, sizeof(t));
        int32_t *off = single_track_offsets(dev, M);
        if (!off) return fail(F110_E_HIP, "f110_pure_pursuit: no device memory for the raceline header");
        t.t.waypoints = waypoints; t.t.offsets = off; t.t.K = 1; t.t.boxes = nullptr; t.track_of_car = nullptr;
        t.lookahead = lookahead; t.vgain = vgain; t.wheelbase = wheelbase; t.max_reacquire = max_reacquire;
        t.state = state; t.n = n; t.actions = actions;
        hipLaunchKernelGGL(pure_pursuit_tracks_kernel, dim3((n + PPG_WAVES - 1) / PPG_WAVES), dim3(PPG_WAVES * 64), 0, (hipStream_t)stream, t);
        HIP_TRY(hipGetLastError());
        return F110_OK;
    }
    if (smem > 64 * 1024 && smem > dl.pp_attr) { // raised once per device and size, not on every call (nor inside a captured policy)
        HIP_TRY(hipFuncSetAttribute((const void *)pure_pursuit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        device_lds(dev).pp_attr = smem;
    }
    hipLaunchKernelGGL(pure_pursuit_kernel, dim3((n + PP_WAVES - 1) / PP_WAVES), dim3(PP_WAVES * 64), smem, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int64_t f110_pure_pursuit_workspace(int32_t total_points, int32_t K)
{
    if (total_points < 0 || K < 0) return 0;
    return (((int64_t)total_points >> 6) + K) * 5;
}

extern "C" int f110_pure_pursuit_tracks(f110_handle *h, const double *waypoints, const int32_t *offsets_dev,
                                        const int32_t *offsets_host, int32_t K, const int32_t *track_of_car, double lookahead,
                                        double vgain, double wheelbase, double max_reacquire, const double *state, int32_t n,
                                        double *actions, double *workspace, int32_t boxes_valid, void *stream)
{
    if (n < 0 || K < 1) return fail(F110_E_INVALID, "f110_pure_pursuit_tracks: bad arguments (n=%d, K=%d)", n, K);
    if (h) if (int rc = check_device(h, "f110_pure_pursuit_tracks")) return rc;
    if (!waypoints || !offsets_dev || !offsets_host || !workspace) return fail(F110_E_INVALID, "f110_pure_pursuit_tracks: null pointer");
    int max_m = 0;
    if (offsets_host[0] != 0) return fail(F110_E_INVALID, "f110_pure_pursuit_tracks: offsets[0] must be 0");
    for (int k = 0; k < K; k++) {
        const int64_t m = (int64_t)offsets_host[k + 1] - offsets_host[k];
        if (m < 2 || m > 0x3fffffff) return fail(F110_E_INVALID, "f110_pure_pursuit_tracks: raceline %d has %lld points (at least 2)", k, (long long)m);
        max_m = std::max(max_m, (int)m);
    }
    TrackSet t;
    t.waypoints = waypoints; t.offsets = offsets_dev; t.K = K; t.boxes = workspace;
    if (!boxes_valid) {
        const int max_blocks = (max_m - 1 + 63) / 64;
        hipLaunchKernelGGL(track_boxes_kernel, dim3((max_blocks + 3) / 4, K), dim3(256), 0, (hipStream_t)stream, t);
        HIP_TRY(hipGetLastError());
    }
    if (n == 0) return F110_OK;
    if (!state || !actions) return fail(F110_E_INVALID, "f110_pure_pursuit_tracks: null pointer");
    PlanTracksArgs a;
    a.t = t; a.track_of_car = track_of_car; a.lookahead = lookahead; a.vgain = vgain; a.wheelbase = wheelbase;
    a.max_reacquire = max_reacquire; a.state = state; a.n = n; a.actions = actions;
    hipLaunchKernelGGL(pure_pursuit_tracks_kernel, dim3((n + PPG_WAVES - 1) / PPG_WAVES), dim3(PPG_WAVES * 64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- what the tracker and the shaper share
// Both read an env's reset off its clock (current_time == timestep): their installs refuse a handle whose clock cannot tell.
static int clock_usable(const f110_handle *h, const char *who)
{
    return h->cfg.timestep > 0.0 ? F110_OK : fail(F110_E_INVALID, "%s: the handle's timestep is %g (an env's reset is read off its clock: it must be positive)", who, h->cfg.timestep);
}

// The opening of a consumer's update (`who`): `what` is installed and bound (f110_<family>_install /
// _bind), the handle is bound and its device is the caller's current one.
static int update_ready(const f110_handle *h, const char *who, const char *what, const char *family, bool on, bool bound)
{
    if (!on) return fail(F110_E_INVALID, "%s: no %s is installed (f110_%s_install)", who, what, family);
    if (!bound) return fail(F110_E_UNBOUND, "%s: f110_%s_bind has not been called", who, family);
    if (!h->bound) return fail(F110_E_UNBOUND, "%s: f110_bind has not been called", who);
    return check_device(h, who);
}

// ---------------------------------------------------------------- progress along the raceline
// What install refuses, on host arrays alone (no handle, no device): the all-or-nothing rule of the map installs.
extern "C" int f110_progress_validate(const double *waypoints, const int32_t *offsets, int32_t K, const double *len, const double *cum,
                                      const double *psi, const double *lap_length, const int32_t *raceline_of_env, int32_t num_envs)
{
    const char *who = "f110_progress_validate";
    if (K < 1) return fail(F110_E_INVALID, "%s: K=%d racelines (at least 1)", who, K);
    if (!waypoints || !offsets || !len || !cum || !psi || !lap_length) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (num_envs < 0 || (raceline_of_env && num_envs < 1)) return fail(F110_E_INVALID, "%s: num_envs=%d", who, num_envs);
    if (offsets[0] != 0) return fail(F110_E_INVALID, "%s: offsets[0] must be 0", who);
    for (int k = 0; k < K; k++) {
        const int64_t m = (int64_t)offsets[k + 1] - offsets[k];
        if (m < 2 || m > 0x3fffffff) return fail(F110_E_INVALID, "%s: raceline %d has %lld points (at least 2)", who, k, (long long)m);
        const size_t o = (size_t)offsets[k];
        for (int64_t i = 0; i < m; i++) {
            if (!std::isfinite(waypoints[2 * (o + i)]) || !std::isfinite(waypoints[2 * (o + i) + 1]))
                return fail(F110_E_INVALID, "%s: raceline %d has a non-finite point (row %lld)", who, k, (long long)i);
            if (!std::isfinite(cum[o + i])) return fail(F110_E_INVALID, "%s: raceline %d: cum[%lld] is not finite", who, k, (long long)i);
        }
        for (int64_t i = 0; i + 1 < m; i++) {
            const double dx = waypoints[2 * (o + i + 1)] - waypoints[2 * (o + i)], dy = waypoints[2 * (o + i + 1) + 1] - waypoints[2 * (o + i) + 1];
            if (dx * dx + dy * dy == 0.0 || !(len[o + i] > 0.0))
                return fail(F110_E_INVALID, "%s: raceline %d has a zero-length segment (%lld)", who, k, (long long)i);
            if (!std::isfinite(len[o + i]) || !std::isfinite(psi[o + i]))
                return fail(F110_E_INVALID, "%s: raceline %d: len / psi of segment %lld is not finite", who, k, (long long)i);
        }
        if (!(lap_length[k] > 0.0) || !std::isfinite(lap_length[k]))
            return fail(F110_E_INVALID, "%s: raceline %d has lap length %g (must be positive and finite)", who, k, lap_length[k]);
    }
    if (raceline_of_env)
        for (int e = 0; e < num_envs; e++)
            if (raceline_of_env[e] < 0 || raceline_of_env[e] >= K)
                return fail(F110_E_INVALID, "%s: env %d on raceline %d (0..%d)", who, e, raceline_of_env[e], K - 1);
    return F110_OK;
}

extern "C" int f110_progress_install(f110_handle *h, const double *waypoints, const int32_t *offsets, int32_t K, const double *len,
                                     const double *cum, const double *psi, const double *lap_length, const int32_t *raceline_of_env,
                                     int32_t grid)
{
    if (!h) return fail(F110_E_INVALID, "f110_progress_install: null handle");
    f110_handle::Progress &p = h->progress;
    if (K == 0 || !waypoints) { // removes the tracker
        if (!p.on) return F110_OK;
        ON_DEVICE(h->cfg.device);
        HIP_TRY(hipDeviceSynchronize()); // an enqueued update may still read the tables
        const f110_progress_buffers bufs = p.bufs;
        const bool bound = p.bound;
        p = f110_handle::Progress();
        p.bufs = bufs; p.bound = bound;
        h->epoch++;
        return F110_OK;
    }
    if (int rc = f110_progress_validate(waypoints, offsets, K, len, cum, psi, lap_length, raceline_of_env, h->cfg.num_envs)) return rc;
    if (int rc = clock_usable(h, "f110_progress_install")) return rc;
    const size_t total = (size_t)offsets[K];
    f110_handle::Progress n;
    n.K = K;
    // one raceline: the planner's grid of candidate lists (a raceline it cannot hold is searched segment by segment: same results)
    PlanGrid g;
    std::vector<uint8_t> count;
    std::vector<uint16_t> cand;
    if (grid && K == 1 && total <= 65535 && build_plan_grid("f110_progress_install", waypoints, 2, (int)total, 0.25, 3.0, g, count, cand) == F110_OK)
        n.use_grid = true;
    ON_DEVICE(h->cfg.device);
    HIP_TRY(n.d_xy.upload(waypoints, total * 2));
    HIP_TRY(n.d_len.upload(len, total));
    HIP_TRY(n.d_cum.upload(cum, total));
    HIP_TRY(n.d_psi.upload(psi, total));
    HIP_TRY(n.d_lap.upload(lap_length, (size_t)K));
    HIP_TRY(n.d_offsets.upload(offsets, (size_t)K + 1));
    if (raceline_of_env) HIP_TRY(n.d_env.upload(raceline_of_env, (size_t)h->cfg.num_envs));
    if (n.use_grid) HIP_TRY(n.grid.upload(g, count, cand));
    HIP_TRY(hipDeviceSynchronize()); // an enqueued update may still read the tables that are replaced
    n.bufs = p.bufs; n.bound = p.bound; n.on = true;
    p = std::move(n);
    h->epoch++; // a captured update takes the tables' pointers by value
    return F110_OK;
}

extern "C" int f110_progress_bind(f110_handle *h, const f110_progress_buffers *b)
{
    if (!h || !b) return fail(F110_E_INVALID, "f110_progress_bind: null argument");
    if (!b->s || !b->d || !b->heading_error || !b->delta || !b->progress || !b->s_prev || !b->seg || !b->seen)
        return fail(F110_E_INVALID, "f110_progress_bind: a buffer is NULL (all eight are required)");
    h->progress.bufs = *b;
    h->progress.bound = true;
    h->epoch++;
    return F110_OK;
}

extern "C" int f110_progress_update(f110_handle *h, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_progress_update: null handle");
    const f110_handle::Progress &p = h->progress;
    if (int rc = update_ready(h, "f110_progress_update", "tracker", "progress", p.on, p.bound)) return rc;
    ProgressArgs a;
    memset(&a, 0, sizeof(a));
    a.state = h->bufs.state; a.n = h->cfg.num_envs * h->cfg.num_agents; a.agents = h->cfg.num_agents;
    a.xy = p.d_xy.get(); a.len = p.d_len.get(); a.cum = p.d_cum.get(); a.psi = p.d_psi.get(); a.lap = p.d_lap.get();
    a.offsets = p.d_offsets.get(); a.raceline_of_env = p.d_env.get(); a.K = p.K; a.use_grid = p.use_grid ? 1 : 0; a.g = p.grid.g;
    a.current_time = h->bufs.current_time; a.timestep = h->cfg.timestep;
    a.s = p.bufs.s; a.d = p.bufs.d; a.heading_error = p.bufs.heading_error; a.delta = p.bufs.delta; a.progress = p.bufs.progress;
    a.s_prev = p.bufs.s_prev; a.seg = p.bufs.seg; a.seen = p.bufs.seen; a.dev_err = h->d_err.get();
    hipLaunchKernelGGL(progress_kernel, dim3((a.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- reward shaping
// What install refuses, on the struct alone (no handle, no device).
extern "C" int f110_shaping_validate(const f110_shaping_config *cfg, int32_t num_agents)
{
    const char *who = "f110_shaping_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->rows < 1 || cfg->cols < 1) return fail(F110_E_INVALID, "%s: image of %d x %d pixels", who, cfg->rows, cfg->cols);
    if (cfg->agent < 0 || cfg->agent >= num_agents) return fail(F110_E_INVALID, "%s: agent %d (0..%d)", who, cfg->agent, num_agents - 1);
    if (cfg->neighborhood < 0) return fail(F110_E_INVALID, "%s: neighborhood %d is negative", who, cfg->neighborhood);
    if (cfg->clip_max < 0) return fail(F110_E_INVALID, "%s: clip_max %d is negative", who, cfg->clip_max);
    const double scalars[] = {cfg->scale, cfg->origin_x, cfg->origin_y, cfg->max_lane_halfwidth, cfg->w_collision, cfg->w_progress, cfg->w_centering};
    for (double v : scalars)
        if (!std::isfinite(v)) return fail(F110_E_INVALID, "%s: a scalar of the config is not finite", who);
    if (!(cfg->max_lane_halfwidth > 0.0)) return fail(F110_E_INVALID, "%s: max_lane_halfwidth %g must be positive", who, cfg->max_lane_halfwidth);
    return F110_OK;
}

extern "C" int f110_shaping_install(f110_handle *h, const f110_shaping_config *cfg)
{
    if (!h) return fail(F110_E_INVALID, "f110_shaping_install: null handle");
    f110_handle::Shaping &s = h->shaping;
    if (!cfg) { // removes the shaper
        if (!s.on) return F110_OK;
        s.on = false;
        h->replay.on = false; // the replay buffer records the shaper's image and reward: it goes with it
        h->epoch++;
        return F110_OK;
    }
    if (int rc = f110_shaping_validate(cfg, h->cfg.num_agents)) return rc;
    if (int rc = clock_usable(h, "f110_shaping_install")) return rc;
    if (h->replay.on && (cfg->rows != h->replay.rows || cfg->cols != h->replay.cols)) h->replay.on = false; // (its ring holds the old size)
    s.cfg = *cfg; // by value in every launch: nothing on the device to replace
    s.on = true;
    h->epoch++;
    return F110_OK;
}

extern "C" int f110_shaping_bind(f110_handle *h, const f110_shaping_buffers *b)
{
    if (!h || !b) return fail(F110_E_INVALID, "f110_shaping_bind: null argument");
    if (!b->collision_term || !b->progress_term || !b->centering_term || !b->total || !b->collided || !b->prev_xy || !b->t_seen)
        return fail(F110_E_INVALID, "f110_shaping_bind: a buffer is NULL (the seven behind the image are required)");
    if ((b->bitmap != nullptr) == (b->bitmap_bits != nullptr))
        return fail(F110_E_INVALID, "f110_shaping_bind: exactly one of bitmap and bitmap_bits is bound");
    h->shaping.bufs = *b;
    h->shaping.bound = true;
    h->epoch++;
    return F110_OK;
}

static int launch_shaping(const ShapingArgs &a, hipStream_t stream)
{
    if (a.n == 0) return F110_OK;
    const dim3 grid((a.n + SHAPING_WAVES - 1) / SHAPING_WAVES), block(64 * SHAPING_WAVES);
    if (a.bitmap_bits) hipLaunchKernelGGL(shaping_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(shaping_kernel<false>, grid, block, 0, stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_shaping_update(f110_handle *h, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_shaping_update: null handle");
    const f110_handle::Shaping &s = h->shaping;
    if (int rc = update_ready(h, "f110_shaping_update", "shaper", "shaping", s.on, s.bound)) return rc;
    ShapingArgs a;
    memset(&a, 0, sizeof(a));
    a.cfg = s.cfg; a.bitmap = s.bufs.bitmap; a.bitmap_bits = s.bufs.bitmap_bits; a.n = h->cfg.num_envs;
    a.xy = h->bufs.state + 7 * (size_t)s.cfg.agent; a.xy_stride = 7LL * h->cfg.num_agents;
    a.current_time = h->bufs.current_time; a.timestep = h->cfg.timestep;
    a.prev_in = s.bufs.prev_xy; a.prev_out = s.bufs.prev_xy; a.t_seen = s.bufs.t_seen;
    a.collision_term = s.bufs.collision_term; a.progress_term = s.bufs.progress_term; a.centering_term = s.bufs.centering_term;
    a.total = s.bufs.total; a.collided = s.bufs.collided; a.dev_err = h->d_err.get();
    return launch_shaping(a, (hipStream_t)stream);
}

// f110_shaping_terms and f110_shaping_terms_bits (`who`): exactly one of `bitmaps` / `packed` is the images
static int shaping_terms(const char *who, const f110_shaping_config *cfg, const uint8_t *bitmaps, const uint64_t *packed, const double *xy,
                         const double *prev_xy, int32_t n, double *collision_term, double *progress_term, double *centering_term,
                         double *total, uint8_t *collided, void *stream)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    f110_shaping_config c = *cfg;
    c.agent = 0;
    if (int rc = f110_shaping_validate(&c, 1)) return rc;
    if (n < 0 || (!bitmaps && !packed) || !xy || !prev_xy || !collision_term || !progress_term || !centering_term || !total || !collided)
        return fail(F110_E_INVALID, "%s: bad arguments", who);
    ShapingArgs a;
    memset(&a, 0, sizeof(a));
    a.cfg = c; a.bitmap = bitmaps; a.bitmap_bits = packed; a.n = n; a.xy = xy; a.xy_stride = 2; a.prev_in = prev_xy;
    a.collision_term = collision_term; a.progress_term = progress_term; a.centering_term = centering_term; a.total = total;
    a.collided = collided;
    return launch_shaping(a, (hipStream_t)stream);
}

extern "C" int f110_shaping_terms(const f110_shaping_config *cfg, const uint8_t *bitmaps, const double *xy, const double *prev_xy,
                                  int32_t n, double *collision_term, double *progress_term, double *centering_term, double *total,
                                  uint8_t *collided, void *stream)
{
    return shaping_terms("f110_shaping_terms", cfg, bitmaps, nullptr, xy, prev_xy, n, collision_term, progress_term, centering_term, total,
                         collided, stream);
}

extern "C" int f110_shaping_terms_bits(const f110_shaping_config *cfg, const uint64_t *packed, const double *xy, const double *prev_xy,
                                       int32_t n, double *collision_term, double *progress_term, double *centering_term, double *total,
                                       uint8_t *collided, void *stream)
{
    return shaping_terms("f110_shaping_terms_bits", cfg, nullptr, packed, xy, prev_xy, n, collision_term, progress_term, centering_term,
                         total, collided, stream);
}

// ---------------------------------------------------------------- path actions
// What install refuses, on the struct alone (no handle, no device).
extern "C" int f110_pathfollow_validate(const f110_pathfollow_config *cfg, int32_t num_agents)
{
    const char *who = "f110_pathfollow_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->agent < 0 || cfg->agent >= num_agents) return fail(F110_E_INVALID, "%s: agent %d (0..%d)", who, cfg->agent, num_agents - 1);
    if (cfg->horizon < 1 || cfg->horizon > PF_MAX_H) return fail(F110_E_INVALID, "%s: horizon %d (1..%d)", who, cfg->horizon, PF_MAX_H);
    if (cfg->replan_at < 1 || cfg->replan_at > PF_POINTS) return fail(F110_E_INVALID, "%s: replan_at %d (1..%d)", who, cfg->replan_at, PF_POINTS);
    const double scalars[] = {cfg->car_length, cfg->vector_length, cfg->max_diff_deg, cfg->dist_threshold, cfg->desired_velocity,
                              cfg->timestep, cfg->max_steer, cfg->q[0], cfg->q[1], cfg->q[2], cfg->q[3], cfg->r[0], cfg->r[1],
                              cfg->p[0], cfg->p[1], cfg->p[2], cfg->p[3]};
    for (double v : scalars)
        if (!std::isfinite(v)) return fail(F110_E_INVALID, "%s: a scalar of the config is not finite", who);
    for (int i = 0; i < 2; i++)
        if (!(cfg->r[i] > 0.0)) return fail(F110_E_INVALID, "%s: input weight r[%d] = %g must be positive (the QP must be strictly convex)", who, i, cfg->r[i]);
    for (int i = 0; i < 4; i++)
        if (cfg->q[i] < 0.0 || cfg->p[i] < 0.0) return fail(F110_E_INVALID, "%s: state weight q[%d] = %g / p[%d] = %g is negative", who, i, cfg->q[i], i, cfg->p[i]);
    if (!(cfg->vector_length > 0.0)) return fail(F110_E_INVALID, "%s: vector_length %g must be positive (the spline's knots are the chord lengths)", who, cfg->vector_length);
    if (!(cfg->timestep > 0.0)) return fail(F110_E_INVALID, "%s: timestep %g must be positive", who, cfg->timestep);
    // limits of a clip and a distance: negative, the kernel's selects and the reference's np.clip (lower bound above upper) disagree.
    // car_length and desired_velocity may be negative (a point behind the axle, a path followed backwards from its first point).
    if (cfg->max_diff_deg < 0.0 || cfg->max_steer < 0.0 || cfg->dist_threshold < 0.0)
        return fail(F110_E_INVALID, "%s: max_diff_deg %g, max_steer %g and dist_threshold %g must not be negative", who, cfg->max_diff_deg,
                    cfg->max_steer, cfg->dist_threshold);
    return F110_OK;
}

// The table of pathfollow_table_doubles(horizon) the act kernel reads: per axis the Hessian (halved) of the QP, H = sum_k wp_k
// a_k a_k' + wv_k b_k b_k' + r I over k = 1 .. horizon with a_k[j] = dt^2 (k - j - 1/2), b_k[j] = dt for j < k, and for every set
// of free variables the inverse of its restriction (Gauss-Jordan with partial pivoting; the matrix is positive definite).
static int pathfollow_tables(const f110_pathfollow_config &c, std::vector<double> &tab)
{
    const int H = c.horizon, HH = H * H;
    const double dt = c.timestep;
    tab.assign(pathfollow_table_doubles(H), 0.0);
    for (int ax = 0; ax < 2; ax++) {
        double *Hm = tab.data() + (size_t)ax * HH;
        for (int k = 1; k <= H; k++) {
            const double wp = k < H ? c.q[ax] : c.p[ax], wv = k < H ? c.q[2 + ax] : c.p[2 + ax];
            for (int i = 0; i < k; i++)
                for (int j = 0; j < k; j++)
                    Hm[i * H + j] += wp * (dt * dt * (k - i - 0.5)) * (dt * dt * (k - j - 0.5)) + wv * dt * dt;
        }
        for (int i = 0; i < H; i++) Hm[i * H + i] += c.r[ax];
        for (unsigned set = 1; set < (1u << H); set++) {
            int id[PF_MAX_H], m = 0;
            for (int i = 0; i < H; i++) if ((set >> i) & 1u) id[m++] = i;
            double aug[PF_MAX_H][2 * PF_MAX_H];
            for (int i = 0; i < m; i++)
                for (int j = 0; j < m; j++) { aug[i][j] = Hm[id[i] * H + id[j]]; aug[i][m + j] = i == j ? 1.0 : 0.0; }
            for (int col = 0; col < m; col++) {
                int piv = col;
                for (int i = col + 1; i < m; i++) if (std::fabs(aug[i][col]) > std::fabs(aug[piv][col])) piv = i;
                if (!(std::fabs(aug[piv][col]) > 0.0)) return fail(F110_E_INVALID, "f110_pathfollow: the QP's Hessian is singular");
                for (int j = 0; j < 2 * m; j++) std::swap(aug[col][j], aug[piv][j]);
                const double d = aug[col][col];
                for (int j = 0; j < 2 * m; j++) aug[col][j] /= d;
                for (int i = 0; i < m; i++) {
                    if (i == col) continue;
                    const double fct = aug[i][col];
                    for (int j = 0; j < 2 * m; j++) aug[i][j] -= fct * aug[col][j];
                }
            }
            double *Z = tab.data() + (size_t)2 * HH + ((size_t)ax * ((size_t)1 << H) + set) * HH;
            for (int i = 0; i < m; i++)
                for (int j = 0; j < m; j++) Z[id[i] * H + id[j]] = 0.5 * (aug[i][m + j] + aug[j][m + i]);
        }
    }
    return F110_OK;
}

extern "C" int f110_pathfollow_install(f110_handle *h, const f110_pathfollow_config *cfg)
{
    if (!h) return fail(F110_E_INVALID, "f110_pathfollow_install: null handle");
    f110_handle::PathFollow &p = h->follow;
    if (!cfg) { // removes the follower (the table stays for the next install: an enqueued act may still read it)
        if (!p.on) return F110_OK;
        p.on = false;
        h->epoch++;
        return F110_OK;
    }
    if (int rc = f110_pathfollow_validate(cfg, h->cfg.num_agents)) return rc;
    if (int rc = clock_usable(h, "f110_pathfollow_install")) return rc;
    std::vector<double> tab;
    if (int rc = pathfollow_tables(*cfg, tab)) return rc;
    ON_DEVICE(h->cfg.device);
    DevBuf<double> n;
    HIP_TRY(n.upload(tab.data(), tab.size()));
    HIP_TRY(hipDeviceSynchronize()); // an enqueued act may still read the table that is replaced
    p.d_qp = std::move(n);
    p.cfg = *cfg;
    p.on = true;
    h->epoch++; // a captured act takes the table's pointer and the configuration by value
    return F110_OK;
}

extern "C" int f110_pathfollow_bind(f110_handle *h, const f110_pathfollow_buffers *b)
{
    if (!h || !b) return fail(F110_E_INVALID, "f110_pathfollow_bind: null argument");
    if (!b->path_points || !b->path_index || !b->path_replanned || !b->mpc_accel || !b->t_seen)
        return fail(F110_E_INVALID, "f110_pathfollow_bind: a buffer is NULL (all five are required)");
    h->follow.bufs = *b;
    h->follow.bound = true;
    h->epoch++;
    return F110_OK;
}

static int launch_pathfollow_act(const PathFollowArgs &a, hipStream_t stream)
{
    if (a.n == 0) return F110_OK;
    hipLaunchKernelGGL(pathfollow_act_kernel, dim3((unsigned)((2LL * a.n + 255) / 256)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

static int launch_pathfollow_advance(const PathAdvanceArgs &a, hipStream_t stream)
{
    if (a.n == 0) return F110_OK;
    hipLaunchKernelGGL(pathfollow_advance_kernel, dim3((a.n + 255) / 256), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_pathfollow_act(f110_handle *h, const double *raw_actions, double *actions_out, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_pathfollow_act: null handle");
    const f110_handle::PathFollow &p = h->follow;
    if (int rc = update_ready(h, "f110_pathfollow_act", "path follower", "pathfollow", p.on, p.bound)) return rc;
    if (!raw_actions || !actions_out) return fail(F110_E_INVALID, "f110_pathfollow_act: null pointer");
    PathFollowArgs a;
    memset(&a, 0, sizeof(a));
    const long long A = h->cfg.num_agents;
    a.cfg = p.cfg; a.n = h->cfg.num_envs; a.raw = raw_actions;
    a.pose = h->bufs.state + 7 * (size_t)p.cfg.agent; a.pose_stride = 7 * A; a.th_off = 4;
    a.vel = h->bufs.state + 7 * (size_t)p.cfg.agent + 3; a.vel_stride = 7 * A; a.has_vy = 0; // linear_vels_y is always 0
    a.path = p.bufs.path_points; a.index = p.bufs.path_index; a.replanned = p.bufs.path_replanned; a.qp = p.d_qp.get();
    a.accel = p.bufs.mpc_accel; a.actions = actions_out + 2 * (size_t)p.cfg.agent; a.act_stride = 2 * A;
    a.dev_err = h->d_err.get();
    return launch_pathfollow_act(a, (hipStream_t)stream);
}

extern "C" int f110_pathfollow_update(f110_handle *h, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_pathfollow_update: null handle");
    const f110_handle::PathFollow &p = h->follow;
    if (int rc = update_ready(h, "f110_pathfollow_update", "path follower", "pathfollow", p.on, p.bound)) return rc;
    PathAdvanceArgs a;
    memset(&a, 0, sizeof(a));
    a.cfg = p.cfg; a.n = h->cfg.num_envs;
    a.xy = h->bufs.state + 7 * (size_t)p.cfg.agent; a.xy_stride = 7LL * h->cfg.num_agents;
    a.path = p.bufs.path_points; a.index_in = p.bufs.path_index; a.index_out = p.bufs.path_index;
    a.current_time = h->bufs.current_time; a.timestep = h->cfg.timestep; a.t_seen = p.bufs.t_seen; a.dev_err = h->d_err.get();
    return launch_pathfollow_advance(a, (hipStream_t)stream);
}

static int pathfollow_stateless(const f110_pathfollow_config *cfg, f110_pathfollow_config &c, const char *who)
{
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    c = *cfg;
    c.agent = 0;
    return f110_pathfollow_validate(&c, 1);
}

extern "C" int f110_pathfollow_decode(const f110_pathfollow_config *cfg, const double *raw_actions, const double *poses, int32_t n,
                                      double *paths, void *stream)
{
    PathFollowArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = pathfollow_stateless(cfg, a.cfg, "f110_pathfollow_decode")) return rc;
    if (n < 0 || !raw_actions || !poses || !paths) return fail(F110_E_INVALID, "f110_pathfollow_decode: bad arguments");
    a.n = n; a.raw = raw_actions; a.pose = poses; a.pose_stride = 3; a.th_off = 2; a.path = paths;
    return launch_pathfollow_act(a, (hipStream_t)stream);
}

extern "C" int f110_pathfollow_mpc(const f110_pathfollow_config *cfg, const double *paths, const double *vels, int32_t n, double *dists,
                                   double *ref_traj, double *accel, double *actions, int32_t *qp_steps, uint32_t *dev_err, void *stream)
{
    PathFollowArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = pathfollow_stateless(cfg, a.cfg, "f110_pathfollow_mpc")) return rc;
    if (n < 0 || !paths || !vels || !dists || !ref_traj || !accel || !actions) return fail(F110_E_INVALID, "f110_pathfollow_mpc: bad arguments");
    std::vector<double> tab;
    if (int rc = pathfollow_tables(a.cfg, tab)) return rc;
    DevBuf<double> d_qp;
    HIP_TRY(d_qp.upload(tab.data(), tab.size()));
    a.n = n; a.path = const_cast<double *>(paths); a.vel = vels; a.vel_stride = 2; a.has_vy = 1; a.qp = d_qp.get();
    a.dists = dists; a.ref_traj = ref_traj; a.accel = accel; a.actions = actions; a.act_stride = 2; a.qp_steps = qp_steps; a.dev_err = dev_err;
    if (int rc = launch_pathfollow_act(a, (hipStream_t)stream)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); // the table is freed on return
    return F110_OK;
}

extern "C" int f110_pathfollow_advance(const f110_pathfollow_config *cfg, const double *paths, const int32_t *index, const double *xy,
                                       int32_t n, int32_t *index_out, void *stream)
{
    PathAdvanceArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = pathfollow_stateless(cfg, a.cfg, "f110_pathfollow_advance")) return rc;
    if (n < 0 || !paths || !index || !xy || !index_out) return fail(F110_E_INVALID, "f110_pathfollow_advance: bad arguments");
    a.n = n; a.xy = xy; a.xy_stride = 2; a.path = paths; a.index_in = index; a.index_out = index_out;
    return launch_pathfollow_advance(a, (hipStream_t)stream);
}

// ---------------------------------------------------------------- replay buffer
// What install refuses, on the structs alone (no handle, no device).  `shaping`: the installed shaper's configuration, NULL = off.
extern "C" int f110_replay_validate(const f110_replay_config *cfg, const f110_shaping_config *shaping, int32_t num_envs)
{
    const char *who = "f110_replay_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (!shaping) return fail(F110_E_INVALID, "%s: reward shaping is off (the buffer records the shaper's bitmap and reward: f110_shaping_install)", who);
    if (shaping->rows < 1 || shaping->cols < 1 || shaping->rows > REPLAY_MAX_DIM || shaping->cols > REPLAY_MAX_DIM)
        return fail(F110_E_INVALID, "%s: image of %d x %d pixels (1..%d)", who, shaping->rows, shaping->cols, REPLAY_MAX_DIM);
    if (cfg->steps < 2) return fail(F110_E_INVALID, "%s: %d step slots (at least 2)", who, cfg->steps);
    if (cfg->action_dim < 1) return fail(F110_E_INVALID, "%s: action_dim %d (at least 1)", who, cfg->action_dim);
    if (num_envs < 1) return fail(F110_E_INVALID, "%s: num_envs=%d", who, num_envs);
    // every size the kernels form, in bytes, stays below 2^62
    const long double lim = 4611686018427387904.0L;
    const long double cells = ((long double)cfg->steps + 1.0L) * (long double)num_envs;
    const long double frame = (long double)shaping->rows * (long double)replay_words(shaping->cols) * 8.0L;
    if (cells * frame >= lim || cells * (long double)cfg->action_dim * 4.0L >= lim || cells * 8.0L >= lim)
        return fail(F110_E_INVALID, "%s: a ring of %d steps x %d envs (frames of %d x %d, %d action values) overflows", who, cfg->steps, num_envs,
                    shaping->rows, shaping->cols, cfg->action_dim);
    return F110_OK;
}

extern "C" int f110_replay_install(f110_handle *h, const f110_replay_config *cfg)
{
    if (!h) return fail(F110_E_INVALID, "f110_replay_install: null handle");
    f110_handle::Replay &r = h->replay;
    if (!cfg) { // removes the buffer (the ring is the caller's)
        if (!r.on) return F110_OK;
        r.on = false; r.bound = false;
        h->priority.on = false; h->priority.bound = false; // the tree is over this ring's transitions
        h->epoch++;
        return F110_OK;
    }
    if (int rc = f110_replay_validate(cfg, h->shaping.on ? &h->shaping.cfg : nullptr, h->cfg.num_envs)) return rc;
    if (int rc = clock_usable(h, "f110_replay_install")) return rc;
    h->priority.on = false; h->priority.bound = false;
    r.cfg = *cfg; r.rows = h->shaping.cfg.rows; r.cols = h->shaping.cfg.cols;
    r.on = true; r.bound = false; // the ring's shape may have changed: bind again
    h->epoch++;
    return F110_OK;
}

extern "C" int f110_replay_bind(f110_handle *h, const f110_replay_buffers *b)
{
    if (!h || !b) return fail(F110_E_INVALID, "f110_replay_bind: null argument");
    if (!b->frames || !b->actions || !b->rewards || !b->dones || !b->valid || !b->count || !b->chain_start || !b->t_seen || !b->last_valid || !b->action_in)
        return fail(F110_E_INVALID, "f110_replay_bind: a buffer is NULL (all ten are required)");
    if ((uintptr_t)b->frames % 16) return fail(F110_E_INVALID, "f110_replay_bind: frames must be 16-byte aligned");
    h->replay.bufs = *b;
    h->replay.bound = true;
    h->epoch++;
    return F110_OK;
}

// `who` may run: the buffer is installed and bound, and the shaper it records still draws images of the ring's size
static int replay_ready(const f110_handle *h, const char *who, ReplayRing &g)
{
    const f110_handle::Replay &r = h->replay;
    if (int rc = update_ready(h, who, "replay buffer", "replay", r.on, r.bound)) return rc;
    const f110_handle::Shaping &s = h->shaping;
    if (!s.on || !s.bound || s.cfg.rows != r.rows || s.cfg.cols != r.cols)
        return fail(F110_E_INVALID, "%s: the shaper is off or draws another image size than the ring holds (install the buffer again)", who);
    memset(&g, 0, sizeof(g));
    g.frames = r.bufs.frames; g.actions = r.bufs.actions; g.rewards = r.bufs.rewards; g.dones = r.bufs.dones; g.valid = r.bufs.valid;
    g.count = (long long *)r.bufs.count; g.steps = r.cfg.steps; g.n_envs = h->cfg.num_envs; g.rows = r.rows; g.cols = r.cols;
    g.action_dim = r.cfg.action_dim; g.dev_err = h->d_err.get();
    return F110_OK;
}

static int priority_push(const f110_handle *h, const ReplayRing &g, hipStream_t stream);

extern "C" int f110_replay_update(f110_handle *h, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_replay_update: null handle");
    ReplayPushArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, "f110_replay_update", a.ring)) return rc;
    const f110_handle::Replay &r = h->replay;
    if (((uintptr_t)h->shaping.bufs.bitmap | (uintptr_t)h->shaping.bufs.bitmap_bits) % 16)
        return fail(F110_E_INVALID, "f110_replay_update: the shaper's bitmap must be 16-byte aligned");
    a.bitmap = h->shaping.bufs.bitmap; a.bitmap_bits = h->shaping.bufs.bitmap_bits; a.action_in = r.bufs.action_in; a.total = h->shaping.bufs.total; a.done = (const uint8_t *)h->bufs.done;
    a.current_time = h->bufs.current_time; a.timestep = h->cfg.timestep; a.chain_start = (const long long *)r.bufs.chain_start;
    a.t_seen = r.bufs.t_seen; a.last_valid = r.bufs.last_valid;
    hipLaunchKernelGGL(replay_push_kernel, dim3((unsigned)a.ring.n_envs), dim3(REPLAY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    if (h->priority.on && h->priority.bound)
        if (int rc = priority_push(h, a.ring, (hipStream_t)stream)) return rc;
    hipLaunchKernelGGL(replay_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a.ring.count);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_draw(f110_handle *h, uint64_t seed, uint64_t first_draw, int32_t n, int64_t *indices, uint8_t *ok, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_replay_draw: null handle");
    ReplayDrawArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, "f110_replay_draw", a.ring)) return rc;
    if (n < 0 || !indices || !ok) return fail(F110_E_INVALID, "f110_replay_draw: bad arguments");
    if (n == 0) return F110_OK;
    a.seed = seed; a.first = first_draw; a.n = n; a.idx = (long long *)indices; a.ok = ok;
    hipLaunchKernelGGL(replay_draw_kernel, dim3((unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_gather(f110_handle *h, const int64_t *indices, int32_t n, void *s, void *ns, int32_t as_f32, double scale,
                                  float *a_out, double *r_out, uint8_t *d_out, uint8_t *ok, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_replay_gather: null handle");
    ReplayGatherArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, "f110_replay_gather", a.ring)) return rc;
    if (n < 0 || !indices || !s || !ns || !a_out || !r_out || !d_out || !ok) return fail(F110_E_INVALID, "f110_replay_gather: bad arguments");
    if ((uintptr_t)s % 16 || (uintptr_t)ns % 16) return fail(F110_E_INVALID, "f110_replay_gather: s and ns must be 16-byte aligned");
    if (n == 0) return F110_OK;
    a.idx = (const long long *)indices; a.n = n;
    if (as_f32) { a.s32 = (float *)s; a.ns32 = (float *)ns; a.on = 255.0f * (float)scale; }
    else { a.s8 = (uint8_t *)s; a.ns8 = (uint8_t *)ns; }
    a.a = a_out; a.r = r_out; a.d = d_out; a.ok = ok;
    hipLaunchKernelGGL(replay_gather_kernel, dim3((unsigned)n, (unsigned)((a.ring.rows + REPLAY_ROWS - 1) / REPLAY_ROWS), 2), dim3(REPLAY_THREADS), 0,
                       (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_locate(f110_handle *h, const int64_t *indices, int32_t n, int64_t *s_frame, int64_t *ns_frame, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_replay_locate: null handle");
    ReplayRing g;
    if (int rc = replay_ready(h, "f110_replay_locate", g)) return rc;
    if (n < 0 || !indices || !s_frame || !ns_frame) return fail(F110_E_INVALID, "f110_replay_locate: bad arguments");
    if (n == 0) return F110_OK;
    hipLaunchKernelGGL(replay_locate_kernel, dim3((unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, (hipStream_t)stream,
                       g, (const long long *)indices, n, (long long *)s_frame, (long long *)ns_frame);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_sample(f110_handle *h, uint64_t seed, uint64_t *counter, int32_t n, int64_t *indices, int64_t *s_frame, int64_t *ns_frame,
                                  float *a_out, double *r_out, uint8_t *d_out, uint8_t *ok, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_replay_sample: null handle");
    ReplaySampleArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, "f110_replay_sample", a.ring)) return rc;
    if (n < 0 || !counter || !indices || !s_frame || !ns_frame || !a_out || !r_out || !d_out || !ok)
        return fail(F110_E_INVALID, "f110_replay_sample: bad arguments");
    if ((uintptr_t)counter % 8) return fail(F110_E_INVALID, "f110_replay_sample: the counter is not 8-byte aligned");
    if (n == 0) return F110_OK;
    a.seed = seed; a.counter = (const unsigned long long *)counter; a.n = n;
    a.idx = (long long *)indices; a.s_frame = (long long *)s_frame; a.ns_frame = (long long *)ns_frame;
    a.a = a_out; a.r = r_out; a.d = d_out; a.ok = ok;
    hipLaunchKernelGGL(replay_sample_kernel, dim3((unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(replay_counter_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long *)counter, (unsigned long long)n);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// what both n-step entries ask of their scalars
static int replay_nstep_scalars(const char *who, int32_t n, int32_t nstep, double gamma)
{
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%d", who, n);
    if (nstep < 1 || nstep > F110_REPLAY_MAX_NSTEP) return fail(F110_E_INVALID, "%s: nstep %d (1..%d)", who, nstep, F110_REPLAY_MAX_NSTEP);
    if (!std::isfinite(gamma)) return fail(F110_E_INVALID, "%s: gamma is not finite", who);
    return F110_OK;
}

// The sample form of ReplayNstepArgs (its ring is the caller's): the scalars and pointers checked, then filled in.  What
// f110_replay_sample_nstep and f110_priority_sample share.
static int replay_sample_nstep_args(const char *who, ReplayNstepArgs &a, uint64_t seed, uint64_t *counter, int32_t n, int32_t nstep, double gamma,
                                    int64_t *indices, int64_t *s_frame, int64_t *ns_frame, float *a_out, double *ret, uint8_t *d_out, uint8_t *ok,
                                    double *discount, int32_t *span)
{
    if (int rc = replay_nstep_scalars(who, n, nstep, gamma)) return rc;
    if (!counter || !indices || !s_frame || !ns_frame || !a_out || !ret || !d_out || !ok || !discount || !span)
        return fail(F110_E_INVALID, "%s: null argument", who);
    if ((uintptr_t)counter % 8) return fail(F110_E_INVALID, "%s: the counter is not 8-byte aligned", who);
    a.seed = seed; a.counter = (const unsigned long long *)counter; a.n = n; a.nstep = nstep; a.gamma = gamma;
    a.idx = (long long *)indices; a.s_frame = (long long *)s_frame; a.ns_frame = (long long *)ns_frame;
    a.a = a_out; a.ret = ret; a.d = d_out; a.ok = ok; a.discount = discount; a.span = span;
    return F110_OK;
}

extern "C" int f110_replay_nstep(f110_handle *h, const int64_t *indices, int32_t n, int32_t nstep, double gamma, int64_t *ns_frame, double *ret,
                                 uint8_t *d_out, double *discount, int32_t *span, void *stream)
{
    const char *who = "f110_replay_nstep";
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    ReplayNstepArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, who, a.ring)) return rc;
    if (int rc = replay_nstep_scalars(who, n, nstep, gamma)) return rc;
    if (!indices || !ns_frame || !ret || !d_out || !discount || !span) return fail(F110_E_INVALID, "%s: null argument", who);
    if (n == 0) return F110_OK;
    a.idx_in = (const long long *)indices; a.n = n; a.nstep = nstep; a.gamma = gamma;
    a.ns_frame = (long long *)ns_frame; a.ret = ret; a.d = d_out; a.discount = discount; a.span = span;
    hipLaunchKernelGGL(replay_nstep_kernel, dim3((unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_sample_nstep(f110_handle *h, uint64_t seed, uint64_t *counter, int32_t n, int32_t nstep, double gamma, int64_t *indices,
                                        int64_t *s_frame, int64_t *ns_frame, float *a_out, double *ret, uint8_t *d_out, uint8_t *ok, double *discount,
                                        int32_t *span, void *stream)
{
    const char *who = "f110_replay_sample_nstep";
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    ReplayNstepArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, who, a.ring)) return rc;
    if (int rc = replay_sample_nstep_args(who, a, seed, counter, n, nstep, gamma, indices, s_frame, ns_frame, a_out, ret, d_out, ok, discount, span)) return rc;
    if (n == 0) return F110_OK;
    hipLaunchKernelGGL(replay_sample_nstep_kernel, dim3((unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, (hipStream_t)stream,
                       a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(replay_counter_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long *)counter, (unsigned long long)n);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_stack(f110_handle *h, const int64_t *frame_rows, int32_t n, int32_t stack, int64_t *rows_out, int32_t *depth, void *stream)
{
    const char *who = "f110_replay_stack";
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    ReplayStackArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = replay_ready(h, who, a.ring)) return rc;
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%d", who, n);
    if (stack < 1 || stack > F110_REPLAY_MAX_STACK) return fail(F110_E_INVALID, "%s: stack %d (1..%d)", who, stack, F110_REPLAY_MAX_STACK);
    if (!frame_rows && n != a.ring.n_envs)
        return fail(F110_E_INVALID, "%s: n=%d rows without frame_rows (the newest frame of each of the %d envs)", who, n, a.ring.n_envs);
    if (!rows_out || !depth) return fail(F110_E_INVALID, "%s: null argument", who);
    if (n == 0) return F110_OK;
    a.rows_in = (const long long *)frame_rows; a.n = n; a.stack = stack; a.rows_out = (long long *)rows_out; a.depth = depth;
    hipLaunchKernelGGL(replay_stack_kernel, dim3((unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// ---------------------------------------------------------------- prioritized replay: the tree alone, then on the handle
static PriorityTree priority_tree(const uint32_t *leaf, const uint64_t *node, int64_t L, uint32_t *dev_err)
{
    PriorityTree t;
    t.leaf = const_cast<uint32_t *>(leaf); t.node = (unsigned long long *)const_cast<uint64_t *>(node); t.lay = priority_layout(L); t.dev_err = dev_err;
    return t;
}

// every level from the leaves, bottom up: one launch per level
static int priority_rebuild(const PriorityTree &t, hipStream_t stream)
{
    for (int lev = 1; lev <= t.lay.levels; lev++) {
        const long long waves = t.lay.count[lev - 1], per = PT_THREADS / 64;
        hipLaunchKernelGGL(ptree_level_kernel, dim3((unsigned)((waves + per - 1) / per)), dim3(PT_THREADS), 0, stream, t, lev);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

// the set's two launches: every named leaf cleared, then raised
static int priority_apply(const PrioritySetArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.n + PT_THREADS - 1) / PT_THREADS));
    hipLaunchKernelGGL(ptree_clear_kernel, grid, dim3(PT_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ptree_raise_kernel, grid, dim3(PT_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int64_t f110_priority_node_words(int64_t L) { return priority_node_words(L); }

extern "C" int f110_ptree_rebuild(const uint32_t *leaf, uint64_t *node, int64_t L, void *stream)
{
    const char *who = "f110_ptree_rebuild";
    if (int rc = priority_tree_check(who, leaf, node, L)) return rc;
    const PriorityTree t = priority_tree(leaf, node, L, nullptr);
    if (t.lay.levels == 0) return F110_OK;
    if (int rc = check_device_pointers(who, (hipStream_t)stream, {{"leaf", leaf}, {"node", node}})) return rc;
    return priority_rebuild(t, (hipStream_t)stream);
}

extern "C" int f110_ptree_set(uint32_t *leaf, uint64_t *node, int64_t L, const int64_t *idx, const uint32_t *q, int32_t n, void *stream)
{
    const char *who = "f110_ptree_set";
    if (int rc = priority_tree_check(who, leaf, node, L)) return rc;
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%d", who, n);
    if (!idx) return fail(F110_E_INVALID, "%s: null idx", who);
    if (!q) return fail(F110_E_INVALID, "%s: null q", who);
    if (n == 0) return F110_OK;
    std::vector<DevicePtr> ptrs = {{"leaf", leaf}, {"idx", idx}, {"q", q}};
    if (node) ptrs.push_back({"node", node});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    PrioritySetArgs a;
    memset(&a, 0, sizeof(a));
    a.tree = priority_tree(leaf, node, L, nullptr); a.idx = (const long long *)idx; a.q_in = q; a.n = n;
    return priority_apply(a, (hipStream_t)stream);
}

extern "C" int f110_ptree_pick(const uint32_t *leaf, const uint64_t *node, int64_t L, uint64_t seed, uint64_t first_draw, int32_t n, int64_t *idx_out,
                               uint32_t *q_out, void *stream)
{
    const char *who = "f110_ptree_pick";
    if (int rc = priority_tree_check(who, leaf, node, L)) return rc;
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%d", who, n);
    if (!idx_out) return fail(F110_E_INVALID, "%s: null idx_out", who);
    if (!q_out) return fail(F110_E_INVALID, "%s: null q_out", who);
    if (n == 0) return F110_OK;
    std::vector<DevicePtr> ptrs = {{"leaf", leaf}, {"idx_out", idx_out}, {"q_out", q_out}};
    if (node) ptrs.push_back({"node", node});
    if (int rc = check_device_pointers(who, (hipStream_t)stream, ptrs)) return rc;
    const int per = PT_THREADS / 64;
    hipLaunchKernelGGL(ptree_pick_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(PT_THREADS), 0, (hipStream_t)stream,
                       priority_tree(leaf, node, L, nullptr), (unsigned long long)seed, (unsigned long long)first_draw, (int)n, (long long *)idx_out, q_out);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_priority_install(f110_handle *h, const f110_priority_config *cfg)
{
    const char *who = "f110_priority_install";
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    f110_handle::Priority &p = h->priority;
    if (!cfg) { // removes the feature (the tree is the caller's)
        if (!p.on) return F110_OK;
        p.on = false; p.bound = false;
        h->epoch++;
        return F110_OK;
    }
    if (int rc = priority_config_check(who, cfg)) return rc;
    if (!h->replay.on) return fail(F110_E_INVALID, "%s: no replay buffer is installed (f110_replay_install)", who);
    const long long L = (long long)h->replay.cfg.steps * (long long)h->cfg.num_envs;
    if (!priority_leaves_ok(L)) return fail(F110_E_INVALID, "%s: a ring of %lld transitions (1..%lld)", who, L, (long long)F110_PRIORITY_MAX_LEAVES);
    p.cfg = *cfg;
    p.on = true; p.bound = false;
    h->epoch++;
    return F110_OK;
}

extern "C" int f110_priority_bind(f110_handle *h, const f110_priority_buffers *b)
{
    const char *who = "f110_priority_bind";
    if (!h || !b) return fail(F110_E_INVALID, "%s: null argument", who);
    if (!h->priority.on || !h->replay.on) return fail(F110_E_INVALID, "%s: no priorities are installed (f110_priority_install)", who);
    const long long L = (long long)h->replay.cfg.steps * (long long)h->cfg.num_envs;
    if (int rc = priority_tree_check(who, b->leaf, b->node, L)) return rc;
    if (!b->state) return fail(F110_E_INVALID, "%s: null state", who);
    if ((uintptr_t)b->state % 8) return fail(F110_E_INVALID, "%s: state is not 8-byte aligned", who);
    h->priority.bufs = *b;
    h->priority.bound = true;
    h->epoch++;
    return F110_OK;
}

// `who` may run: priorities are installed and bound behind a ring that is
static int priority_ready(const f110_handle *h, const char *who, ReplayRing &g, PriorityTree &t)
{
    const f110_handle::Priority &p = h->priority;
    if (!p.on) return fail(F110_E_INVALID, "%s: no priorities are installed (f110_priority_install)", who);
    if (!p.bound) return fail(F110_E_UNBOUND, "%s: f110_priority_bind has not been called", who);
    if (int rc = replay_ready(h, who, g)) return rc;
    t = priority_tree(p.bufs.leaf, p.bufs.node, g.steps * (long long)g.n_envs, h->d_err.get());
    return F110_OK;
}

static int priority_push(const f110_handle *h, const ReplayRing &g, hipStream_t stream)
{
    PriorityPushArgs a;
    memset(&a, 0, sizeof(a));
    a.tree = priority_tree(h->priority.bufs.leaf, h->priority.bufs.node, g.steps * (long long)g.n_envs, g.dev_err);
    a.valid = g.valid; a.count = g.count; a.steps = g.steps; a.n_envs = g.n_envs; a.qmax = &h->priority.bufs.state->qmax;
    const int waves = g.n_envs / PT_FANOUT + 2, per = PT_THREADS / 64;      // level-1 nodes a row of n_envs leaves can touch
    hipLaunchKernelGGL(priority_push_kernel, dim3((unsigned)((waves + per - 1) / per)), dim3(PT_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    if (a.tree.lay.levels >= 2) {
        hipLaunchKernelGGL(priority_upper_kernel, dim3(1), dim3(PT_THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return F110_OK;
}

extern "C" int f110_priority_reset(f110_handle *h, void *stream)
{
    const char *who = "f110_priority_reset";
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    ReplayRing g;
    PriorityTree t;
    if (int rc = priority_ready(h, who, g, t)) return rc;
    hipLaunchKernelGGL(priority_fill_kernel, dim3((unsigned)((t.lay.leaves + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, (hipStream_t)stream, t,
                       (const uint8_t *)g.valid, (const uint32_t *)&h->priority.bufs.state->qmax);
    HIP_TRY(hipGetLastError());
    return priority_rebuild(t, (hipStream_t)stream);
}

extern "C" int f110_priority_sample(f110_handle *h, uint64_t seed, uint64_t *counter, int32_t n, int32_t nstep, double gamma, int64_t *indices,
                                    int64_t *s_frame, int64_t *ns_frame, float *a_out, double *ret, uint8_t *d_out, uint8_t *ok, double *discount,
                                    int32_t *span, uint32_t *prio, float *weight, void *stream)
{
    const char *who = "f110_priority_sample";
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    PrioritySampleArgs p;
    memset(&p, 0, sizeof(p));
    if (int rc = priority_ready(h, who, p.s.ring, p.tree)) return rc;
    if (!prio || !weight) return fail(F110_E_INVALID, "%s: null argument", who);
    if (int rc = replay_sample_nstep_args(who, p.s, seed, counter, n, nstep, gamma, indices, s_frame, ns_frame, a_out, ret, d_out, ok, discount, span)) return rc;
    if (n == 0) return F110_OK;
    p.prio = prio;
    const int per = PT_THREADS / 64;
    hipLaunchKernelGGL(priority_sample_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(PT_THREADS), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    PriorityWeightArgs w;
    w.prio = prio; w.ok = ok; w.weight = weight; w.n = n; w.counter = (unsigned long long *)counter; w.state = h->priority.bufs.state;
    hipLaunchKernelGGL(priority_weight_kernel, dim3(1), dim3(PT_THREADS), 0, (hipStream_t)stream, w);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// f110_priority_update (td) and f110_priority_set (q): the set's rule on the rows with ok whose transition is valid
static int priority_write(f110_handle *h, const char *who, const int64_t *idx, const uint8_t *ok, const float *td, const uint32_t *q, int32_t n,
                          uint32_t *q_out, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    PrioritySetArgs a;
    memset(&a, 0, sizeof(a));
    ReplayRing g;
    if (int rc = priority_ready(h, who, g, a.tree)) return rc;
    if (n < 0) return fail(F110_E_INVALID, "%s: n=%d", who, n);
    if (!idx) return fail(F110_E_INVALID, "%s: null idx", who);
    if (td ? !ok : !q) return fail(F110_E_INVALID, "%s: null %s", who, td ? "ok" : "q");
    if (n == 0) return F110_OK;
    a.idx = (const long long *)idx; a.ok = ok; a.q_in = q; a.td = td; a.valid = g.valid; a.n = n;
    a.exponent = h->priority.cfg.exponent; a.eps = h->priority.cfg.eps; a.q_out = q_out; a.qmax = &h->priority.bufs.state->qmax;
    return priority_apply(a, (hipStream_t)stream);
}

extern "C" int f110_priority_update(f110_handle *h, const int64_t *idx, const uint8_t *ok, const float *td, int32_t n, uint32_t *q_out, void *stream)
{
    if (h && !td) return fail(F110_E_INVALID, "f110_priority_update: null td");   // (without it the call would read as the set's)
    return priority_write(h, "f110_priority_update", idx, ok, td, nullptr, n, q_out, stream);
}

extern "C" int f110_priority_set(f110_handle *h, const int64_t *idx, const uint32_t *q, int32_t n, void *stream)
{
    return priority_write(h, "f110_priority_set", idx, nullptr, nullptr, q, n, nullptr, stream);
}

// ---------------------------------------------------------------- episodes
// What install refuses, on the struct alone (no handle, no device).
extern "C" int f110_episodes_validate(const f110_episodes_config *cfg)
{
    const char *who = "f110_episodes_validate";
    if (!cfg) return fail(F110_E_INVALID, "%s: null config", who);
    if (cfg->limit < 0) return fail(F110_E_INVALID, "%s: step limit %d is negative (0: no limit)", who, cfg->limit);
    if (cfg->log < 1 || cfg->log > (1 << 24)) return fail(F110_E_INVALID, "%s: a log of %d records (1..%d)", who, cfg->log, 1 << 24);
    return F110_OK;
}

extern "C" int f110_episodes_install(f110_handle *h, const f110_episodes_config *cfg)
{
    if (!h) return fail(F110_E_INVALID, "f110_episodes_install: null handle");
    f110_handle::Episodes &e = h->episodes;
    if (!cfg) { // removes the tracker (the arrays are the caller's)
        if (!e.on) return F110_OK;
        e.on = false;
        h->epoch++;
        return F110_OK;
    }
    if (int rc = f110_episodes_validate(cfg)) return rc;
    if (int rc = clock_usable(h, "f110_episodes_install")) return rc;
    if (e.on && e.cfg.log != cfg->log) e.bound = false; // the log's arrays have another length: bind again
    e.cfg = *cfg; // by value in every launch
    e.on = true;
    h->epoch++;
    return F110_OK;
}

static bool episodes_buffers_complete(const f110_episodes_buffers *b)
{
    return b->ep_return && b->ep_length && b->ep_open && b->t_seen && b->truncated && b->log_env && b->log_length && b->log_return &&
           b->log_reason && b->log_time && b->log_laps && b->count && b->block_counts;
}

extern "C" int f110_episodes_bind(f110_handle *h, const f110_episodes_buffers *b)
{
    if (!h || !b) return fail(F110_E_INVALID, "f110_episodes_bind: null argument");
    if (!episodes_buffers_complete(b)) return fail(F110_E_INVALID, "f110_episodes_bind: an array is NULL (all but `limit` are required)");
    if ((uintptr_t)b->count % 8) return fail(F110_E_INVALID, "f110_episodes_bind: count is not 8-byte aligned");
    h->episodes.bufs = *b;
    h->episodes.bound = true;
    h->epoch++;
    return F110_OK;
}

static int launch_episodes(EpisodesArgs &a, const f110_episodes_config &c, const f110_episodes_buffers &b, hipStream_t stream)
{
    if (a.n == 0) return F110_OK;
    a.log = c.log; a.limit_all = c.limit;
    a.ep_return = b.ep_return; a.ep_length = b.ep_length; a.ep_open = b.ep_open; a.t_seen = b.t_seen; a.truncated = b.truncated;
    a.limit = b.limit; a.log_env = b.log_env; a.log_length = b.log_length; a.log_return = b.log_return; a.log_reason = b.log_reason;
    a.log_time = b.log_time; a.log_laps = b.log_laps; a.count = (const long long *)b.count; a.block_counts = b.block_counts;
    const int blocks = (a.n + EPISODES_THREADS - 1) / EPISODES_THREADS;
    hipLaunchKernelGGL(episodes_count_kernel, dim3(blocks), dim3(EPISODES_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(episodes_update_kernel, dim3(blocks), dim3(EPISODES_THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(episodes_advance_kernel, dim3(1), dim3(64), 0, stream, (long long *)b.count, (const int32_t *)b.block_counts, blocks);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_episodes_update(f110_handle *h, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_episodes_update: null handle");
    const f110_handle::Episodes &e = h->episodes;
    if (int rc = update_ready(h, "f110_episodes_update", "episode tracker", "episodes", e.on, e.bound)) return rc;
    EpisodesArgs a;
    memset(&a, 0, sizeof(a));
    a.n = h->cfg.num_envs; a.timestep = h->cfg.timestep;
    a.reward = h->shaping.on && h->shaping.bound ? h->shaping.bufs.total : nullptr; // follows the shaper being switched on and off
    a.done = (const uint8_t *)h->bufs.done; a.current_time = h->bufs.current_time;
    a.laps = h->bufs.lap_counts + h->cfg.ego_idx; a.laps_stride = h->cfg.num_agents;
    a.pending_reset = h->cfg.autoreset ? h->bufs.pending_reset : nullptr;
    a.dev_err = h->d_err.get();
    return launch_episodes(a, e.cfg, e.bufs, (hipStream_t)stream);
}

extern "C" int f110_episodes_apply(const f110_episodes_config *cfg, int32_t n, double timestep, const double *reward, const uint8_t *done,
                                   const double *current_time, const int32_t *laps, int64_t laps_stride, uint8_t *pending_reset,
                                   const f110_episodes_buffers *bufs, void *stream)
{
    if (!cfg) return fail(F110_E_INVALID, "f110_episodes_apply: null config");
    if (int rc = f110_episodes_validate(cfg)) return rc;
    if (!bufs || !done || !current_time || !episodes_buffers_complete(bufs)) return fail(F110_E_INVALID, "f110_episodes_apply: null pointer");
    if (n < 0 || !(timestep > 0.0) || laps_stride < 0) return fail(F110_E_INVALID, "f110_episodes_apply: bad arguments (n=%d, timestep=%g)", n, timestep);
    if ((uintptr_t)bufs->count % 8) return fail(F110_E_INVALID, "f110_episodes_apply: count is not 8-byte aligned");
    EpisodesArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.timestep = timestep; a.reward = reward; a.done = done; a.current_time = current_time;
    a.laps = laps; a.laps_stride = laps_stride; a.pending_reset = pending_reset;
    return launch_episodes(a, *cfg, *bufs, (hipStream_t)stream);
}

static int replay_pack_args(const char *who, const void *in, const void *out, int64_t n, int32_t rows, int32_t cols)
{
    if (n < 0 || n > 0x7fffffff || rows < 1 || cols < 1 || rows > REPLAY_MAX_DIM || cols > REPLAY_MAX_DIM)
        return fail(F110_E_INVALID, "%s: n=%lld images of %d x %d pixels (1..%d)", who, (long long)n, rows, cols, REPLAY_MAX_DIM);
    if (n > 0 && (!in || !out)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if ((uintptr_t)in % 16 || (uintptr_t)out % 16) return fail(F110_E_INVALID, "%s: both arrays must be 16-byte aligned", who);
    return F110_OK;
}

extern "C" int f110_replay_pack(const uint8_t *bitmaps, int64_t n, int32_t rows, int32_t cols, uint64_t *packed, void *stream)
{
    if (int rc = replay_pack_args("f110_replay_pack", bitmaps, packed, n, rows, cols)) return rc;
    if (n == 0) return F110_OK;
    ReplayPackArgs a;
    a.bitmaps = bitmaps; a.packed = packed; a.rows = rows; a.cols = cols;
    hipLaunchKernelGGL(replay_pack_kernel, dim3((unsigned)n), dim3(REPLAY_THREADS), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_replay_unpack(const uint64_t *packed, int64_t n, int32_t rows, int32_t cols, uint8_t *bitmaps, void *stream)
{
    if (int rc = replay_pack_args("f110_replay_unpack", packed, bitmaps, n, rows, cols)) return rc;
    if (n == 0) return F110_OK;
    ReplayPackArgs a;
    a.bitmaps = nullptr; a.packed = const_cast<uint64_t *>(packed); a.rows = rows; a.cols = cols;
    hipLaunchKernelGGL(replay_unpack_kernel, dim3((unsigned)n, (unsigned)((rows + REPLAY_ROWS - 1) / REPLAY_ROWS)), dim3(REPLAY_THREADS), 0,
                       (hipStream_t)stream, a, bitmaps);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
