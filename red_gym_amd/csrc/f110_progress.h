// f110_progress.h -- progress along the raceline (Frenet pose and metres driven), one lane per car.  The nearest point is the
// reference's nearest_point_on_trajectory (examples/waypoint_follow.py:16-47) -- the search pure_pursuit_grid_kernel does
// (f110_planner.h: the same per-segment function, the same grid of candidate lists) -- and the rest is a look-up in tables
// the HOST computed with NumPy (red_gym_amd/progress.py): the device evaluates neither the sqrt of a segment nor an atan2.
// fp64, plain mul/add in the order DESIGN.md section 3 fixes; the tests demand `==` of a NumPy checker for every output.
#pragma once
#include "f110_bounds.h"
#include "f110_device.h"
#include "f110_planner.h"

#pragma clang fp contract(off)

namespace f110 {

struct ProgressArgs {
    const double *state;            // [n,7]: x, y, yaw = columns 0, 1, 4
    int n, agents;
    const double *xy;               // [total,2] the K racelines back to back
    const double *len, *cum, *psi;  // [total] per raceline k at offsets[k]: len / psi of segment i, cum of point i
    const double *lap;              // [K] lap length
    const int32_t *offsets;         // [K+1] first point of raceline k (offsets[K] = total)
    const int32_t *raceline_of_env; // [B] or NULL (all on raceline 0)
    int K;
    int use_grid;                   // K == 1: candidates from `g`; else every segment of the car's raceline
    PlanGrid g;
    const double *current_time;     // [B] f110_buffers.current_time: == timestep exactly when the env's last step was a reset
    double timestep;
    double *s, *d, *heading_error, *delta, *progress, *s_prev; // [n]
    int32_t *seg;                   // [n]
    uint8_t *seen;                  // [n]
    uint32_t *dev_err;
};

static __global__ __launch_bounds__(256) void progress_kernel(ProgressArgs a)
{
    const int car = blockIdx.x * blockDim.x + threadIdx.x;
    if (car >= a.n) return;
    const int env = car / a.agents;
    int k = a.raceline_of_env ? a.raceline_of_env[env] : 0;
    F110_BCHK((unsigned)k < (unsigned)a.K, BT_PROGRESS, a.dev_err);
    if ((unsigned)k >= (unsigned)a.K) k = 0;
    const int off = a.offsets[k], nseg = a.offsets[k + 1] - off - 1;
    const double *__restrict__ xy = a.xy + (size_t)off * 2;
    const double px = a.state[(size_t)car * 7], py = a.state[(size_t)car * 7 + 1], yaw = a.state[(size_t)car * 7 + 4];
    // An env's clock restarts at 0 in the step that resets it and every step adds the time step (env_kernel): it reads
    // exactly `timestep` if and only if the last step that touched the env was its reset -- f110_reset (masked or not) and
    // autoreset alike, and an env a masked reset left alone keeps the answer of its own last step.
    const bool restart = a.current_time[env] == a.timestep || a.seen[car] == 0;
    const double nan = __builtin_nan("");
    double s = nan, d = nan, e = nan, delta = nan;
    int seg = 0;
    if (__builtin_isfinite(px) && __builtin_isfinite(py)) {
        // 1. nearest_point_on_trajectory (:16-47): strict `<` in ascending index order = np.argmin's first minimum
        double best = __builtin_inf(), best_t = 0;
        int best_i = 0;
        auto consider = [&](int i) {
            double t;
            const double dist = seg_nearest(px, py, xy[2 * i], xy[2 * i + 1], xy[2 * i + 2], xy[2 * i + 3], t);
            if (dist < best) { best = dist; best_i = i; best_t = t; }
        };
        unsigned cnt = PG_ALL;
        size_t cell = 0;
        if (a.use_grid) {
            const double fx = floor((px - a.g.x0) * a.g.inv_cell), fy = floor((py - a.g.y0) * a.g.inv_cell);
            if (fx >= 0.0 && fx < (double)a.g.gw && fy >= 0.0 && fy < (double)a.g.gh) {
                cell = (size_t)(int)fy * (size_t)a.g.gw + (size_t)(int)fx;
                F110_BCHK(cell < (size_t)a.g.gw * (size_t)a.g.gh, BT_PROGRESS, a.dev_err);
                cnt = a.g.count[cell];
            }
        }
        if (cnt == PG_ALL) for (int i = 0; i < nseg; i++) consider(i);
        else {
            const uint16_t *lst = a.g.cand + cell * PG_CAP;
            for (unsigned j = 0; j < cnt; j++) {
                int i = (int)lst[j];
                F110_BCHK(i < nseg, BT_PROGRESS, a.dev_err);
                F110_BOUNDS_ONLY(if (i >= nseg) i = 0;)
                consider(i);
            }
        }
        seg = best_i;
        F110_BCHK(seg >= 0 && seg < nseg, BT_PROGRESS, a.dev_err);
        const size_t r = (size_t)off + (size_t)seg;
        // 2. arc length of the projection
        s = a.cum[r] + best_t * a.len[r];
        // 3. signed lateral offset: left of the line is positive
        const double x0 = xy[2 * seg], y0 = xy[2 * seg + 1];
        const double dx = xy[2 * seg + 2] - x0, dy = xy[2 * seg + 3] - y0;
        const double cross = dx * (py - y0) - dy * (px - x0);
        d = cross >= 0 ? best : -best;
        // 4. heading relative to the segment, one wrap each way (the step keeps yaw in [0, 2 pi])
        e = yaw - a.psi[r];
        if (e > F110_PI) e -= 2 * F110_PI;
        if (e <= -F110_PI) e += 2 * F110_PI;
        // 5. metres driven since the reset: the shorter way round the lap
        double progress = 0.0;
        delta = 0.0;
        if (!restart) {
            const double L = a.lap[k];
            delta = s - a.s_prev[car];
            if (delta >= L / 2) delta -= L;
            if (delta < -L / 2) delta += L;
            progress = a.progress[car] + delta;
        }
        a.progress[car] = progress;
        a.s_prev[car] = s;
        a.seen[car] = 1;
    } else if (restart) {
        // 6. a pose that cannot be placed: progress and s_prev stay; a restart it hides is taken at the next finite pose
        a.seen[car] = 0;
    }
    a.s[car] = s; a.d[car] = d; a.heading_error[car] = e; a.delta[car] = delta; a.seg[car] = seg;
}

} // namespace f110
