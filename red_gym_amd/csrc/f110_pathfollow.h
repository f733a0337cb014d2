// f110_pathfollow.h -- the action side of the reference's RL consumer, SACF110Env.step (src/SAL.py): the policy's 16 numbers
// become a path of 8 points (compute_vectors_with_angle_clamp :585-608, _calculate_global_path :157-181), the path becomes
// an acceleration (MPC_controller :615-739: two not-a-knot cubic splines over the chord length, the reference states, the
// first of its QPs) and the acceleration a (steer, speed) pair (MPC_converter :741-764); behind the step the waypoint index
// follows the new pose (_update_path_index :252-259).
// Two lanes per env, one per axis: the spline of a coordinate, its share of the reference states and its QP belong to one
// lane; the chord lengths, the reference speed and the converter need the partner lane's value (one cross-lane exchange each,
// always outside divergent control flow).  The QP of an axis, min 1/2 u'Hu + f'u over -1 <= u <= 1 with H = the options'
// Hessian (strictly convex: the weights on the inputs are positive), is solved by a primal active-set walk over tables the
// HOST inverted: for every set of free variables the inverse of H restricted to it (pathfollow_tables).  The walk starts
// at the clipped unconstrained optimum and has a hard step limit (PF_QP_LIMIT); a walk that reaches it keeps its last
// feasible point and raises DEVERR_QP_LIMIT in the device error word.  Numerically degenerate cases: a free variable within
// PF_TOL_U outside a bound is clamped onto it and counts as feasible; a multiplier within PF_TOL_G * max(1, |f|_inf) of zero
// counts as having the right sign (the variable stays bound) -- both change u by far less than the 1e-9 the tests allow.
// fp64; sin / cos / atan2 / fmod are the device library's: the tests allow 1e-9 * max(1, |value|).
// Non-finite inputs (a diverged policy's NaN action, a NaN or infinite velocity) stay in their env: the points from the first
// non-finite row on, or the env's acceleration and action, come out non-finite; no index is formed from such a value (the spline
// piece is a count of comparisons, the free set a bit mask), the walk ends at PF_QP_LIMIT at the latest and may raise
// DEVERR_QP_LIMIT, and no other env changes by a bit -- the lane exchanges never leave the env's own pair of lanes.
#pragma once
#include "../../include/f110_hip.h" // f110_pathfollow_config
#include "f110_bounds.h"
#include "f110_device.h"

#pragma clang fp contract(off)

namespace f110 {

constexpr uint32_t DEVERR_QP_LIMIT = 4u;
constexpr int PF_POINTS = 8;                  // points of a path = rows of the raw action
constexpr int PF_MAX_H = 8;                   // longest horizon (variables of one QP)
constexpr int PF_QP_LIMIT = 64;               // steps of the active-set walk
constexpr double PF_TOL_U = 1e-12, PF_TOL_G = 1e-12;

// Table the kernels read (host-built, f110_consumers.hip): per axis the Hessian [H, H], then per axis and per set of free
// variables (bit i of the set's number: u_i is free) the inverse of the Hessian restricted to the set, [H, H] with zero rows
// and columns for the variables that are not free.
__host__ __device__ inline size_t pathfollow_table_doubles(int H) { return (size_t)2 * H * H * (1 + ((size_t)1 << H)); }

struct PathFollowArgs {
    f110_pathfollow_config cfg;
    int n;
    const double *raw;           // [n,16] raw actions, or NULL: no path is decoded
    const double *pose;          // env e: x, y, theta = pose[e * pose_stride + (0, 1, th_off)]
    long long pose_stride;
    int th_off;
    const double *vel;           // env e: vx = vel[e * vel_stride], vy = vel[e * vel_stride + 1] if has_vy else 0; NULL: decode only
    long long vel_stride;
    int has_vy;
    double *path;                // [n,8,2] read, or written where a path is decoded
    int32_t *index;              // [n] waypoint index (< 0: no path), or NULL: no episode logic (decode wherever raw is given)
    uint8_t *replanned;          // [n] or NULL
    const double *qp;            // pathfollow_table_doubles(horizon)
    double *accel;               // [n,2]
    double *actions;             // (steer, speed) of env e at actions[e * act_stride]
    long long act_stride;
    double *dists, *ref_traj;    // [n,8], [n, horizon + 1, 4] or NULL
    int32_t *qp_steps;           // [n,2] steps of the two walks, or NULL
    uint32_t *dev_err;
};

struct PathAdvanceArgs {
    f110_pathfollow_config cfg;
    int n;
    const double *xy;            // position of env e: xy[e * xy_stride + (0, 1)]
    long long xy_stride;
    const double *path;          // [n,8,2]
    const int32_t *index_in;     // [n]
    int32_t *index_out;          // [n]
    const double *current_time;  // [n] the envs' clocks, or NULL: no episode logic
    double timestep;
    double *t_seen;              // [n] or NULL
    uint32_t *dev_err;
};

// Python's float %: the result has the divisor's sign (m > 0)
__device__ inline double pf_floor_mod(double a, double m)
{
    double r = fmod(a, m);
    if (r < 0.0) r += m;
    return r;
}

static __global__ __launch_bounds__(256) void pathfollow_act_kernel(PathFollowArgs a)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int env = gid >> 1, ax = gid & 1;      // the two lanes of an env are neighbours in one wave
    if (env >= a.n) return;
    const f110_pathfollow_config &c = a.cfg;
    const int H = c.horizon;
    double *__restrict__ path = a.path + (size_t)env * 2 * PF_POINTS;
    double y[PF_POINTS];                          // this lane's coordinate of the 8 points
    // ---- 1. the path: decoded from the raw action at the car's pose, or the one kept
    bool need = a.raw != nullptr;
    if (a.index) {
        const int idx = a.index[env];
        need = need && (idx < 0 || idx >= c.replan_at);
    }
    if (need) {
        const double *__restrict__ raw = a.raw + (size_t)env * 2 * PF_POINTS;
        const double px = a.pose[(size_t)env * (size_t)a.pose_stride + ax], th = a.pose[(size_t)env * (size_t)a.pose_stride + a.th_off];
        const double ct = cos(th), st = sin(th);
        const double max_diff = c.max_diff_deg * (F110_PI / 180.0);
        double prev = 0.0, last = px + c.car_length * (ax ? st : ct);
#pragma unroll
        for (int i = 0; i < PF_POINTS; i++) {
            double ix = 1.0, iy = 0.0;           // row 0 of the action is ignored: the first increment points ahead
            if (i > 0) {
                const double vx = raw[2 * i], vy = raw[2 * i + 1];
                const double nrm = sqrt(vx * vx + vy * vy) + 1e-8;
                const double desired = atan2(vy / nrm, vx / nrm);
                double diff = pf_floor_mod(desired - prev + F110_PI, 2.0 * F110_PI) - F110_PI;
                diff = diff < -max_diff ? -max_diff : (diff > max_diff ? max_diff : diff);
                prev = prev + diff;
                ix = cos(prev); iy = sin(prev);
            }
            const double dxs = ix * c.vector_length, dys = iy * c.vector_length;
            last = last + (ax ? dxs * st + dys * ct : dxs * ct - dys * st);
            y[i] = last;
            path[2 * i + ax] = last;
        }
        if (a.index && ax == 0) a.index[env] = 0;
    } else {
#pragma unroll
        for (int i = 0; i < PF_POINTS; i++) y[i] = path[2 * i + ax];
    }
    if (a.replanned && ax == 0) a.replanned[env] = need ? 1 : 0;
    if (!a.vel) return;
    // ---- 2. chord lengths and the not-a-knot spline of this lane's coordinate (scipy.interpolate.CubicSpline's system, solved
    // without pivoting: the chords all have the length vector_length, for which the elimination's pivots stay away from 0)
    double x[PF_POINTS], dx[PF_POINTS - 1], slope[PF_POINTS - 1];
    x[0] = 0.0;
#pragma unroll
    for (int i = 0; i < PF_POINTS - 1; i++) {
        const double mine = y[i + 1] - y[i], other = __shfl_xor(mine, 1);
        const double ex = ax ? other : mine, ey = ax ? mine : other;
        dx[i] = sqrt(ex * ex + ey * ey);
        x[i + 1] = x[i] + dx[i];
        slope[i] = mine / dx[i];
    }
    if (a.dists && ax == 0) {
#pragma unroll
        for (int i = 0; i < PF_POINTS; i++) a.dists[(size_t)env * PF_POINTS + i] = x[i];
    }
    double s[PF_POINTS];                          // the spline's first derivative at the knots
    {
        constexpr int N = PF_POINTS;
        double diag[N], up[N], b[N];
        const double d0 = x[2] - x[0], d1 = x[N - 1] - x[N - 3];
        diag[0] = dx[1]; up[0] = d0;
        b[0] = ((dx[0] + 2.0 * d0) * dx[1] * slope[0] + dx[0] * dx[0] * slope[1]) / d0;
#pragma unroll
        for (int i = 1; i < N - 1; i++) {
            const double lo = dx[i];
            diag[i] = 2.0 * (dx[i - 1] + dx[i]); up[i] = dx[i - 1];
            b[i] = 3.0 * (dx[i] * slope[i - 1] + dx[i - 1] * slope[i]);
            const double m = lo / diag[i - 1];
            diag[i] = diag[i] - m * up[i - 1];
            b[i] = b[i] - m * b[i - 1];
        }
        {
            diag[N - 1] = dx[N - 3];
            b[N - 1] = (dx[N - 2] * dx[N - 2] * slope[N - 3] + (2.0 * d1 + dx[N - 2]) * dx[N - 3] * slope[N - 2]) / d1;
            const double m = d1 / diag[N - 2];
            diag[N - 1] = diag[N - 1] - m * up[N - 2];
            b[N - 1] = b[N - 1] - m * b[N - 2];
        }
        s[N - 1] = b[N - 1] / diag[N - 1];
#pragma unroll
        for (int i = N - 2; i >= 0; i--) s[i] = (b[i] - up[i] * s[i + 1]) / diag[i];
    }
    // ---- 3. the reference states and this axis' linear term f: with p_k = p0 + k dt v0 + sum_j A[k][j] u_j, A[k][j] =
    // dt^2 (k - j - 1/2), and v_k = v0 + dt sum_{j<k} u_j, the cost is 1/2 u'Hu + f'u + const (halved), f_j = sum_k
    // wp_k A[k][j] (p0 + k dt v0 - rp_k) + wv_k dt (v0 - rv_k) over k = j+1 .. H; wp, wv = Q's for k < H and P's for k = H.
    const double dt = c.timestep, p0 = y[0];
    const double v0 = ax == 0 ? a.vel[(size_t)env * (size_t)a.vel_stride] : (a.has_vy ? a.vel[(size_t)env * (size_t)a.vel_stride + 1] : 0.0);
    double f[PF_MAX_H];
#pragma unroll
    for (int j = 0; j < PF_MAX_H; j++) f[j] = 0.0;
#pragma unroll
    for (int k = 0; k <= PF_MAX_H; k++) {
        if (k <= H) {                             // (uniform: the horizon is an option)
            double sk = c.desired_velocity * ((double)k * dt);
            if (sk > x[PF_POINTS - 1]) sk = x[PF_POINTS - 1];
            // piece j = the knots x[1..6] at or below sk; its data by selects, so that the arrays stay in registers
            int piece = 0;
#pragma unroll
            for (int i = 1; i < PF_POINTS - 1; i++) piece += x[i] <= sk ? 1 : 0;
            F110_BCHK(piece >= 0 && piece < PF_POINTS - 1, BT_PATHFOLLOW, a.dev_err);
            double xj = x[0], yj = y[0], sj = s[0], sj1 = s[1], dxj = dx[0], slj = slope[0];
#pragma unroll
            for (int i = 1; i < PF_POINTS - 1; i++)
                if (piece == i) { xj = x[i]; yj = y[i]; sj = s[i]; sj1 = s[i + 1]; dxj = dx[i]; slj = slope[i]; }
            const double t = (sj + sj1 - 2.0 * slj) / dxj;
            const double c0 = t / dxj, c1 = (slj - sj) / dxj - t;
            const double z = sk - xj;
            const double rp = ((c0 * z + c1) * z + sj) * z + yj;
            const double dp = (3.0 * c0 * z + 2.0 * c1) * z + sj;
            const double dq = __shfl_xor(dp, 1);
            const double speed = sqrt(dp * dp + dq * dq);
            const double rv = speed > 1e-3 ? c.desired_velocity * dp / speed : 0.0;
            if (a.ref_traj) {
                double *r = a.ref_traj + ((size_t)env * (size_t)(H + 1) + (size_t)k) * 4;
                r[ax] = rp; r[2 + ax] = rv;
            }
            if (k >= 1) {
                const double wp = k < H ? c.q[ax] : c.p[ax], wv = k < H ? c.q[2 + ax] : c.p[2 + ax];
                const double ep = wp * (p0 + (double)k * dt * v0 - rp), ev = wv * dt * (v0 - rv);
#pragma unroll
                for (int j = 0; j < PF_MAX_H; j++)
                    if (j < k) f[j] = f[j] + (dt * dt * ((double)(k - j) - 0.5) * ep + ev);
            }
        }
    }
    // ---- 4. the QP of this axis: primal active-set walk over the host's tables
    const int HH = H * H;
    const double *__restrict__ Hm = a.qp + (size_t)ax * HH;
    const double *__restrict__ Zs = a.qp + (size_t)2 * HH + (size_t)ax * ((size_t)HH << H);
    const unsigned all = (1u << H) - 1u;
    double fmax = 1.0;
#pragma unroll
    for (int j = 0; j < PF_MAX_H; j++) fmax = fabs(f[j]) > fmax ? fabs(f[j]) : fmax;
    const double tolg = PF_TOL_G * fmax;
    double u[PF_MAX_H];
    unsigned hi = 0, lo = 0;                      // bit i: u_i is held at +1 / at -1
    {
        const double *__restrict__ Z = Zs + (size_t)all * HH;
#pragma unroll
        for (int i = 0; i < PF_MAX_H; i++) {
            double t = 0.0;
            if (i < H) {
#pragma unroll
                for (int j = 0; j < PF_MAX_H; j++)
                    if (j < H) t = t - Z[i * H + j] * f[j];
            }
            if (t >= 1.0) { t = 1.0; hi |= 1u << i; }
            if (t <= -1.0) { t = -1.0; lo |= 1u << i; }
            u[i] = t;
        }
    }
    int steps = 0;
    bool done = false;
    for (; steps < PF_QP_LIMIT && !done; steps++) {
        const unsigned bound = hi | lo, fm = all & ~bound;
        F110_BCHK(fm <= all && (hi & lo) == 0, BT_PATHFOLLOW, a.dev_err);
        const double *__restrict__ Z = Zs + (size_t)fm * HH;
        // the optimum on the face: t_F = -inv(H_FF) (f_F + H_FB u_B)
        double r[PF_MAX_H], t[PF_MAX_H];
#pragma unroll
        for (int i = 0; i < PF_MAX_H; i++) {
            r[i] = f[i];
            if (i < H) {
#pragma unroll
                for (int j = 0; j < PF_MAX_H; j++)
                    if (j < H) r[i] = r[i] + Hm[i * H + j] * ((bound >> j) & 1u ? u[j] : 0.0);
            }
        }
        double alpha = 1.0;
        int blk = -1;
#pragma unroll
        for (int i = 0; i < PF_MAX_H; i++) {
            t[i] = u[i];
            if (i < H && ((fm >> i) & 1u)) {
                double v = 0.0;
#pragma unroll
                for (int j = 0; j < PF_MAX_H; j++)
                    if (j < H) v = v - Z[i * H + j] * r[j];
                t[i] = v;
                if (v > 1.0 + PF_TOL_U) { const double al = (1.0 - u[i]) / (v - u[i]); if (al < alpha) { alpha = al; blk = i; } }
                if (v < -1.0 - PF_TOL_U) { const double al = (-1.0 - u[i]) / (v - u[i]); if (al < alpha) { alpha = al; blk = i; } }
            }
        }
        if (blk >= 0) {
            // the face's optimum lies outside the box: go as far as the first bound on the way and hold it
#pragma unroll
            for (int i = 0; i < PF_MAX_H; i++) {
                const bool up_side = t[i] > u[i];
                u[i] = u[i] + alpha * (t[i] - u[i]);
                if (i == blk) { u[i] = up_side ? 1.0 : -1.0; if (up_side) hi |= 1u << i; else lo |= 1u << i; }
                u[i] = u[i] > 1.0 ? 1.0 : (u[i] < -1.0 ? -1.0 : u[i]);
            }
        } else {
            // it lies inside: take it, and release the held variable whose multiplier has the wrong sign most, if any
            double worst = tolg;
            int rel = -1;
#pragma unroll
            for (int i = 0; i < PF_MAX_H; i++) u[i] = t[i] > 1.0 ? 1.0 : (t[i] < -1.0 ? -1.0 : t[i]);
#pragma unroll
            for (int i = 0; i < PF_MAX_H; i++) {
                if (i < H && ((bound >> i) & 1u)) {
                    double g = f[i];
#pragma unroll
                    for (int j = 0; j < PF_MAX_H; j++)
                        if (j < H) g = g + Hm[i * H + j] * u[j];
                    const double viol = (hi >> i) & 1u ? g : -g;   // at +1 the gradient must be <= 0, at -1 >= 0
                    if (viol > worst) { worst = viol; rel = i; }
                }
            }
            if (rel < 0) done = true;
            else { hi &= ~(1u << rel); lo &= ~(1u << rel); }
        }
    }
    if (!done && a.dev_err) atomicOr(a.dev_err, DEVERR_QP_LIMIT);
    if (a.qp_steps) a.qp_steps[2 * (size_t)env + ax] = steps;
    // ---- 5. MPC_converter with current_steer = 0 (the observation has no 'steering' key)
    const double mine = u[0], other = __shfl_xor(mine, 1);
    a.accel[2 * (size_t)env + ax] = mine;
    if (ax == 0) {
        const double acx = mine, acy = other;
        double steer = pf_floor_mod(atan2(acy, acx) - 0.0 + F110_PI, 2.0 * F110_PI) - F110_PI;
        steer = steer < -c.max_steer ? -c.max_steer : (steer > c.max_steer ? c.max_steer : steer);
        double throttle = acx * 1.0 + acy * 0.0;
        throttle = throttle < -1.0 ? -1.0 : (throttle > 1.0 ? 1.0 : throttle);
        double *o = a.actions + (size_t)env * (size_t)a.act_stride;
        o[0] = steer; o[1] = throttle;
    }
}

// _update_path_index (:252-259) behind the step, one lane per env.  Episode logic as in the shaper: an env whose clock reads
// exactly `timestep` was reset by its last step and loses its path (SAL's reset(), :84-85); an env whose clock stands still
// since the previous update (a masked reset left it alone) is not touched.
static __global__ __launch_bounds__(256) void pathfollow_advance_kernel(PathAdvanceArgs a)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.n) return;
    int idx = a.index_in[env];
    if (a.current_time) {
        const double now = a.current_time[env];
        if (now == a.timestep) { a.index_out[env] = -1; a.t_seen[env] = now; return; }
        if (now == a.t_seen[env]) return;
        a.t_seen[env] = now;
    }
    if (idx >= 0 && idx < PF_POINTS) {
        F110_BCHK(idx >= 0 && idx < PF_POINTS, BT_PATHFOLLOW, a.dev_err);
        const double *__restrict__ p = a.path + (size_t)env * 2 * PF_POINTS + 2 * (size_t)idx;
        const double dx = a.xy[(size_t)env * (size_t)a.xy_stride] - p[0], dy = a.xy[(size_t)env * (size_t)a.xy_stride + 1] - p[1];
        if (sqrt(dx * dx + dy * dy) < a.cfg.dist_threshold) idx++;
    }
    a.index_out[env] = idx;
}

} // namespace f110
