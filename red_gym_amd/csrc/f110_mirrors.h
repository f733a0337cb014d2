// f110_mirrors.h -- the function-level kernels of the parity entry points (f110_step.hip): one reference function each.
#pragma once
#include "f110_bounds.h"
#include "f110_device.h"
#include "f110_scan_plan.h" // WAVE

#pragma clang fp contract(off)

namespace f110 {

// ------------------------------------------------------------------ function-level kernels
// dynamic_models.py:91-121 / :124-176 right-hand sides (the reference's KAT surface)
static __global__ void rhs_kernel(const double *x, const double *u, int n, int kinematic, const Params *params, double *f)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Params P = params[1]; // slot 0, agent 0
    double xs[7], fs[7];
    for (int k = 0; k < 7; k++) xs[k] = x[(size_t)i * 7 + k];
    if (kinematic) {
        const double *p = P.v;
        const double lwb = p[P_LF] + p[P_LR];
        const double u0 = steering_constraint(xs[2], u[2 * i], p[P_SMIN], p[P_SMAX], p[P_SVMIN], p[P_SVMAX]);
        const double u1 = accl_constraints(xs[3], u[2 * i + 1], p[P_VSWITCH], p[P_AMAX], p[P_VMIN], p[P_VMAX]);
        fs[0] = xs[3] * cos(xs[4]); fs[1] = xs[3] * sin(xs[4]); fs[2] = u0; fs[3] = u1; fs[4] = xs[3] / lwb * tan(xs[2]);
        fs[5] = 0; fs[6] = 0;
    } else {
        vehicle_dynamics_st(xs, u[2 * i], u[2 * i + 1], P, fs);
    }
    for (int k = 0; k < 7; k++) f[(size_t)i * 7 + k] = fs[k];
}

static __global__ void vertices_kernel(const double *poses, int n, double L, double W, double *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v[4][2];
    get_vertices(poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], L, W, v);
    for (int k = 0; k < 4; k++) { out[(size_t)i * 8 + 2 * k] = v[k][0]; out[(size_t)i * 8 + 2 * k + 1] = v[k][1]; }
}

static __global__ void gjk_pairs_kernel(const double *va, const double *vb, int n, uint8_t *hit)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[4][2], b[4][2];
    for (int k = 0; k < 4; k++) {
        a[k][0] = va[(size_t)i * 8 + 2 * k]; a[k][1] = va[(size_t)i * 8 + 2 * k + 1];
        b[k][0] = vb[(size_t)i * 8 + 2 * k]; b[k][1] = vb[(size_t)i * 8 + 2 * k + 1];
    }
    hit[i] = gjk_collision(a, b) ? 1 : 0;
}

static __global__ void collision_multiple_kernel(const double *verts, int n, int A, uint8_t *col, int32_t *cidx)
{
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const double *v = verts + (size_t)g * A * 8;
    uint8_t *c = col + (size_t)g * A;
    int32_t *x = cidx + (size_t)g * A;
    for (int i = 0; i < A; i++) { c[i] = 0; x[i] = -1; }
    for (int i = 0; i < A - 1; i++) {
        double vi[4][2];
        for (int k = 0; k < 4; k++) { vi[k][0] = v[i * 8 + 2 * k]; vi[k][1] = v[i * 8 + 2 * k + 1]; }
        for (int j = i + 1; j < A; j++) {
            double vj[4][2];
            for (int k = 0; k < 4; k++) { vj[k][0] = v[j * 8 + 2 * k]; vj[k][1] = v[j * 8 + 2 * k + 1]; }
            if (gjk_collision(vi, vj)) { c[i] = 1; c[j] = 1; x[i] = j; x[j] = i; }
        }
    }
}

// check_ttc_jit (laser_models.py:189-217): wave per scan
// slot_of_row (f110_check_ttc_slots): row r is tested against row slot_of_row[r] of side_distances [n_slots][nb]; NULL: the one table
static __global__ void ttc_kernel(const double *scans, const double *vel, int n, int nb, const double *beam_cosines,
                           const double *side_distances, double thresh, uint8_t *hit, const int32_t *slot_of_row, int n_slots,
                           uint32_t *dev_err)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    if (slot_of_row) {
        int sl = slot_of_row[row]; // (the caller's device array: a slot outside the table reads slot 0; reported in the bounds build)
        F110_BCHK((unsigned)sl < (unsigned)n_slots, BT_SIDE_SLOT, dev_err);
        if ((unsigned)sl >= (unsigned)n_slots) sl = 0;
        (void)dev_err;
        side_distances += (size_t)sl * nb;
    }
    const double v = vel[row];
    bool h = false;
    if (v != 0.0) {
        for (int i = lane; i < nb; i += WAVE) {
            const double proj_vel = v * beam_cosines[i];
            const double ttc = (scans[(size_t)row * nb + i] - side_distances[i]) / proj_vel;
            if ((ttc < thresh) && (ttc >= 0.0)) h = true;
        }
    }
    const bool any = __ballot(h) != 0ull;
    if (lane == 0) hit[row] = any ? 1 : 0;
}

// ray_cast (laser_models.py:319-346): wave per (ego, opponent quad)
static __global__ void ray_cast_kernel(const double *ego, const double *verts, int n, int nb, const double *scan_angles,
                                const double2 *beam_cs,
                                double *scans, int32_t *span)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    double v[4][2];
    for (int k = 0; k < 4; k++) { v[k][0] = verts[(size_t)row * 8 + 2 * k]; v[k][1] = verts[(size_t)row * 8 + 2 * k + 1]; }
    ray_cast_wave(ego[3 * row], ego[3 * row + 1], ego[3 * row + 2], v, scan_angles, beam_cs, nb, lane,
                  scans + (size_t)row * nb, nullptr, span ? span + 2 * row : nullptr);
}

} // namespace f110
