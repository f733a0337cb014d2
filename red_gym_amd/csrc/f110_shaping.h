// f110_shaping.h -- reward shaping from the previous step's FILL bitmap and the new pose: the three terms of the reference's RL
// consumer, SACF110Env._calculate_rewards (src/SAL.py:219-250) with detect_collison (:766-790), centerline_reward /
// distance_from_row_center (:879-935) and _world_to_pixel (:139-142), restated with their quirks (255 = the FILLED region counts
// as a collision; the centering row and column are raw metres truncated, not pixels).  One wave64 per env: the row of the
// centering term is loaded once, 64 pixels per load, a ballot of "pixel != 255" turns each 64-pixel chunk into a mask, and the
// ends of the run of 255 around the car come from count-leading / count-trailing zeros on those masks -- no pixel load
// depends on another.  The neighbours of the collision test are read by the first lanes and reduced by a ballot.
// The image is bytes, or the renderer's bits (f110_bitmap_render_bits: bit k of word w of a row = pixel 64 w + k is 255): then the
// mask of a 64-pixel chunk is the complemented word -- no byte loads, no ballot -- and a neighbour is one bit.
// fp64, plain mul/add in the order DESIGN.md section 3 fixes; the tests demand `==` of a NumPy checker for every output.
#pragma once
#include "../../include/f110_hip.h" // f110_shaping_config
#include "f110_bounds.h"
#include "f110_device.h"

#pragma clang fp contract(off)

namespace f110 {

constexpr int SHAPING_WAVES = 4; // envs (= waves) per workgroup

struct ShapingArgs {
    f110_shaping_config cfg;
    const uint8_t *bitmap;       // [n, rows, cols] the image of the PREVIOUS step's scan, or (exactly one of the two)
    const uint64_t *bitmap_bits; // [n, rows, ceil(cols / 64)] the same image as bits
    const double *xy;            // pose of env e: (xy[e * xy_stride], xy[e * xy_stride + 1]) -- state + 7 * agent with stride 7 * A, or [n,2]
    long long xy_stride;
    int n;
    const double *current_time;  // [n] the envs' clocks, or NULL: no episode logic (the function-level entry)
    double timestep;
    const double *prev_in;       // [n,2] position at the previous update (read)
    double *prev_out;            // [n,2] or NULL (the function-level entry keeps nothing)
    double *t_seen;              // [n] clock at the env's previous update (< 0: none yet), or NULL
    double *collision_term, *progress_term, *centering_term, *total; // [n]
    uint8_t *collided;           // [n]
    uint32_t *dev_err;
};

// _world_to_pixel (:139-142): clip(int(origin + v * scale), 0, clip_max) for every finite v.  Python's int is unbounded and
// truncates toward zero; clamping the double to [0, clip_max] first changes no result (everything below 0 clips to 0,
// everything above clip_max to clip_max, and truncation never leaves the interval) and keeps the conversion defined, a
// product that overflowed to +-inf included.  (origin, scale and v are finite: the sum is never NaN.)
__device__ inline int shaping_pixel(double origin, double v, double scale, int clip_max)
{
    double p = origin + v * scale;
    p = p < 0.0 ? 0.0 : p;
    p = p > (double)clip_max ? (double)clip_max : p;
    return (int)p;
}

// The "not 255" mask `m` of columns b0 .. b0 + 63 of the centering row, folded into the two ends of the run around car_x.
__device__ inline void shaping_run_ends(unsigned long long m, int b0, int car_x, int cols, int &stop_l, int &stop_r)
{
    if (b0 <= car_x) {
        const int k = car_x - b0;                 // columns b0 .. car_x of this chunk
        const unsigned long long ml = k >= 63 ? m : m & ((2ull << k) - 1ull);
        if (ml) stop_l = b0 + 63 - __builtin_clzll(ml);
    }
    if (b0 + 63 >= car_x && stop_r == cols) {
        const int k = car_x - b0;                 // columns car_x .. b0 + 63 of this chunk
        const unsigned long long mr = k <= 0 ? m : m & (~0ull << k);
        if (mr) stop_r = b0 + __builtin_ctzll(mr);
    }
}

// BITS: the image is a.bitmap_bits (else a.bitmap)
template <bool BITS>
static __global__ __launch_bounds__(64 * SHAPING_WAVES) void shaping_kernel(ShapingArgs a)
{
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x * SHAPING_WAVES + (threadIdx.x >> 6);
    if (env >= a.n) return;      // (a whole wave leaves: env is the same for its 64 lanes)
    const f110_shaping_config &c = a.cfg;
    const double x = a.xy[(size_t)env * (size_t)a.xy_stride], y = a.xy[(size_t)env * (size_t)a.xy_stride + 1];
    double x0 = a.prev_in[2 * (size_t)env], y0 = a.prev_in[2 * (size_t)env + 1];
    if (a.current_time) {
        const double now = a.current_time[env];
        // An env's clock reads exactly `timestep` if and only if the last step that touched it was its reset (f110_progress.h):
        // no reward is paid, the reset pose becomes the previous position (SAL's reset(), :69-89).  Idempotent.
        if (now == a.timestep) {
            if (lane == 0) {
                a.collision_term[env] = 0.0; a.progress_term[env] = 0.0; a.centering_term[env] = 0.0; a.total[env] = 0.0;
                a.collided[env] = 0;
                a.prev_out[2 * (size_t)env] = x; a.prev_out[2 * (size_t)env + 1] = y;
                a.t_seen[env] = now;
            }
            return;
        }
        const double seen = a.t_seen[env];
        if (now == seen) return;                 // not stepped since its previous update (a masked reset left it alone)
        if (seen < 0.0) { x0 = x; y0 = y; }      // no previous update (install, or a checkpoint without the shaper's state)
    }
    const double nan = __builtin_nan("");
    double t_col = nan, t_prog = nan, t_cen = nan, tot = nan;
    int hit = 0;
    const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y);
    if (finite) {
        const int words = (c.cols + 63) >> 6;
        const uint8_t *__restrict__ img = BITS ? nullptr : a.bitmap + (size_t)env * (size_t)c.rows * (size_t)c.cols;
        const uint64_t *__restrict__ bits = BITS ? a.bitmap_bits + (size_t)env * (size_t)c.rows * (size_t)words : nullptr;
        // collision (detect_collison): any neighbour of (px, py) inside the image equal to 255, the centre excluded.  Only
        // the part of the (2n+1)^2 window that lies inside the image is visited, so the trip count is bounded by the image.
        const int px = shaping_pixel(c.origin_x, x, c.scale, c.clip_max), py = shaping_pixel(c.origin_y, y, c.scale, c.clip_max);
        F110_BCHK(px >= 0 && px <= c.clip_max && py >= 0 && py <= c.clip_max, BT_SHAPING, a.dev_err);
        const long long nb = c.neighborhood;
        const long long wx0 = (long long)px - nb < 0 ? 0 : (long long)px - nb, wx1 = (long long)px + nb > c.cols - 1 ? c.cols - 1 : (long long)px + nb;
        const long long wy0 = (long long)py - nb < 0 ? 0 : (long long)py - nb, wy1 = (long long)py + nb > c.rows - 1 ? c.rows - 1 : (long long)py + nb;
        const long long ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;
        if (ww > 0 && wh > 0) {
            const long long cells = ww * wh;
            for (long long i0 = 0; i0 < cells; i0 += 64) {
                const long long i = i0 + lane;
                bool h = false;
                if (i < cells) {
                    const long long ny = wy0 + i / ww, nx = wx0 + i % ww;
                    F110_BCHK(nx >= 0 && nx < c.cols && ny >= 0 && ny < c.rows, BT_SHAPING, a.dev_err);
                    F110_BCHK(!BITS || (nx >> 6) < words, BT_SHAPING, a.dev_err);
                    const bool on = BITS ? ((bits[(size_t)ny * (size_t)words + (size_t)(nx >> 6)] >> (nx & 63)) & 1ull) != 0ull
                                         : img[(size_t)ny * (size_t)c.cols + (size_t)nx] == 255;
                    h = !(nx == px && ny == py) && on;
                }
                if (vote(h) != 0ull) { hit = 1; break; }
            }
        }
        t_col = hit ? c.w_collision : 0.0;
        // progress: metres moved since the previous update
        const double dx = x - x0, dy = y - y0;
        t_prog = sqrt(dx * dx + dy * dy) * c.w_progress;
        // centering (centerline_reward): car_x = int(x), car_y = int(y) -- metres truncated toward zero, used as pixel
        // indices.  int(v) lies in 0 .. m-1 exactly when -1 < v < m.
        double reward = -1.0;
        if (x > -1.0 && x < (double)c.cols && y > -1.0 && y < (double)c.rows) {
            const int car_x = (int)x, car_y = (int)y;
            F110_BCHK(car_x >= 0 && car_x < c.cols && car_y >= 0 && car_y < c.rows, BT_SHAPING, a.dev_err);
            // stop_l: the last column <= car_x that is not 255 (-1: none); stop_r: the first column >= car_x that is not 255
            // (cols: none).  The reference's walks end there: left = stop_l + 1, right = stop_r - 1.
            int stop_l = -1, stop_r = c.cols;
            if (BITS) {
                const uint64_t *__restrict__ row = bits + (size_t)car_y * (size_t)words;
                for (int w0 = 0; w0 < words; w0 += 4) {           // four independent loads in flight, the same in every lane
                    uint64_t v[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) v[j] = w0 + j < words ? row[w0 + j] : 0ull;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int b0 = 64 * (w0 + j);
                        if (b0 >= c.cols) break;
                        // beyond the row: not 255, the walk stops at the edge
                        const unsigned long long m = ~v[j] | (c.cols - b0 < 64 ? ~0ull << (c.cols - b0) : 0ull);
                        shaping_run_ends(m, b0, car_x, c.cols, stop_l, stop_r);
                    }
                }
            } else {
                const uint8_t *__restrict__ row = img + (size_t)car_y * (size_t)c.cols;
                for (int c0 = 0; c0 < c.cols; c0 += 256) {          // four independent 64-pixel loads in flight
                    uint8_t v[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int col = c0 + 64 * j + lane;
                        v[j] = col < c.cols ? row[col] : (uint8_t)0;   // beyond the row: not 255, the walk stops at the edge
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++) shaping_run_ends(vote(v[j] != 255), c0 + 64 * j, car_x, c.cols, stop_l, stop_r);
                }
            }
            stop_r = stop_r > c.cols ? c.cols : stop_r;          // (a virtual column beyond the row stands for the edge)
            const int left = stop_l + 1, right = stop_r - 1;
            if (left < right) {
                const double dist = fabs((double)car_x - (double)(left + right) / 2.0);
                const double r = 1.0 - dist / c.max_lane_halfwidth;
                reward = r > 0.0 ? r : 0.0;
            }
        }
        t_cen = reward * c.w_centering;
        tot = ((0.0 + t_prog) + t_col) + t_cen;                  // sum(rewards.values()) in the dict's order
    }
    if (lane == 0) {
        a.collision_term[env] = t_col; a.progress_term[env] = t_prog; a.centering_term[env] = t_cen; a.total[env] = tot;
        a.collided[env] = (uint8_t)hit;
        if (a.prev_out && finite) { a.prev_out[2 * (size_t)env] = x; a.prev_out[2 * (size_t)env + 1] = y; }
        if (a.t_seen) a.t_seen[env] = a.current_time[env];
    }
}

} // namespace f110
