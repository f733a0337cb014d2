// f110_plangrid.h -- a raceline's grid of candidate lists as the kernels take it (f110_planner.h explains it; the planner and the
// progress tracker search it, PlanGridDev in f110_handle.h owns its tables).  No kernels.
#pragma once
#include <stdint.h>

namespace f110 {

constexpr int PG_CAP = 30;            // candidates a cell's list holds
constexpr unsigned PG_ALL = 255;      // count value: take every segment
struct PlanGrid {
    double x0, y0, inv_cell;          // cell (ix, iy) covers x0 + ix / inv_cell ...
    int gw, gh;
    const uint8_t *count;             // [gh * gw]
    const uint16_t *cand;             // [gh * gw][PG_CAP] ascending segment indices
    int degenerate;                   // the raceline has a zero-length segment: plan() answers (0, 4.0) for every pose
};

} // namespace f110
