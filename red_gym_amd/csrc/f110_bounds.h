// f110_bounds.h -- the device error word and the bounds-checked build: what every kernel family takes to report an index
// that is out of range (F110_BCHK, F110_BOUNDS_ONLY, the BT_* tags).  No kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace f110 {

// bits of the device error word (f110_device_errors; include/f110_hip.h F110_DEVERR_*)
constexpr uint32_t DEVERR_NOISE_WINDOW = 1u, DEVERR_BOUNDS = 2u;

// Bounds-checked debug build (-DF110_BOUNDS; `tools/build_variant.sh bounds -DF110_BOUNDS`, selected with F110_LIB; SURVEY 5
// "race detection / sanitizers": GPU AddressSanitizer is not available on this pool, the CPU oracle runs under ASan / UBSan).
// Every index a kernel of the step path forms from DATA -- a cell code, a rank, a slot number, a beam number, a noise row --
// is checked against its table before use; a violation ORs DEVERR_BOUNDS and the table's bit (8 + BT_*) into the handle's
// device error word (f110_device_errors) and the access is redirected to a valid element, so the run goes on and the
// report names the table.  The whole -m gpu suite is run against this build once per round (profiles/r04_bounds_build.txt).
enum { BT_LUT_CODE, BT_CELLS_FAR, BT_LUT_RANK, BT_DT, BT_NOISE_BEAM, BT_CS_TABLE, BT_CHUNK_ORDER, BT_MAP_SLOT, BT_NOISE_SLOT,
       BT_PARAMS_SLOT, BT_SCAN_STORE, BT_OPP_BEAM, BT_STAGE_LIST, BT_SELFTEST, BT_SIDE_SLOT,
       // the step's consumers (every header here includes this one and takes its tag from this list: a new family appends)
       BT_PROGRESS,   // an index of the tracker (raceline slot, grid cell, candidate, segment)
       BT_SHAPING,    // a pixel index of the shaper (px, py, car_x, car_y, a neighbour)
       BT_PATHFOLLOW, // an index of the follower (waypoint index, free set, spline piece)
       BT_REPLAY,     // a slot the replay kernels derive from `count`, a drawn index
       BT_EPISODES }; // a rank or a slot of the episode log
static_assert(BT_PROGRESS == 15 && BT_REPLAY == 18, "the tags are bits of the device error word (8 + BT_*): the ABI fixes their values");
#if defined(F110_BOUNDS)
#define F110_BCHK(ok, table, errp) \
    do { if (!(ok)) { uint32_t *e_ = (errp); if (e_) atomicOr(e_, DEVERR_BOUNDS | (1u << (8 + (table)))); } } while (0)
#define F110_BOUNDS_ONLY(...) __VA_ARGS__
#else
#define F110_BCHK(ok, table, errp) do { } while (0)
#define F110_BOUNDS_ONLY(...)
#endif

} // namespace f110
