/*
 * f110_hip.h -- C ABI of the MI355X-native batched F1TENTH step path.
 *
 * This is the drop-in boundary for the reference's hot path
 *   F110Env.step / reset          gym/f110_gym/envs/f110_env.py:261-347
 *   Simulator.step / reset        gym/f110_gym/envs/base_classes.py:546-623
 *   ScanSimulator2D.scan/set_map  gym/f110_gym/envs/laser_models.py:383-454
 * The reference has no FFI layer (it is Python + Numba); these are the entry
 * points a ctypes binding of that path needs (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success or a negative F110_E_* code and never
 *     throws; f110_last_error() gives the message of the calling thread's last
 *     failure.
 *   - plain pointers and sizes only.  "dev" pointers are device (HBM) addresses
 *     owned by the caller (e.g. torch tensors' data_ptr()); "host" pointers are
 *     read during the call and not retained.  Nothing is allocated in
 *     f110_step/f110_reset; kernels are enqueued on `stream` (a hipStream_t
 *     passed as void*, NULL = default stream) and the call does not synchronise.
 *   - a handle is bound to one device and is not thread-safe.  Calls that allocate or upload (f110_create, map
 *     installs, table uploads, f110_graph_create, f110_destroy ...) make the handle's device current for their own
 *     duration and RESTORE the caller's current device before returning.  Calls that launch on the caller's stream
 *     (f110_step, f110_reset, f110_graph_launch, the function-level entry points, f110_bitmap_render) do not switch:
 *     the stream belongs to the calling thread's current device, so that must be the handle's -- otherwise
 *     F110_E_INVALID.  Several handles (on one device or on several) may be driven from one process.
 *   - there is no f110_get_state / f110_set_state: the whole simulation state lives in the CALLER-owned
 *     buffers of the f110_buffers struct, bound once with f110_bind, so reading, checkpointing or overwriting the state is
 *     an ordinary access to the caller's own memory between steps (F110VecEnv.state_dict / load_state_dict).
 *   - two test hooks are read from the environment: F110_SCAN_STORES = plain|stream (which store instantiation of
 *     the scan kernel a step launches) and F110_BM_GRID = <n> (workgroups of a bitmap launch); results do not
 *     depend on them.
 *   - all arithmetic that decides an index, a collision or a lap toggle is
 *     IEEE fp64 in the reference's operation order (no FMA contraction).
 */
#ifndef F110_HIP_H
#define F110_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F110_OK 0
#define F110_E_INVALID (-1)  /* bad argument / state (ValueError in the reference) */
#define F110_E_HIP (-2)      /* HIP runtime failure */
#define F110_E_NOMAP (-3)    /* scan before set_map (laser_models.py:445-446) */
#define F110_E_INDEX (-4)    /* agent index out of range (base_classes.py:525-527) */
#define F110_E_UNBOUND (-5)  /* step/reset before f110_bind */

#define F110_MAX_CARS (1 << 26) /* num_envs * num_agents of one handle (32-bit wave / lane indices; offsets into the
                                  * per-car tensors are 64-bit): 67 M cars, 290 GB of fp32 scans alone at 1080 beams */
#define F110_MAX_AGENTS 32
#define F110_MAX_MAPS 4096  /* map slots of one handle (f110_set_map_slot_*, f110_assign_maps) */
#define F110_MAX_NOISE_SLOTS 64 /* noise slots (= distinct seeds) of one handle (f110_set_noise_generator, f110_assign_noise) */
#define F110_NOISE_INITIAL_ROWS 1024 /* rows per slot of a generated noise table when it is first allocated (it doubles on demand) */
#define F110_NUM_PARAMS 18
#define F110_RK4 1   /* Integrator.RK4   base_classes.py:40-42 */
#define F110_EULER 2 /* Integrator.Euler */

typedef struct f110_handle f110_handle;

/* Constructor arguments of F110Env (f110_env.py:100-157), Simulator
 * (base_classes.py:459) and ScanSimulator2D (laser_models.py:360), plus the
 * batch extension (num_envs, autoreset, device). */
typedef struct {
    int32_t num_envs;    /* B: independent envs on this device */
    int32_t num_agents;  /* A: cars per env (1..F110_MAX_AGENTS) */
    int32_t num_beams;   /* 1080 */
    int32_t theta_dis;   /* 2000 */
    int32_t integrator;  /* F110_RK4 | F110_EULER */
    int32_t ego_idx;
    int32_t device;      /* HIP device ordinal */
    int32_t autoreset;   /* 1: an env that reports done is reset to its spawn pose by the next f110_step */
    double fov;          /* 2*pi */
    double eps;          /* 1e-4 */
    double max_range;    /* 30.0 */
    double timestep;     /* 0.01 */
    double ttc_thresh;   /* 0.005 (base_classes.py:113) */
    /* mu C_Sf C_Sr lf lr h m I s_min s_max sv_min sv_max v_switch a_max v_min v_max width length */
    double params[F110_NUM_PARAMS];
} f110_config;

/* Caller-owned device buffers the step reads and writes (N = B*A cars).
 * Simulation state (carried from step to step): */
typedef struct {
    double *state;          /* [N,7]  x y steer v yaw yaw_rate slip   base_classes.py:95-96 */
    double *steer_buf;      /* [N,2]  steering delay FIFO, [0] newest  :269-276 */
    int32_t *steer_cnt;     /* [N]    entries in the FIFO (0..2) */
    int32_t *noise_step;    /* [N]    scans drawn since the car's reset (row of the noise table) */
    double *spawn;          /* [N,3]  pose used by reset / autoreset */
    double *start_rot;      /* [B,4]  f110_env.py:329 */
    uint8_t *near_start;    /* [N]    f110_env.py:182 */
    int32_t *toggles;       /* [N]    f110_env.py:183 toggle_list */
    double *current_time;   /* [B]    f110_env.py:177 */
    uint8_t *pending_reset; /* [B]    1: next f110_step performs reset(spawn) + zero-action step for this env */
    /* observations (overwritten every step): */
    float *scans;           /* [N,num_beams] fp32 lidar ranges (noise, opponents applied) */
    double *scans_f64;      /* [N,num_beams] same in fp64, or NULL to skip (parity tests, single-env facade) */
    double *pose_snap;      /* [N,3]  poses after integration, before iTTC zeroing (base_classes.py:567) */
    uint8_t *collisions;    /* [N]    obs['collisions'] (GJK or iTTC)  :543,:581-582 */
    int32_t *collision_idx; /* [N]    Simulator.collision_idx, -1 = none */
    uint8_t *in_collision;  /* [N]    RaceCar.in_collision (iTTC only) */
    int32_t *lap_counts;    /* [N]    f110_env.py:238 */
    double *lap_times;      /* [N]    f110_env.py:240 */
    uint8_t *done;          /* [B]    f110_env.py:242 (0/1, so the buffer may be a bool tensor) */
    uint8_t *checkpoint_done; /* [N]  info['checkpoint_done'] = toggles >= 4 (f110_env.py:244), or NULL */
    uint32_t *lookups;      /* [N]    distance-table reads per car, ACCUMULATED over steps until the caller
                                      zeroes it (instrumentation for the byte model), or NULL */
} f110_buffers;

int f110_create(const f110_config *cfg, f110_handle **out);
void f110_destroy(f110_handle *h);
const char *f110_last_error(void);

/* Simulator.update_params (base_classes.py:507-527): agent_idx < 0 updates every agent,
 * otherwise agent `agent_idx` of every env (F110_E_INDEX if >= num_agents).  As in the
 * reference this changes the cars' dynamics and the size they attribute to opponents
 * (base_classes.py:221), not the Simulator's own copy used by the GJK check (:542) nor
 * the beam tables fixed at construction (:116-156). */
int f110_update_params(f110_handle *h, const double *params18_host, int32_t agent_idx);

/* Per-env constructor arguments.  One handle stands in for num_envs F110Env instances; the reference constructs each
 * with its own `params` (f110_env.py:125-128) and `seed` (:102-105).  Like maps (slots + f110_assign_maps), both exist
 * as SLOTS plus an env -> slot table:
 *   params slot = the `params` dict of one reference env: Simulator.params (the GJK quads, base_classes.py:542) and the
 *     RaceCar.params of every agent (:84,169).  f110_set_params_slots replaces the whole slot table ([n_slots,18] host,
 *     1 <= n_slots <= num_envs: "every env its own vehicle" is n_slots = num_envs with the identity assignment);
 *     f110_set_params_slot changes one slot -- agent_idx < 0: as at construction (Simulator copy + every agent), else only
 *     RaceCar.params of that agent (Simulator.update_params on that env, :507-527); a slot beyond the current count extends
 *     the table with copies of slot 0.  f110_update_params (above) keeps applying to every slot.  f110_assign_params: host
 *     int32 [num_envs], NULL = all envs on slot 0.  The beam tables (scan angles, cosines, side distances) are per handle
 *     by default: in the reference they are class-level statics fixed by the FIRST RaceCar a process constructs
 *     (base_classes.py:116-156), so envs created in one process share env 0's.  The side distances -- the only one of the
 *     three that depends on the vehicle -- can be given per params slot instead (f110_set_side_distance_slots below):
 *     num_envs independently constructed envs, each with the table of its own `params`.
 *   noise slot = one seed: see f110_set_noise_generator / f110_set_noise_slot / f110_assign_noise below. */
int f110_set_params_slots(f110_handle *h, const double *params_host, int32_t n_slots);
int f110_set_params_slot(f110_handle *h, int32_t slot, const double *params18_host, int32_t agent_idx);
int f110_assign_params(f110_handle *h, const int32_t *slot_of_env_host);
/* Side distances of the iTTC test (base_classes.py:116-156, laser_models.py:189-217) per VEHICLE: side_host = [n_slots,
 * num_beams] fp64, one table per params slot; the scan of env e tests its beams against row slot_of_env[e] (the table
 * f110_assign_params installed; all envs on row 0 when none is).  Any values are legal, as for f110_set_tables (negative,
 * infinite, NaN).  NULL / n_slots == 0 removes the tables: the handle is back on the one table of f110_set_tables, which
 * is kept beside them and never changed by this call.  Device memory: n_slots x num_beams x 8 B (4 096 vehicles of 1 080
 * beams: 35 MB).  A successful install or removal moves the launch epoch.
 * While tables are installed every params slot has one and no other exists: n_slots must equal the handle's current params
 * slot count (F110_E_INVALID otherwise); f110_set_params_slots with another slot count is refused (F110_E_INVALID: remove
 * the side tables first); f110_set_params_slot on a slot beyond the count extends the side tables with copies of row 0, as
 * it does for the params.  f110_update_params and f110_set_params_slot on an existing slot leave the side tables alone: in
 * the reference they are fixed at construction (base_classes.py:158-169 only replaces self.params).  A refused call
 * changes nothing, the launch epoch included. */
int f110_set_side_distance_slots(f110_handle *h, const double *side_host, int32_t n_slots);

/* Optional: replace the library's libm-computed tables by the caller's
 * (numpy-computed, as in the reference).  sines/cosines: [theta_dis]
 * (laser_models.py:379-381); scan_angles/beam_cosines/side_distances:
 * [num_beams] (base_classes.py:123-156).  Any pointer may be NULL = keep. */
int f110_set_tables(f110_handle *h, const double *sines_host, const double *cosines_host,
                    const double *scan_angles_host, const double *beam_cosines_host,
                    const double *side_distances_host);

/* ScanSimulator2D.set_map (laser_models.py:383-427) after image decoding.
 * free_mask: [H*W] row-major, row 0 = bottom of the image (already flipped,
 * :399), nonzero = free (>128, :403-404).  The library runs an exact Euclidean
 * distance transform (replaces scipy.ndimage.distance_transform_edt, :52). */
int f110_set_map_occupancy(f110_handle *h, const uint8_t *free_mask_host, int32_t height,
                           int32_t width, double resolution, double orig_x, double orig_y,
                           double orig_c, double orig_s);
/* Same with the mask already on the device (e.g. drawn by a track generator): the whole pipeline -- EDT,
 * rank coding, LUT, fp64 table -- runs on the GPU; only two scalars and the 8 KiB LDS image of the LUT visit
 * the host.  An all-free mask (no occupied cell) is the caller's responsibility here. */
int f110_set_map_occupancy_dev(f110_handle *h, const uint8_t *free_mask_dev, int32_t height, int32_t width,
                               double resolution, double orig_x, double orig_y, double orig_c, double orig_s);
/* Walls of a generated track (replaces the drawing half of unittest/random_trackgen.py:161-218): mask_dev
 * [H*W] gets 0 where the distance from the pixel centre (x0 + (ix+.5)*pixel, y0 + (iy+.5)*pixel) to the
 * polyline pts_dev [n_pts,2] (closed: last point joins the first) is within half_stroke of `offset`, else 1.
 * Feed the result to f110_set_map_occupancy_dev. */
int f110_track_mask(const double *pts_dev, int32_t n_pts, int32_t closed, int32_t height, int32_t width, double x0,
                    double y0, double pixel, double offset, double half_stroke, uint8_t *mask_dev, void *stream);
/* Map slots: one handle stands in for many F110Env instances, each of which may have its own map
 * (f110_env.py:100-157 takes `map` per env).  Slot 0 is the map of the calls above; f110_set_map_slot_* fill
 * slots 0..F110_MAX_MAPS-1 the same way, and f110_assign_maps gives every env its slot (host int32 [num_envs],
 * NULL = all envs on slot 0; F110_E_INDEX for a slot that holds no map).  Any assignment is valid.  The scan keeps its
 * full occupancy when the 2 consecutive cars of every scan workgroup share a map, i.e. maps assigned to blocks of envs
 * with an even car count; otherwise (a map per env) it runs one wave per workgroup, each staging its own map's table:
 * same bits, ~24 % fewer env-steps/s at 65 536 cars (profiles/r05_map_per_env.txt).  Maps of different kinds ("resolution is a power of two",
 * "origin unrotated") may be mixed: the shard is then scanned block by block, each run of envs with the instantiation
 * its own maps allow (one more launch per change of kind along the env index).  An install that fails leaves its slot
 * as it was: the old map stays in place, and the envs assigned to the slot keep scanning it. */
int f110_set_map_slot_occupancy(f110_handle *h, int32_t slot, const uint8_t *free_mask_host, int32_t height, int32_t width,
                                double resolution, double orig_x, double orig_y, double orig_c, double orig_s);
int f110_set_map_slot_occupancy_dev(f110_handle *h, int32_t slot, const uint8_t *free_mask_dev, int32_t height,
                                    int32_t width, double resolution, double orig_x, double orig_y, double orig_c,
                                    double orig_s);
int f110_assign_maps(f110_handle *h, const int32_t *map_of_env_host);
int f110_get_map_slot_dt(f110_handle *h, int32_t slot, double *dt_host_out);
/* Same, from a precomputed distance table dt = resolution*edt(img) (host, [H*W] fp64).  Every map entry refuses
 * height > 524286 or width >= 2^26: the scan addresses cells with signed 24-bit multiplies. */
int f110_set_map_dt(f110_handle *h, const double *dt_host, int32_t height, int32_t width,
                    double resolution, double orig_x, double orig_y, double orig_c, double orig_s);
/* Copies the fp64 distance table the handle holds to the host (tests). */
int f110_get_map_dt(f110_handle *h, double *dt_host_out);

/* Exact squared Euclidean distance transform on the host (cells to nearest
 * zero cell), the integer kernel behind f110_set_map_occupancy. */
int f110_edt_squared(const uint8_t *free_mask_host, int32_t height, int32_t width, uint32_t *d2_out_host);
/* The same transform on the GPU (dev pointers; synchronises `stream` before returning): a column pass and a
 * row pass with the row's g^2 in LDS, exact like the host version.  height, width <= 32768. */
int f110_edt_squared_dev(const uint8_t *free_mask_dev, int32_t height, int32_t width, uint32_t *d2_out_dev, void *stream);

/* Lidar noise.  Reference: every scan adds `rng.normal(0, std, num_beams)` drawn from the car's own
 * np.random.default_rng(seed), re-created at every reset (laser_models.py:450-452, base_classes.py:117,202); all cars of an
 * env share the seed, so a car's noise row is a function of (seed, scans since its reset).  The handle keeps the rows of
 * each seed ONCE, in a noise slot, indexed by every car's own counter (f110_buffers.noise_step); f110_assign_noise gives
 * every env its slot (host int32 [num_envs], NULL = all on slot 0).  A slot is filled either way:
 *   f110_set_noise_generator -- the rows are PRODUCED ON THE DEVICE by a bit-level restatement of NumPy's PCG64 +
 *     ziggurat `normal` (csrc/f110_noise.h).  pcg64_state_inc = {state_lo, state_hi, inc_lo, inc_hi} of
 *     np.random.PCG64(seed).state['state'] (NumPy's SeedSequence hashing stays with NumPy; a C caller may pass any
 *     128-bit state and odd increment).  Setting a generator restarts every generated slot at row 0.
 *   f110_set_noise_slot -- rows [T,num_beams] fp64 from the host (any table; tests, non-NumPy streams).
 *     f110_set_noise_table(h, tbl, T) is slot 0; T = 0 / NULL switches noise off for the whole handle.
 * Rows: f110_noise_ensure(h, rows, stream) makes rows 0 .. rows-1 (above the floor) readable for work enqueued on
 * `stream` afterwards -- call it before a step with rows > the largest noise_step any car can have in that step;
 * generated slots produce what is missing (a one-wavefront kernel per slot; the table doubles when it must: cold path,
 * synchronises), host tables that are too short give F110_E_INVALID.  f110_noise_prefetch(h, rows) starts producing
 * ahead of time on the handle's own stream, beside the caller's work; a later f110_noise_ensure only waits for it.
 * Floor: when no car will read rows below `lo` in any step enqueued FROM NOW ON (autoreset off and, by the host's own step
 * count, every car past them), f110_noise_set_floor(h, lo, stream) lets the table recycle them -- it is a ring, so a run of any
 * length holds a window of rows in constant memory.  Steps already enqueued on `stream` may still read those rows: the call
 * records an event there, and the next prefetch (which writes the recycled places from the handle's own stream) waits for it;
 * so does a generator launch that f110_noise_ensure put on the caller's stream (both work on the same generator states).
 * Lowering the floor again (a masked reset sends cars back to row 0 while others run on) re-produces the dropped rows in
 * `stream` from the MARKS the generators leave every 64 rows -- one wavefront per slot and 64 rows, all at once; the generators
 * stay where they are (round 4 rewound them to the seeds: ~15 us per row of the whole run).  The ring then spans floor .. rows
 * produced, i.e. the ages of the youngest and the oldest car: rows x num_beams x 8 B per slot (20 000 steps: 173 MB per seed).
 * A car whose row lies outside [floor, rows produced) sets F110_DEVERR_NOISE_WINDOW in the device error word instead of
 * reading silently.
 * Launch epoch: the scan takes the table's base and size by value (a pointer chase per wave costs 0.9 % of the launch), so
 * a RE-ALLOCATION -- the ring too small for the rows between the floor and the fastest car: it doubles -- moves the launch
 * epoch like every other table change; the window of rows present (floor, rows produced) moves without it, behind a
 * device-resident descriptor.  A run whose floor follows its cars never re-allocates: one captured hipGraph serves it
 * for any length (tests/test_gpu_noise.py: 20 000 replays). */
int f110_set_noise_table(f110_handle *h, const double *table_host, int64_t T);
int f110_set_noise_slot(f110_handle *h, int32_t slot, const double *table_host, int64_t T);
int f110_set_noise_generator(f110_handle *h, int32_t slot, const uint64_t *pcg64_state_inc, double std_dev);
int f110_assign_noise(f110_handle *h, const int32_t *slot_of_env_host);
/* Every env its own seed, any number of them (F110_MAX_NOISE_SLOTS does not apply): pcg64_state_inc_host = [num_envs][4]
 * {state_lo, state_hi, inc_lo, inc_hi} of np.random.PCG64(seed_e).state['state'].  The env's generator state lives on the
 * device; the row its scan adds is produced by the step itself, in front of the scan (one wavefront per env and step), into
 * ONE row per env -- no table to keep ahead of the cars, no floor, no growth: f110_noise_ensure / _prefetch / _set_floor
 * are no-ops in this mode.  A reset restarts the env's stream at its seed; a row counter that does not continue the
 * generator's (a loaded checkpoint) makes the generator run forward from the seed without storing.  Costs one more kernel
 * per step (~1 500 wave-instructions per env).  Setting a table or a slot generator leaves the mode; an f110_set_noise_*
 * call that refuses its arguments changes nothing, the mode and the launch epoch included.
 * Reference: f110_env.py:102-105 (`seed` of every env), base_classes.py:117,202, laser_models.py:450-452. */
int f110_set_noise_per_env(f110_handle *h, const uint64_t *pcg64_state_inc_host, double std_dev);
int f110_noise_ensure(f110_handle *h, int64_t rows, void *stream);
int f110_noise_prefetch(f110_handle *h, int64_t rows);
int f110_noise_set_floor(f110_handle *h, int64_t lo, void *stream);
/* floor, rows readable by the kernels (a prefetch still in flight not counted), rows per slot of the ring, slots, bytes held
 * (host-side bookkeeping, no synchronisation; any pointer may be NULL) */
int f110_noise_info(f110_handle *h, int64_t *lo, int64_t *hi, int64_t *cap, int32_t *slots, int64_t *bytes);
/* Tests / diagnostics: the noise values of rows row0 .. row0+n_rows-1 of a slot, [n_rows,num_beams] fp64 to the host
 * (synchronises; F110_E_INDEX when a row is not in the table). */
int f110_noise_read(f110_handle *h, int32_t slot, int64_t row0, int64_t n_rows, double *out_host);

/* Device error word: conditions a kernel can only detect while it runs are OR-ed into one word per handle instead of
 * being silent.  Synchronises the device, returns the word and clears it.  F110_DEVERR_NOISE_WINDOW: a car's noise row
 * was not in the table (f110_noise_ensure not called, or the floor above a live car).  F110_DEVERR_BOUNDS: only in the
 * bounds-checked debug build of the library (-DF110_BOUNDS, tools/build_variant.sh): an index into a device table was out
 * of range; bits 8.. name the table (csrc/f110_bounds.h BT_*). */
#define F110_DEVERR_NOISE_WINDOW 0x1u
#define F110_DEVERR_BOUNDS 0x2u
#define F110_DEVERR_QP_LIMIT 0x4u /* the path follower's active-set walk reached its step limit (see f110_pathfollow_act) */
int f110_device_errors(f110_handle *h, uint32_t *flags_out);

int f110_bind(f110_handle *h, const f110_buffers *bufs);

/* F110Env.reset(poses) (f110_env.py:304-347) for the envs selected by mask
 * (dev [B] uint8, NULL = all): stores poses as spawn, resets those envs and
 * runs their zero-action step; other envs are untouched.  poses: dev [B,A,3]. */
int f110_reset(f110_handle *h, const double *poses_dev, const uint8_t *mask_dev, void *stream);

/* F110Env.step(action) for all B envs (f110_env.py:261-302).  actions: dev
 * [B,A,2] fp64, column 0 = steer, column 1 = speed.  Envs with pending_reset
 * ignore their action and perform reset(spawn) + zero-action step instead. */
int f110_step(f110_handle *h, const double *actions_dev, void *stream);

/* One env's observation gathered into ONE fp64 row on the device (the single-env Gym facade copies it to the host with
 * one transfer instead of one per field): out_dev[f110_pack_env_size(h)] =
 *   [A*7 state | A collisions | A lap_times | A lap_counts | A toggles | current_time | done | A*num_beams scans]
 * (scans from scans_f64 when bound, else the fp32 scans widened).  Enqueued on `stream`, no synchronisation. */
int64_t f110_pack_env_size(f110_handle *h);
int f110_pack_env(f110_handle *h, int32_t env, double *out_dev, void *stream);

/* Tuning / test hook: how a scan launch maps wavefronts to cars, as "cars:lg,cars:lg,..." in launch order with one
 * "*" for the remaining cars: a car of a stage gets 2^lg wavefronts (lg = 0..3; several short-lived waves per car pay
 * for small batches and at the end of a launch).  NULL or "" restores the built-in choice (scan_stage_list in
 * csrc/f110_scan_plan.h).  A malformed list (syntax, lg > 3, two "*", more than 6 stages, more cars than the handle
 * has) is refused with F110_E_INVALID and changes nothing.  A list that does not fit a launch -- a stage before the last
 * with an odd car count (only "*" can have one), fixed stages of more cars than the launch has -- is replaced by one
 * stage of whole cars for that launch.  Results do not depend on it. */
int f110_set_scan_stages(f110_handle *h, const char *spec);

/* hipGraph support.  f110_step only enqueues kernels (no allocation, no synchronisation), so it can be captured
 * into a HIP graph and replayed.  A capture freezes the kernel selection and the by-value launch arguments; the
 * calls that change them -- f110_bind, f110_set_tables, f110_set_side_distance_slots, every map install, f110_assign_maps / _params / _noise, a
 * re-allocation of the noise table, a successful f110_pure_pursuit_prepare (it frees and re-allocates the grid that a
 * captured f110_pure_pursuit reads) -- bump the handle's launch epoch.  A graph captured at epoch e is valid while
 * f110_launch_epoch still reports e; after that it must be re-captured (F110VecEnv.step_graph does so itself). */
/* Launch order of the step's scan (performance only; no reference counterpart): order_dev = dev int32 [num_envs * num_agents], a
 * PERMUTATION of the car indices (the caller's responsibility: a wrong array scans some cars twice and others not at all), or NULL
 * = car order.  The wave that would march car i marches car order[i]; every result is stored under the car's own index, so the
 * outputs do not depend on it.  Purpose: cars that stand on the same noise row launched side by side share that row in the L1 / L2 --
 * a batch whose envs were reset at different times otherwise streams one 8.6 KB row per env from HBM (10 % of the step at 65 536
 * envs).  The array stays owned by the caller and may be re-written in stream order between steps (red_gym_amd.Engine re-sorts it
 * by the envs' row counters every 64 steps); changing the POINTER moves the launch epoch.  Ignored while envs are on different maps. */
int f110_set_scan_order(f110_handle *h, const int32_t *order_dev);
int f110_launch_epoch(f110_handle *h, int64_t *epoch);

/* The form of the step's scan (performance only; results do not depend on it).  Besides the classic form -- two cars per
 * workgroup sharing one 1 024-slot LDS copy of the map's distance LUT -- every install of map slot 0 builds two COMPACT forms (two more cell
 * tables, 2 x the cell table's bytes, and the row-padded byte table of f110_scan_codes_info / f110_scan_pad_rows), S = 256 and 512: an LDS image of the LUT's first S - 2 ranks and a cell table in which every cell of a higher rank carries the far
 * marker (such cells take the second table, as cells beyond the classic image always did).  A compact form runs workgroups of
 * one wave, each with its own image.  It applies to the step's scan on a single map whose origin is unrotated and whose
 * resolution is a power of two; the rule that picks it (scan_compact_choice in csrc/f110_scan_plan.h) reads, per form, the
 * share of free cells behind its marker among the cells a car can reach, averaged over the cars (scan_reach_shares, same
 * file): the free cells 8-connected to the car's spawn cell.  Until those shares are learnt the scan keeps the classic form.
 * The environment variable F110_SCAN_FORM = classic | compact256 | compact512, read once per process, overrides the rule where
 * the form applies (tests, A/B runs).
 * f110_scan_form_learn(h, poses_dev, stream): learns the shares from poses_dev = dev [num_envs * num_agents][3] (x, y, yaw),
 * the spawn poses of a reset of ALL envs; call it beside that reset (red_gym_amd.Engine.reset does).  Unlike f110_reset it
 * SYNCHRONISES `stream`, copies the poses and map slot 0's cell table to the host, allocates there (4 bytes per map cell) and
 * floods the cars' free components -- tens of ms on a 1 600 x 1 600 map.  It does all that once per map install and only
 * where the answer is used: it returns at once on a handle the rule cannot route (several agents per env, fewer than 32 768
 * cars, a map per env, a rotated origin or a resolution that is not 2^k), under F110_SCAN_FORM, when the shares are known,
 * and on a stream that is being captured.  Learning moves the launch epoch.  Never calling it is safe: the classic form.
 * f110_scan_form_info: *form = the S a step of n_cars cars launches now (0: classic); out_share[4] = the shares for S = 256 and
 * 512 over ALL free cells of map slot 0, recorded at install (1.0 each where the compact tables were not built: a table beyond
 * 64 MB, a failed allocation, a slot other than 0), then the learnt ones (-1.0 each while not learnt). */
int f110_scan_form_learn(f110_handle *h, const double *poses_dev, void *stream);
int f110_scan_form_info(f110_handle *h, int32_t n_cars, int32_t *form, double *out_share);
/* The fp32 rows of the step's scan (performance only).  The compact form of 256 slots leaves 2 816 B of a workgroup's share of
 * the LDS idle; with an fp32 output it stages the results of the last 11 of a wave's 64-beam chunks there and writes them out
 * as whole chunks when its march has ended, instead of one scattered dword per finished beam (scan_rowbuf_plan in
 * csrc/f110_scan_plan.h).  The environment variable F110_SCAN_ROWS = lds | direct, read once per process, overrides the rule
 * (tests, A/B runs); neither value changes which form is launched.
 * f110_scan_rows_info: *lds = 1 where a step of n_cars cars with an fp32 output stages its rows now, else 0. */
int f110_scan_rows_info(f110_handle *h, int32_t n_cars, int32_t *lds);
/* The cell codes of the step's scan (performance only).  The codes of the compact form of 256 slots are multiples of 8 below
 * 2 048, so every install of map slot 0 also builds that form's table as BYTES (the slot, code >> 3) in strips of 16 columns:
 * half the cell table's bytes more, and a 128-byte line then holds 8 rows x 16 columns of cells instead of 8 x 8.  The launch
 * that stages its rows in LDS (above) reads that table.  The environment variable F110_SCAN_CODES = byte | word, read once per
 * process, overrides the rule (tests, A/B runs); neither value changes the form or where the rows are staged.
 * f110_scan_codes_info: *bytes = 1 where a step of n_cars cars with an fp32 output reads byte codes now, else 0. */
int f110_scan_codes_info(f110_handle *h, int32_t n_cars, int32_t *bytes);
/* The byte table is ROW-PADDED: every strip carries P rows of 0 above its first and below its last border row, P the smallest
 * multiple of 8 that is >= ceil(max_range / resolution) + 2, so that the march of a car standing on the map clamps no row
 * (every look-up of a ray lies within max_range of its car).  Its bytes are those of a map of H + 2 P rows -- example_map:
 * 4.2 MB at P = 488 -- and count toward the compact tables' 64 MB limit; a map whose padded table does not fit gets none and
 * reads word codes.
 * f110_scan_pad_rows: *rows = P of map slot 0's byte table, or -1 where the map has none. */
int f110_scan_pad_rows(f110_handle *h, int32_t *rows);

/* The step as a HIP graph the library builds itself, for callers without a capturing framework and as the reference
 * point for framework captures: F110_GRAPH_NODES = one kernel node per kernel of f110_step(actions_dev), chained
 * (hipGraphAddKernelNode); F110_GRAPH_CAPTURE = the same launches captured on a private non-blocking stream.
 * f110_graph_launch enqueues one step on `stream` (the actions are read from actions_dev at execution time) and
 * refuses a graph whose handle's launch epoch has moved (F110_E_INVALID: create it again).  f110_graph_info reports
 * the node count and, with a path, writes the graph in dot form (hipGraphDebugDotPrint). */
#define F110_GRAPH_NODES 0
#define F110_GRAPH_CAPTURE 1
typedef struct f110_graph f110_graph;
int f110_graph_create(f110_handle *h, const double *actions_dev, int32_t how, f110_graph **out);
int f110_graph_launch(f110_graph *g, void *stream);
int f110_graph_info(f110_graph *g, int32_t *nodes, const char *dot_path);
void f110_graph_destroy(f110_graph *g);

/* Measurement aid (bench.py): between begin and end every f110_step attaches a start / stop
 * hipEvent pair to its scan_kernel dispatch on the step's stream (up to max_launches
 * steps).  f110_profile_end synchronises on the last event and returns the summed
 * kernel time in milliseconds and the number of launches measured. */
int f110_profile_begin(f110_handle *h, int32_t max_launches);
/* Sampling: events ride on every `every`-th step only (default 1 = all).  A dispatch that carries events costs the
 * stream about 10 us of idle time around it (measured, profiles/r03_event_cost.txt), which a 4 096-env step notices. */
int f110_profile_every(f110_handle *h, int32_t every);
/* While the aid is active (between begin and end) f110_buffers.lookups is only fed by the steps that carry an event
 * pair: the counters then hold the table reads of exactly the measured launches. */
int f110_profile_end(f110_handle *h, double *scan_ms_total, int32_t *launches);

/* Batched pure-pursuit planner, the caller on the other side of F110Env.step
 * (examples/waypoint_follow.py:15-217: nearest point on the raceline, first intersection
 * of the lookahead circle with the polyline incl. wrap-around, actuation).  waypoints:
 * dev [M,3] (x, y, speed); state: dev [n,7] (f110_buffers.state); writes actions dev [n,2]
 * = (steer, vgain*speed), ready to be passed to f110_step.  The planner keeps no state: h may be NULL (the
 * kernel is then enqueued on `stream` of the calling thread's current device). */
/* Optional: PREPARES one raceline (dev [M,3], M <= 65 535) for f110_pure_pursuit -- a grid of `cell` metres (0: 0.25) reaching
 * `margin` metres (0: 3) around the raceline whose cells list the segments that can be the nearest one for any pose in the cell
 * (conservative: every segment within 2 half-diagonals of the cell centre's nearest).  f110_pure_pursuit(h, the same pointer,
 * the same M, ...) then plans with ONE LANE per car over that list instead of one wavefront per car over 64-segment blocks
 * (65 536 cars on the 783-point example raceline: see profiles/r05_planner.txt); poses outside the grid, NaN poses and
 * cells with more than 30 candidates take every segment -- the results are the same in every case (tests: `==` both
 * kernels and oracle/planner.py).  A cold path (copies the raceline to the host, synchronises); call it again when the raceline's
 * VALUES change: f110_pure_pursuit matches the grid by pointer and M alone (pass h = NULL to plan without it).  A failed call
 * (e.g. M > 65 535, a grid beyond 16 M cells) leaves the handle without a grid.
 * Reference: examples/waypoint_follow.py:15-47 (nearest point), :183-217 (plan). */
int f110_pure_pursuit_prepare(f110_handle *h, const double *waypoints, int32_t M, double cell, double margin, void *stream);
int f110_pure_pursuit(f110_handle *h, const double *waypoints, int32_t M, double lookahead, double vgain,
                      double wheelbase, double max_reacquire, const double *state, int32_t n,
                      double *actions, void *stream);

/* The same planner for MANY racelines in one launch, of any length (the reference builds one planner per env from any
 * CSV, examples/waypoint_follow.py:146-162): waypoints dev [total,3] = the K racelines back to back; offsets [K+1] =
 * first row of each (offsets[0] = 0, offsets[K] = total) given both as a dev and as a host array; track_of_car dev
 * [n] int32 = raceline of every car (NULL: all on raceline 0).  workspace: dev doubles,
 * f110_pure_pursuit_workspace(total, K) of them, holding the bounding boxes of the racelines' 64-segment blocks;
 * boxes_valid != 0 says the workspace still holds them from an earlier call with the same racelines (skips the small
 * kernel that fills it).  Racelines are read from global memory (L1 / L2), so there is no length limit.  A raceline
 * with two equal consecutive waypoints gives (steer 0, speed 4.0) for every car on it, as the reference does (NaN
 * nearest distance).  f110_pure_pursuit itself stages its raceline in LDS while it fits (gfx950: about 6 400 points)
 * and otherwise runs this form without a workspace (every block evaluated). */
int64_t f110_pure_pursuit_workspace(int32_t total_points, int32_t K);
int f110_pure_pursuit_tracks(f110_handle *h, const double *waypoints, const int32_t *offsets_dev,
                             const int32_t *offsets_host, int32_t K, const int32_t *track_of_car, double lookahead,
                             double vgain, double wheelbase, double max_reacquire, const double *state, int32_t n,
                             double *actions, double *workspace, int32_t boxes_valid, void *stream);

/* Progress along the raceline: per car the Frenet pose on its raceline and the metres driven since its reset, from the
 * state the step left (no reference counterpart as a function; the nearest point is examples/waypoint_follow.py:16-47,
 * the consumer the reference's own RL loop, src/SAL.py:233-236, which pays for metres moved).
 * A raceline is M >= 2 points (x, y); its segments are i = 0 .. M-2 as nearest_point_on_trajectory sees them (the closing
 * segment from the last point back to the first is not searched).  The caller computes the tables on the HOST (NumPy in
 * red_gym_amd/progress.py) and the library uploads them -- the device takes no sqrt of a segment and no atan2:
 *   len[i] = sqrt(dx*dx + dy*dy), cum = [0, cumsum(len)], psi[i] = atan2(dy, dx), lap_length = cum[M-1] + |first - last|.
 * Per car and f110_progress_update, fp64 without contraction, (px, py, yaw) = state[car, (0, 1, 4)]:
 *   1. (seg, t, dist) = the reference's nearest point: first minimum over the segments in ascending order
 *   2. s = cum[seg] + t * len[seg]
 *   3. d = dist with the sign of cross = dx*(py - y0) - dy*(px - x0), >= 0 -> +dist: left of the line is positive
 *   4. heading_error = yaw - psi[seg]; if > pi: -= 2 pi; if <= -pi: += 2 pi (one pass each)
 *   5. the env was reset by the last step that stepped it, or the car has not been seen (seen[car] == 0): delta = 0,
 *      progress = 0; else delta = s - s_prev; if >= L/2: -= L; if < -L/2: += L; progress += delta.  Then s_prev = s, seen = 1.
 *   6. px or py not finite: s, d, heading_error, delta = NaN, seg = 0; progress and s_prev stay (and seen goes to 0 when 5.
 *      asked for a restart, which the next finite pose then takes).
 * "Reset by its last step" is read off the env's clock: f110_buffers.current_time[env] == timestep exactly, which holds
 * after the step that reset the env (f110_reset, masked or not, and autoreset alike) and after no other, since every
 * further step adds the time step.  So the update after the step in which an env reports done still sees the terminal
 * pose and pays that step's delta, and the update after the NEXT step starts the new episode at 0; an env a masked
 * f110_reset left alone is not restarted; two updates without a step between give delta = 0 the second time.
 * f110_progress_install: host arrays; waypoints [total,2] = the K racelines back to back, offsets [K+1] (offsets[0] = 0,
 * offsets[K] = total), len / cum / psi [total] (raceline k's at offsets[k]; the last len / psi entry of a raceline is
 * unused), lap_length [K], raceline_of_env [num_envs] or NULL (all envs on raceline 0).  The handle keeps its OWN device
 * copy of all of it (nothing of the caller's is retained or matched later).  grid != 0 and K == 1 with at most 65 535
 * points: the search runs over the planner's grid of candidate lists (see f110_pure_pursuit_prepare; cell 0.25 m, margin
 * 3 m, same escapes to every segment); otherwise over every segment of the car's raceline -- the same results.
 * Refused with F110_E_INVALID, nothing installed and the previous tracker kept: fewer than 2 points, a zero-length
 * segment, a non-finite coordinate or table entry, a lap length that is not positive, a raceline index outside 0..K-1
 * (f110_progress_validate is that check alone: no handle, no device).  K = 0 or waypoints = NULL removes the tracker.
 * A cold path (allocates, synchronises); install and removal move the launch epoch.
 * f110_progress_bind: the caller-owned outputs, dev, one element per car (N = num_envs * num_agents); progress, s_prev
 * and seen are state carried from update to update (zero them to start; checkpoint them with the step's buffers).
 * f110_progress_update: one kernel on `stream`, no allocation, no synchronisation (capturable behind f110_step).
 * F110_E_INVALID without a tracker, F110_E_UNBOUND before f110_progress_bind or f110_bind. */
typedef struct {
    double *s;             /* [N] arc length of the projection on the car's raceline, 0 .. cum[M-1] */
    double *d;             /* [N] lateral offset, left positive */
    double *heading_error; /* [N] yaw relative to the segment, (-pi, pi] */
    double *delta;         /* [N] metres along the raceline since the previous update (0 at a restart) */
    double *progress;      /* [N] sum of delta since the car's reset */
    double *s_prev;        /* [N] s of the previous update */
    int32_t *seg;          /* [N] nearest segment */
    uint8_t *seen;         /* [N] 1 once the car has been placed */
} f110_progress_buffers;
int f110_progress_validate(const double *waypoints_host, const int32_t *offsets_host, int32_t K, const double *len_host,
                           const double *cum_host, const double *psi_host, const double *lap_length_host,
                           const int32_t *raceline_of_env_host, int32_t num_envs);
int f110_progress_install(f110_handle *h, const double *waypoints_host, const int32_t *offsets_host, int32_t K,
                          const double *len_host, const double *cum_host, const double *psi_host,
                          const double *lap_length_host, const int32_t *raceline_of_env_host, int32_t grid);
int f110_progress_bind(f110_handle *h, const f110_progress_buffers *bufs);
int f110_progress_update(f110_handle *h, void *stream);

/* Reward shaping: per env the three bitmap reward terms of the reference's RL consumer, SACF110Env._calculate_rewards
 * (src/SAL.py:219-250), from the FILL bitmap of the env's PREVIOUS step's scan and the pose the step left.  The reference
 * restated with its quirks; fp64 without contraction.  (x, y) = state[env, agent, (0, 1)], img = bitmap[env] [rows, cols],
 * (x0, y0) = prev_xy[env]:
 *   pixel       px = clip(trunc(origin_x + x * scale), 0, clip_max), py likewise (_world_to_pixel, :139-142; trunc toward
 *               zero like Python's int(); equal to the reference's for every finite x, however large)
 *   collision   collided = 1 if any of the (2n+1)^2 - 1 neighbours (px + dx, py + dy), |dx|, |dy| <= n = neighborhood, the
 *               centre excluded, with 0 <= px + dx < cols and 0 <= py + dy < rows has img[py + dy, px + dx] == 255
 *               (detect_collison, :766-790; with a black-background FILL image 255 is the FILLED region: the reference's
 *               behaviour, kept); collision_term = collided ? w_collision : 0.0
 *   progress    progress_term = sqrt(dx*dx + dy*dy) * w_progress, dx = x - x0, dy = y - y0
 *   centering   car_x = trunc(x), car_y = trunc(y): metres truncated, NOT pixels (the reference's quirk, :239-243).  Outside
 *               the image: reward = -1.  Otherwise left = car_x, walk left while left >= 0 and img[car_y, left] == 255, then
 *               left += 1; right = car_x, walk right while right < cols and img[car_y, right] == 255, then right -= 1;
 *               left >= right (the car's pixel is not 255, or a one-pixel run): reward = -1; else dist = |car_x - (left +
 *               right) / 2.0| and reward = max(0.0, 1.0 - dist / max_lane_halfwidth) (centerline_reward, :879-935);
 *               centering_term = reward * w_centering
 *   total       ((0.0 + progress_term) + collision_term) + centering_term  (sum() over the reference's dict; its lap term
 *               tests a key the env never produces and is not built)
 *   x or y not finite: the four outputs are NaN, collided = 0 and prev_xy[env] stays.
 * Episode logic of f110_shaping_update, read off the env's clock like the progress tracker's: (1) current_time[env] ==
 * timestep exactly (the env was reset by its last step: f110_reset, masked or not, or autoreset): all four outputs 0,
 * collided 0, prev_xy = (x, y) -- the reference's reset() pays nothing and stores the reset pose; idempotent.  (2) else
 * current_time[env] == t_seen[env]: the env has not stepped since its previous update (a masked reset left it alone):
 * nothing of it is written.  (3) else the terms above (t_seen[env] < 0, "no update yet": with (x0, y0) = (x, y)); then
 * prev_xy = (x, y), t_seen = current_time.  The step in which an env reports done is paid with its terminal pose.
 * The caller renders the new scan's bitmap INTO THE SAME buffer after the update, on the same stream.
 * The image is bound in one of two forms, with the same results: bytes (bitmap, f110_bitmap_render's output) or bits (bitmap_bits,
 * f110_bitmap_render_bits' output = the replay ring's frame format: [B, rows, ceil(cols / 64)] uint64, bit k of word w of a row =
 * (pixel[64 w + k] == 255), bits beyond cols 0).  f110_shaping_bind: exactly one of the two is not NULL, else F110_E_INVALID.
 * f110_shaping_validate: host only.  F110_E_INVALID for rows or cols < 1, agent outside 0..num_agents-1, neighborhood < 0,
 * clip_max < 0, a scalar that is not finite, max_lane_halfwidth <= 0.
 * f110_shaping_install: cfg NULL removes the shaper; a refused cfg installs nothing and keeps what was there.  Install and
 * removal move the launch epoch.  f110_shaping_bind: the caller-owned buffers, dev (all required; binding moves the epoch).
 * f110_shaping_update: one kernel on `stream`, no allocation, no synchronisation (capturable behind f110_step).
 * F110_E_INVALID without a shaper, F110_E_UNBOUND before f110_shaping_bind or f110_bind. */
typedef struct {
    int32_t rows, cols;         /* the bitmap's output_image_dims (256, 256) */
    int32_t agent;              /* whose pose is read (0: SAL reads index 0) */
    int32_t neighborhood;       /* n of detect_collison (1) */
    int32_t clip_max;           /* upper clip of _world_to_pixel (255, whatever the image size: the reference's constant) */
    double scale;               /* map_scale, pixels per metre (10.0) */
    double origin_x, origin_y;  /* map_origin (128, 128) */
    double max_lane_halfwidth;  /* centerline_reward's normaliser (50) */
    double w_collision, w_progress, w_centering; /* -100.0, 10.0, 2.0 */
} f110_shaping_config;
typedef struct {
    const uint8_t *bitmap;      /* [B, rows, cols] in: the image of the previous step's scan (NULL: bitmap_bits is bound) */
    double *collision_term;     /* [B] */
    double *progress_term;      /* [B] */
    double *centering_term;     /* [B] */
    double *total;              /* [B] */
    uint8_t *collided;          /* [B] */
    double *prev_xy;            /* [B,2] state: position at the env's previous update */
    double *t_seen;             /* [B] state: current_time at the env's previous update; start at -1 (no clock is negative) */
    const uint64_t *bitmap_bits; /* [B, rows, ceil(cols / 64)] in: the same image as bits, 16-byte aligned (NULL: bitmap is bound) */
} f110_shaping_buffers;
int f110_shaping_validate(const f110_shaping_config *cfg, int32_t num_agents);
int f110_shaping_install(f110_handle *h, const f110_shaping_config *cfg);
int f110_shaping_bind(f110_handle *h, const f110_shaping_buffers *bufs);
int f110_shaping_update(f110_handle *h, void *stream);

/* Path actions: the action side of the reference's RL consumer, SACF110Env.step (src/SAL.py).  Per env, for car `agent`:
 *   decode   compute_vectors_with_angle_clamp (:585-608) on the raw action [16] = 8 rows of 2: rows are normalised by
 *            (norm + 1e-8), row 0 is ignored (the first increment is (1, 0)), each further heading follows the row's atan2
 *            by at most max_diff_deg per row (Python's floor-modulo wrap); _calculate_global_path (:157-181) from the point
 *            car_length ahead of the pose, increments of vector_length rotated by the yaw; that start point is dropped: 8 points.
 *   mpc      MPC_controller (:615-739): chord lengths `dists`, scipy's not-a-knot CubicSpline per coordinate, reference states
 *            ref_traj[i] = (x, y, vx, vy) at s = min(desired_velocity * (i * timestep), dists[7]), i = 0 .. horizon, the
 *            derivative rescaled to desired_velocity (0 where its norm is <= 1e-3), and the FIRST of the reference's QPs (the
 *            only one whose result it uses, :206-207): x_0 = (path[0], vx, vy) -- the path's first point, not the pose --
 *            double integrator, cost sum_{k<horizon} (x_k - ref_k)'Q(x_k - ref_k) + u_k'R u_k + terminal P, -1 <= u <= 1.  Q, R,
 *            P diagonal: one strictly convex box QP per axis, solved exactly by a primal active-set walk over host-built
 *            inverses for every set of free variables (csrc/f110_pathfollow.h).  mpc_accel = u_0 of the two axes.
 *   convert  MPC_converter (:741-764) with current_steer = 0: steer = clip(wrap(atan2(ay, ax)), +-max_steer), speed =
 *            clip(ax, -1, 1), written as (steer, speed) of car `agent`.
 * State: path_points [B,8,2], path_index [B] (< 0: no path) and t_seen [B].  f110_pathfollow_act decodes a new path for the
 * envs with path_index < 0 or >= replan_at (path_replanned = 1, path_index = 0) and computes the action of every env.  The
 * reference waits for index 16 on a path of 8 points and raises IndexError at index 8; replan_at (1..8, default 8) decodes
 * the new path where it would raise.  Its pending_action is never set and is not built.  f110_pathfollow_update, behind the
 * step: _update_path_index (:252-259), path_index += 1 if |pos - path[path_index]| < dist_threshold; episode logic read off
 * the env's clock as for the shaper: current_time == timestep exactly (reset by its last step): path_index = -1; current_time
 * == t_seen (a masked reset left it alone): untouched.
 * f110_pathfollow_validate: host only.  F110_E_INVALID for agent outside 0..num_agents-1, horizon or replan_at outside 1..8,
 * a weight of R <= 0, a weight of Q or P < 0, a scalar that is not finite, vector_length or timestep <= 0, max_diff_deg,
 * max_steer or dist_threshold < 0 (car_length and desired_velocity may be negative).
 * f110_pathfollow_install: cfg NULL removes the follower; a refused cfg installs nothing.  It builds and uploads the QP's
 * tables (cold path, synchronises).  Install, removal and bind move the launch epoch.  _act and _update: one kernel each on
 * `stream`, no allocation, no synchronisation (capturable).  raw_actions dev [B,16]; actions_out dev [B, num_agents, 2]:
 * only car `agent`'s pair is written. */
typedef struct {
    int32_t agent;              /* whose pose is read and whose action is written (0) */
    int32_t replan_at;          /* a new path is decoded at this waypoint index (8) */
    int32_t horizon;            /* horizon_length (5), 1..8 */
    int32_t reserved;
    double car_length, vector_length; /* 0.3, 0.5 */
    double max_diff_deg;        /* 10 */
    double dist_threshold;      /* DIST_THRESHOLD (0.2) */
    double desired_velocity, timestep; /* MPC_PARAMS: 2.0, 0.1 */
    double q[4], r[2], p[4];    /* diagonals of state_cost (1, 1, .1, .1), input_cost (.1, .1), terminal_cost (10, 10, 1, 1) */
    double max_steer;           /* 0.4189 */
} f110_pathfollow_config;
typedef struct {
    double *path_points;        /* [B,8,2] state */
    int32_t *path_index;        /* [B] state; start at -1 */
    uint8_t *path_replanned;    /* [B] the last act decoded a new path */
    double *mpc_accel;          /* [B,2] */
    double *t_seen;             /* [B] state: current_time at the env's previous update; start at -1 */
} f110_pathfollow_buffers;
int f110_pathfollow_validate(const f110_pathfollow_config *cfg, int32_t num_agents);
int f110_pathfollow_install(f110_handle *h, const f110_pathfollow_config *cfg);
int f110_pathfollow_bind(f110_handle *h, const f110_pathfollow_buffers *bufs);
int f110_pathfollow_act(f110_handle *h, const double *raw_actions, double *actions_out, void *stream);
int f110_pathfollow_update(f110_handle *h, void *stream);

/* Replay buffer: the ReplayBuffer of the reference's RL consumer (src/SAL.py:447-463) and the push of its training loop
 * (:996-1001), on the device behind the reward shaper.  A ring of T = steps step slots for all B envs; FIFO by step slot like
 * the reference's deque(maxlen).  Push number c (c = count, an int64 that lives on the device and is advanced by a one-lane
 * kernel behind the push, so that a captured push replays correctly: no slot ever crosses the ABI by value) writes
 *   frame slot c % (T + 1)   the shaper's bitmap as the step left it, bit-packed: a row of cols pixels is words = ceil(cols /
 *                            64) uint64, bit k of word w = (pixel[64 w + k] == 255), tail bits 0 -- np.packbits(row == 255,
 *                            bitorder='little') padded with zeros to 8 * words bytes.  Frames are stored once: T step slots
 *                            own T + 1 frame slots, the transition of push c is (frame c - 1, frame c)
 *   step slot c % T          action = action_in[env] (fp32 [action_dim]), reward = the shaper's total (fp64), done (uint8) and
 *                            valid (uint8); last_valid[env] = the same valid.
 * valid = 0 (never sampled) when (1) current_time[env] == timestep exactly: the step was the env's reset (f110_reset, masked
 * or not, or autoreset) -- terminal frame and spawn frame are no transition; (2) current_time[env] == t_seen[env]: the env was
 * not stepped by the call; (3) c <= chain_start[0]: there is no previous frame (chain_start starts at 0; the caller sets it to
 * count after restoring a checkpoint).  The terminal step itself (done = 1) is valid, its next frame the terminal observation.
 * A transition is named by index = step slot * B + env.
 * f110_replay_validate: host only; `shaping` = the shaper's configuration, NULL = shaping is off.  F110_E_INVALID for shaping
 * off, steps < 2, action_dim < 1, rows or cols above 16384, a ring whose byte sizes overflow.
 * f110_replay_install: behind an installed shaper (whose rows / cols the ring takes); cfg NULL removes it.  An install needs
 * a new f110_replay_bind.  f110_shaping_install(NULL), or one with another image size, removes the buffer too.  Install,
 * removal and bind move the launch epoch.
 * f110_replay_update: the push, two kernels on `stream` behind f110_shaping_update and the render of the new bitmap; no
 * allocation, no synchronisation (capturable).  Behind a shaper bound to bitmap_bits the frame is copied as it is (it is the
 * ring's format); installing the shaper again with the same image size in the other form keeps the buffer.
 * f110_replay_draw: n indices uniform over the valid transitions, no synchronisation.  Attempt k < F110_REPLAY_TRIES of draw j
 * (j counts from first_draw) takes z = splitmix64(seed + 0x9E3779B97F4A7C15 * (1 + j * F110_REPLAY_TRIES + k)) and the candidate
 * mulhi64(z, stored * B), stored = min(count, T); candidate / B = age (0: the newest push), candidate % B = env; the first
 * candidate whose valid is set wins.  None: indices[j] = -1 and ok[j] = 0.
 * f110_replay_gather: for n indices (dev int64) s = frame before, ns = frame after, unpacked to uint8 [n, rows, cols] (as_f32
 * = 0) or to fp32 [n, 1, rows, cols] = pixel * (float)scale; a [n, action_dim] fp32, r [n] fp64, d [n], ok [n] uint8.  An index
 * outside 0 .. T * B - 1 (-1 included) or of an invalid transition yields zeros in every output and ok = 0. */
#define F110_REPLAY_TRIES 64
typedef struct {
    int32_t steps;              /* T: step slots of the ring (capacity in transitions / num_envs), at least 2 */
    int32_t action_dim;         /* values of the stored action (16: SAL's raw action) */
} f110_replay_config;
typedef struct {
    uint64_t *frames;           /* [T + 1, B, rows, words] */
    float *actions;             /* [T, B, action_dim] */
    double *rewards;            /* [T, B] */
    uint8_t *dones;             /* [T, B] */
    uint8_t *valid;             /* [T, B]; start at 0 */
    int64_t *count;             /* [1] pushes made; start at 0 */
    int64_t *chain_start;       /* [1] the push that has no previous frame; start at 0 */
    double *t_seen;             /* [B] current_time at the env's previous push; start at -1 */
    uint8_t *last_valid;        /* [B] valid of the push just made */
    const float *action_in;     /* [B, action_dim] in: what the next push stores */
} f110_replay_buffers;
int f110_replay_validate(const f110_replay_config *cfg, const f110_shaping_config *shaping, int32_t num_envs);
int f110_replay_install(f110_handle *h, const f110_replay_config *cfg);
int f110_replay_bind(f110_handle *h, const f110_replay_buffers *bufs);
int f110_replay_update(f110_handle *h, void *stream);
int f110_replay_draw(f110_handle *h, uint64_t seed, uint64_t first_draw, int32_t n, int64_t *indices, uint8_t *ok, void *stream);
int f110_replay_gather(f110_handle *h, const int64_t *indices, int32_t n, void *s, void *ns, int32_t as_f32, double scale,
                       float *a, double *r, uint8_t *d, uint8_t *ok, void *stream);
/* f110_replay_locate: where the gather would read.  For n indices (dev int64) the rows of the frame tensor, viewed as
 * [(T + 1) * B, rows, words], that hold the transition's frame before (s_frame [n]) and its frame after (ns_frame [n], both dev
 * int64); -1 for both where the gather writes zeros.  It reads count on the device like every replay kernel (capturable). */
int f110_replay_locate(f110_handle *h, const int64_t *indices, int32_t n, int64_t *s_frame, int64_t *ns_frame, void *stream);
/* f110_replay_sample: a whole batch in one kernel from a draw counter that lives on the device, so that a captured sample replays
 * with fresh draws.  counter [1] dev uint64 is the caller's (8-byte aligned; start at 0): draw i of the call is draw number
 * counter[0] + i of the stream `seed`, drawn exactly as f110_replay_draw draws it with first_draw = counter[0]; indices [n] is what
 * that draw gives, s_frame and ns_frame [n] what f110_replay_locate gives for it, a [n, action_dim] fp32, r [n] fp64, d [n] and ok
 * [n] uint8 what f110_replay_gather gives (-1, -1, zeros and ok = 0 where the draw found no valid transition).  A one-lane kernel
 * behind it adds n to the counter: no lane reads a counter that has moved.  All arrays dev; two launches on `stream`, no
 * allocation, no synchronisation.  The handle keeps no draw counter: f110_replay_draw's first_draw stays the caller's host value. */
int f110_replay_sample(f110_handle *h, uint64_t seed, uint64_t *counter, int32_t n, int64_t *indices, int64_t *s_frame, int64_t *ns_frame,
                       float *a, double *r, uint8_t *d, uint8_t *ok, void *stream);
/* N-step returns: the truncated, uncorrected n-step return of a stored transition, walked through the ring on the device (the
 * reference has one-step targets only).  For index = step slot * B + env, c0 is the push f110_replay_locate resolves it to.  The
 * span is the largest m, 1 <= m <= nstep, such that every push c0 .. c0 + m - 1 is stored (c0 + m - 1 <= count - 1; a push after a
 * stored push is still in the ring, newer pushes are overwritten later than older ones), each of them has valid[(c0 + k) % T][env]
 * != 0, and none of c0 .. c0 + m - 2 has done = 1: the walk stops behind a terminal step, in front of an invalid slot (a reset, an
 * env a masked reset left alone, a chain break at chain_start) and at the newest push.  The episode tracker's LIMIT step is stored
 * valid with d = 0 and the reset behind it is invalid, so a span ends ON the LIMIT step and bootstraps from the frame after it.
 * Per row:
 *   ns_frame  the row of the frame tensor, viewed as [(T + 1) * B, rows, words], that holds the frame after push c0 + m - 1:
 *             ((c0 + m - 1) % (T + 1)) * B + env (step slots wrap at T, frame slots at T + 1)
 *   ret       R = r_0; g = gamma; for k = 1 .. m - 1: R = R + g * r_k; g = g * gamma -- fp64, every product and every sum rounded
 *             on its own (no fused multiply-add)
 *   discount  g as it stands behind the loop: gamma for m = 1, gamma^m by running products (not pow) otherwise
 *   d         done of push c0 + m - 1;  span = m (int32)
 * A row the locate refuses (an index outside 0 .. T * B - 1, a slot no push has reached, an invalid transition) is the zero
 * transition: ns_frame = -1, ret = 0, d = 0, span = 0 and discount = gamma; f110_replay_sample_nstep also returns s_frame = -1,
 * a zero action and ok = 0 for it.  With nstep = 1 every output of every row equals f110_replay_locate's / f110_replay_sample's
 * (ret = r), and discount holds gamma's bits in every row.
 * f110_replay_nstep: for n indices the caller names (dev int64), one lane per index; one launch.
 * f110_replay_sample_nstep: f110_replay_sample -- the same draws from the caller's device counter, the same one-lane advance
 * behind it -- with the walk in the same kernel; a captured call replays with fresh draws.  Two launches.
 * Both read count on the device, allocate nothing, do not synchronise and use no atomics; all arrays dev, discount and ret [n]
 * fp64, span [n] int32.  F110_E_INVALID without a launch for nstep outside 1 .. F110_REPLAY_MAX_NSTEP, a gamma that is not
 * finite, n < 0 or a NULL array.  Kernels of their own: the one-step entries above keep their code and bits. */
#define F110_REPLAY_MAX_NSTEP 64
int f110_replay_nstep(f110_handle *h, const int64_t *indices, int32_t n, int32_t nstep, double gamma, int64_t *ns_frame, double *ret, uint8_t *d,
                      double *discount, int32_t *span, void *stream);
int f110_replay_sample_nstep(f110_handle *h, uint64_t seed, uint64_t *counter, int32_t n, int32_t nstep, double gamma, int64_t *indices,
                             int64_t *s_frame, int64_t *ns_frame, float *a, double *ret, uint8_t *d, uint8_t *ok, double *discount, int32_t *span,
                             void *stream);
/* Frame stacks: the last `stack` frames of one env as rows of the frame tensor, walked backwards through the ring on the device
 * (the mirror of the n-step walk; the reference feeds its policy one frame).  No frame is stored twice and none is copied: a
 * stack is `stack` row numbers into the tensor f110_replay_locate's rows point into.
 * Input.  frame_rows[i] is a row of the frame tensor viewed as [(T + 1) * B, rows, words] -- what f110_replay_locate, _sample,
 * _nstep, _sample_nstep and f110_priority_sample write into s_frame / ns_frame: slot = row / B, env = row % B, and the push it stands
 * for is the newest push c <= count - 1 with c % (T + 1) == slot (unique among the T + 1 live frames).  count is read on the device.
 * Link.  Push p of env e links frame p to frame p - 1 iff p >= max(count - T, 0) (its step slot is still the ring's) and
 * valid[p % T][e] != 0 (push 0 has no frame before it and is never valid).
 * Output.  rows_out[i][0] = frame_rows[i]; for j = 1 .. stack - 1, rows_out[i][j] = ((c - j) % (T + 1)) * B + e as long as the
 * pushes c, c - 1, ..., c - j + 1 all link; beyond that the oldest row reached is repeated (Gym's FrameStack: an episode's first
 * observation fills the stack).  depth[i] = the number of distinct frames reached, 1 .. stack.  A row outside 0 .. (T + 1) * B - 1
 * (-1 is the conventional one) or one whose slot no push has written gives -1 in every column and depth = 0.  A stack so ends in
 * front of a reset, at an env a masked reset left alone, at a chain break (chain_start) and at the ring's oldest frame; it never
 * crosses an episode: the terminal step's frame stacks over its episode, the spawn frame behind it over itself.
 * Latest mode.  frame_rows == NULL: n must equal B and row i is env i's newest frame (c = count - 1), the stack a policy acts on;
 * with count = 0 every column is -1 and depth 0.  No host value changes from call to call: a captured call replays correctly.
 * For a one-step transition that the locate accepts, stack(ns_frame)[1:] == stack(s_frame)[:-1] wherever depth(s_frame) = stack.
 * A stack computed at learning time can be shorter than the one the actor saw: only for the stack - 1 oldest pushes of the ring,
 * whose predecessors are overwritten.  depth shows it; nothing corrects it.
 * One launch, one lane per row, at most stack - 1 loads of valid; no atomics, no allocation, no synchronisation.  rows_out [n,
 * stack] dev int64, depth [n] dev int32.  F110_E_INVALID without a launch for stack outside 1 .. F110_REPLAY_MAX_STACK, n < 0,
 * latest mode with n != B, a NULL output, no bound ring and the wrong device, as f110_replay_nstep refuses it.  stack = 1 copies
 * the rows (only the range checks apply). */
#define F110_REPLAY_MAX_STACK 8
int f110_replay_stack(f110_handle *h, const int64_t *frame_rows, int32_t n, int32_t stack, int64_t *rows_out, int32_t *depth, void *stream);

/* Prioritized replay (Schaul et al., "Prioritized Experience Replay"; the reference draws uniformly): an exact integer sum tree over
 * the ring's transitions, on the device, opt-in.  Without f110_priority_install nothing here launches and f110_replay_update's launch
 * sequence is unchanged.
 * The tree.  Leaves: uint32 leaf[L], L = T * B, leaf position = the transition index step slot * B + env; 0 = never drawn.  Above them
 * levels of fanout 64 (a wave): level 1 has ceil(L / 64) uint64 nodes, level k + 1 has ceil(count_k / 64), until a level has at most
 * 64 nodes: the top.  No root is stored; the total is the sum of the top level, formed by the wave that needs it.  With L <= 64 there
 * is no node and the leaves are the top.  All nodes live in one array uint64 node[f110_priority_node_words(L)], level 1 first (-1 for
 * an L outside 1 .. F110_PRIORITY_MAX_LEAVES).  After every entry point below has run, every node equals the sum of its (up to 64)
 * children.  Words are integers and sums are exact, so the result of every entry is the same in every run and in any order of rows;
 * the integer atomics used by the set do not change that.
 * A word: q = clamp(llrint(p * 2^F110_PRIORITY_SHIFT), 1, 2^32 - 1) with p = pow(double(td) + eps, exponent), one fp64 pow of the
 * device library (`exponent` is PER's alpha; the name keeps it apart from SAC's temperature); a td that is NaN or +inf gives 2^32 - 1.
 * At exponent == 1 p is the sum double(td) + eps itself, without the pow (the library's is within an ulp, not exact there), so the word
 * is rint((td + eps) * 2^16) exactly, ties to even.
 * State: f110_priority_state, 64 bytes on the device, the caller's: qmax (the word a new transition enters with; start at 1 <<
 * F110_PRIORITY_SHIFT = priority 1.0), beta, beta_step, beta_end (fp64), reserved words 0.
 * Stateless entries (leaf, node dev; no handle, no allocation, no synchronisation, capturable):
 * f110_ptree_rebuild: every level from the leaves, one launch per level.
 * f110_ptree_set: leaf[idx[i]] = q[i] for the rows with 0 <= idx[i] < L (others are skipped); where several rows name one leaf it
 *   becomes the MAXIMUM of their q; every ancestor is fixed.  Two launches whatever L: the first takes the old word out of each named
 *   leaf (atomicExch to 0; the lane that got it subtracts it from every ancestor with 64-bit atomicAdd), the second raises the leaf
 *   (atomicMax; a lane that raised it adds the difference to every ancestor, and the raises of one leaf telescope to its final word).
 * f110_ptree_pick: n draws, one wave each.  Draw j (counted from first_draw) takes z = splitmix64(seed + 0x9E3779B97F4A7C15 * (1 + j *
 *   F110_REPLAY_TRIES)) -- attempt 0 of f110_replay_draw's draw j -- and u = mulhi64(z, total).  From the top level down the lanes load
 *   the current node's children (0 beyond the end), form the inclusive prefix sum across lanes, the first child whose prefix exceeds u is
 *   taken, its exclusive prefix is subtracted from u.  At the leaves this gives idx_out[j] and q_out[j] = leaf[idx] > 0; total == 0 gives
 *   -1 and 0.  The result equals searchsorted(cumsum(leaf), u, 'right') over the flat leaves.
 * On the handle, behind an installed and bound replay ring (L = T * B):
 * f110_priority_install: cfg = {exponent in [0, 8], eps >= 0 and finite}; NULL removes the feature.  f110_priority_bind: leaf [L]
 *   uint32, node [f110_priority_node_words(L)] uint64 (may be NULL while that is 0), state (8-byte aligned).  f110_replay_install
 *   (removal included) removes the priorities too.  Install, removal and bind move the launch epoch.
 * f110_priority_reset: leaf = valid[index] ? qmax : 0 for every index, then the rebuild.
 * f110_replay_update, while priorities are bound: between the push and the advance of count (so it reads the same count) the row of
 *   step slot count % T gets leaf = valid ? qmax : 0 and every node whose children changed is recomputed -- one launch of one wave per
 *   level-1 node the row touches (with B % 64 != 0 the row shares its first or last one with the neighbouring rows), and with more
 *   than one level one launch of one workgroup for the levels above.  Captured with the push.
 * f110_priority_sample: f110_replay_sample_nstep with f110_ptree_pick's draw (first_draw = counter[0]) in place of the uniform one:
 *   for the indices it returns every ring output is what f110_replay_nstep / f110_replay_locate give (nstep = 1: the one-step values);
 *   prio [n] uint32 = the drawn leaf's word.  A second launch of one workgroup forms qmin = the minimum of prio over the rows with ok
 *   and weight[i] = ok ? float(pow(double(qmin) / double(prio[i]), beta)) : 0, then adds n to the counter and sets beta = min(beta_end,
 *   beta + beta_step).  That is the importance weight (N * P(i))^-beta divided by the batch's maximum: P(i) = prio[i] / total, so N and
 *   the total cancel in the ratio.  The weights use the beta read before its advance; rows with prio == qmin are exactly 1.0f and beta
 *   = 0 gives all ones.  Two launches.
 * f110_priority_update: q = the word of td[i] (above) for the rows with ok[i], an index inside the ring and valid[idx] != 0, applied
 *   with f110_ptree_set's rule; other rows are skipped and have q_out = 0 (q_out may be NULL).  qmax is raised to the largest q
 *   applied.  f110_priority_set: the same with the words given (for tests and for loading).  Two launches each.
 * F110_E_INVALID before any launch, naming the culprit: a NULL array, n < 0, a misaligned counter or state, exponent outside [0, 8],
 * eps negative or not finite, L outside its limits, and the wrong device as f110_replay_update refuses it. */
#define F110_PRIORITY_SHIFT 16
#define F110_PRIORITY_MAX_LEAVES (1ll << 31)
#define F110_PRIORITY_STATE_BYTES 64
typedef struct f110_priority_config {
    double exponent;            /* PER's alpha: priority = (|td| + eps)^exponent */
    double eps;
} f110_priority_config;
typedef struct f110_priority_state { /* on the device; 64 bytes */
    uint32_t qmax;              /* the word of a new transition */
    uint32_t reserved0;
    double beta, beta_step, beta_end;
    uint64_t reserved[4];
} f110_priority_state;
typedef struct f110_priority_buffers {
    uint32_t *leaf;             /* [T * B] */
    uint64_t *node;             /* [f110_priority_node_words(T * B)] */
    f110_priority_state *state;
} f110_priority_buffers;
int64_t f110_priority_node_words(int64_t L);
int f110_ptree_rebuild(const uint32_t *leaf, uint64_t *node, int64_t L, void *stream);
int f110_ptree_set(uint32_t *leaf, uint64_t *node, int64_t L, const int64_t *idx, const uint32_t *q, int32_t n, void *stream);
int f110_ptree_pick(const uint32_t *leaf, const uint64_t *node, int64_t L, uint64_t seed, uint64_t first_draw, int32_t n, int64_t *idx_out,
                    uint32_t *q_out, void *stream);
int f110_priority_install(f110_handle *h, const f110_priority_config *cfg);
int f110_priority_bind(f110_handle *h, const f110_priority_buffers *bufs);
int f110_priority_reset(f110_handle *h, void *stream);
int f110_priority_sample(f110_handle *h, uint64_t seed, uint64_t *counter, int32_t n, int32_t nstep, double gamma, int64_t *indices,
                         int64_t *s_frame, int64_t *ns_frame, float *a, double *ret, uint8_t *d, uint8_t *ok, double *discount, int32_t *span,
                         uint32_t *prio, float *weight, void *stream);
int f110_priority_update(f110_handle *h, const int64_t *idx, const uint8_t *ok, const float *td, int32_t n, uint32_t *q_out, void *stream);
int f110_priority_set(f110_handle *h, const int64_t *idx, const uint32_t *q, int32_t n, void *stream);

/* Episodes: the episode of the reference's training loop (src/SAL.py:986-1015: `obs = env.reset(); ep_reward = 0; for st in
 * range(max_steps): ...; ep_reward += reward; if done: break; print(f"Episode {ep} Reward={ep_reward:.2f}")`) for every env, on
 * the device behind the step: the return and the length of the running episode, a step limit per env, and a log of the finished
 * episodes.  State per env: ep_return (fp64), ep_length, ep_open, t_seen, truncated; limit[env] is the env's step limit (0: none,
 * statistics only).  The rules, read off the env's clock as the shaper's are (now = current_time[env]):
 *   (2) now == t_seen[env]: the env was not stepped since its previous update (a masked reset left it alone): nothing of it is
 *       written -- the update is idempotent.  Else
 *   (1) now == timestep exactly: the last step was the env's reset (f110_reset, masked or not, or autoreset), the reference's
 *       env.reset().  If the episode was still open and ep_length > 0 -- a masked reset cut it -- it is closed with reason RESET
 *       (its record holds the accumulators as they stood; time and laps are those of the reset step).  Then ep_return = 0,
 *       ep_length = 0, ep_open = 1, truncated = 0: the reset step pays nothing and counts no step.  Else
 *   (3) ep_open: ep_return = ep_return + reward[env] (a plain fp64 add in step order), ep_length += 1; reward is the shaper's total
 *       while a shaper is installed and bound, else the constant `timestep`.  If done[env]: closed with reason DONE; else if
 *       limit[env] > 0 and ep_length >= limit[env]: closed with reason LIMIT, truncated = 1, and, if the handle runs with autoreset,
 *       pending_reset[env] = 1 -- the flag the step raises on done: the next step respawns the env at its spawn pose and every
 *       other consumer sees an ordinary reset.  done is never written; with autoreset off only the flag `truncated` is raised and
 *       the env keeps stepping.  A closed episode has ep_open = 0.  Else
 *   (4) a step of a closed episode (autoreset off): the accumulators stay frozen, no second record, until the reset.
 *   In cases (1), (3) and (4) t_seen = now.
 * Closing appends one record {env, length, return, reason, time = now, laps = lap_counts of the ego} to a ring of L = cfg.log
 * records kept as separate arrays.  count [1] (int64, on the device) holds the episodes closed so far; record k of the run lives
 * in slot k % L, and the records of one update appear in ascending env order (a compaction by wave ballots, LDS and per-workgroup
 * counts: no atomics, the same slots in every run).  If more than L episodes close in one update only the last L in env order are
 * written, each to its own slot; count advances by all of them, in a one-wave kernel behind the writes, so that a captured update
 * replays with fresh slots.
 * f110_episodes_validate: host only.  F110_E_INVALID for limit < 0 and for log outside 1..2^24.
 * f110_episodes_install: cfg NULL removes the tracker; a refused cfg installs nothing and keeps what was there.  Install, removal and
 * bind move the launch epoch.  f110_episodes_bind: the caller-owned arrays, dev; all required but `limit` (NULL: cfg.limit for every
 * env).  Start with ep_open = 1, t_seen = -1 and zeros elsewhere.  block_counts is scratch of ceil(B / F110_EPISODES_BLOCK) int32.
 * f110_episodes_update: three kernels on `stream`, no allocation, no synchronisation (capturable behind f110_step and the other
 * consumers' updates: it reads the shaper's total, and the replay push in front of it sees pending_reset as the step left it).
 * F110_E_INVALID without a tracker, F110_E_UNBOUND before f110_episodes_bind or f110_bind.
 * f110_episodes_apply: the same kernels on caller-supplied arrays, no handle: n envs (n = 0: nothing is launched), reward [n] or NULL
 * (= timestep), done [n], current_time [n], laps NULL (0 is logged) or the laps of env e at laps[e * laps_stride], pending_reset [n]
 * or NULL (autoreset off); bufs as for the bind, with block_counts of ceil(n / F110_EPISODES_BLOCK) int32.  All arrays dev; launches on the calling
 * thread's current device.  F110_E_INVALID for a NULL cfg, bufs or required array, a refused cfg, n < 0, timestep <= 0. */
#define F110_EPISODE_DONE 1  /* the env reported done */
#define F110_EPISODE_LIMIT 2 /* the step limit was reached (truncated) */
#define F110_EPISODE_RESET 3 /* a reset cut the running episode */
#define F110_EPISODES_BLOCK 256 /* envs per entry of block_counts (the kernels' workgroup size) */
typedef struct {
    int32_t limit;              /* the step limit of every env while no limit array is bound (2000: the reference's max_steps); 0: none */
    int32_t log;                /* L: records the log holds, 1..2^24 */
} f110_episodes_config;
typedef struct {
    double *ep_return;          /* [B] state: the running episode's return */
    int32_t *ep_length;         /* [B] state: its steps */
    uint8_t *ep_open;           /* [B] state: 1 while it runs; start at 1 */
    double *t_seen;             /* [B] state: current_time at the env's previous update; start at -1 */
    uint8_t *truncated;         /* [B] state: 1 from the step that hit the limit until the env's reset */
    const int32_t *limit;       /* [B] in: the step limit of every env, or NULL */
    int32_t *log_env;           /* [L] */
    int32_t *log_length;        /* [L] */
    double *log_return;         /* [L] */
    uint8_t *log_reason;        /* [L] F110_EPISODE_* */
    double *log_time;           /* [L] */
    int32_t *log_laps;          /* [L] */
    int64_t *count;             /* [1] episodes closed; start at 0 */
    int32_t *block_counts;      /* [ceil(B / F110_EPISODES_BLOCK)] scratch */
} f110_episodes_buffers;
int f110_episodes_validate(const f110_episodes_config *cfg);
int f110_episodes_install(f110_handle *h, const f110_episodes_config *cfg);
int f110_episodes_bind(f110_handle *h, const f110_episodes_buffers *bufs);
int f110_episodes_update(f110_handle *h, void *stream);
int f110_episodes_apply(const f110_episodes_config *cfg, int32_t n, double timestep, const double *reward, const uint8_t *done,
                        const double *current_time, const int32_t *laps, int64_t laps_stride, uint8_t *pending_reset,
                        const f110_episodes_buffers *bufs, void *stream);

/* First convolution of the policy from bits: the nn.Conv2d(1, C, kernel, stride) that opens the reference's Actor and Critic
 * (src/SAL.py:397, 429) on an image of two values, forward and backward, stateless (no handle; cfg host; all arrays dev; launches
 * on the calling thread's current device, no allocation, no synchronisation).  `on` is what a set pixel is worth: 1 for
 * FloatTensor(state) / 255 (:510), 255 for the raw images of update() (:536).  Output size as nn.Conv2d without padding: OH =
 * (rows - kernel) / stride + 1, OW likewise.
 * frames: [n_frames, rows, ceil(cols / 64)] uint64 in the replay ring's format (bit k of word w = pixel 64 w + k), 8-byte
 * aligned; the _u8 entry reads uint8 images [n_frames, rows, cols] instead, a pixel set iff it == 255, thresholded on the fly.
 * index: NULL (sample i reads frame i; n <= n_frames) or dev int64 [n]: the frame of sample i; an entry outside 0 .. n_frames
 * - 1 (-1 is the conventional one) reads a frame of zeros and is never dereferenced; repeats are allowed.
 * weight [channels, 1, kernel, kernel] fp32 (finite), bias [channels] fp32 or NULL (= zeros), out [n, channels, OH, OW] fp32.
 * Numerics, in fp32: acc = 0; for the taps ky major, kx minor: acc = acc + w[c][ky][kx] if the tap's pixel is set; out = (acc *
 * on) + bias[c], two roundings; then out < 0 ? 0 : out if relu.  The output is a function of the bits alone.
 * f110_bitconv_backward: from grad_out [n, channels, OH, OW] fp32 and the same frames / index, grad_weight[c][ky][kx] = on *
 * sum over samples and outputs of grad_out * bit and grad_bias[c] = sum of grad_out (NULL: skipped); fp32 sums in an order fixed
 * by the shape and n (no atomics: two calls give the same bits), through `workspace` (16-byte aligned) of
 * f110_bitconv_workspace bytes (0 for an invalid configuration or n < 1).  With relu the caller has already zeroed grad_out
 * where out is 0.  There is no gradient with respect to the image.
 * f110_bitconv_validate: host only.  F110_E_INVALID for kernel outside 1..8 (a window is one 64-bit mask), stride outside
 * 1..kernel, channels outside 1..64, rows or cols below kernel or above 16384, a non-finite `on`. */
typedef struct {
    int32_t rows, cols;         /* the image */
    int32_t kernel, stride;     /* square window, 1..8; stride 1..kernel */
    int32_t channels;           /* output channels, 1..64 */
    int32_t relu;               /* nonzero: max(out, 0) */
    float on;                   /* the value of a set pixel */
} f110_bitconv_config;
int f110_bitconv_validate(const f110_bitconv_config *cfg);
int64_t f110_bitconv_workspace(const f110_bitconv_config *cfg, int64_t n);
int f110_bitconv_forward(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                         const float *weight, const float *bias, float *out, void *stream);
int f110_bitconv_forward_u8(const f110_bitconv_config *cfg, const uint8_t *images, int64_t n_frames, const int64_t *index, int64_t n,
                            const float *weight, const float *bias, float *out, void *stream);
int f110_bitconv_backward(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                          const float *grad_out, float *grad_weight, float *grad_bias, float *workspace, void *stream);
/* The same layer on a stack of frames: nn.Conv2d(stack, C, kernel, stride) whose input channels are `stack` frames of the frame
 * tensor (f110_replay_stack's rows), still from bits.  cfg is f110_bitconv_config unchanged; frames is the packed form only (there
 * is no _u8 entry); index [n, stack] dev int64 is required: channel j of sample i is frame index[i][j], an entry outside 0 ..
 * n_frames - 1 reads a frame of zeros, repeats are allowed.  weight and grad_weight are [channels, stack, kernel, kernel].
 * Forward numerics, in fp32: acc = 0; for the frames j major, then ky, then kx minor: acc = acc + w[c][j][ky][kx] if that tap of
 * frame index[i][j] is set; out = (acc * on) + bias[c]; then the relu.  With stack = 1 this is f110_bitconv_forward's contract, so
 * its bits.  One launch per group of samples, as f110_bitconv_forward.
 * f110_bitconv_backward_stack: grad_weight[:, j] is, bit for bit, what f110_bitconv_backward returns for the index column
 * index[:, j], and grad_bias its grad_bias -- that fixes every summation order.  It is built as a loop over the columns on
 * f110_bitconv_backward's own kernels: one launch that transposes the index into the workspace, then per column the partial sums
 * and a reduction that writes with the [channels, stack, kernel, kernel] stride (1 + 2 * stack launches; grad_out is read once per
 * column).  workspace: 16-byte aligned, f110_bitconv_workspace_stack bytes (0 for an invalid configuration, a stack outside its
 * range or n < 1).  No allocation, no synchronisation, no atomics.
 * F110_E_INVALID for stack outside 1 .. F110_BITCONV_MAX_STACK, a NULL index and whatever f110_bitconv_validate and the one-frame
 * entries refuse. */
#define F110_BITCONV_MAX_STACK 8
int f110_bitconv_forward_stack(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                               int64_t n, const float *weight, const float *bias, float *out, void *stream);
int64_t f110_bitconv_workspace_stack(const f110_bitconv_config *cfg, int32_t stack, int64_t n);
int f110_bitconv_backward_stack(const f110_bitconv_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                                int64_t n, const float *grad_out, float *grad_weight, float *grad_bias, float *workspace, void *stream);

/* Policy stem for acting: relu(conv2(relu(conv1(x)))) of the reference's Actor and Critic (src/SAL.py:397-398, 405-406, 429-430,
 * 436-437; conv2 = nn.Conv2d(16, 32, kernel_size=4, stride=2)) from bits in one kernel.  The first layer's activations never
 * reach memory: `out` [n, channels2, OH2, OW2] fp32 is all that is written, OH2 = (OH1 - kernel2) / stride2 + 1 on the first
 * layer's OH1 = (rows - kernel) / stride + 1, OW2 likewise.  Stateless, forward only (learning keeps f110_bitconv_forward and
 * _backward with the framework's second layer); cfg host, all arrays dev; launches on `stream` of the calling thread's current
 * device, no allocation, no synchronisation, no atomics.  frames / images / index / n_frames / n as for f110_bitconv_forward and
 * f110_bitconv_forward_u8; w1 [channels, 1, kernel, kernel], b1 [channels] or NULL, w2 [channels2, channels, kernel2, kernel2],
 * b2 [channels2] or NULL, all fp32 and finite.  F110_E_INVALID for a null frames, w1, w2 or out with n > 0; n == 0 does nothing.
 * Numerics.  Layer 1 is the contract of f110_bitconv_forward unchanged, with `on`, b1 (or NULL) and `relu`; call its result a1
 * [channels, OH1, OW1].  Layer 2 in fp32: acc = 0; for ci major, then ky, then kx minor: acc = fmaf(w2[co][ci][ky][kx],
 * a1[ci][stride2 oy + ky][stride2 ox + kx], acc), one rounding per step; out = acc + b2[co] (+ 0.0f for NULL); then out < 0 ? 0
 * : out if relu2.  The output is a function of the bits and the four parameter tensors alone: two calls give the same bits, and
 * a sample's result depends neither on n nor on its place in the batch.
 * f110_bitconv2_validate: host only.  F110_E_INVALID for what f110_bitconv_validate refuses in the first layer's fields, for
 * channels outside 1..16, kernel2 outside 1..4, stride2 outside 1..kernel2, channels2 outside 1..64, for OH1 or OW1 below
 * kernel2, and for a first layer's output wider than 64 (OW1 > 64: the kernel works on whole rows of it and has no halo in x;
 * any number of rows is accepted).
 * f110_bitconv2_forward_stack: the stem on a stack of frames, for acting with f110_replay_stack's rows: the composition of the two
 * contracts above.  Layer 1 is the contract of f110_bitconv_forward_stack unchanged (packed frames only, there is no _u8 entry;
 * index [n, stack] dev int64 is required, an entry outside 0 .. n_frames - 1 reads a frame of zeros, repeats are allowed; w1
 * [channels, stack, kernel, kernel]; acc = 0; for the frames j major, then ky, then kx minor: acc = fmaf(w1[c][j][ky][kx], bit ? 1.0f
 * : 0.0f, acc); a1 = (acc * on) + b1[c] (+ 0.0f for NULL), then the relu -- `on`, the bias and the relu once, after the last frame);
 * layer 2 is the contract of f110_bitconv2_forward on that a1.  So its output is, bit for bit, f110_bitconv2_forward's layer 2 on
 * f110_bitconv_forward_stack's output, and with stack = 1 f110_bitconv2_forward's own.  One kernel, one launch for any n; the first
 * layer's activations and the running sums over the frames live in LDS; the launch geometry does not depend on `stack`.
 * F110_E_INVALID for stack outside 1 .. F110_BITCONV_MAX_STACK, a NULL index, n < 1, a null frames, w1, w2 or out, and whatever
 * f110_bitconv2_validate refuses: every configuration it accepts is accepted at every stack. */
typedef struct {
    int32_t rows, cols;         /* the image */
    int32_t kernel, stride;     /* layer 1, as f110_bitconv_config */
    int32_t channels;           /* layer 1 output channels, 1..16 */
    int32_t relu;               /* between the layers */
    float on;                   /* the value of a set pixel */
    int32_t kernel2, stride2;   /* layer 2: kernel2 1..4, stride2 1..kernel2 */
    int32_t channels2;          /* 1..64 */
    int32_t relu2;              /* nonzero: max(out, 0) */
} f110_bitconv2_config;
int f110_bitconv2_validate(const f110_bitconv2_config *cfg);
int f110_bitconv2_forward(const f110_bitconv2_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int64_t n,
                          const float *w1, const float *b1, const float *w2, const float *b2, float *out, void *stream);
int f110_bitconv2_forward_u8(const f110_bitconv2_config *cfg, const uint8_t *images, int64_t n_frames, const int64_t *index, int64_t n,
                             const float *w1, const float *b1, const float *w2, const float *b2, float *out, void *stream);
int f110_bitconv2_forward_stack(const f110_bitconv2_config *cfg, const uint64_t *frames, int64_t n_frames, const int64_t *index, int32_t stack,
                                int64_t n, const float *w1, const float *b1, const float *w2, const float *b2, float *out, void *stream);

/* Dense convolution of fp32 feature maps, forward and backward: conv2 = nn.Conv2d(16, 32, 4, 2) and conv3 = nn.Conv2d(32, 32, 3, 1)
 * of the reference's Actor and Critic (src/SAL.py:398-399, 406-407, 430-431, 437-438) with their ReLU, on the fp32 matrix cores.
 * Stateless (no handle; cfg host; all arrays dev); launches on `stream` of the calling thread's current device, no allocation, no
 * synchronisation, no atomics.  x [n, in_channels, rows, cols] fp32 NCHW contiguous, weight [out_channels, in_channels, kernel,
 * kernel] fp32 (finite), bias [out_channels] fp32 or NULL (= zeros), out [n, out_channels, OH, OW] fp32 with OH = (rows - kernel) /
 * stride + 1, OW likewise: square kernel and stride, no padding, no dilation, no groups.  n == 0 does nothing.
 * Numerics, forward, in fp32 (the contract of f110_bitconv2's second layer): acc = 0; for ci major, then ky, then kx minor: acc =
 * fmaf(weight[co][ci][ky][kx], x[ci][stride oy + ky][stride ox + kx], acc), one rounding per step; out = acc + bias[co] (+ 0.0f for
 * NULL); then out < 0 ? 0 : out if relu.  Two calls give the same bits, and a sample's result depends neither on n nor on its place
 * in the batch.
 * f110_featconv_backward: from x, out (the forward's result, read only where relu is set, for the mask), grad_out [n, out_channels,
 * OH, OW] and weight; each of grad_x [n, in_channels, rows, cols] and the pair grad_weight [as weight] / grad_bias [out_channels]
 * may be NULL and is then skipped (grad_bias alone may be NULL too).  With g = out > 0 ? grad_out : 0 under relu, else g = grad_out:
 *   grad_x[n][ci][iy][ix]: acc = 0; for co major, then ky, then kx minor: acc = fmaf(weight[co][ci][ky][kx], g[n][co][(iy - ky) /
 *   stride][(ix - kx) / stride], acc) over the terms whose output pixel exists (divisible by stride, inside the plane); a missing
 *   term is fed as fmaf(w, 0, acc), which for finite weights leaves acc (never -0) unchanged.
 *   grad_weight in two stages.  Stage 1, per sample: P[n][co][ci][ky][kx]: acc = 0; for oy major, ox minor: acc = fmaf(g[n][co][oy]
 *   [ox], x[n][ci][stride oy + ky][stride ox + kx], acc).  Stage 2: grad_weight = ((P[0] + P[1]) + P[2]) + ..., plain fp32 adds,
 *   samples ascending.  grad_bias: the same two stages with acc = acc + g[n][co][oy][ox] from 0.
 * The order depends on the shape and n alone, never on the grid or on timing: two calls give the same bits, and a sample's grad_x
 * and partials do not depend on the batch around it.  P lives in `workspace` (16-byte aligned, required with grad_weight or
 * grad_bias) of f110_featconv_workspace bytes = n * out_channels * (in_channels * kernel^2 + 1) * 4 (0 for an invalid configuration,
 * for n < 1 and where the count does not fit int64): per sample out_channels * in_channels * kernel^2 weight partials, then out_channels bias partials.  That is 2.4 MB for
 * conv3 at a batch of 64 and 151 MB at 4 096 rows.
 * f110_featconv_validate: host only.  F110_E_INVALID for kernel outside 1..4, stride outside 1..4, in_channels outside 1..32,
 * out_channels outside 1..64, in_channels * kernel^2 or out_channels * kernel^2 above 512, rows below kernel, cols below kernel or
 * above 64 (the kernels work on whole rows and have no halo in x; any number of rows is accepted). */
typedef struct {
    int32_t in_channels;        /* 1..32 */
    int32_t rows, cols;         /* the input planes; cols <= 64 */
    int32_t out_channels;       /* 1..64 */
    int32_t kernel, stride;     /* square window 1..4, stride 1..4 */
    int32_t relu;               /* nonzero: max(out, 0), and its mask in the backward */
    int32_t reserved;           /* 0 */
} f110_featconv_config;
int f110_featconv_validate(const f110_featconv_config *cfg);
int64_t f110_featconv_workspace(const f110_featconv_config *cfg, int64_t n);
int f110_featconv_forward(const f110_featconv_config *cfg, const float *x, int64_t n, const float *weight, const float *bias, float *out,
                          void *stream);
int f110_featconv_backward(const f110_featconv_config *cfg, const float *x, const float *out, const float *grad_out, int64_t n,
                           const float *weight, float *grad_x, float *grad_weight, float *grad_bias, float *workspace, void *stream);

/* Dense layer of fp32 features, forward and backward: fc1 = nn.Linear(32 * 28 * 28, 512) of the reference's Actor and the feature
 * columns of nn.Linear(32 * 28 * 28 + 16, 512) of its Critic (src/SAL.py:400, 408, 432, 440) with their ReLU, on the fp32 matrix
 * cores.  Stateless (no handle; cfg host; all arrays dev); launches on `stream` of the calling thread's current device, no
 * allocation, no synchronisation, no atomics.  x [n, K] fp32 contiguous (K = in_features), weight [H, K] fp32 (H = out_features)
 * whose rows lie ld >= K elements apart -- a column view of a wider matrix, such as the feature columns of the critics' [H, F + A]
 * weight; neither its base nor its rows need be 16-byte aligned -- bias [H] fp32 or NULL (= zeros), out [n, H] fp32.  n == 0 does
 * nothing; F110_E_INVALID, not a launch, for n outside 0 .. 2^24, for a null required pointer with n > 0, for what
 * f110_dense_validate refuses, and for a wrong device as f110_featconv_forward refuses it.
 * Numerics, forward, in fp32.  K is cut into segments j = 0 .. ceil(K / S) - 1 of S = segment consecutive k's (the last may be
 * shorter).  Per segment: acc_j = 0; for k ascending in the segment: acc_j = fmaf(x[r][k], weight[h][k], acc_j), one rounding per
 * step.  Then sum = acc_0; sum = sum + acc_j for j ascending, plain fp32 adds.  Then out = sum + bias[h] (+ 0.0f for NULL); then
 * out < 0 ? 0 : out if relu.  (A step padded to a multiple of 4 feeds 0 * 0, which leaves the never negative-zero acc as it is.)
 * S belongs to the configuration, not to the launch: a row's result depends on x[r], the parameters and S alone -- not on n, on the
 * row's place in the batch or on the grid -- and two calls give the same bits.  The launch plan either gives every segment a
 * workgroup of its own, which writes acc_j to `workspace`, and adds them in a second kernel (small n), or lets one workgroup walk
 * the segments and add in registers (large n); both give the same bits.  f110_dense_workspace: the bytes the FORWARD needs for n
 * rows: ceil(K / S) * n * H * 4 on the first path, 0 on the second (then `workspace` may be NULL), 0 for an invalid configuration
 * and for n outside 1 .. 2^24.  The first path is taken where K has more than one segment and ceil(n / 32) * ceil(H / 64) < 256.
 * The workspace's contents before the call do not matter.
 * f110_dense_backward: from x, out (the forward's result, read only where relu is set, for the mask), grad_out [n, H] and weight;
 * each of grad_x [n, K], grad_weight [H, K] with the row stride ld (the elements between the rows are not touched) and grad_bias
 * [H] may be NULL and is then skipped.  x is read only for grad_weight, weight only for grad_x.  With g = out > 0 ? grad_out : 0
 * under relu, else g = grad_out:
 *   grad_x[r][k]: acc = 0; for h ascending: acc = fmaf(g[r][h], weight[h][k], acc).
 *   grad_weight[h][k]: acc = 0; for r ascending: acc = fmaf(g[r][h], x[r][k], acc).
 *   grad_bias[h]: acc = 0; for r ascending: acc = acc + g[r][h].
 * No workspace, no atomics: the order depends on the shape and n alone, two calls give the same bits, and a row's grad_x does not
 * depend on the batch around it.
 * f110_dense_validate: host only.  F110_E_INVALID for in_features outside 1 .. 2^20, out_features outside 1 .. 4096, ld below
 * in_features, segment not a multiple of 4 in 4 .. 4096, and reserved other than 0. */
typedef struct {
    int32_t in_features;        /* K, 1 .. 2^20 */
    int32_t out_features;       /* H, 1 .. 4096 */
    int32_t ld;                 /* row stride of weight AND grad_weight in elements, >= K */
    int32_t segment;            /* S: k's per chain, a multiple of 4 in 4 .. 4096 */
    int32_t relu;               /* nonzero: max(out, 0), and its mask in the backward */
    int32_t reserved;           /* 0 */
} f110_dense_config;
int f110_dense_validate(const f110_dense_config *cfg);
int64_t f110_dense_workspace(const f110_dense_config *cfg, int64_t n);
int f110_dense_forward(const f110_dense_config *cfg, const float *x, int64_t n, const float *weight, const float *bias, float *out,
                       float *workspace, void *stream);
int f110_dense_backward(const f110_dense_config *cfg, const float *x, const float *out, const float *grad_out, int64_t n,
                        const float *weight, float *grad_x, float *grad_weight, float *grad_bias, void *stream);

/* Policy head: the end of the reference's Actor.forward and Actor.sample (src/SAL.py:410-421) -- fc_mean and fc_log_std on the
 * features h of fc1, clamp(-20, 2), exp, rsample, tanh and the squashed-Gaussian log_prob summed over the action -- forward in one
 * kernel, and a backward without atomics.  Stateless (no handle; cfg host; all arrays dev); launches on `stream` of the calling
 * thread's current device, no allocation, no synchronisation.
 * h [n, K] fp32 (K = in_features), w_mean [A, K], b_mean [A] or NULL, w_log_std [A, K], b_log_std [A] or NULL (A = action_dim),
 * eps [n, A] fp32 (the standard normal draws of rsample) or NULL (the reference's evaluate=True).
 * Outputs: pre [n, 2A] fp32, required (columns 0 .. A - 1 the mean's pre-activations, A .. 2A - 1 the log_std's before the clamp);
 * action [n, A] and log_prob [n], fp64 when out_fp64 is nonzero, else fp32, rounded once.  log_prob must be NULL exactly when eps
 * is NULL.  n == 0 does nothing; F110_E_INVALID, not a launch, for a null h, w_mean, w_log_std, pre or action with n > 0, for n
 * outside 0 .. 2^24, for what f110_policyhead_validate refuses, and for a wrong device: a required pointer that is not memory of the
 * calling thread's current device (host memory included), or a non-null `stream` of another device (both entry points).
 * Numerics.  Pre-activations in fp32, bit for bit: for row j of w_mean, then of w_log_std: acc = 0; for k ascending: acc =
 * fmaf(w[j][k], h[b][k], acc), one rounding per step; pre = acc + bias[j] (+ 0.0f for NULL).  The tail in fp64, from the fp32 pre
 * and eps widened exactly: ls = min(max(pre_ls, -20), 2); std = exp(ls); x = mean + std * eps; y = tanh(x) = the action;
 * log_prob[b] = the sum over j ascending, from 0, of ((-(eps * eps) / 2 - ls) - log(2 pi) / 2) - log((1.0 - y * y) + 1e-6).
 * With eps NULL: y = tanh(mean), no log_prob.  -(eps * eps) / 2 is what Normal.log_prob(x_t) means; the reference evaluates ((x_t -
 * mean) / std)^2 on the rounded x_t in fp32, which loses every digit when std is small (a log_prob off by 1.15 at log_std near
 * -19.9): a deliberate difference.  A row's result depends neither on n nor on its place in the batch; two calls give the same bits.
 * f110_policyhead_backward: from grad_action [n, A] (required) and grad_log_prob [n] or NULL, both of the width out_fp64 names,
 * and h, pre, eps and the weights of the forward call; it recomputes the tail from pre and eps and reads no other forward output.
 * grad_log_prob must be NULL when eps is.  In fp64: g_x = g_y (1 - y y) + g_lp * (2 y (1 - y y) / ((1 - y y) + 1e-6)); g_mean =
 * g_x; g_ls = g_x std eps - g_lp where -20 <= pre_ls <= 2 (torch's clamp gradient, bounds included) and 0 elsewhere and with eps
 * NULL; grad_pre [n, 2A] fp32 or NULL is a gradient that arrives at pre itself (through the mean, or through the caller's clamp of
 * the log_std, whose mask the caller has applied) and is added to g_mean and g_ls in fp64; each sum rounded once to fp32: g_pre
 * [n, 2A], kept in the workspace.  Then in fp32: grad_h[b][k]: acc = 0; for j ascending
 * over the 2A columns of g_pre (w = w_mean's rows, then w_log_std's): acc = fmaf(w[j][k], g_pre[b][j], acc).  grad_w[j][k] in two
 * stages: for each slice of F110_POLICYHEAD_SLICE_ROWS consecutive rows, acc = 0; for b ascending: acc = fmaf(g_pre[b][j], h[b][k],
 * acc); then the slices are added in ascending order from 0.  grad_b[j] likewise with acc = acc + g_pre[b][j].  No atomics: the
 * result is a function of the inputs alone, whatever the device.  Every gradient output may be NULL (skipped).  `workspace`: 16-byte
 * aligned, f110_policyhead_workspace bytes (0 for an invalid configuration or n outside 1 .. 2^24); it need not be initialised.
 * f110_policyhead_validate: host only.  F110_E_INVALID for in_features outside 1..4096 and action_dim outside 1..32. */
#define F110_POLICYHEAD_SLICE_ROWS 256
typedef struct {
    int32_t in_features;        /* K, 1..4096 (SAL: 512) */
    int32_t action_dim;         /* A, 1..32 (SAL: 16) */
    int32_t out_fp64;           /* nonzero: action, log_prob and their gradients are double, else float */
} f110_policyhead_config;
int f110_policyhead_validate(const f110_policyhead_config *cfg);
int64_t f110_policyhead_workspace(const f110_policyhead_config *cfg, int64_t n);
int f110_policyhead_forward(const f110_policyhead_config *cfg, const float *h, int64_t n, const float *w_mean, const float *b_mean,
                            const float *w_log_std, const float *b_log_std, const float *eps, float *pre, void *action, void *log_prob,
                            void *stream);
int f110_policyhead_backward(const f110_policyhead_config *cfg, const float *h, int64_t n, const float *w_mean, const float *w_log_std,
                             const float *pre, const float *eps, const void *grad_action, const void *grad_log_prob, const float *grad_pre,
                             float *grad_h, float *grad_w_mean, float *grad_b_mean, float *grad_w_log_std, float *grad_b_log_std, float *workspace,
                             void *stream);

/* Critic head: what the reference's twin critics do behind the feature part of fc1 (src/SAL.py:440-442 and :546-549) -- the action
 * columns of fc1, its bias, ReLU, fc2, the min over the two critics and the TD target -- forward in one kernel, and a backward without
 * atomics, for C = 1 or 2 critics at once.  fc1(cat([f, a])) = f @ W[:, :F].T + a @ W[:, F:].T + b: the first term is the caller's
 * GEMM and arrives as `pre`; the concatenated input never exists.  Stateless (no handle; cfg and the two pointer structs host; all
 * arrays dev); launches on `stream` of the calling thread's current device, no allocation, no synchronisation.
 * Per critic c < C (f110_qhead_critics): pre[c] [n, H] fp32, the feature part of fc1 without bias; w_act[c] the action columns of
 * fc1.weight, [H, A] fp32 with a row stride of cfg->ld elements (a view into the [H, F + A] weight with ld = F + A; no alignment
 * of its rows is assumed); b1[c] [H] or NULL; w2[c] [H]; b2[c] [1] or NULL.  Shared: action [n, A], double when action_fp64 is
 * nonzero, else float; a double is rounded to fp32 once on load.
 * Outputs: q [C, n] fp32, required; qmin [n] fp32 or NULL; target [n] fp32 or NULL.  A target needs reward [n] fp64, done [n] uint8
 * and next_log_prob [n] of the action's width, and gamma and alpha finite.  n == 0 does nothing; F110_E_INVALID, not a launch, for
 * what f110_qhead_validate refuses, n outside 0 .. 2^24, a null p, action, q or pre, w_act or w2 of a critic c < C, a target without
 * all three of its inputs, and a wrong device as f110_policyhead_forward refuses it.
 * Numerics, fp32, bit for bit, for row b and hidden unit j: acc = 0; for a ascending: acc = fmaf(w_act[j][a], (float)action[b][a],
 * acc); z = (pre[b][j] + acc) + b1[j] (+ 0.0f for NULL); h = z > 0 ? z : 0.  q[b]: 64 partial sums s_l = 0; for j = l, l + 64, ...
 * ascending while j < H: s_l = fmaf(w2[j], h_j, s_l); a tree: for m = 32, 16, 8, 4, 2, 1: s_l = s_l + s_{l + m} for l < m; q = s_0 +
 * b2 (+ 0.0f for NULL).  qmin = q[0] < q[1] ? q[0] : q[1] (C = 1: q[0]).  The target in fp64 from values widened exactly, every
 * operation rounded on its own, in the reference's order: tq = qmin - alpha * next_log_prob; tv = reward + ((1.0 - done) * gamma) *
 * tq; rounded once to fp32.  A row's result depends neither on n nor on its place in the batch; two calls give the same bits.
 * f110_qhead_backward: from the forward's inputs, its output q, grad_q [C, n] fp32 or NULL and grad_qmin [n] fp32 or NULL (a missing
 * one counts as 0); it recomputes z with the same chain, so the ReLU's mask is the forward's.  G_c[b] = grad_q[c][b] + grad_qmin[b] *
 * m_c[b], m_c = 1 where q_c < q_other, 0.5 where they are equal, 0 where greater (torch's rule for minimum; C = 1: 1).  g_z = z > 0 ?
 * G_c * w2[j] : 0, which is grad_pre[c] [n, H].  grad_w_act[c][j][a], grad_b1[c][j], grad_w2[c][j], grad_b2[c] in two stages: for each
 * slice of F110_QHEAD_SLICE_ROWS consecutive rows acc = 0; for b ascending: acc = fmaf(g_z, (float)action[b][a], acc), acc = acc +
 * g_z, acc = fmaf(G_c, h, acc), acc = acc + G_c respectively; then acc = 0 and the slices are added in ascending order.  grad_w_act
 * is written with the row stride ld, and nothing between its rows is touched.  grad_action[b][a], of the action's width: per critic
 * the 64 partial sums s_l = fmaf(g_z[j], w_act[j][a], s_l) over j = l, l + 64, ... and the tree as in q; then acc = 0; for c
 * ascending: acc = acc + that.  No atomics.  Every gradient output may be NULL (skipped).  `workspace`: 16-byte aligned,
 * f110_qhead_workspace bytes (0 for an invalid configuration or n outside 1 .. 2^24), required when a parameter gradient is asked
 * for; it need not be initialised.
 * f110_qhead_validate: host only.  F110_E_INVALID for hidden outside 1..4096, action_dim outside 1..32, critics outside 1..2 and
 * ld below action_dim. */
#define F110_QHEAD_SLICE_ROWS 256
typedef struct {
    int32_t hidden;             /* H, 1..4096 (SAL: 512) */
    int32_t action_dim;         /* A, 1..32 (SAL: 16) */
    int32_t critics;            /* C, 1..2 */
    int32_t ld;                 /* row stride of w_act and grad_w_act in elements, >= A */
    int32_t action_fp64;        /* nonzero: action, next_log_prob and grad_action are double, else float */
} f110_qhead_config;
typedef struct {                /* entries c >= C are not read */
    const float *pre[2], *w_act[2], *b1[2], *w2[2], *b2[2];
} f110_qhead_critics;
typedef struct {
    float *grad_pre[2], *grad_w_act[2], *grad_b1[2], *grad_w2[2], *grad_b2[2];
} f110_qhead_grads;
int f110_qhead_validate(const f110_qhead_config *cfg);
int64_t f110_qhead_workspace(const f110_qhead_config *cfg, int64_t n);
int f110_qhead_forward(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const double *reward,
                       const uint8_t *done, const void *next_log_prob, double gamma, double alpha, float *q, float *qmin, float *target,
                       void *stream);
int f110_qhead_backward(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const float *q,
                        const float *grad_q, const float *grad_qmin, const f110_qhead_grads *g, void *grad_action, float *workspace,
                        void *stream);

/* Parameter update: Adam with the reference's defaults (src/SAL.py:487-492: weight_decay 0, no amsgrad, no maximize) and the soft
 * update of a target network (:575-578), over up to F110_ADAM_MAX_TENSORS tensors per call in ONE pass: p, g, m, v read once, p, m, v
 * written once, and the target moved from the new p in the same pass.  Stateless but for the caller's f110_adam_state on the device
 * (cfg and table host, every array dev); launches on `stream` of the calling thread's current device, no allocation, no
 * synchronisation.  The table is copied into the kernel's arguments, so it may change from call to call (a fresh .grad buffer) and a
 * captured call keeps the addresses it was captured with.  More tensors than F110_ADAM_MAX_TENSORS: further calls with advance = 0.
 * f110_adam_step: per tensor p, g, m, v [n] fp32 and, with cfg->with_target nonzero, target [n] fp32 (else ignored).  With
 * cfg->advance nonzero the call begins a step: a one-wave launch in front advances the state (t += 1; pow1 *= beta1; pow2 *= beta2,
 * one fp64 multiplication each; k2 = float(sqrt(1 - pow2)), a = float(lr / (1 - pow1)), formed in fp64 with a correctly rounded
 * division and square root and rounded to fp32 once).  With advance zero the call belongs to the step begun before it and reads the
 * same k2 and a; `lr` is then unused.  `lr` is a host scalar of the call: a captured step replays the lr it was captured with.  A
 * fresh state is t = 0, pow1 = pow2 = 1.0 (k2 and a are outputs); a resumed one t = step, pow = beta ** step.  n_tensors == 0 with
 * advance nonzero only advances the state.
 * Numerics, fp32, bit for bit, every line one correctly rounded operation (fmaf fused, division and square root correctly rounded,
 * denormals kept, nothing contracted), with c1 = float(1 - beta1), c2 = float(1 - beta2), b2 = float(beta2), e = float(eps), tau_f =
 * float(tau), each formed in fp64 and rounded once:
 *   d = g - m;  m' = fmaf(c1, d, m);  t1 = g * g;  t2 = t1 * c2;  v' = fmaf(b2, v, t2);  s = sqrt(v');  r = s / k2;  den = r + e;
 *   q = m' / den;  p' = fmaf(-a, q, p);  and with a target: u = p' - tp;  tp' = fmaf(tau_f, u, tp).
 * f110_soft_update: the last line alone with p for p' on p and target of every tensor (g, m, v ignored); p is not written.
 * An element's result depends on nothing but its own inputs and the state; tensors whose pointers are all 16-byte aligned take 16-byte
 * accesses, any other (a view at an odd element offset) 4-byte ones, with the same result.  No element outside [0, n) is touched.
 * F110_E_INVALID, before any launch, naming the culprit: a null cfg, table (with n_tensors > 0) or state; n_tensors outside 0 ..
 * F110_ADAM_MAX_TENSORS; a tensor with n < 0 or n > 2^31; with n > 0: a null p, m or v (Adam), a null g (Adam), a null target (target
 * modes), target == p, a pointer that is not 4-byte aligned; beta1 or beta2 outside [0, 1); eps <= 0 or not finite; lr or tau not
 * finite; tau outside [0, 1]; and a wrong device as f110_policyhead_forward refuses it (p and target of every tensor and the state).
 * f110_adam_validate: the checks on cfg alone, host only.  f110_adam_state_bytes: sizeof(f110_adam_state). */
#define F110_ADAM_CHUNK 4096        /* elements of one tensor a workgroup updates */
#define F110_ADAM_MAX_TENSORS 64    /* tensors of one call: 64 entries of 48 bytes fit a kernel's 4 KiB of arguments */
typedef struct {
    double beta1, beta2, eps;       /* SAL: 0.9, 0.999, 1e-8 */
    double tau;                     /* of the target update, read when with_target is nonzero (SAL: 0.005) */
    int32_t with_target;            /* nonzero: Adam plus target */
    int32_t advance;                /* nonzero: the call begins a step and advances the state first */
} f110_adam_config;
typedef struct {
    float *p;
    const float *g;
    float *m, *v, *target;
    int64_t n;
} f110_adam_tensor;
typedef struct {                    /* on the device; 32 bytes */
    int64_t t;                      /* steps taken */
    double pow1, pow2;              /* beta1 ** t, beta2 ** t as running products */
    float k2, a;                    /* of step t: float(sqrt(1 - pow2)), float(lr / (1 - pow1)) */
} f110_adam_state;
int f110_adam_validate(const f110_adam_config *cfg);
int64_t f110_adam_state_bytes(void);
int f110_adam_step(const f110_adam_config *cfg, const f110_adam_tensor *table, int32_t n_tensors, f110_adam_state *state, double lr,
                   void *stream);
int f110_soft_update(const f110_adam_tensor *table, int32_t n_tensors, double tau, void *stream);

/* Gradient clipping: the global L2 norm of the gradients of one optimizer step, the clip coefficient and a non-finite guard, formed on
 * the device in a fixed order and consumed by the Adam pass while g is in a register.  Opt-in: f110_adam_step keeps its launches, its
 * kernels and its bits.  One step is f110_adam_gradnorm (per call of up to F110_ADAM_MAX_TENSORS tensors), then f110_adam_clip once,
 * then f110_adam_step_clipped (per call); all launch on `stream` of the calling thread's current device, no allocation, no
 * synchronisation, no atomics.  The step covers the tensors that have a gradient, in table order, in chunks of F110_ADAM_CHUNK elements
 * partitioned exactly as f110_adam_step partitions them (tensor i owns ceil(n_i / F110_ADAM_CHUNK) chunks; an empty tensor none); the
 * chunks are numbered consecutively over the whole step, across calls: a further call takes chunk_base = the chunks of the calls before it.
 * Numerics, bit for bit, every + one fp64 addition, nothing contracted:
 *   chunk partial P_c   a chunk is 1 024 quads of four consecutive elements.  Chain l (0 <= l < 256) takes the elements j of the chunk
 *                       with (j >> 2) & 255 == l, j ascending: S_l = S_l + double(g_j) * double(g_j) from 0.0 (the product of two fp32
 *                       values is exact in fp64); a chain without an element is 0.0.  Then for s = 128, 64, .., 1: S_l = S_l + S_(l + s)
 *                       for every l < s (the tree of the losses above), and P_c = S_0.  The membership is by element index, not by
 *                       access width: a tensor on the 4-byte path gives the same P_c.
 *   step sum S          chain l over the partials c = l mod 256, c ascending, from 0.0; the same tree.  finite = (S < +inf), false for
 *                       NaN.  Finite fp32 inputs cannot overflow: at most 2^31 elements a tensor, each term <= 1.2e77.
 *   norm, coefficient   norm = sqrt(S), correctly rounded (0.0 for S = 0); c = max_norm / (norm + 1e-6), one fp64 addition and one IEEE
 *                       division (torch.nn.utils.clip_grad_norm_'s formula); coef = (c < 1.0) ? float(c) : 1.0f.  max_norm = +inf is
 *                       allowed and gives coef = 1.0f always: the guard alone.
 *   decision            skip = !finite (the guard is on whenever clipping is in use); clipped = !skip && coef < 1.0f, after rounding.
 *                       On a skip the state holds sumsq = norm = +inf and coef = 1.0f, whatever NaN the sum was (a NaN's payload is
 *                       no part of the contract, in a partial neither).  steps_clipped += clipped; steps_skipped += skip.
 *   element             gc = g * coef, one fp32 multiplication, then the lines d .. p' of f110_adam_step's contract with gc in g's
 *                       place; with coef == 1.0f this is the unclipped step bit for bit.  g itself is NOT written (torch's
 *                       clip_grad_norm_ scales .grad in place; this saves a pass of stores).
 *   skipped step        p, m, v and the Adam state (t, pow1, pow2, k2, a) keep their bits: the advance in front of the step returns at
 *                       once.  The target is still moved from the unchanged p, as for a parameter without a gradient.
 * f110_adam_gradnorm: one workgroup of 256 per chunk writes partials[chunk_base + c] (dev fp64 [partials_len]) for the table's chunks
 * c; it reads g and n of each tensor and nothing else (p, m, v, target are ignored), with 16-byte loads where g is 16-byte aligned and
 * 4-byte loads otherwise.
 * f110_adam_clip: one workgroup of 256 on partials[0 .. n_chunks) forms S, norm, coef and skip, advances the two counters and writes
 * *clip (dev) with plain stores from one lane.  n_chunks = 0 gives S = 0.  A fresh clip state is all zero bytes.
 * f110_adam_step_clipped: f110_adam_step -- the same arguments, refusals and partition -- with an advance launch that returns at once
 * when clip->skip is set and update kernels of their own that read coef and skip from *clip; skip is tested in a wave-uniform branch
 * around the Adam half, the target half is untouched.
 * F110_E_INVALID, before any launch, naming the culprit: what f110_adam_step refuses (gradnorm: of n_tensors, table, n and g alone);
 * a null partials or clip; chunk_base < 0; a table whose chunks do not fit partials_len behind chunk_base; n_chunks < 0; max_norm NaN
 * or <= 0; partials or clip not 8-byte aligned; and partials or clip on a wrong device as f110_policyhead_forward refuses it.
 * f110_adam_clip_state_bytes: sizeof(f110_adam_clip_state), F110_ADAM_CLIP_STATE_BYTES.
 * (The struct carries a tag, as the temperature's: it lives on the device, _lib.ADAM_CLIP_STRUCTS mirrors it and
 * tests/test_clip_cpu.py checks its fields, size and offsets by the C compiler.) */
#define F110_ADAM_CLIP_STATE_BYTES 64
typedef struct f110_adam_clip_state {   /* on the device; 64 bytes */
    double sumsq, norm;             /* S and sqrt(S) of the last step (+inf on a skip) */
    float coef;                     /* what the step multiplied g by */
    int32_t skip;                   /* 1: the last step was skipped */
    int64_t steps_clipped, steps_skipped;
    int64_t reserved[3];            /* 0 */
} f110_adam_clip_state;
int64_t f110_adam_clip_state_bytes(void);
int f110_adam_gradnorm(const f110_adam_tensor *table, int32_t n_tensors, int64_t chunk_base, double *partials, int64_t partials_len,
                       void *stream);
int f110_adam_clip(const double *partials, int64_t n_chunks, double max_norm, f110_adam_clip_state *clip, void *stream);
int f110_adam_step_clipped(const f110_adam_config *cfg, const f110_adam_tensor *table, int32_t n_tensors, f110_adam_state *state,
                           const f110_adam_clip_state *clip, double lr, void *stream);

/* The two losses of SACAgent.update (src/SAL.py:553-554, :568) and their gradients with respect to the arrays given, one launch each,
 * stateless (all arrays dev, n rows, 1 <= n <= 2^24; launches on `stream` of the calling thread's current device, no allocation, no
 * synchronisation, no atomics).  Neither knows of autograd: the caller hands the gradients to the layers behind q, log_prob and min_q.
 * The sum of every loss, over terms t_i in fp64: chain l (0 <= l < 256) S_l = ((0.0 + t_l) + t_{l + 256}) + ... over i = l mod 256
 * ascending (0.0 for a chain without a term); then for s = 128, 64, .., 1: S_l = S_l + S_{l + s} for every l < s; loss = float(S_0 /
 * double(n)).  Every + is one fp64 addition, the division one fp64 division, rounded to fp32 once; nothing is contracted.  n alone fixes
 * the order, whatever the launch's shape.
 * f110_sac_critic_loss: q1, q2, tv [n] fp32 -> loss [2] fp32 = mean((q_c - tv)^2) with e = double(q_c[i]) - double(tv[i]), t_i = e * e;
 * grad_q1, grad_q2 [n] fp32 (either may be NULL) = (q_c[i] - tv[i]) * k in fp32, one subtraction and one multiplication, k = float(2.0 /
 * double(n)).
 * f110_sac_actor_loss: logp [n] fp64 (logp_fp64 nonzero) or fp32, qn [n] fp32 -> loss [1] fp32 = mean(alpha * logp - qn) with m =
 * alpha * double(logp[i]), t_i = m - double(qn[i]); grad_logp [n] of logp's type = alpha / double(n) (rounded to fp32 from that for
 * fp32) and grad_qn [n] fp32 = float(-1.0 / double(n)) (either may be NULL).
 * Where n is a power of two every gradient equals what autograd gives for F.mse_loss and for (alpha * logp - qn).mean(), bit for bit.
 * F110_E_INVALID, before any launch: n outside 1 .. 2^24, a null input or loss, alpha not finite, logp or grad_logp not aligned to its
 * type, and a wrong device as f110_policyhead_forward refuses it. */
int f110_sac_critic_loss(const float *q1, const float *q2, const float *tv, int64_t n, float *loss, float *grad_q1, float *grad_q2, void *stream);
int f110_sac_actor_loss(const void *logp, int32_t logp_fp64, const float *qn, double alpha, int64_t n, float *loss, void *grad_logp,
                        float *grad_qn, void *stream);
/* f110_sac_critic_loss_weighted: the critic loss under per-row importance weights w [n] fp32 (f110_priority_sample's), a kernel of its
 * own: the unweighted entry keeps its code and bits.  e = double(q_c[i]) - double(tv[i]); t_i = double(w[i]) * (e * e) -- the square
 * first, every product rounded on its own; the sum order, the division by n and the rounding exactly as above.  grad_q_c[i] = ((q_c[i] -
 * tv[i]) * k) * w[i] in fp32, k = float(2.0 / double(n)).  td_out [n] fp32 (may be NULL) = fmaxf(fabsf(q1[i] - tv[i]), fabsf(q2[i] -
 * tv[i])): what f110_priority_update takes.  With w = 1 everywhere the loss and both gradients are f110_sac_critic_loss's bits.  Refused
 * as that entry refuses, and for a NULL w. */
int f110_sac_critic_loss_weighted(const float *q1, const float *q2, const float *tv, const float *w, int64_t n, float *loss, float *grad_q1,
                                  float *grad_q2, float *td_out, void *stream);

/* The entropy temperature of SAC, learnt on the device: log_alpha moves by Adam towards a target entropy (the usual default is
 * -action_dim), and alpha = exp(log_alpha) lives in device memory where the two kernels that consume it read it, so a captured update
 * replays with a temperature that changes from replay to replay.  (The reference fixes alpha = 0.2, src/SAL.py:479; the by-value
 * entry points above are that case and are unchanged.)  Stateless but for the caller's f110_temperature_state on the device (cfg host,
 * logp and state dev); launches on `stream` of the calling thread's current device, no allocation, no synchronisation, no atomics.
 * f110_temperature_step: ONE launch of ONE 256-thread workgroup on logp [n] fp64 (logp_fp64 nonzero) or fp32, 1 <= n <= 2^24.
 * Numerics, bit for bit, nothing contracted:
 *   terms     t_i = double(logp[i]) + target_entropy           one fp64 addition; a fp32 logp is widened exactly
 *   sum       S_0 in the order of the two losses above: 256 chains over i mod 256 ascending, then the tree 128 .. 1; n alone fixes it
 *   mean      mean = S_0 / double(n)                            one fp64 division
 *   loss      loss = float(-(double(log_alpha) * mean))         log_alpha as it stands BEFORE the step; one fp64 multiplication, the
 *                                                               negation exact, one rounding to fp32
 *   gradient  grad = float(-mean)                               d loss / d log_alpha
 *   state     adam advances as f110_adam_step advances its state with advance nonzero: t += 1; pow1 *= beta1; pow2 *= beta2; k2 =
 *             float(sqrt(1 - pow2)); a = float(lr / (1 - pow1))
 *   Adam      the lines d .. p' of f110_adam_step's contract on the one element p = log_alpha, g = grad, m, v (c1, c2, b2, e from
 *             cfg as there), each one correctly rounded fp32 operation, fmaf fused, denormals kept
 *   alpha     alpha = exp(double(log_alpha'))                   one fp64 exp of the device's library (the one value here that is not
 *                                                               fixed to the last bit: within an ulp of the correctly rounded one)
 * Lane 0 forms everything behind the sum and writes the state.  A mean that is not finite is NOT caught: it propagates into loss, grad,
 * the moments, log_alpha and alpha as it would in any framework's optimizer.  `lr` is a host scalar of the call: a captured step
 * replays the lr it was captured with.
 * A fresh state is written by the host: adam = {0, 1.0, 1.0, 0, 0}, alpha = init_alpha exactly, log_alpha = float(log(init_alpha)),
 * m = v = grad = loss = 0, reserved = 0; the temperature before the first step is the number the user gave, bit for bit.  A resumed
 * one: adam.t = step, pow = beta ** step.
 * F110_E_INVALID, before any launch, naming the culprit: a null cfg, logp or state; n outside 1 .. 2^24; beta1 or beta2 outside [0, 1);
 * eps <= 0 or not finite; lr or target_entropy not finite; logp not aligned to its type; state not 8-byte aligned; and a wrong device
 * as f110_policyhead_forward refuses it (logp and state).
 * f110_temperature_validate: the checks on cfg alone, host only.  f110_temperature_state_bytes: sizeof(f110_temperature_state), 64.
 * f110_qhead_forward_alpha_dev, f110_sac_actor_loss_alpha_dev: f110_qhead_forward and f110_sac_actor_loss -- the same kernels, the same
 * numerics -- with alpha read from device memory (one fp64 load; typically &state->alpha) instead of passed by value; in the actor loss
 * grad_logp = alpha / double(n) is then one fp64 division on the device (IEEE: the host's bits).  alpha cannot be checked for
 * finiteness on the host any more; a null `alpha` (for the critic head: where a target is asked for) and one on a wrong device are
 * refused, everything else as the by-value entry refuses it.
 * (The two structs carry a tag: tests/abi_header.py reads the untagged typedefs, whose fields are scalars, arrays and pointers, for
 * the flat mirror of red_gym_amd/_lib.py; f110_temperature_state nests f110_adam_state by value, so these two are mirrored as
 * _lib.TEMPERATURE_STRUCTS and tests/test_temperature_cpu.py checks their fields, sizes and offsets by the C compiler.) */
typedef struct f110_temperature_config {
    double beta1, beta2, eps;       /* 0.9, 0.999, 1e-8 */
    double target_entropy;          /* SAC's default: -action_dim */
} f110_temperature_config;
typedef struct f110_temperature_state { /* on the device; 64 bytes */
    f110_adam_state adam;           /* 32 B: t, pow1, pow2, k2, a -- advanced as f110_adam_step advances its state */
    double alpha;                   /* what the *_alpha_dev entries read */
    float log_alpha, m, v;          /* the parameter and its Adam moments */
    float grad, loss;               /* of the last step (outputs) */
    int32_t reserved;               /* 0 */
} f110_temperature_state;
int f110_temperature_validate(const f110_temperature_config *cfg);
int64_t f110_temperature_state_bytes(void);
int f110_temperature_step(const f110_temperature_config *cfg, const void *logp, int32_t logp_fp64, int64_t n,
                          f110_temperature_state *state, double lr, void *stream);
int f110_qhead_forward_alpha_dev(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const double *reward,
                                 const uint8_t *done, const void *next_log_prob, double gamma, const double *alpha, float *q, float *qmin,
                                 float *target, void *stream);
int f110_sac_actor_loss_alpha_dev(const void *logp, int32_t logp_fp64, const float *qn, const double *alpha, int64_t n, float *loss,
                                  void *grad_logp, float *grad_qn, void *stream);
/* f110_qhead_forward_rows: f110_qhead_forward -- the same kernel, the same numerics -- with a discount per row in gamma's place, for
 * targets built on n-step returns (f110_replay_sample_nstep's ret, d and discount): discount [n] dev fp64, and the target's second
 * line is tv = reward + ((1.0 - done) * discount[b]) * tq.  Where discount[b] holds gamma's bits the row's target is the by-value
 * entry's, bit for bit.  One entry serves both temperature modes: alpha_dev non-NULL (dev fp64 [1]) is read on the device and wins;
 * NULL: `alpha` by value, which must then be finite.  The values of discount cannot be checked on the host; a null discount where a
 * target is asked for, and one on a wrong device, are refused, everything else as f110_qhead_forward refuses it.  The backward pass
 * does not read the target. */
int f110_qhead_forward_rows(const f110_qhead_config *cfg, const f110_qhead_critics *p, const void *action, int64_t n, const double *reward,
                            const uint8_t *done, const void *next_log_prob, const double *discount, double alpha, const double *alpha_dev,
                            float *q, float *qmin, float *target, void *stream);

/* The policy's Gaussian draws: the eps of f110_policyhead_forward (Actor.sample's normal.rsample(), src/SAL.py:414-421) made on the
 * device, so that the one random input of acting and of an update is the library's own, named by numbers a checkpoint can hold.
 * One draw is named by five numbers -- seed (64 bits), stream (64 bits; an agent uses 0 for acting, 1 for an update's next_action and
 * 2 for its new_action), call t (64 bits), row r (64 bits) and column j < A -- and its value is
 *     float32( numpy.random.Generator( numpy.random.Philox(key=[seed, stream], counter=[0, j, r, t]) ).standard_normal() )
 * the FIRST fp64 normal of that generator, rounded once to fp32 (ties to even): NumPy's bits, compared with == and no tolerance.
 * Restated (checked on NumPy 2.2.6):
 *   bit generator  Philox4x64-10: multipliers 0xD2E7470EE14C6C93 (word 0) and 0xCA5A826395121157 (word 2), Weyl increments of the
 *                  key 0x9E3779B97F4A7C15 and 0xBB67AE8584CAA73B, ten rounds.  NumPy increments the counter BEFORE it produces a
 *                  block: the first four raw words are the block of counter [1, j, r, t], the next four of [2, j, r, t].  Word 0 of
 *                  the counter so belongs to the element's own block count, and two elements' streams never overlap.
 *   normal         random_standard_normal's 256-layer ziggurat: one raw word per trial (index, sign, 52-bit magnitude; accepted by
 *                  one table compare in 98.5 % of the elements), one more for a wedge test (against exp() of the device's library:
 *                  a decision, and the one place where a library rounding could show), two per tail trial (|x| > 3.6541528853610088,
 *                  log1p as glibc rounds it).  About 1.5 % of the elements take two to four words; a handful in 65 536 take five or
 *                  more and cross into the second block.
 *   cost           an element computes a whole block of four words and, on the common path, uses one; the other three are thrown
 *                  away.  That is the price of lane independence: a row's draws are the same alone, among 65 536, and whatever was
 *                  drawn before.
 * The state is 64 bytes of caller-owned device memory: seed, one call counter per stream, padding (zeros).  The host writes a fresh
 * one; f110_gauss_fill reads seed and t = calls[stream] ON THE DEVICE and, with advance nonzero, a one-lane kernel behind the fill
 * adds 1 to calls[stream] -- the pattern of f110_replay_sample's draw counter and of f110_adam_step's state -- so a captured fill
 * replays with a fresh t.  f110_gauss_fill_at is the same kernel with seed, stream and t by value, for callers that keep their own
 * counter.  out [n, A] fp32, contiguous; rows NULL: row i is i, else an int64 [n] device array of row ids (their 64 bits as they
 * stand).  One lane per element, a grid-stride walk beyond 2 048 workgroups of 256; stores are 16 bytes wide where out is 16-byte
 * aligned.  Both launch on `hip_stream` of the calling thread's current device: no allocation, no synchronisation, no atomics, no LDS.
 * F110_E_INVALID, before any launch, naming the culprit: a null state (f110_gauss_fill) or out; a state or rows not 8-byte aligned;
 * stream outside 0 .. F110_GAUSS_STREAMS - 1; n < 1; A outside 1 .. F110_GAUSS_MAX_COLUMNS (the policy head's action_dim limit);
 * n * A above 2^31; out not 4-byte aligned; and a wrong device as f110_policyhead_forward refuses it (state, rows, out).
 * f110_gauss_state_bytes: sizeof(f110_gauss_state), 64.
 * (The struct carries a tag for the reason f110_temperature_state does: it is mirrored as _lib.GAUSS_STRUCTS and
 * tests/test_gauss_cpu.py checks its fields, size and offsets by the C compiler.) */
#define F110_GAUSS_STREAMS 4
#define F110_GAUSS_MAX_COLUMNS 32
typedef struct f110_gauss_state {   /* on the device; 64 bytes */
    uint64_t seed;
    uint64_t calls[F110_GAUSS_STREAMS]; /* calls[s]: the t of the next f110_gauss_fill of stream s */
    uint64_t reserved[3];           /* 0 */
} f110_gauss_state;
int64_t f110_gauss_state_bytes(void);
int f110_gauss_fill(f110_gauss_state *state, int32_t stream, int64_t n, int32_t A, const int64_t *rows, float *out, int32_t advance,
                    void *hip_stream);
int f110_gauss_fill_at(uint64_t seed, int32_t stream, uint64_t t, int64_t n, int32_t A, const int64_t *rows, float *out, void *hip_stream);

/* ---- function-level entry points (parity tests; all pointers dev) ---- */
/* ScanSimulator2D.scan(pose, None): n poses [n,3] -> [n,num_beams] (noise off).
 * scans_f32 / lookups may be NULL; lookups [n] is overwritten-by-accumulation like
 * f110_buffers.lookups (zero it first). */
int f110_scan(f110_handle *h, const double *poses, int32_t n, double *scans_f64, float *scans_f32,
              uint32_t *lookups, void *stream);
/* RaceCar.update_pose without the scan (base_classes.py:254-402), n cars in place. */
int f110_update_pose(f110_handle *h, double *state, double *steer_buf, int32_t *steer_cnt,
                     const double *actions, int32_t n, void *stream);
/* vehicle_dynamics_st (dynamic_models.py:124-176; kinematic == 1: vehicle_dynamics_ks
 * :91-121 on the first 5 states): right-hand sides f [n,7] for states x [n,7] and inputs
 * u [n,2] = (steering velocity, acceleration), with the handle's agent-0 parameters. */
int f110_vehicle_dynamics(f110_handle *h, const double *x, const double *u, int32_t n, int32_t kinematic,
                          double *f, void *stream);
/* get_vertices (collision_models.py:238-260): [n,3] -> [n,4,2] */
int f110_get_vertices(f110_handle *h, const double *poses, int32_t n, double *verts, void *stream);
/* collision (GJK, collision_models.py:114-182) on n quad pairs -> hit[n] */
int f110_gjk_pairs(f110_handle *h, const double *verts_a, const double *verts_b, int32_t n,
                   uint8_t *hit, void *stream);
/* collision_multiple (collision_models.py:185-212): n groups of A quads [n,A,4,2] */
int f110_collision_multiple(f110_handle *h, const double *verts, int32_t n, int32_t A,
                            uint8_t *collisions, int32_t *collision_idx, void *stream);
/* check_ttc_jit (laser_models.py:189-217): scans [n,num_beams], vel [n] -> hit[n] */
int f110_check_ttc(f110_handle *h, const double *scans, const double *vel, int32_t n, uint8_t *hit,
                   void *stream);
/* The same for n rows with the side table of params slot slot_of_row[r] each (dev int32 [n]; f110_set_side_distance_slots;
 * F110_E_INVALID when no tables are installed).  A slot outside the installed tables reads row 0 (reported through the
 * device error word in the bounds-checked build). */
int f110_check_ttc_slots(f110_handle *h, const double *scans, const double *vel, const int32_t *slot_of_row, int32_t n,
                         uint8_t *hit, void *stream);
/* ray_cast (laser_models.py:319-346): scans [n,num_beams] modified in place by one
 * opponent quad each; span [n,2] = get_blocked_view_indices (may be NULL). */
int f110_ray_cast(f110_handle *h, const double *ego_poses, const double *opp_verts, int32_t n,
                  double *scans, int32_t *span, void *stream);

/* F110Env._check_done (f110_env.py:202-244) on n envs of num_agents cars, stateless (h may be NULL):
 * poses [n,A,3] (x, y, theta) and start_poses [n,A,3] (the poses given to reset: start_xs / start_ys, :321-323),
 * start_rot [n,4] the EGO's 2x2 start rotation, row-major (:329), current_time [n] (already advanced by the
 * step, :293), collisions [n,A] (only the ego's entry is read, :242).  In/out: near_start [n,A] (0/1, True after
 * reset), toggles [n,A], lap_times [n,A] (frozen once a car has 4 toggles).  Out: lap_counts [n,A] = toggles // 2,
 * done [n] = collisions[ego] or all(toggles >= 4), checkpoint_done [n,A] = toggles >= 4 (may be NULL).
 * f110_step runs the same device function inside its env kernel. */
int f110_check_done(f110_handle *h, const double *poses, const double *start_poses, const double *start_rot,
                    const double *current_time, const uint8_t *collisions, int32_t n, int32_t num_agents,
                    int32_t ego_idx, uint8_t *near_start, int32_t *toggles, int32_t *lap_counts, double *lap_times,
                    uint8_t *done, uint8_t *checkpoint_done, void *stream);
/* The reward terms of f110_shaping_update without its episode logic, stateless (no handle; cfg host, cfg->agent is not
 * read): n images bitmaps [n, rows, cols], positions xy [n,2] and prev_xy [n,2] -> collision_term, progress_term,
 * centering_term, total [n] and collided [n] (SACF110Env._calculate_rewards on last_obs['lidar_bitmap'] = bitmaps[i],
 * prev_position = prev_xy[i] and the new pose xy[i]).  Launches on the calling thread's current device. */
int f110_shaping_terms(const f110_shaping_config *cfg, const uint8_t *bitmaps, const double *xy, const double *prev_xy,
                       int32_t n, double *collision_term, double *progress_term, double *centering_term, double *total,
                       uint8_t *collided, void *stream);
/* The same from images held as bits: packed [n, rows, ceil(cols / 64)] uint64 (f110_replay_pack's, f110_bitmap_render_bits'). */
int f110_shaping_terms_bits(const f110_shaping_config *cfg, const uint64_t *packed, const double *xy, const double *prev_xy,
                            int32_t n, double *collision_term, double *progress_term, double *centering_term, double *total,
                            uint8_t *collided, void *stream);
/* The follower's two halves for n independent cases, stateless, no episode logic (no handle; cfg host, cfg->agent is not read;
 * all arrays dev).  f110_pathfollow_decode: raw actions [n,16] and poses [n,3] = (x, y, yaw) -> paths [n,8,2].
 * f110_pathfollow_mpc: paths [n,8,2] and velocities [n,2] = (vx, vy) -> dists [n,8], ref_traj [n, horizon + 1, 4], accel [n,2],
 * actions [n,2] = (steer, speed) and qp_steps [n,2] (steps of the two active-set walks; may be NULL); dev_err (may be NULL): a
 * device word that gets F110_DEVERR_QP_LIMIT OR-ed in.  It builds the QP's tables, waits for the kernel and frees them.
 * f110_pathfollow_advance: _update_path_index for paths [n,8,2], index [n] (0..7; any other is copied) and positions xy [n,2]
 * -> index_out [n]. */
int f110_pathfollow_decode(const f110_pathfollow_config *cfg, const double *raw_actions, const double *poses, int32_t n,
                           double *paths, void *stream);
int f110_pathfollow_mpc(const f110_pathfollow_config *cfg, const double *paths, const double *vels, int32_t n, double *dists,
                        double *ref_traj, double *accel, double *actions, int32_t *qp_steps, uint32_t *dev_err, void *stream);
int f110_pathfollow_advance(const f110_pathfollow_config *cfg, const double *paths, const int32_t *index, const double *xy,
                            int32_t n, int32_t *index_out, void *stream);
/* The replay buffer's frame format, stateless (no handle; all arrays dev, 16-byte aligned; rows, cols 1..16384): n images
 * bitmaps [n, rows, cols] uint8 -> packed [n, rows, words] uint64 (bit = pixel == 255) and back (0 / 255). */
int f110_replay_pack(const uint8_t *bitmaps, int64_t n, int32_t rows, int32_t cols, uint64_t *packed, void *stream);
int f110_replay_unpack(const uint64_t *packed, int64_t n, int32_t rows, int32_t cols, uint8_t *bitmaps, void *stream);

/* ---- scan -> bird's-eye bitmap (the first consumer of the step's scans) ----
 * Replaces weap_util/weap_util/lidar.py:105-154 `lidar_to_bitmap` (same body in src/SAL.py:274-395
 * and src/bitmap.py:4-140), which draws one scan with OpenCV 4.11 (fillPoly / polylines / line /
 * rectangle, 8-bit, LINE_8).  A renderer holds the scan-independent tables the reference rebuilds
 * per call (lidar.py:63-72): indices = np.linspace(0, num_beams-1, T, dtype=int) and cos / sin of
 * angles = starting_angle + dir*fov*np.linspace(0, 1, T) -- computed by the caller with numpy so that
 * they are the reference's own values (host pointers, copied). */
#define F110_BITMAP_FILL 0
#define F110_BITMAP_POLYGON 1
#define F110_BITMAP_RAYS 2
typedef struct f110_bitmap f110_bitmap;
typedef struct {
    int32_t device;
    int32_t num_beams;          /* len(scan) */
    int32_t target_beam_count;  /* T, 0 < T < num_beams, T <= 2048 */
    int32_t rows, cols;         /* output_image_dims */
    int32_t channels;           /* 1, 3 or 4 (alpha = 255) */
    int32_t draw_mode;          /* F110_BITMAP_* */
    int32_t bg_value, draw_value; /* grey levels (0/255 white-on-black etc., lidar.py:61; 0/180 in src/bitmap.py:60) */
    int32_t draw_center;
    double scaling_factor;      /* pixels per metre (min(dims)/max_scan_radius when that is given) */
} f110_bitmap_config;
int f110_bitmap_create(const f110_bitmap_config *cfg, const int32_t *indices, const double *cosines,
                       const double *sines, f110_bitmap **out);
void f110_bitmap_destroy(f110_bitmap *b);
/* n scans (dev, f32 or f64, `stride` elements apart) -> out dev uint8 [n, rows, cols(, channels)].
 * Enqueued on `stream`; no allocation, no synchronisation. */
int f110_bitmap_render(f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                       uint8_t *out, void *stream);
/* The same images as one bit per pixel: out dev uint64 [n, rows, words], words = ceil(cols / 64), 16-byte aligned.  Bit k of
 * word w of row y is set iff f110_bitmap_render would write draw_value at (y, 64 w + k) -- the centre marker of a FILL image is
 * background: 0 -- and bits at columns >= cols are 0.  All three draw modes; `channels` plays no part.  The kernel is
 * f110_bitmap_render's up to its last phase, which stores the 1-bit image it drew instead of expanding it to grey bytes.  With
 * bg_value 0 and draw_value 255 this is the replay ring's frame format (f110_replay_pack of the byte image).  Enqueued on
 * `stream`; no allocation, no synchronisation. */
int f110_bitmap_render_bits(f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                            uint64_t *out, void *stream);
/* Function-level view of the renderer's first stage (parity tests): the integer points the reference computes
 * at lidar.py:63-73 and hands to cv2.fillPoly / polylines / line -- points dev int32 [n, T, 2] = (x, y) of
 * np.rint(center + scaling_factor * scan[indices] * {cos, sin}(angles)).astype(int), center = (rows//2, cols//2). */
int f110_bitmap_points(f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                       int32_t *points, void *stream);
/* Point-occupancy grid of f1tenth_gym/examples/lidar.py:212-244 (the routine that wrote the
 * reference's lidar_datasets): out dev uint8 [n, grid, grid] of 0/1.  cosines / sines: dev [num_beams],
 * of np.linspace(-135, 135, num_beams) * pi / 180. */
int f110_scan_occupancy(const void *scans, int32_t scans_f64, int64_t n, int64_t stride, int32_t num_beams,
                        const double *cosines, const double *sines, double max_range, double lo, double hi,
                        int32_t grid, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* F110_HIP_H */
