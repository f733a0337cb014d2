// f110_scan_plan.h -- the launch plan of a scan: which cars each scan_kernel launch marches, with which instantiation, stage
// list and grid.  Plain C++17 without HIP (tests/test_scan_plan_cpu.py compiles it for the host); f110_step.hip emits it.
#pragma once
#include "../../include/f110_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

int fail(int code, const char *fmt, ...);

namespace f110 {

constexpr int WAVE = 64;
constexpr int SCAN_WAVES = 2;   // cars per workgroup, one wavefront each (one-car workgroups: profiles/r05_one_wave_groups.txt)
constexpr int SCAN_THREADS = SCAN_WAVES * WAVE;
constexpr int SCAN_MAX_STAGES = 8, SCAN_MAX_LOG2W = 3;
constexpr int MAX_CHUNKS = 64; // beams are handed out in chunks of 64 (num_beams <= 4096)

// one stage of a scan launch's wave -> car mapping: `cars` cars (< 0: "*", the remaining cars) at 2^lg waves each
struct StageSpec { int cars, lg; };

// "cars:log2waves,..." with at most one "*": strict syntax (f110_set_scan_stages refuses what this refuses)
inline bool parse_stage_spec(const char *p, std::vector<StageSpec> &spec, const char **why)
{
    spec.clear();
    int stars = 0;
    if (!p || !*p) { *why = "empty"; return false; }
    for (;;) {
        int cars = -1, lg = 0;
        if (*p == '*') { p++; stars++; }
        else if (*p >= '0' && *p <= '9') {
            long v = strtol(p, (char **)&p, 10);
            if (v > 0x3fffffff) { *why = "car count too large"; return false; }
            cars = (int)v;
        } else { *why = "expected a car count or *"; return false; }
        if (*p == ':') {
            p++;
            if (!(*p >= '0' && *p <= '9')) { *why = "expected log2(waves per car) after ':'"; return false; }
            long v = strtol(p, (char **)&p, 10);
            if (v > SCAN_MAX_LOG2W) { *why = "log2(waves per car) above 3"; return false; }
            lg = (int)v;
        }
        spec.push_back({cars, lg});
        if (*p == ',') { p++; continue; }
        if (*p) { *why = "unexpected character"; return false; }
        break;
    }
    if (stars > 1) { *why = "more than one *"; return false; }
    if (spec.size() > 6) { *why = "more than 6 stages"; return false; }
    return true;
}

// The wave -> car mapping of a scan launch of n_cars cars: a list of stages (cars, log2 waves per car), from the
// f110_set_scan_stages override or, without one, the built-in choice.
// Drain of a launch: workgroups are dispatched in index order and nothing follows the last ones,
// so the chip empties over one wave lifetime (about half of it lost: ~5 % at 65 536 cars -- the gap
// that two half-size launches from two processes close by overlapping).  The last cars therefore
// run as 4 short waves each ("*:0,2048:2" for big launches of one agent per env).
// Measured (profiles/r01j): 65 536 cars 0.702 -> 0.672 ms for any tail of 1 000 .. 2 048 cars (it has to
// cover the last of the slowest cars), 32 768: 0.380 -> 0.368, 16 384: 0.225 -> 0.218, 8 192: neutral,
// 4 096: 0.126 -> 0.105 with half of the cars split; graded tails (halves, quarters, eighths) and graded
// heads changed nothing.
// (Measured and dropped in round 2, profiles/r02_multicar_waves_sweep.txt: stages that give one wave K = 2, 4, 8
// consecutive cars to march back to back, so that a wave drains once per K cars -- 0.705 ms at best against
// 0.664 ms: the leaner refill of one car per wave and the finer-grained launch win.)
inline std::vector<StageSpec> scan_stage_list(const std::vector<StageSpec> &override_spec, int n_cars, int agents, int num_beams)
{
    std::vector<StageSpec> spec = override_spec;
    if (spec.empty()) {
        // Waves per car.  Measured on MI355X (profiles/r01g, r01i): a wave's lifetime is bounded
        // below by its longest ray (~50 us), so splitting a car's beams over several waves only
        // pays while the chip is nearly empty: scan time at 256 / 1024 cars 76 -> 49 us and
        // 87 -> 65 us with 8 waves per car, but 121 -> 143 us at 4096 cars (prologues and the
        // shorter queues' tails eat the extra parallelism).
        int wpc = n_cars <= 1024 ? 8 : (n_cars <= 2048 ? 4 : 1);
        const int nch = (num_beams + 63) / 64;
        while (wpc > 1 && wpc > nch) wpc /= 2;
        // split cars (a small launch) or a short scan (fewer than 8 chunks of 64 beams): one stage
        if (wpc > 1 || nch < 8) return {{n_cars, wpc >= 8 ? 3 : wpc >= 4 ? 2 : wpc >= 2 ? 1 : 0}};
        // (envs of several agents: 4 096 -- 16 384 x 2: scan 0.396 -> 0.388 ms, 32 768 x 2: 0.697 -> 0.672; 8 192 x 4: flat;
        // one agent: 4 096 is 1 % worse than 2 048 at 65 536 cars and 2.5 % worse at 32 768; profiles/r04_scan_stores.txt N)
        const int tail = std::min(agents >= 2 ? 4096 : 2048, n_cars / 2);
        spec = {{-1, 0}, {tail, 2}};
    }
    int fixed = 0;
    for (StageSpec &x : spec) if (x.cars >= 0) { x.cars -= x.cars % SCAN_WAVES; fixed += x.cars; }
    // a list written for the step's car count may not fit a function-level scan of fewer poses: whole cars then
    if (fixed > n_cars) { spec = {{-1, 0}}; fixed = 0; }
    bool star = false;
    for (StageSpec &x : spec) if (x.cars < 0 && !star) { x.cars = n_cars - fixed; star = true; }
    if (!star) spec.push_back({n_cars - fixed, 0});
    std::vector<StageSpec> stv;
    for (const StageSpec &x : spec) if (x.cars > 0) stv.push_back(x);
    // Every stage but the last has a car count that is a multiple of SCAN_WAVES, so that every stage starts at such a car
    // (and a wave count that is one too: a workgroup never mixes two stages).  The two waves of a workgroup of whole cars
    // then march cars (2k, 2k+1) of the launch, which is the pair f110_assign_maps checks for a shared map: they stage one
    // LUT copy between them, half each from their own car's map (scan_kernel).  Only the "*" stage can be odd; a wave count
    // that is even is not enough (65 cars x 2 waves, then whole cars from car 65: cars 79 and 80 in one workgroup).
    for (size_t i = 0; i + 1 < stv.size(); i++)
        if (stv[i].cars % SCAN_WAVES) return {{n_cars, 0}};
    if (stv.size() > (size_t)SCAN_MAX_STAGES) return {{n_cars, 0}};
    return stv;
}

// The compact form of the step's scan: workgroups of ONE wave, each with its own LDS copy of a LUT image of S slots instead of
// LUT_LDS (f110_map.h: the cells behind slot S - 1 carry the far marker in a cell table of their own and take the rare path).
// A map whose road is a few dozen cells wide has a few hundred distinct distances, so the short image loses next to nothing
// there, and a slot of the CU is free again when ONE car is done instead of two.
constexpr int SCAN_COMPACT_N = 2;
constexpr int SCAN_COMPACT_S[SCAN_COMPACT_N] = {256, 512};
// The rule's constants, all MEASURED (profiles/r24_scan_compact.txt, MI355X).
//  CAP: a compact form is chosen while the share of the cars' reachable free cells behind its marker is UNDER it.  With no cell
//   behind the marker (example_map) the forms are 2.3 - 2.6 % faster than the classic one at 65 536 cars; every cell behind it
//   parks its ray until the next refill, and the bundled tracks re-installed at 0.0625 m lose 5 % at a share of 0.027 (S = 512),
//   15 % at 0.06 - 0.08 and 53 % at 0.29 (S = 256): about 2 - 2.8 % per 0.01 of share, break-even near 0.01.  0.004 keeps the
//   interpolated cost (1.1 %) under half the gain.
//  MIN_CARS: below 32 768 cars the one-wave groups lose (4 096: +1 %, 8 192: +0.6 .. 1.2 %, 16 384: +0.3 .. 0.9 % with S = 256).
//  One agent per env only: 16 384 x 2 measured 1 % slower with S = 256 (its tail of split cars is twice as long).
// F110_SCAN_FORM forces a form for tests and A/B runs.
constexpr double SCAN_COMPACT_CAP = 0.004;
constexpr int SCAN_COMPACT_MIN_CARS = 32768;

// The smallest S whose share of reachable free cells outside the image is under the cap, or 0 = the classic form.
// out_share[i]: that share for SCAN_COMPACT_S[i].
inline int scan_compact_choice(const double *out_share, int n_cars, int agents, double cap = SCAN_COMPACT_CAP,
                               int min_cars = SCAN_COMPACT_MIN_CARS)
{
    if (n_cars < min_cars || agents != 1) return 0;
    for (int i = 0; i < SCAN_COMPACT_N; i++)
        if (out_share[i] < cap) return SCAN_COMPACT_S[i];
    return 0;
}

// The shares scan_compact_choice reads, from a map's cell codes and the cars' spawn poses.  A ray only crosses free cells and
// a car that leaves its free component has collided, so until the next reset a car's look-ups stay inside the free cells
// 8-connected to its spawn cell.  share[i] = the MEAN OVER THE CARS of (cells of the car's component whose code is at or
// beyond off_far[i]) / (cells of the component): the expected fraction of look-ups behind the marker of SCAN_COMPACT_S[i] if a
// car's look-ups are spread over its component.  A car off the map or on a cell that is not free never marches and counts 0;
// a handful of cars jittered off a track weigh what they are.  (The share over ALL free cells of a map cannot serve: the open
// ground around a track may be most of them and holds next to no car.)
//   code_at(r, c): the classic cell code of map cell (r, c), 0 <= r < H, 0 <= c < W; free: code > code_zero (distance not 0)
//   poses: n_cars x (x, y, .), pose_stride doubles apart; cell = floor((x - ox) * rinv), floor((y - oy) * rinv) (origin unrotated)
template <typename CodeAt>
void scan_reach_shares(int H, int W, CodeAt code_at, unsigned code_zero, const unsigned *off_far, const double *poses,
                       int pose_stride, int n_cars, double ox, double oy, double rinv, double *share)
{
    std::vector<int> label((size_t)H * W, 0);            // 0: not visited, k > 0: component k - 1
    std::vector<double> comp_share;                      // [component][SCAN_COMPACT_N]
    std::vector<int> stack;
    double sum[SCAN_COMPACT_N] = {};
    for (int i = 0; i < n_cars; i++) {
        const double qx = std::floor((poses[(size_t)i * pose_stride] - ox) * rinv), qy = std::floor((poses[(size_t)i * pose_stride + 1] - oy) * rinv);
        if (!(qx >= 0 && qx < W && qy >= 0 && qy < H)) continue; // (a NaN pose fails the test too)
        const int r0 = (int)qy, c0 = (int)qx;
        if (!(code_at(r0, c0) > code_zero)) continue;
        int &l0 = label[(size_t)r0 * W + c0];
        if (!l0) {   // a component no earlier car stood in: flood fill it
            const int id = (int)(comp_share.size() / SCAN_COMPACT_N) + 1;
            size_t n_free = 0, n_out[SCAN_COMPACT_N] = {};
            l0 = id;
            stack.push_back(r0 * W + c0);
            while (!stack.empty()) {
                const int at = stack.back(), r = at / W, c = at % W;
                stack.pop_back();
                const unsigned code = code_at(r, c);
                n_free++;
                for (int k = 0; k < SCAN_COMPACT_N; k++) n_out[k] += code >= off_far[k];
                for (int dr = -1; dr <= 1; dr++)
                    for (int dc = -1; dc <= 1; dc++) {
                        const int rr = r + dr, cc = c + dc;
                        if (rr < 0 || rr >= H || cc < 0 || cc >= W || label[(size_t)rr * W + cc] || !(code_at(rr, cc) > code_zero)) continue;
                        label[(size_t)rr * W + cc] = id;
                        stack.push_back(rr * W + cc);
                    }
            }
            for (int k = 0; k < SCAN_COMPACT_N; k++) comp_share.push_back((double)n_out[k] / (double)n_free);
        }
        for (int k = 0; k < SCAN_COMPACT_N; k++) sum[k] += comp_share[(size_t)(label[(size_t)r0 * W + c0] - 1) * SCAN_COMPACT_N + k];
    }
    for (int k = 0; k < SCAN_COMPACT_N; k++) share[k] = n_cars > 0 ? sum[k] / (double)n_cars : 1.0;
}

// The row buffer of the compact form with S = 256 (scan_kernel<.., 256, true>).  Its workgroup of one wave uses 2 304 B of LDS for
// the LUT image and the chunk table; with 32 workgroups on a CU, SCAN_LDS_PER_GROUP are there for each, and the rest holds a
// fixed set of the wave's 64-beam chunks as fp32: the LAST SCAN_ROWBUF_CHUNKS positions of its queue (the short rays; the
// long rays of the first positions keep the direct store).  A finished beam of a staged chunk is written to LDS instead of to
// its scattered dword of the row, and the wave writes the staged chunks out as whole 256-B pieces once its march has ended.
// Nothing moves: no slot is re-bound, no counter kept (profiles/r25_scan_rowbuf.txt).
constexpr int SCAN_LDS_PER_CU = 163840, SCAN_GROUPS_PER_CU = 32;
constexpr int SCAN_LDS_PER_GROUP = SCAN_LDS_PER_CU / SCAN_GROUPS_PER_CU;                        // 5 120 B
constexpr int SCAN_ROWBUF_LUT = 256;                                                             // the form that has the room
constexpr int SCAN_ROWBUF_BASE = SCAN_ROWBUF_LUT * 8 + MAX_CHUNKS * 4;                           // LUT image + chunk table
constexpr int SCAN_ROWBUF_CHUNKS = (SCAN_LDS_PER_GROUP - SCAN_ROWBUF_BASE) / (64 * 4);           // 11 chunks = 704 beams
static_assert(SCAN_ROWBUF_CHUNKS >= 1 && SCAN_ROWBUF_BASE + SCAN_ROWBUF_CHUNKS * 256 <= SCAN_LDS_PER_GROUP, "row buffer within a group's LDS");

#if defined(__HIPCC__)
#define F110_PLAN_HD __host__ __device__
#else
#define F110_PLAN_HD
#endif
// The slice of a car's beam queue that wave `part` of 2^lg marches -- chunk positions part, part + 2^lg, ... of the
// ceil(nb / 64) chunks, wave-local position j = 0 .. my_chunks - 1 -- and what of it is staged: positions j0 .. my_chunks - 1
// in slots 0 .. n_slots - 1 (slot = j - j0).  nbl: beams of the wave (the car's last chunk may be short).
struct ScanRowbufPlan { int my_chunks, nbl, j0, n_slots; };
F110_PLAN_HD inline ScanRowbufPlan scan_rowbuf_plan(int nb, int lg, int part)
{
    const int wpc = 1 << lg, nch = (nb + 63) >> 6;
    ScanRowbufPlan p;
    p.my_chunks = nch > part ? (nch - part + wpc - 1) >> lg : 0;
    const int owns_last = p.my_chunks > 0 && ((nch - 1) & (wpc - 1)) == part;
    p.nbl = p.my_chunks * 64 - (owns_last ? nch * 64 - nb : 0);
    p.j0 = p.my_chunks > SCAN_ROWBUF_CHUNKS ? p.my_chunks - SCAN_ROWBUF_CHUNKS : 0;
    p.n_slots = p.my_chunks - p.j0;
    return p;
}
// First staged position of the wave's queue (64 * j0) from its beam count alone: what scan_kernel recomputes where it needs it.
F110_PLAN_HD inline int scan_rowbuf_k0(int nbl)
{
    const int k0 = ((nbl + 63) & ~63) - SCAN_ROWBUF_CHUNKS * 64;
    return k0 > 0 ? k0 : 0;
}
// Byte offset in the row buffer of queue position k >= k0.  The beam at position k is chunk start + (k & 63) and chunk starts
// are multiples of 64 (set_beam_order), so this is slot (k >> 6) - j0, dword (beam & 63): (j - j0) * 256 + (beam & 63) * 4.
F110_PLAN_HD inline unsigned scan_rowbuf_offset(int k, int k0) { return (unsigned)(k - k0) * 4u; }
// F110_SCAN_ROWS: "lds" -> 1, "direct" -> 0; unset or anything else -> -1 (the rule decides)
inline int scan_rows_override(const char *v)
{
    if (!v) return -1;
    if (!strcmp(v, "lds")) return 1;
    if (!strcmp(v, "direct")) return 0;
    return -1;
}
// The rule: rows are staged exactly when the compact form of 256 slots is launched with an fp32 output (measured:
// profiles/r25_scan_rowbuf.txt).  S = 512 has 768 B to spare and the classic form none.
inline bool scan_rowbuf_choice(int lut, bool has_f32, int forced) { return lut == SCAN_ROWBUF_LUT && has_f32 && forced != 0; }

// Byte cell codes (f110_map.h: cell_elem_b; scan_kernel<.., 256, true, true>): the march of the compact form of 256 slots reads
// its codes from a table of bytes in 16-column strips, twice the cells per cache line (profiles/r26_scan_bytes.txt).
// F110_SCAN_CODES: "byte" -> 1, "word" -> 0; unset or anything else -> -1 (the rule decides)
inline int scan_codes_override(const char *v)
{
    if (!v) return -1;
    if (!strcmp(v, "byte")) return 1;
    if (!strcmp(v, "word")) return 0;
    return -1;
}
// The rule: bytes exactly where the row buffer is launched (the one instantiation of the 256-slot form the default run uses;
// every code of that form is below slot 256 by construction, so nothing else has to hold).
inline bool scan_codes_choice(int lut, bool rowbuf, int forced) { return lut == SCAN_ROWBUF_LUT && rowbuf && forced != 0; }
// `forced` as the rule may see it: a map without the byte table (the row-padded table did not fit the compact tables' limit,
// f110_map.h: map_bytes_fit) reads word codes whatever the override says
inline int scan_codes_available(bool has_table, int forced) { return has_table ? forced : 0; }

// F110_SCAN_FORM: "classic" -> 0, "compact256" -> 256, "compact512" -> 512; unset or anything else -> -1 (the rule decides)
inline int scan_form_override(const char *v)
{
    if (!v) return -1;
    if (!strcmp(v, "classic")) return 0;
    if (!strcmp(v, "compact256")) return 256;
    if (!strcmp(v, "compact512")) return 512;
    return -1;
}

struct ScanPlanIn {
    int n_cars, agents, num_beams;      // of the whole scan: the shard's cars, or f110_scan's poses (one agent each)
    const std::vector<StageSpec> *stages; // f110_set_scan_stages override (empty: the built-in choice)
    bool step;                          // the step's scan (else f110_scan's)
    const char *stores;                 // F110_SCAN_STORES: "plain", anything else (streaming stores) or NULL (unset)
    bool multi, wg_single;              // the scan reads a map per env; neighbouring cars on different maps (f110_assign_maps)
    int kind;                           // AND over the used map slots of their kinds (ScanLaunch::kind)
    int compact = 0;                    // S of the compact form the map offers and the rule (or the override) chose, 0: classic
    bool out_f32 = false;               // the scan writes an fp32 row
    int rows = -1;                      // scan_rows_override(F110_SCAN_ROWS)
    int codes = -1;                     // scan_codes_override(F110_SCAN_CODES)
};

struct ScanLaunch {
    int car_base, n_cars;
    int kind;                           // scan_kernel's IDENT | POW2 << 1 (origin unrotated / resolution 2^k on all its maps)
    int sm;                             // scan_kernel's SM: 0 f110_scan, 1 the step's, 2 the step's with plain stores
    int n_stages, stage_cars[SCAN_MAX_STAGES], stage_log2w[SCAN_MAX_STAGES]; // as in ScanArgs
    int grid, block;
    bool wg_single, order, events;      // workgroups of one wave; f110_set_scan_order applies (not on a map per env: a
                                        // workgroup stages one LUT); carries the event pair
    int lut;                            // 0: the classic instantiation (LUT_LDS slots); S: the compact one of S slots
    bool rowbuf;                        // the instantiation that stages fp32 rows in LDS (scan_rowbuf_choice)
    bool bytes;                         // the instantiation that reads the byte cell table (scan_codes_choice)
};

// The launches of one scan in launch order, or an error code (message through fail) where they would break what scan_kernel
// assumes of its stage list.  env_kind(env), the kind of an env's map, is called only when the scan is split.
template <typename EnvKind>
int plan_scan(const ScanPlanIn &in, EnvKind env_kind, std::vector<ScanLaunch> &out)
{
    // env blocks on maps of different kinds: one launch per run of envs of one kind, so that a single map with an odd
    // resolution or a rotated origin does not put every car on the general instantiation
    const bool split = in.multi && in.kind != 3;
    const int num_envs = in.n_cars / in.agents;
    out.clear();
    for (int e0 = 0, e1 = num_envs; e0 < num_envs; e0 = e1) {
        ScanLaunch l = {};
        l.kind = split ? env_kind(e0) : in.kind;
        if (split)
            for (e1 = e0 + 1; e1 < num_envs && env_kind(e1) == l.kind; e1++) {}
        l.car_base = e0 * in.agents; l.n_cars = (e1 - e0) * in.agents;
        // the compact form: the step's scan of a single map, origin unrotated and resolution 2^k (the written-out march)
        l.lut = in.step && !in.multi && in.kind == 3 ? in.compact : 0;
        l.rowbuf = scan_rowbuf_choice(l.lut, in.out_f32, in.rows);
        l.bytes = scan_codes_choice(l.lut, l.rowbuf, in.codes);
        l.wg_single = (in.multi && in.wg_single) || l.lut != 0; l.order = in.step && !in.multi; l.events = in.step && e0 == 0;
        const std::vector<StageSpec> stv = scan_stage_list(*in.stages, l.n_cars, in.agents, in.num_beams);
        // what the kernel assumes about the stage list, checked here where a mistake costs an error code instead of a
        // wave -> car mapping that runs off the argument block
        if (stv.size() < 1 || stv.size() > (size_t)SCAN_MAX_STAGES) return fail(F110_E_INVALID, "scan launch: %d stages (1..%d)", (int)stv.size(), SCAN_MAX_STAGES);
        // cars on different maps in two-wave workgroups: f110_assign_maps vouched for the pairs (2k, 2k+1) of ALL cars, so the
        // launch and each of its stages must start at an even car (a car_base across a kind boundary is even: an odd one sets
        // wg_single)
        long long cars = 0, waves = 0;
        for (const StageSpec &x : stv) {
            if (x.cars < 0 || x.lg < 0 || x.lg > SCAN_MAX_LOG2W) return fail(F110_E_INVALID, "scan launch: stage (%d cars, 2^%d waves per car) out of range", x.cars, x.lg);
            if (in.multi && !l.wg_single && (l.car_base + cars) % SCAN_WAVES) return fail(F110_E_INVALID, "scan launch: a stage of two-wave workgroups on a map per env starts at car %lld", l.car_base + cars);
            l.stage_cars[l.n_stages] = x.cars; l.stage_log2w[l.n_stages++] = x.lg;
            cars += x.cars; waves += x.cars << x.lg;
        }
        if (cars != l.n_cars) return fail(F110_E_INVALID, "scan launch: the stages cover %lld cars, the launch has %d", cars, l.n_cars);
        // the step's scan with streaming stores, except in very large launches (profiles/r04_scan_stores.txt L)
        const bool plain = in.stores ? strcmp(in.stores, "plain") == 0 : l.n_cars > 327680;
        l.sm = !in.step ? 0 : plain ? 2 : 1;
        l.grid = (int)(l.wg_single ? waves : (waves + SCAN_WAVES - 1) / SCAN_WAVES);
        l.block = l.wg_single ? WAVE : SCAN_THREADS;
        out.push_back(l);
    }
    return F110_OK;
}

} // namespace f110
