// f110_noise_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_handle.h"
#include "f110_noise_kernels.h"

// ---------------------------------------------------------------- lidar noise (f110_noise.h)
__global__ void noise_publish_kernel(NoiseDesc *dst, NoiseDesc d) { *dst = d; }

static constexpr u128 PCG_MULT = ((u128)0x2360ED051FC65DA4ull << 64) | (u128)0x4385DF649FCCF645ull; // PCG_DEFAULT_MULTIPLIER_128

// The generator whose first output is the first raw value of np.random.PCG64 with state words w = {state_lo, state_hi, inc_lo,
// inc_hi}: one LCG step from NumPy's stored state (pcg64.h: step, then output).
static NoiseGen noise_gen_from_numpy(const uint64_t *w, double std_dev)
{
    const u128 t = (((u128)w[1] << 64) | w[0]) * PCG_MULT + (((u128)w[3] << 64) | w[2]);
    return NoiseGen{(unsigned long long)t, (unsigned long long)(t >> 64), w[2], w[3], std_dev, 0, 1, 0};
}

static long long pow2_at_least(long long n)
{
    long long c = 1;
    while (c < n) c <<= 1;
    return c;
}

// rows every generator slot holds; -1: no slot holds a generator
static long long generator_rows(const f110_handle *h)
{
    for (int sl = 0; sl < h->noise.slots; sl++)
        if (h->noise.slot[sl].kind == NoiseKind::generator) return h->noise.gen_rows;
    return -1;
}

// rows every active slot can serve
static void noise_recompute_hi(f110_handle *h)
{
    NoiseState &n = h->noise;
    long long hi = generator_rows(h);
    for (int sl = 0; sl < n.slots; sl++)
        if (n.slot[sl].kind == NoiseKind::host_table) hi = hi < 0 ? n.slot[sl].T : std::min(hi, n.slot[sl].T);
    n.on = hi >= 0;
    n.hi = hi < 0 ? 0 : hi;
}

// the descriptor the kernels read, written in stream order
static int noise_publish(f110_handle *h, hipStream_t st)
{
    const NoiseState &n = h->noise;
    const NoiseRows w = n.where(h->cfg.num_envs);
    // noise off: every row is the row of zeros; per-env: one row per env, produced on demand: every row counter is "in the table"
    const bool window = n.on && !n.per_env;
    const int lo = window ? (int)std::min(n.lo, (long long)0x7fffffff) : 0, hi = window ? (int)std::min(n.hi, (long long)0x7fffffff) : 0x7fffffff;
    const NoiseDesc d{w.base, w.mask, w.cap, lo, hi, w.slots, 0};
    hipLaunchKernelGGL(noise_publish_kernel, dim3(1), dim3(1), 0, st, n.d_desc.get(), d);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// publishes on `st` and records `order_ev` there: the next prefetch runs behind the work enqueued on `st` so far
static int noise_publish_ordered(f110_handle *h, hipStream_t st)
{
    if (int rc = noise_publish(h, st)) return rc;
    HIP_TRY(hipEventRecord(h->noise.order_ev.get(), st));
    h->noise.order_ev_set = true;
    return F110_OK;
}

// Cold paths publish on the null stream and wait for it: the callers' streams do not synchronise with the null stream, and a
// later publish in stream order must not be overtaken by this one.
static int noise_publish_cold(f110_handle *h)
{
    if (int rc = noise_publish(h, nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return F110_OK;
}

// (Re)allocates the table for `slots` slots of `cap` rows, every pair {0, side}; rows lo .. hi-1 of the old table move
// over.  Cold path: synchronises the device, so nothing reads the old table any more and the new one is complete on return.
static int noise_resize(f110_handle *h, int slots, long long cap)
{
    NoiseState &n = h->noise;
    const int nb = h->cfg.num_beams;
    if ((long long)slots * cap >= 0x7fffffffll) return fail(F110_E_INVALID, "noise table: %d slots x %lld rows exceed 2^31 rows", slots, cap);
    HIP_TRY(hipDeviceSynchronize());
    DevBuf<double> nt;
    const size_t total = (size_t)slots * (size_t)cap;
    HIP_TRY(nt.alloc(total * nb));
    {
        const long long items = (long long)total * nb;
        hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, nullptr, (const double *)nullptr,
                           (long long)total, nb, nt.get(), 0, (long long)total, (long long)0x7fffffffffffffffll);
    }
    if (n.d_rows.get() && n.on && n.hi > n.lo) {
        const int ms = std::min(slots, n.slots);
        const long long items = (n.hi - n.lo) * nb * ms;
        hipLaunchKernelGGL(noise_move_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, nullptr, n.d_rows.get(), n.cap,
                           n.cap - 1, nt.get(), cap, cap - 1, ms, n.lo, n.hi, nb);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    n.d_rows = std::move(nt);
    n.cap = cap;
    n.slots = slots;
    h->epoch++; // the scan takes the table's base and size by value (ScanArgs::noise_base): a re-allocation is a new launch
    return noise_publish_cold(h);
}

int noise_init(f110_handle *h)
{
    NoiseState &n = h->noise;
    HIP_TRY(n.d_desc.alloc(1));
    HIP_TRY(n.d_gen.alloc(F110_MAX_NOISE_SLOTS));
    HIP_TRY(hipMemset(n.d_gen.get(), 0, sizeof(NoiseGen) * F110_MAX_NOISE_SLOTS));
    HIP_TRY(h->d_err.alloc(1));
    HIP_TRY(hipMemset(h->d_err.get(), 0, sizeof(uint32_t)));
    HIP_TRY(hipStreamCreateWithFlags(n.stream.put(), hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(n.ev.put(), hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(n.order_ev.put(), hipEventDisableTiming));
    {   // M^j and 1 + M + ... + M^(j-1), j = 0 .. 64 (mod 2^128)
        u128 tab[130];
        u128 pw = 1, sm = 0;
        for (int j = 0; j <= 64; j++) { tab[j] = pw; tab[65 + j] = sm; sm = sm * PCG_MULT + 1; pw *= PCG_MULT; }
        HIP_TRY(n.d_pcg_tab.upload(tab, 130));
    }
    return noise_resize(h, 1, 1); // noise off: one row of zeros
}

// a prefetch in flight on the generator's stream becomes part of the table for work enqueued on `st` from now on
static int noise_absorb_pending(f110_handle *h, hipStream_t st)
{
    NoiseState &n = h->noise;
    if (!n.pending_hi) return F110_OK;
    HIP_TRY(hipStreamWaitEvent(st, n.ev.get(), 0));
    n.gen_rows = std::max(n.gen_rows, n.pending_hi);
    n.pending_hi = 0;
    noise_recompute_hi(h);
    return noise_publish(h, st);
}

// room for the marks of rows 0 .. rows-1 of every slot (cold path when it grows: synchronises)
static int noise_marks_reserve(f110_handle *h, long long rows)
{
    NoiseState &n = h->noise;
    const long long need = rows / NOISE_MARK_ROWS + 2;
    if (n.d_marks.get() && n.marks_slots == n.slots && need <= n.marks_cap) return F110_OK;
    long long cap = std::max<long long>(n.marks_cap, 1 << 12);
    while (cap < need) cap <<= 1;
    HIP_TRY(hipDeviceSynchronize());
    DevBuf<NoiseMark> nm;
    HIP_TRY(nm.alloc((size_t)cap * (size_t)n.slots));
    HIP_TRY(hipMemset(nm.get(), 0, sizeof(NoiseMark) * (size_t)cap * (size_t)n.slots));
    if (n.d_marks.get() && n.marks_cap > 0)
        for (int sl = 0; sl < std::min(n.marks_slots, n.slots); sl++)
            HIP_TRY(hipMemcpy(nm.get() + (size_t)sl * cap, n.d_marks.get() + (size_t)sl * n.marks_cap, sizeof(NoiseMark) * (size_t)n.marks_cap, hipMemcpyDeviceToDevice));
    n.d_marks = std::move(nm); n.marks_cap = cap; n.marks_slots = n.slots;
    return F110_OK;
}

// what both launches of noise_rows_kernel on the ring pass: generator states, table from row `lo`, marks
static NoiseGenArgs ring_gen_args(const f110_handle *h, long long lo)
{
    const NoiseState &n = h->noise;
    NoiseGenArgs g;
    memset(&g, 0, sizeof(g));
    g.gen = n.d_gen.get(); g.base = n.d_rows.get(); g.mask = n.cap - 1; g.cap = n.cap; g.lo = lo; g.nb = h->cfg.num_beams;
    g.marks = n.d_marks.get(); g.marks_cap = n.marks_cap; g.pcg_tab = n.d_pcg_tab.get();
    return g;
}

// Brings every generator slot (there is one at least) to r1 rows (a multiple of 64), 64 rows per launch: every launch leaves
// the mark of the row it starts at (f110_noise.h NoiseMark), so that dropped rows can be produced again without rewinding the stream.
static int noise_launch_generator(f110_handle *h, long long r1, hipStream_t st)
{
    const NoiseState &n = h->noise;
    const long long have = std::min(r1, std::max(generator_rows(h), n.pending_hi));
    if (int rc = noise_marks_reserve(h, r1)) return rc;
    NoiseGenArgs g = ring_gen_args(h, n.lo);
    for (long long r = (have / NOISE_MARK_ROWS + 1) * NOISE_MARK_ROWS; ; r += NOISE_MARK_ROWS) {
        g.r1 = std::min(r, r1);
        hipLaunchKernelGGL(noise_rows_kernel, dim3(n.slots), dim3(64), 0, st, g);
        if (r >= r1) break;
    }
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// Rows [lo, hi) of every generator slot are produced AGAIN from the marks (they were dropped from the ring when the floor rose):
// one wavefront per slot and 64 rows, all at once -- the generators stay where they are.
static int noise_redo_rows(f110_handle *h, long long lo, long long hi, hipStream_t st)
{
    if (hi <= lo) return F110_OK;
    NoiseGenArgs g = ring_gen_args(h, lo);
    g.r1 = hi; g.redo = 1; g.chunk0 = lo / NOISE_MARK_ROWS;
    const long long chunks = (hi + NOISE_MARK_ROWS - 1) / NOISE_MARK_ROWS - g.chunk0;
    for (long long c0 = 0; c0 < chunks; c0 += 32768) { // (grid.y <= 65535)
        NoiseGenArgs gg = g;
        gg.chunk0 = g.chunk0 + c0;
        hipLaunchKernelGGL(noise_rows_kernel, dim3(h->noise.slots, (unsigned)std::min<long long>(32768, chunks - c0)), dim3(64), 0, st, gg);
    }
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

// The cold-path entry of the calls below, once their arguments are validated (NOISE_COLD_ENTRY): the handle's device, nothing
// running on it any more (the side stream included), and a call that sets ring-mode noise leaves per-env mode.
static int noise_quiesce(f110_handle *h, bool leave_per_env)
{
    HIP_TRY(hipStreamSynchronize(h->noise.stream.get()));
    HIP_TRY(hipDeviceSynchronize());
    if (leave_per_env && h->noise.per_env) { h->noise.per_env = false; h->epoch++; }
    return F110_OK;
}

#define NOISE_COLD_ENTRY(h, leave_per_env) \
    ON_DEVICE((h)->cfg.device);            \
    if (int rc_ = noise_quiesce(h, leave_per_env)) return rc_

// every generator slot restarts at row 0 (its seed state); rows below the floor will be skipped, not stored
static int noise_restart_generators(f110_handle *h)
{
    if (int rc = noise_quiesce(h, false)) return rc;
    NoiseState &n = h->noise;
    n.pending_hi = 0; n.gen_rows = 0;
    for (int sl = 0; sl < n.slots; sl++)
        if (n.slot[sl].kind == NoiseKind::generator)
            HIP_TRY(hipMemcpy(n.d_gen.get() + sl, &n.slot[sl].seed, sizeof(NoiseGen), hipMemcpyHostToDevice));
    noise_recompute_hi(h);
    return F110_OK;
}

static int check_noise_slot(f110_handle *h, int slot, const char *who)
{
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    if (slot < 0 || slot >= F110_MAX_NOISE_SLOTS) return fail(F110_E_INDEX, "%s: noise slot %d outside 0..%d", who, slot, F110_MAX_NOISE_SLOTS - 1);
    return F110_OK;
}

extern "C" int f110_set_noise_slot(f110_handle *h, int32_t slot, const double *tbl, int64_t T)
{
    int rc = check_noise_slot(h, slot, "f110_set_noise_slot");
    if (rc) return rc;
    if (T < 1 || !tbl) return fail(F110_E_INVALID, "f110_set_noise_slot: bad table (T >= 1 rows; f110_set_noise_table(h, NULL, 0) switches noise off)");
    NOISE_COLD_ENTRY(h, true);
    NoiseState &n = h->noise;
    const int nb = h->cfg.num_beams;
    if (n.lo > 0) { n.lo = 0; if ((rc = noise_restart_generators(h))) return rc; } // host-fed rows start at 0
    n.slot[slot] = {NoiseKind::host_table, T, NoiseGen{}};
    HIP_TRY(hipMemset(n.d_gen.get() + slot, 0, sizeof(NoiseGen))); // (the slot may have held a generator)
    const int slots = std::max(n.slots, slot + 1);
    const long long cap = std::max(n.cap, pow2_at_least(T));
    if (slots != n.slots || cap != n.cap || !n.on) {
        // (first table after "noise off": the one-row table makes way)
        if (!n.on) { n.lo = 0; n.hi = 0; }
        if ((rc = noise_resize(h, slots, std::max(cap, (long long)2)))) return rc;
    }
    {   // stage the rows on the device and place them in the slot's ring
        DevBuf<double> stage;
        HIP_TRY(stage.upload(tbl, (size_t)T * nb));
        const long long items = (long long)T * nb;
        hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, nullptr, (const double *)stage.get(),
                           (long long)T, nb, n.d_rows.get(), slot, n.cap, n.cap - 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    noise_recompute_hi(h);
    return noise_publish_cold(h);
}

extern "C" int f110_set_noise_table(f110_handle *h, const double *tbl, int64_t T)
{
    if (!h) return fail(F110_E_INVALID, "f110_set_noise_table: null handle");
    if (T < 0 || (T > 0 && !tbl)) return fail(F110_E_INVALID, "f110_set_noise_table: bad table");
    if (T > 0) return f110_set_noise_slot(h, 0, tbl, T);
    // noise off: every slot forgets its table / generator
    NOISE_COLD_ENTRY(h, true);
    NoiseState &n = h->noise;
    for (auto &ns : n.slot) { ns.kind = NoiseKind::unset; ns.T = 0; }
    n.pending_hi = 0; n.gen_rows = 0;
    HIP_TRY(hipMemset(n.d_gen.get(), 0, sizeof(NoiseGen) * F110_MAX_NOISE_SLOTS));
    n.on = false; n.lo = 0; n.hi = 0;
    if (n.multi) { n.multi = false; h->epoch++; }
    return noise_resize(h, 1, 1);
}

extern "C" int f110_set_noise_generator(f110_handle *h, int32_t slot, const uint64_t *pcg64, double std_dev)
{
    int rc = check_noise_slot(h, slot, "f110_set_noise_generator");
    if (rc) return rc;
    if (!pcg64 || !(std_dev >= 0) || !std::isfinite(std_dev)) return fail(F110_E_INVALID, "f110_set_noise_generator: bad arguments");
    if (!(pcg64[2] & 1ull)) return fail(F110_E_INVALID, "f110_set_noise_generator: the PCG64 increment must be odd");
    NOISE_COLD_ENTRY(h, true);
    NoiseState &n = h->noise;
    n.slot[slot] = {NoiseKind::generator, 0, noise_gen_from_numpy(pcg64, std_dev)};
    const int slots = std::max(n.slots, slot + 1);
    if (slots != n.slots || !n.on || n.cap < 2) {
        if (!n.on) { n.lo = 0; n.hi = 0; }
        if ((rc = noise_resize(h, slots, std::max(n.cap, (long long)F110_NOISE_INITIAL_ROWS)))) return rc;
    }
    // a new stream in one slot: every generator slot goes back to row 0, so that all of them stand at the same row again
    n.lo = 0;
    n.on = true;
    if ((rc = noise_restart_generators(h))) return rc;
    return noise_publish_cold(h);
}

// Every env its own stream (reference: every F110Env is constructed with its own `seed`, f110_env.py:102-105; its cars re-create
// default_rng(seed) at every reset, base_classes.py:117,202).  No table of rows per seed and no limit on the number of seeds:
// an env's generator state lives on the device and the row its scan adds is produced in front of the scan, every step
// (noise_rows_kernel in per-env mode, one wavefront per env).  pcg64 = host [num_envs][4] {state_lo, state_hi, inc_lo, inc_hi}.
extern "C" int f110_set_noise_per_env(f110_handle *h, const uint64_t *pcg64, double std_dev)
{
    if (!h || !pcg64 || !(std_dev >= 0) || !std::isfinite(std_dev)) return fail(F110_E_INVALID, "f110_set_noise_per_env: bad arguments");
    const int B = h->cfg.num_envs, nb = h->cfg.num_beams;
    std::vector<NoiseGen> seeds((size_t)B);
    for (int e = 0; e < B; e++) {
        const uint64_t *w = pcg64 + (size_t)e * 4;
        if (!(w[2] & 1ull)) return fail(F110_E_INVALID, "f110_set_noise_per_env: env %d: the PCG64 increment must be odd", e);
        seeds[(size_t)e] = noise_gen_from_numpy(w, std_dev);
    }
    NOISE_COLD_ENTRY(h, false);
    NoiseState &n = h->noise;
    if (!n.d_env_gen.get()) { // all four buffers, or none
        DevBuf<NoiseGen> gen, seed;
        DevBuf<double> rows;
        DevBuf<int32_t> ident;
        std::vector<int32_t> id((size_t)B);
        for (int e = 0; e < B; e++) id[(size_t)e] = e;
        HIP_TRY(gen.alloc((size_t)B));
        HIP_TRY(seed.alloc((size_t)B));
        HIP_TRY(rows.alloc((size_t)B * nb));
        HIP_TRY(ident.upload(id.data(), (size_t)B));
        n.d_env_gen = std::move(gen); n.d_env_seed = std::move(seed); n.d_env_rows = std::move(rows); n.d_env_ident = std::move(ident);
    }
    HIP_TRY(hipMemcpy(n.d_env_seed.get(), seeds.data(), sizeof(NoiseGen) * (size_t)B, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(n.d_env_gen.get(), seeds.data(), sizeof(NoiseGen) * (size_t)B, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(n.d_env_rows.get(), 0, sizeof(double) * (size_t)B * nb));
    n.per_env = true;
    n.on = true;
    h->epoch++;
    return noise_publish_cold(h);
}

extern "C" int f110_noise_prefetch(f110_handle *h, int64_t rows)
{
    if (!h) return fail(F110_E_INVALID, "f110_noise_prefetch: null handle");
    NoiseState &n = h->noise;
    if (n.per_env || !n.on || n.pending_hi) return F110_OK;
    const long long have = generator_rows(h);
    if (have < 0 || rows <= have) return F110_OK;
    const long long r1 = (rows + 63) & ~63ll;
    if (r1 - n.lo > n.cap) return F110_OK; // needs a larger table: f110_noise_ensure grows it when the rows are due
    ON_DEVICE(h->cfg.device);
    // The generator appends rows have .. r1-1 into ring places whose previous tenants lie below the floor.  Steps that were
    // enqueued BEFORE the floor was raised may still read those tenants, and a generator kernel enqueued on the caller's
    // stream (f110_noise_ensure) works on the same generator states: both recorded `order_ev` there, and this launch waits for it.
    if (n.order_ev_set) { HIP_TRY(hipStreamWaitEvent(n.stream.get(), n.order_ev.get(), 0)); n.order_ev_set = false; }
    if (int rc = noise_launch_generator(h, r1, n.stream.get())) return rc;
    HIP_TRY(hipEventRecord(n.ev.get(), n.stream.get()));
    n.pending_hi = r1;
    return F110_OK;
}

extern "C" int f110_noise_ensure(f110_handle *h, int64_t rows, void *stream)
{
    if (!h) return fail(F110_E_INVALID, "f110_noise_ensure: null handle");
    NoiseState &n = h->noise;
    if (n.per_env || !n.on || rows <= n.hi) return F110_OK; // (per-env rows are produced by the step itself)
    if (int rc = check_device(h, "f110_noise_ensure")) return rc;
    hipStream_t st = (hipStream_t)stream;
    int rc = noise_absorb_pending(h, st);
    if (rc) return rc;
    if (rows <= n.hi) return F110_OK;
    for (int sl = 0; sl < n.slots; sl++)
        if (n.slot[sl].kind == NoiseKind::host_table && n.slot[sl].T < rows)
            return fail(F110_E_INVALID, "f110_noise_ensure: noise slot %d is a host table of %lld rows, %lld are needed (upload a longer "
                        "table with f110_set_noise_slot, or use f110_set_noise_generator)", sl, n.slot[sl].T, (long long)rows);
    const long long r1 = (rows + 63) & ~63ll;
    if (r1 - n.lo > n.cap) // the ring is too small for rows lo .. r1-1: a larger one (cold path, synchronises)
        if ((rc = noise_resize(h, n.slots, pow2_at_least(std::max(2 * n.cap, r1 - n.lo))))) return rc;
    if ((rc = noise_launch_generator(h, r1, st))) return rc;
    n.gen_rows = r1;
    noise_recompute_hi(h);
    return noise_publish_ordered(h, st); // the next prefetch (side stream) runs behind this generator launch
}

extern "C" int f110_noise_set_floor(f110_handle *h, int64_t lo, void *stream)
{
    if (!h || lo < 0) return fail(F110_E_INVALID, "f110_noise_set_floor: bad arguments");
    NoiseState &n = h->noise;
    if (n.per_env || !n.on || lo == n.lo) return F110_OK;
    if (int rc = check_device(h, "f110_noise_set_floor")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (lo > n.lo) {
        for (int sl = 0; sl < n.slots; sl++)
            if (n.slot[sl].kind == NoiseKind::host_table) return fail(F110_E_INVALID, "f110_noise_set_floor: noise slot %d is a host table (rows are only dropped from generated noise)", sl);
        if (lo > n.hi) return fail(F110_E_INVALID, "f110_noise_set_floor: floor %lld above the %lld rows produced", (long long)lo, n.hi);
        n.lo = lo;
        // the steps enqueued so far may read rows below the new floor: the prefetch that recycles their places waits for them
        return noise_publish_ordered(h, st);
    }
    // The floor comes down (a car was reset while others run on): rows lo .. old floor - 1 are produced again, from the marks
    // the generators left every 64 rows -- one wavefront per slot and 64 rows, in the caller's stream; the generators themselves
    // stay where they are.  The ring has to span floor .. rows produced: it grows if it must (cold path).
    int rc = noise_absorb_pending(h, st);
    if (rc) return rc;
    const long long old_lo = n.lo;
    if (n.hi - lo > n.cap)
        if ((rc = noise_resize(h, n.slots, pow2_at_least(n.hi - lo)))) return rc;
    n.lo = lo;
    if ((rc = noise_redo_rows(h, lo, std::min(old_lo, n.hi), st))) return rc;
    return noise_publish_ordered(h, st);
}

extern "C" int f110_noise_info(f110_handle *h, int64_t *lo, int64_t *hi, int64_t *cap, int32_t *slots, int64_t *bytes)
{
    if (!h) return fail(F110_E_INVALID, "f110_noise_info: null handle");
    const NoiseState &n = h->noise;
    if (lo) *lo = n.lo;
    if (hi) *hi = n.on ? n.hi : 0; // (rows a prefetch is still producing are not counted: f110_noise_ensure makes them readable)
    if (cap) *cap = n.cap;
    if (slots) *slots = n.slots;
    if (bytes) *bytes = (long long)n.slots * n.cap * h->cfg.num_beams * (long long)sizeof(double);
    return F110_OK;
}

extern "C" int f110_noise_read(f110_handle *h, int32_t slot, int64_t row0, int64_t n_rows, double *out)
{
    int rc = check_noise_slot(h, slot, "f110_noise_read");
    if (rc) return rc;
    if (!out || n_rows < 0) return fail(F110_E_INVALID, "f110_noise_read: bad arguments");
    NOISE_COLD_ENTRY(h, false);
    const NoiseState &n = h->noise;
    const long long hi = n.on ? std::max(n.hi, n.pending_hi) : 0;
    if (slot >= n.slots || row0 < n.lo || row0 + n_rows > hi)
        return fail(F110_E_INDEX, "f110_noise_read: rows %lld..%lld of slot %d; the table holds rows %lld..%lld of %d slots", (long long)row0,
                    (long long)(row0 + n_rows - 1), slot, n.lo, hi - 1, n.slots);
    const int nb = h->cfg.num_beams;
    for (long long r = row0; r < row0 + n_rows; r++)
        HIP_TRY(hipMemcpy(out + (size_t)(r - row0) * nb, n.d_rows.get() + ((size_t)slot * n.cap + (size_t)(r & (n.cap - 1))) * nb,
                          (size_t)nb * sizeof(double), hipMemcpyDeviceToHost));
    return F110_OK;
}

extern "C" int f110_assign_noise(f110_handle *h, const int32_t *slot_of_env)
{
    if (!h) return fail(F110_E_INVALID, "f110_assign_noise: null handle");
    NoiseState &n = h->noise;
    const int B = h->cfg.num_envs;
    std::vector<int32_t> m(B, 0);
    bool multi = false;
    if (slot_of_env)
        for (int e = 0; e < B; e++) {
            const int k = slot_of_env[e];
            if (k < 0 || k >= n.slots || (n.on && n.slot[k].kind == NoiseKind::unset))
                return fail(F110_E_INDEX, "f110_assign_noise: env %d uses noise slot %d, which holds neither a table nor a generator", e, k);
            m[e] = k;
            multi = multi || k != 0;
        }
    ON_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(n.d_env_slot.upload(m.data(), B));
    n.multi = multi;
    h->epoch++;
    return F110_OK;
}
