// f110_noise_kernels.h -- the kernels that produce, fill and move the noise rows (f110_noise.h holds the generator they run).
#pragma once
#include "f110_noise.h"

#pragma clang fp contract(off)

namespace f110 {

struct NoiseGenArgs {
    NoiseGen *gen;        // [slots]
    double *base;         // the table being filled
    long long mask, cap;
    long long lo;         // rows below lo are generated (the stream must advance) but not stored
    long long r1;         // every active slot is brought to r1 rows (a multiple of NOISE_MARK_ROWS when marks are kept)
    int nb;
    NoiseMark *marks;     // [slots][marks_cap] or NULL
    long long marks_cap;
    // re-production of dropped rows (blockIdx.y = chunk): rows [max(lo, 64 * (chunk0 + y)), min(r1, 64 * (chunk0 + y + 1))) from
    // marks[slot][chunk0 + y]; the generators' own states are neither read nor written
    int redo;
    long long chunk0;
    // powers and partial sums of the LCG multiplier: pcg_tab[j] = M^j, pcg_tab[65 + j] = 1 + M + ... + M^(j-1), j = 0 .. 64
    // (f110_noise_abi.hip computes them once): lane j's start state and the 64-step jump are two multiply-adds instead of loops
    const u128 *pcg_tab;
    // PER-ENV mode (f110_set_noise_per_env: every env its own seed, no limit on their number): slot = env, the table holds ONE
    // row per env (cap = 1), and every step produces the row the env's scan is about to add -- row `pend ? 0 : env_row[slot *
    // env_row_stride]` of the env's stream -- from the state the previous step left (or from the seed after a reset; or, after
    // a checkpoint was loaded, by running the stream forward from the seed without storing).  blockDim = 64 * waves, one
    // wavefront per env.
    const int32_t *env_row;
    int env_row_stride, n_env, reset_only;
    const uint8_t *env_pending;
    const NoiseGen *seeds;
};

// One wavefront per noise slot (grid = slots).
//
// The stream is walked in WINDOWS of 64 raw values, one per lane, and a window is always consumed whole: every lane treats
// its raw value as a candidate (99.3 % are accepted by one table compare); a rejected candidate resolves itself
// SPECULATIVELY, stepping a private copy of its own generator state through the raw values it would consume if it really
// were a candidate (wedge: one; tail: two per trial) -- no lane needs another lane's value.  Which lanes ARE candidates is
// then settled in stream order with a few scalar operations: a candidate's extra raws are not candidates (they are skipped,
// into the next window if need be: `skip`), everything else is.  The accepted candidates are numbered by a prefix count and
// stored as consecutive beams.  The window then advances by exactly 64 positions (one 128-bit multiply-add per lane), so
// there is no re-basing shuffle and the only state carried from window to window is (skip, beams produced).
static __global__ __launch_bounds__(256) void noise_rows_kernel(NoiseGenArgs a)
{
    __shared__ unsigned long long s_ki[256];
    __shared__ double s_wi[256], s_fi[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) { s_ki[i] = ZIG_KI[i]; s_wi[i] = ZIG_WI[i]; s_fi[i] = ZIG_FI[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int slot = a.env_row ? blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6) : blockIdx.x;
    if (a.env_row && slot >= a.n_env) return;
    NoiseGen g = a.gen[slot];
    if (a.env_row) {
        const bool pend = a.env_pending && a.env_pending[slot];
        if (a.reset_only && !pend) return;
        const long long r = pend ? 0 : (long long)a.env_row[(size_t)slot * (size_t)a.env_row_stride];
        if (r <= 0 || g.rows > r) { const NoiseGen sd = a.seeds[slot]; g.t_lo = sd.t_lo; g.t_hi = sd.t_hi; g.rows = 0; }
        a.lo = r < 0 ? 0 : r; a.r1 = a.lo + 1;
    }
    if (a.redo) {
        const long long ch = a.chunk0 + blockIdx.y;
        if (!g.on || !a.marks || ch >= a.marks_cap) return;
        const NoiseMark mk = a.marks[(size_t)slot * (size_t)a.marks_cap + (size_t)ch];
        g.t_lo = mk.t_lo; g.t_hi = mk.t_hi; g.rows = ch * NOISE_MARK_ROWS;
        a.r1 = a.r1 < g.rows + NOISE_MARK_ROWS ? a.r1 : g.rows + NOISE_MARK_ROWS;
    }
    if (!g.on || g.rows >= a.r1) return; // (wave-uniform)
    // the mark of the row this launch starts at (a launch ends where the next one starts: every multiple of 64 rows gets one)
    if (!a.redo && a.marks && lane == 0 && g.rows % NOISE_MARK_ROWS == 0 && g.rows / NOISE_MARK_ROWS < a.marks_cap) {
        NoiseMark mk; mk.t_lo = g.t_lo; mk.t_hi = g.t_hi;
        a.marks[(size_t)slot * (size_t)a.marks_cap + (size_t)(g.rows / NOISE_MARK_ROWS)] = mk;
    }
    const u128 M = pcg_mult(), inc = ((u128)g.inc_hi << 64) | (u128)g.inc_lo;
    // 64 steps at once: s -> A * s + C, A = M^64, C = (1 + M + ... + M^63) * inc
    const u128 A = a.pcg_tab[64], C = a.pcg_tab[65 + 64] * inc;
    u128 T = ((u128)g.t_hi << 64) | (u128)g.t_lo;
    T = a.pcg_tab[lane] * T + a.pcg_tab[65 + lane] * inc; // lane j: the state whose output is raw value p + j (j LCG steps ahead)
    const double std = g.std;
    const int nb = a.nb;
    const unsigned long long below = (1ull << lane) - 1ull;
    long long row = g.rows;
    int o = 0;     // beams of `row` produced so far
    int skip = 0;  // leading raw values of this window that belong to a candidate of an earlier window
    for (;;) {
        // distributions.c random_standard_normal: r = next_uint64; idx = r & 0xff; r >>= 8; sign = r & 1;
        // rabs = (r >> 1) & 0x000fffffffffffff; x = rabs * wi[idx]; if (sign) x = -x; if (rabs < ki[idx]) return x;
        unsigned long long r = pcg_out(T);
        const int idx = (int)(r & 0xffull);
        r >>= 8;
        const bool neg = (r & 1ull) != 0;
        const unsigned long long rabs = (r >> 1) & 0x000fffffffffffffull;
        double val = (double)rabs * s_wi[idx];
        if (neg) val = -val;
        const bool fast = rabs < s_ki[idx];
        int extras = 0;   // raw values this lane consumes beyond its own IF it is a candidate
        bool emits = true; // ... and whether it then yields a value (a rejected wedge draw does not: the draw starts over)
        const unsigned long long slow = __builtin_amdgcn_ballot_w64(!fast);
        if (slow != 0ull) {
            if (!fast) {
                u128 Q = T;
                if (idx == 0) {
                    // tail: xx = -inv_r * log1p(-U), yy = -log1p(-U) until yy + yy > xx * xx
                    for (;;) {
                        Q = Q * M + inc; const double u1 = pcg_double(pcg_out(Q));
                        Q = Q * M + inc; const double u2 = pcg_double(pcg_out(Q));
                        extras += 2;
                        const double xx = -ZIG_NOR_INV_R * log1p_glibc(-u1);
                        const double yy = -log1p_glibc(-u2);
                        if (yy + yy > xx * xx) { val = ((rabs >> 8) & 1ull) ? -(ZIG_NOR_R + xx) : ZIG_NOR_R + xx; break; }
                    }
                } else {
                    // wedge: ((fi[idx-1] - fi[idx]) * U + fi[idx]) < exp(-0.5 * x * x) ? return x : draw again
                    Q = Q * M + inc; const double u = pcg_double(pcg_out(Q));
                    extras = 1;
                    emits = ((s_fi[idx - 1] - s_fi[idx]) * u + s_fi[idx]) < exp(-0.5 * val * val);
                }
            }
        }
        // ---- which lanes are candidates: in stream order, a candidate's extras are not
        unsigned long long skipped = skip >= 64 ? ~0ull : ((1ull << skip) - 1ull);
        int carry = skip > 64 ? skip - 64 : 0;
        unsigned long long m = slow & ~skipped;
        while (m) {
            const int l = (int)__builtin_ctzll(m);
            m &= m - 1ull;
            const int e = __builtin_amdgcn_readlane(extras, l);
            int end = l + e;
            if (end > 63) { carry = carry > end - 63 ? carry : end - 63; end = 63; }
            if (end > l) {
                const unsigned long long hi = end == 63 ? ~0ull : ((1ull << (end + 1)) - 1ull);
                const unsigned long long range = hi & ~((2ull << l) - 1ull); // positions l+1 .. end
                skipped |= range;
                m &= ~range;
            }
        }
        const unsigned long long emitm = ~skipped & __builtin_amdgcn_ballot_w64(emits);
        const int n_emit = __popcll(emitm);
        const bool mine = (emitm >> lane) & 1ull;
        const int rank = __popcll(emitm & below);
        const long long left = (a.r1 - row) * (long long)nb - (long long)o; // beams this launch still has to produce
        const bool last = (long long)n_emit >= left;
        // ---- store: beam number o + rank of row `row`, running on into the next rows
        if (mine && (!last || (long long)rank < left)) {
            int gb = o + rank;
            long long rw = row;
            while (gb >= nb) { gb -= nb; rw++; }
            if (rw >= a.lo)
                a.base[((size_t)slot * (size_t)a.cap + (size_t)(rw & a.mask)) * (size_t)nb + gb] = 0.0 + std * val; // random_normal: loc + scale * x
        }
        if (last) {
            // the launch ends inside this window: the stream stands behind the candidate that produced the last beam
            unsigned long long mm = emitm;
            for (long long i = 1; i < left; i++) mm &= mm - 1ull;
            const int L = (int)__builtin_ctzll(mm);
            const int q = L + 1 + __builtin_amdgcn_readlane(extras, L); // (extras is 0 for a fast candidate)
            u128 Tq = shfl128(T, q < 63 ? q : 63);
            for (int i = 63; i < q; i++) Tq = Tq * M + inc;
            if (lane == 0 && !a.redo) {
                a.gen[slot].t_lo = (unsigned long long)Tq;
                a.gen[slot].t_hi = (unsigned long long)(Tq >> 64);
                a.gen[slot].rows = a.r1;
            }
            return;
        }
        o += n_emit;
        while (o >= nb) { o -= nb; row++; }
        skip = carry;
        T = A * T + C;
    }
}

// host-fed slot: plain fp64 rows [T, nb] (device staging copy; NULL: zeros) -> rows 0 .. T-1 of the slot's ring
static __global__ void noise_fill_kernel(const double *rows, long long T, int nb, double *base, int slot, long long cap, long long mask)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * nb) return;
    const long long r = i / nb;
    const int b = (int)(i - r * nb);
    base[((size_t)slot * (size_t)cap + (size_t)(r & mask)) * (size_t)nb + b] = rows ? rows[i] : 0.0;
}

// growth: rows lo .. hi-1 of every slot move to their places in a larger ring
static __global__ void noise_move_kernel(const double *src, long long scap, long long smask, double *dst, long long dcap,
                                  long long dmask, int slots, long long lo, long long hi, int nb)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (hi - lo) * nb;
    if (i >= per * slots) return;
    const int s = (int)(i / per);
    const long long k = i - (long long)s * per;
    const long long r = lo + k / nb;
    const int b = (int)(k % nb);
    dst[((size_t)s * (size_t)dcap + (size_t)(r & dmask)) * (size_t)nb + b] = src[((size_t)s * (size_t)scap + (size_t)(r & smask)) * (size_t)nb + b];
}

} // namespace f110
