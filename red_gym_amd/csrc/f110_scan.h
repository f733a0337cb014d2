// f110_scan.h -- scan_kernel (wave per car): ScanSimulator2D.scan + noise + iTTC, with its map view, look-ups and march loops.
#pragma once
#include "f110_bounds.h"
#include "f110_device.h"
#include "f110_map.h"
#include "f110_scan_plan.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace f110 {

constexpr int REFILL_MIN_IDLE = 44; // refill the wave's beam slots once this many lanes idle (32 .. 56 swept: profiles/r05_scan_budget.txt)

// device-side view of MapDev with the cell table behind a buffer resource descriptor
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct MapView {
    __amdgpu_buffer_rsrc_t cells_rsrc;
    u32x4 cells_words;   // the same descriptor as four words (an asm statement's operand)
    unsigned row_bias, strip_m16; // row_bias = strip_bytes + 16, strip_m16 = strip_bytes - 16
    const MapDev *desc;  // rare paths (far cells, escape cells) re-read their table pointers from the descriptor:
                         // pointers that need not be kept in scalar registers across the march loop
    int H, W;
    double res, rinv, ox, oy, oc, os, wres, hres;
    double nox, noy; // -ox * rinv, -oy * rinv (exact when rinv is a power of two)
    F110_BOUNDS_ONLY(uint32_t *err = nullptr; unsigned cells_bytes = 0; unsigned off_far = OFF_FAR; unsigned cells_skip = 0;)
    // cells: the table the march reads, m.cells or one of m.cells_c (same layout and size) or m.cells_b (bytes, 16-column strips);
    // bytes: its size; off_far: its far marker's code
    __device__ void init(const MapDev &m, const void *cells, unsigned bytes, unsigned far_code)
    {
        F110_BOUNDS_ONLY(cells_bytes = bytes; off_far = far_code;)
        (void)far_code;
        cells_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(cells), 0, (int)bytes, 0x00020000);
        cells_words.x = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)cells);
        cells_words.y = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)cells >> 32) & 0xffffu);
        cells_words.z = __builtin_amdgcn_readfirstlane(bytes); cells_words.w = __builtin_amdgcn_readfirstlane(0x00020000u);
        row_bias = m.strip_bytes + 16u; strip_m16 = m.strip_bytes - 16u; desc = &m; H = m.H; W = m.W; res = m.res; rinv = m.rinv;
        ox = m.ox; oy = m.oy; oc = m.oc; os = m.os; wres = m.wres; hres = m.hres;
        nox = -m.ox * m.rinv; noy = -m.oy * m.rinv;
    }
    // The row-padded byte table (m.cells_b, 16-column strips of strip_bytes_b bytes, row r stored at r + P: f110_map.h) behind a
    // descriptor that starts at strip 1, map row 0 -- skip = strip_bytes_b + 16 * (1 + P) bytes INTO the table -- and is that
    // much shorter: the +1 strip, the +1 border row and the P padding rows of a cell's offset are in the base, so the march
    // forms (c >> 4) * (strip_bytes_b - 16) + c + (r << 4) with one shift-add for row and column together.  What lies in front
    // of the new base is strip 0 (columns -16 .. -1) and the padding and border rows of strip 1: bytes that hold 0, whose
    // offsets are now negative, i.e. out of range, and read as 0 -- the slot they hold.  row_bias and strip_m16 are the byte
    // table's here; the second table (dist_lookup_far) keeps the u16 tables' geometry, which it reads from the descriptor.
    __device__ void init_bytes(const MapDev &m, unsigned far_code)
    {
        const unsigned skip = m.strip_bytes_b + 16u * (1u + m.pad_rows);
        init(m, m.cells_b + skip, m.cells_b_bytes - skip, far_code);
        row_bias = m.strip_bytes_b + 16u; strip_m16 = m.strip_bytes_b - 16u;
        F110_BOUNDS_ONLY(cells_bytes = m.cells_b_bytes; cells_skip = skip;)
    }
};

struct ScanDev {
    int nb, theta_dis;
    double fov, eps, max_range, inc; // inc = theta_index_increment (laser_models.py:368)
    unsigned long long inc_fx;       // inc in 24.40 fixed point
    int cs_len;                      // entries of cs (theta_dis * repetitions)
    const double2 *cs;               // [cs_len] {cos, sin} of the LUT angles (laser_models.py:379-381), repeated
};

// laser_models.py:56-104: (x, y) -> distance-table value, branch-free.  IDENT: origin
// yaw == 0 (c=1, s=0: the rotation is the identity in exact arithmetic).  POW2:
// resolution is a power of two, so q = x_rot * (1/res) IS the reference's quotient and
// "x_rot < 0 or x_rot >= width*res" (:79) is exactly "floor(q) outside [0, W)".
// laser_models.py:71-84 (xy_2_rc): the cell (column ci, row ri) of a point, un-clamped (a saturating conversion: any value
// outside [0, W) x [0, H) means "out of bounds", which cell_offset maps onto the table's border = the reference's dt[-1, -1] read).
template <bool IDENT, bool POW2>
__device__ inline void cell_index(const MapView &m, double x, double y, int &ci, int &ri)
{
    double xr = 0, yr = 0, qx, qy;
    if (IDENT && POW2) {
        // q = (x - ox) * 2^k is ONE fma: scaling by a power of two commutes with rounding, so
        // fma(x, 2^k, -ox*2^k) == fl(x - ox) * 2^k bit for bit (the reference's two roundings
        // collapse because the second is exact).  Explicit fma: contraction stays off.
        qx = __builtin_fma(x, m.rinv, m.nox);
        qy = __builtin_fma(y, m.rinv, m.noy);
    } else {
        const double xt = x - m.ox, yt = y - m.oy;
        if (IDENT) { xr = xt; yr = yt; }
        else { xr = xt * m.oc + yt * m.os; yr = -xt * m.os + yt * m.oc; }
        qx = xr * m.rinv;
        qy = yr * m.rinv;
    }
    const double fx = floor(qx), fy = floor(qy);
    ci = (int)fx; ri = (int)fy; // saturating conversion; the clamp in cell_offset finishes the job
    if (!POW2) {
        // int(x_rot/resolution) and the bounds test need the IEEE quotient: x_rot*(1/res) is
        // within ~2e-12 of it, so only quotients within 1e-9 of an integer (where truncation
        // or a bound could flip) replay the reference's own expressions.
        const double rx = qx - fx, ry = qy - fy;
        const bool near_int = (rx < 1e-9) || (rx > 1. - 1e-9) || (ry < 1e-9) || (ry > 1. - 1e-9);
        if (__builtin_expect(vote(near_int) != 0ull, 0)) {
            if (near_int) {
                const bool out = (xr < 0) || (xr >= m.wres) || (yr < 0) || (yr >= m.hres);
                ci = out ? -1 : min((int)(xr / m.res), m.W - 1);
                ri = out ? -1 : min((int)(yr / m.res), m.H - 1);
            }
        }
    }
}

// byte offset of the cell under (column ci, row ri) in the strip table: both clamped onto the border.  BYTES: in the byte table
// of 16-column strips (f110_map.h: cell_elem_b), (c >> 4) * (S - 16) + c -- the column is added, not shift-added
// (row_bias, strip_m16: of the table the offset is for -- MapView's, except for the second table under the byte march)
template <bool BYTES = false>
__device__ inline unsigned cell_offset(const MapView &m, int ci, int ri, unsigned row_bias, unsigned strip_m16)
{
    const int cc = med3_i32(ci, -1, m.W);      // column -1..W (both ends are border cells)
    const int rr = med3_i32(ri, -1, m.H);      // row -1..H
    // strip (cc >> 3) + 1 (arithmetic shift: column -1 is the last column of strip 0), 16 bytes per row inside a strip.  The
    // +1 strip and the +1 border row ride in the constant of the shift-add (`row_bias` = strip_bytes + 16, a multiple of 16),
    // so no add is spent on the padding and the offset never goes negative; asm so that the constant is not re-associated
    // into a trailing add.  (c >> 3) * S + (c & 7) * 2 == (c >> 3) * (S - 16) + c * 2: no masking of the column bits needed
    unsigned row16;
    asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(row16) : "v"(rr), "s"(row_bias));
    if (BYTES) return (unsigned)(__mul24(cc >> 4, (int)strip_m16) + (int)(((unsigned)rr << 4) + (unsigned)cc)); // (against init_bytes' base)
    unsigned rc;
    asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(rc) : "v"(cc), "v"(row16));
    return (unsigned)(__mul24(cc >> 3, (int)strip_m16) + (int)rc);
}
template <bool BYTES = false>
__device__ inline unsigned cell_offset(const MapView &m, int ci, int ri) { return cell_offset<BYTES>(m, ci, ri, m.row_bias, m.strip_m16); }

// One table look-up (laser_models.py:56-104 distance_transform): the value of the cell under (x, y), or -0.0 when the cell
// carries the far marker (dist_lookup_far finishes those).  The caller runs it under the EXEC mask of the rays that are
// still marching: a finished ray issues nothing.
template <bool IDENT, bool POW2, bool BYTES = false>
__device__ inline double dist_lookup(const MapView &m, const double *lds_lut, double x, double y)
{
    int ci, ri;
    cell_index<IDENT, POW2>(m, x, y, ci, ri);
    const unsigned off = cell_offset<BYTES>(m, ci, ri);
    // buffer load: 32-bit per-lane offset against a scalar descriptor (BYTES: the cell holds the slot, 8 bytes each)
    unsigned code = BYTES ? (unsigned)(unsigned char)__builtin_amdgcn_raw_buffer_load_b8(m.cells_rsrc, (int)off, 0, 0) << 3
                          : (unsigned)(unsigned short)__builtin_amdgcn_raw_buffer_load_b16(m.cells_rsrc, (int)off, 0, 0);
#if defined(F110_BOUNDS)
    // the offset inside the table (BYTES: counted from the table's start, where init_bytes' descriptor starts cells_skip later;
    // the border row and column lie in front of it and wrap back)
    F110_BCHK(BYTES ? off + m.cells_skip < m.cells_bytes : off + 2u <= m.cells_bytes, BT_LUT_CODE, m.err);
    F110_BCHK(code <= m.off_far && (code & 7u) == 0u, BT_LUT_CODE, m.err); // (a compact table: nothing behind ITS marker)
    code = code <= m.off_far ? (code & ~7u) : 0u;
#endif
    // the loaded value IS the LDS byte offset of the distance: one ds_read_b64
    double d = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(lds_lut) + code);
    asm volatile("" : "+v"(d)); // pin the LDS read (keeps it a ds_read, not a flat load through a selected pointer)
    return d;
}

// the rare path behind the far marker: the cell's full rank from the second table, then the global LUT or the fp64 table
// (BYTES: the view's geometry is the byte table's; the u16 tables' strip is re-read from the descriptor here)
template <bool IDENT, bool POW2, bool BYTES = false>
__device__ inline double dist_lookup_far(const MapView &m, double x, double y)
{
    int ci, ri;
    cell_index<IDENT, POW2>(m, x, y, ci, ri);
    unsigned off = 0;
    if (!BYTES) off = cell_offset(m, ci, ri);
    const MapDev *dp = m.desc;
    asm volatile("" : "+s"(dp)); // opaque: the loads below stay here instead of being hoisted to the kernel entry
    if (BYTES) { const unsigned sb = dp->strip_bytes; off = cell_offset(m, ci, ri, sb + 16u, sb - 16u); }
#if defined(F110_BOUNDS)
    F110_BCHK(off + 2u <= dp->cells_bytes, BT_CELLS_FAR, m.err);
    if (off + 2u > dp->cells_bytes) off = 0u;
#endif
    unsigned rank = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(dp->cells_far) + (size_t)off);
    const bool inside = (unsigned)ri < (unsigned)m.H && (unsigned)ci < (unsigned)m.W; // (a border cell never carries the far marker)
#if defined(F110_BOUNDS)
    F110_BCHK(rank == CODE_ESC || rank < dp->lut_len, BT_LUT_RANK, m.err);
    if (rank != CODE_ESC && rank >= dp->lut_len) rank = 0u;
    F110_BCHK(rank != CODE_ESC || inside, BT_DT, m.err);
#endif
    if (rank == CODE_ESC && !inside) return dp->oob;
    return (rank != CODE_ESC) ? dp->lut[rank] : dp->dt[(size_t)(unsigned)ri * (unsigned)m.W + (unsigned)ci];
}
__device__ inline bool is_far_marker(double d) { return __double2hiint(d) == (int)0x80000000; } // -0.0 (no table value is negative)

// np.fmod(t, td) (laser_models.py:170) without the generic library loop: for |t/td| < 2^31
// the result t - trunc(t/td)*td is exact (fmod results are representable and q*td is an
// exact product); the rounded quotient can only be one too large in magnitude, which
// shows as a remainder of the wrong sign and is redone with the corrected quotient.
__device__ inline double fmod_small(double t, double td)
{
    const double qf = trunc(t / td);
    if (!(fabs(qf) < 2147483648.0)) return fmod(t, td);
    double r = t - qf * td;
    if ((t >= 0 && r < 0) || (t < 0 && r > 0)) r = t - (qf - (t >= 0 ? 1.0 : -1.0)) * td;
    return r;
}

// laser_models.py:167-184: LUT index of beam b.  The reference advances theta_index by
// num_beams sequential fp64 adds (wrapping at theta_dis); in 24.40 fixed point
// T0 + b*INC differs from that recurrence by < 1e-9, so the integer part agrees unless
// the fraction is within 1e-7 of 0 or 1 -- then this lane replays the recurrence exactly.
// The index is NOT wrapped: the {cos, sin} table is stored `cs_reps` times back to back
// (wrapping subtracts theta_dis exactly, so entry idx and idx - theta_dis are the same).
// `guard2`: twice the guard band in units of 2^-32, less one (860 = 2 x 1e-7), or 0xffffffff when T0 is not a valid fixed-point
// start (NaN / infinite yaw): then every lane replays.  For a valid T0 the un-wrapped index stays inside the repeated table
// (upload_cs sizes it), so no per-lane compare against its length -- and no re-read of that length in every refill -- is needed.
__device__ inline int beam_theta_index(unsigned long long T0, double t0w, int b, const ScanDev &s, unsigned guard2)
{
    const unsigned inc_lo = (unsigned)s.inc_fx, inc_hi = (unsigned)(s.inc_fx >> 32);
    unsigned long long t = (unsigned long long)(unsigned)b * inc_lo + T0;    // v_mad_u64_u32
    unsigned hi = (unsigned)(t >> 32) + (unsigned)b * inc_hi;                // inc_hi, b < 2^24
    const unsigned lo = (unsigned)t;
    int idx = (int)(hi >> 8);
    const unsigned frac = __builtin_amdgcn_alignbit(hi, lo, 8);             // top 32 fraction bits
    if (__builtin_expect(frac + 430u <= guard2, 0)) {                         // within 1e-7 of an integer
        const double td = (double)s.theta_dis;
        double tt = t0w;
        for (int j = 0; j < b; j++) {
            tt += s.inc;
            while (tt >= td) tt -= td;
        }
        idx = (int)tt;
    }
    return idx;
}

// The march phase of a wave for a map whose origin is not rotated and whose resolution is a power of two (cell_index's
// one-fma form), written out: every ray that is still marching takes table look-ups (laser_models.py:129-142) until at most
// `go` rays are left.  The loop runs under the EXEC mask of the marching rays and narrows it with v_cmpx as rays finish, so a
// finished ray issues no look-up, keeps its total and costs no select; what remains per iteration is
//   2 fma + 2 floor + 2 cvt (the cell), 2 med3 + 2 shift-add + shift + mad (its byte offset), the look-up (buffer_load_ushort ->
//   ds_read_b64), total += d, x += d * c, y += d * s (5, contraction off), 2 v_cmpx          = 19 VALU, 5 SALU
// against 21 VALU + 11 SALU for the compiler's branch-free form of round 4 (a select that parked finished lanes on an
// out-of-range offset, a compare for the far marker, the active mask kept in SGPRs by s_and / s_andn2 / s_or).
//   am: in, the rays marching; out, the rays still marching.  nlook += look-ups made.  d: every lane's last table value.
// The loads and their waits are inside the statement (the compiler does not count an asm load).  The LDS LUT must sit at LDS
// address 0 (scan_kernel checks it).
// BYTES (the byte table of 16-column strips behind MapView::init_bytes' descriptor): the strip is c >> 4, ONE shift-add forms
// (r << 4) + c (the constant is in the descriptor's base), the load is buffer_load_ubyte and one v_lshlrev_b32 turns the slot
// into the LDS byte offset: 19 VALU as before.  The statements' texts differ in exactly those lines (the macros below).
#define F110_MARCH_CELL_WORD_CLAMPED(strip, row, col) \
        "v_lshl_add_u32 " row ", " row ", 4, %[rb]\n\t" \
        "v_ashrrev_i32 " strip ", 3, " col "\n\t" \
        "v_lshl_add_u32 " row ", " col ", 1, " row "\n\t"
#define F110_MARCH_CELL_WORD_FAST(strip, row, col) \
        "v_ashrrev_i32 " strip ", 3, " col "\n\t" \
        "v_lshl_add_u32 " row ", " row ", 4, %[rb]\n\t" \
        "v_lshl_add_u32 " row ", " col ", 1, " row "\n\t"
#define F110_MARCH_CELL_BYTE(strip, row, col) \
        "v_ashrrev_i32 " strip ", 4, " col "\n\t" \
        "v_lshl_add_u32 " row ", " row ", 4, " col "\n\t"
#define F110_MARCH_LOAD_WORD(code) \
        "buffer_load_ushort " code ", " code ", %[rsrc], 0 offen\n\t" \
        "s_waitcnt vmcnt(0)\n\t"
#define F110_MARCH_LOAD_BYTE(code) \
        "buffer_load_ubyte " code ", " code ", %[rsrc], 0 offen\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "v_lshlrev_b32 " code ", 3, " code "\n\t"
template <bool BYTES = false>
__device__ inline void march_ident_pow2(const MapView &m, double &x, double &y, double &total, double &d, double c, double s,
                                        double eps, double max_range, unsigned long long &am, int go, unsigned &nlook, int &nact)
{
    unsigned long long sx;
    double q0, q1;
    int t0, t1, t2;
#define F110_MARCH_CLAMPED(CELL, LOAD) \
    asm volatile( \
        "s_mov_b64 %[sx], exec\n\t" \
        "s_mov_b64 exec, %[am]\n" \
        "1:\n\t" \
        "s_add_u32 %[nl], %[nl], %[na]\n\t" \
        "v_fma_f64 %[q0], %[rinv], %[x], %[nox]\n\t" \
        "v_fma_f64 %[q1], %[rinv], %[y], %[noy]\n\t" \
        "v_floor_f64 %[q0], %[q0]\n\t" \
        "v_floor_f64 %[q1], %[q1]\n\t" \
        "v_cvt_i32_f64 %[t0], %[q0]\n\t" \
        "v_cvt_i32_f64 %[t1], %[q1]\n\t" \
        "v_med3_i32 %[t0], %[t0], -1, %[W]\n\t" \
        "v_med3_i32 %[t1], %[t1], -1, %[H]\n\t" \
        CELL("%[t2]", "%[t1]", "%[t0]") \
        "v_mad_i32_i24 %[t2], %[t2], %[sm], %[t1]\n\t" \
        LOAD("%[t2]") \
        "ds_read_b64 %[d], %[t2]\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_add_f64 %[tot], %[tot], %[d]\n\t" \
        "v_mul_f64 %[q0], %[c], %[d]\n\t" \
        "v_mul_f64 %[q1], %[s], %[d]\n\t" \
        "v_add_f64 %[x], %[x], %[q0]\n\t" \
        "v_add_f64 %[y], %[y], %[q1]\n\t" \
        "v_cmpx_lt_f64 vcc, %[eps], %[d]\n\t" \
        "v_cmpx_ge_f64 vcc, %[mr], %[tot]\n\t" \
        "s_bcnt1_i32_b64 %[na], exec\n\t" \
        "s_cmp_gt_i32 %[na], %[go]\n\t" \
        "s_cbranch_scc1 1b\n\t" \
        "s_mov_b64 %[am], exec\n\t" \
        "s_mov_b64 exec, %[sx]" \
        : [x] "+v"(x), [y] "+v"(y), [tot] "+v"(total), [d] "+v"(d), [am] "+s"(am), [nl] "+s"(nlook), [na] "+s"(nact), \
          [sx] "=&s"(sx), [q0] "=&v"(q0), [q1] "=&v"(q1), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2) \
        : [c] "v"(c), [s] "v"(s), [nox] "v"(m.nox), [noy] "v"(m.noy), [rinv] "s"(m.rinv), [W] "s"(m.W), [H] "s"(m.H), \
          [rb] "s"(m.row_bias), [sm] "s"(m.strip_m16), [rsrc] "s"(m.cells_words), [eps] "s"(eps), [mr] "s"(max_range), [go] "s"(go) \
        : "vcc", "scc", "memory")
    if constexpr (BYTES) F110_MARCH_CLAMPED(F110_MARCH_CELL_BYTE, F110_MARCH_LOAD_BYTE);
    else F110_MARCH_CLAMPED(F110_MARCH_CELL_WORD_CLAMPED, F110_MARCH_LOAD_WORD);
#undef F110_MARCH_CLAMPED
}

// The same loop for a car that is not absurdly far from its map (scan_kernel decides per car: |cell coordinates of the car| +
// max_range / resolution + 2 below `march_fast_limit`; every look-up of a ray is made within max_range of the car, because the
// march only continues while total <= max_range).  Two things become possible, both exact:
//  * floor + int conversion by the MAGIC NUMBER: q + 1.5 * 2^52 rounded TOWARD MINUS INFINITY is floor(q) + 1.5 * 2^52 exactly (the
//    sum's ulp is 1), and the low dword of that double is floor(q) as a two's complement int for |q| < 2^31: one v_add_f64 under
//    round mode -inf (s_setreg on MODE's f64 rounding field around the pair; the fma that forms q and the sums of the march stay
//    round-to-nearest) instead of v_floor_f64 + v_cvt_i32_f64;
//  * no clamp of the COLUMN: a column outside [-8, W + 8) forms an offset outside the table (negative ones wrap to large
//    unsigned values), which the descriptor's range check answers with 0 = the border's code; the columns in between lie in the
//    border strips.  That needs (c >> 3) * strip_bytes below 2^31, which the limit guarantees.  (The row still needs its clamp:
//    a row beyond the strip would land in the neighbouring strip.)  16 VALU + 6 SALU per iteration.
// BYTES: the row-padded byte table (f110_map.h: P = pad_rows zero rows above row -1 and below row H of every 16-column strip,
// S = strip_bytes_b) behind init_bytes' descriptor, which starts at strip 1, map row 0.  NEITHER coordinate is clamped; the
// offset the statement forms is (c >> 4) * S + r * 16 + (c & 15).  scan_kernel takes this march only for a car whose own row
// lies in [-1, H] (and whose reach the table was padded for), so every row r of a look-up lies in [-1 - P, H + P]:
//  * rows: the table stores row r of a strip at r + 1 + P in 0 .. H + 2 P + 1 < S / 16, so r * 16 + (c & 15) stays inside
//    [-16 (1 + P), S - 16 (1 + P)) and the look-up never leaves the strip of its column.  Rows -1 - P .. -1 and H .. H + P
//    are the strip's own padding and border rows, which hold 0; in strip 1 the rows below 0 lie in front of the descriptor
//    (a negative offset, out of range), in later strips they are the strip's first rows, ordinary bytes that hold 0;
//  * columns, as before: a column outside [-16, 16 * ((W >> 4) + 1)) has strip index (c >> 4) + 1 below 0 or at or above the
//    table's (W >> 4) + 2 strips -- against the descriptor an offset that is negative (wraps to 2^31 or more) or at or beyond
//    its bytes, ((W >> 4) + 1) * S - 16 (1 + P).  The columns in between that are no map cell lie in strip 0 (negative too) or
//    in the last strip's padding columns, which hold 0;
//  * the descriptor's range check answers 0 for those offsets, the slot of the border; 0 << 3 is its code.  The limit keeps
//    ((c >> 4) + 1) * S below 2^31 and c >> 4 inside the multiply's 24 bits.
// 15 VALU + 6 SALU per iteration, one buffer_load_ubyte, one ds_read_b64 (tests/test_scan_rowpad_cpu.py replays the offset
// arithmetic over every such row and column).  A car standing off those rows takes the clamped twin above.
// The magic sums and the products live in v[60:63]: an asm operand cannot name the low dword
// of a register pair, so the statement uses those four registers by name and declares them clobbered.
template <bool BYTES = false>
__device__ inline void march_ident_pow2_fast(const MapView &m, double &x, double &y, double &total, double &d, double c, double s,
                                             double eps, double max_range, unsigned long long &am, int go, unsigned &nlook, int &nact)
{
    unsigned long long sx;
#define F110_MARCH_FAST(ROW, CELL, LOAD, GEOM) \
    asm volatile( \
        "s_mov_b64 %[sx], exec\n\t" \
        "s_mov_b64 exec, %[am]\n" \
        "1:\n\t" \
        "s_add_u32 %[nl], %[nl], %[na]\n\t" \
        "v_fma_f64 v[60:61], %[rinv], %[x], %[nox]\n\t" \
        "v_fma_f64 v[62:63], %[rinv], %[y], %[noy]\n\t" \
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 2, 2), 2\n\t"      /* f64 rounding: toward -inf */ \
        "v_add_f64 v[60:61], v[60:61], %[magic]\n\t" \
        "v_add_f64 v[62:63], v[62:63], %[magic]\n\t" \
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 2, 2), 0\n\t"      /* back to nearest-even */ \
        ROW \
        CELL("v61", "v62", "v60") \
        "v_mad_i32_i24 v61, v61, %[sm], v62\n\t" \
        LOAD("v61") \
        "ds_read_b64 %[d], v61\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_add_f64 %[tot], %[tot], %[d]\n\t" \
        "v_mul_f64 v[60:61], %[c], %[d]\n\t" \
        "v_mul_f64 v[62:63], %[s], %[d]\n\t" \
        "v_add_f64 %[x], %[x], v[60:61]\n\t" \
        "v_add_f64 %[y], %[y], v[62:63]\n\t" \
        "v_cmpx_lt_f64 vcc, %[eps], %[d]\n\t" \
        "v_cmpx_ge_f64 vcc, %[mr], %[tot]\n\t" \
        "s_bcnt1_i32_b64 %[na], exec\n\t" \
        "s_cmp_gt_i32 %[na], %[go]\n\t" \
        "s_cbranch_scc1 1b\n\t" \
        "s_mov_b64 %[am], exec\n\t" \
        "s_mov_b64 exec, %[sx]" \
        : [x] "+v"(x), [y] "+v"(y), [tot] "+v"(total), [d] "+v"(d), [am] "+s"(am), [nl] "+s"(nlook), [na] "+s"(nact), [sx] "=&s"(sx) \
        : [c] "v"(c), [s] "v"(s), [nox] "v"(m.nox), [noy] "v"(m.noy), [rinv] "s"(m.rinv), GEOM \
          [sm] "s"(m.strip_m16), [rsrc] "s"(m.cells_words), [eps] "s"(eps), [mr] "s"(max_range), [go] "s"(go), \
          [magic] "s"(6755399441055744.0) \
        : "vcc", "scc", "memory", "v60", "v61", "v62", "v63")
#define F110_MARCH_ROW_CLAMP "v_med3_i32 v62, v62, -1, %[H]\n\t"
#define F110_MARCH_GEOM_WORD [H] "s"(m.H), [rb] "s"(m.row_bias),
    if constexpr (BYTES) F110_MARCH_FAST("", F110_MARCH_CELL_BYTE, F110_MARCH_LOAD_BYTE, );
    else F110_MARCH_FAST(F110_MARCH_ROW_CLAMP, F110_MARCH_CELL_WORD_FAST, F110_MARCH_LOAD_WORD, F110_MARCH_GEOM_WORD);
#undef F110_MARCH_GEOM_WORD
#undef F110_MARCH_ROW_CLAMP
#undef F110_MARCH_FAST
}
// The march for a map whose resolution is NOT a power of two (most F1TENTH maps: 0.05 m) and whose origin is not rotated, for
// cars near their map (the same per-car test as above).  q = (x - ox) * (1 / res) is within ~2e-16 relative of the reference's
// quotient (x - ox) / res, so its floor is the reference's cell unless q lies within 1e-9 of an integer: the loop computes the
// fractions of both coordinates and LEAVES (flag = 1, nothing of the iteration done) when any marching ray is that close; the
// caller then runs that one iteration through dist_lookup, which replays the reference's own division (cell_index), and comes
// back.  Otherwise as march_ident_pow2_fast: floor by the magic number under round-toward -inf (and back to a double to form the
// fraction), EXEC-masked, v_cmpx.  27 VALU + 7 SALU per iteration; the compiler's loop over dist_lookup is ~33 + ~20.
// a wave-uniform double as a scalar-register operand (the compiler may hold it in vector registers where it feeds vector code)
__device__ inline double uniform_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__device__ inline int march_ident_np_fast(const MapView &m, double &x, double &y, double &total, double &d, double c, double s,
                                          double eps, double max_range, unsigned long long &am, int go, unsigned &nlook, int &nact)
{
    unsigned long long sx;
    double qx, qy, fx, fy;
    int flag;
    // (wave-uniform by construction; said again for the register allocator: the values travel round a loop through compiler code)
    am = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(am >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)am);
    nlook = (unsigned)__builtin_amdgcn_readfirstlane((int)nlook);
    nact = __builtin_amdgcn_readfirstlane(nact);
    go = __builtin_amdgcn_readfirstlane(go);
    asm volatile(
        "s_mov_b64 %[sx], exec\n\t"
        "s_mov_b64 exec, %[am]\n"
        "1:\n\t"
        "v_add_f64 %[qx], %[x], -%[ox]\n\t"
        "v_add_f64 %[qy], %[y], -%[oy]\n\t"
        "v_mul_f64 %[qx], %[rinv], %[qx]\n\t"
        "v_mul_f64 %[qy], %[rinv], %[qy]\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 2, 2), 2\n\t"      // f64 rounding: toward -inf
        "v_add_f64 v[60:61], %[qx], %[magic]\n\t"
        "v_add_f64 v[62:63], %[qy], %[magic]\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 2, 2), 0\n\t"      // back to nearest-even
        "v_add_f64 %[fx], v[60:61], -%[magic]\n\t"                // floor(q) as a double (exact)
        "v_add_f64 %[fy], v[62:63], -%[magic]\n\t"
        "v_add_f64 %[fx], %[qx], -%[fx]\n\t"                      // fraction (exact)
        "v_add_f64 %[fy], %[qy], -%[fy]\n\t"
        "v_add_f64 %[fx], %[fx], -0.5\n\t"
        "v_add_f64 %[fy], %[fy], -0.5\n\t"
        "v_max_f64 %[fx], |%[fx]|, |%[fy]|\n\t"
        "v_cmp_lt_f64 vcc, %[thr], %[fx]\n\t"                     // a fraction within 1e-9 of 0 or 1
        "s_cbranch_vccnz 3f\n\t"
        "s_add_u32 %[nl], %[nl], %[na]\n\t"
        "v_med3_i32 v62, v62, -1, %[H]\n\t"
        "v_ashrrev_i32 v61, 3, v60\n\t"
        "v_lshl_add_u32 v62, v62, 4, %[rb]\n\t"
        "v_lshl_add_u32 v62, v60, 1, v62\n\t"
        "v_mad_i32_i24 v61, v61, %[sm], v62\n\t"
        "buffer_load_ushort v61, v61, %[rsrc], 0 offen\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "ds_read_b64 %[d], v61\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_add_f64 %[tot], %[tot], %[d]\n\t"
        "v_mul_f64 v[60:61], %[c], %[d]\n\t"
        "v_mul_f64 v[62:63], %[s], %[d]\n\t"
        "v_add_f64 %[x], %[x], v[60:61]\n\t"
        "v_add_f64 %[y], %[y], v[62:63]\n\t"
        "v_cmpx_lt_f64 vcc, %[eps], %[d]\n\t"
        "v_cmpx_ge_f64 vcc, %[mr], %[tot]\n\t"
        "s_bcnt1_i32_b64 %[na], exec\n\t"
        "s_cmp_gt_i32 %[na], %[go]\n\t"
        "s_cbranch_scc1 1b\n\t"
        "s_mov_b32 %[flag], 0\n\t"
        "s_branch 4f\n"
        "3:\n\t"
        "s_mov_b32 %[flag], 1\n"
        "4:\n\t"
        "s_mov_b64 %[am], exec\n\t"
        "s_mov_b64 exec, %[sx]"
        : [x] "+v"(x), [y] "+v"(y), [tot] "+v"(total), [d] "+v"(d), [am] "+s"(am), [nl] "+s"(nlook), [na] "+s"(nact), [sx] "=&s"(sx),
          [qx] "=&v"(qx), [qy] "=&v"(qy), [fx] "=&v"(fx), [fy] "=&v"(fy), [flag] "=&s"(flag)
        : [c] "v"(c), [s] "v"(s), [ox] "s"(uniform_f64(m.ox)), [oy] "s"(uniform_f64(m.oy)), [rinv] "s"(uniform_f64(m.rinv)), [H] "s"(m.H),
          [rb] "s"(m.row_bias), [sm] "s"(m.strip_m16), [rsrc] "s"(m.cells_words), [eps] "s"(eps), [mr] "s"(max_range), [go] "s"(go),
          [magic] "s"(6755399441055744.0), [thr] "s"(0.5 - 1e-9)
        : "vcc", "scc", "memory", "v60", "v61", "v62", "v63");
    return flag;
}
// the largest |cell coordinate| a look-up of the fast march may have: (c >> 3) * strip_bytes stays below 2^31 with room to
// spare, and far inside the magic number's 2^31 (a NaN or infinite pose fails the test and takes the clamped loop)
__device__ inline double march_fast_limit(const MapView &m) { return (double)((0x7fffffffu / (m.row_bias + 16u)) * 8u) - 64.0; }
// the same for the byte table: (c >> 4) * strip_bytes below 2^31 and c >> 4 a signed 24-bit operand of the multiply-add
__device__ inline double march_fast_limit_bytes(const MapView &m)
{
    const unsigned strips = 0x7fffffffu / (m.row_bias + 16u);
    return (double)((strips < 0x7fffffu ? strips : 0x7fffffu) * 16u) - 64.0;
}

struct ScanArgs {
    const MapDev *maps;         // dev [K] map descriptors
    const int32_t *env_map;     // dev [B] map of every env, or NULL (all envs on maps[0]); the cars of one
                                // workgroup share a map (f110_assign_maps checks it for the pairs 2k, 2k+1 of all
                                // cars; plan_scan keeps every launch and stage at an even car): its LUT is staged per group
    ScanDev scan;
    int n_cars;             // cars of THIS launch: car_base .. car_base + n_cars - 1
    int car_base;           // first car (a shard whose env blocks sit on maps of different kinds -- resolution a power
                            // of two or not, origin rotated or not -- is scanned block by block, each with its own instantiation)
    int agents;             // A (cars of one env are consecutive)
    int wpc;                // unused (the waves per car come from the stage list below); kept so that the fields behind
                            // it keep their offsets in the argument block
    // Wave -> (car, part) mapping: consecutive STAGES of cars, stage s giving each of its stage_cars[s] cars
    // 2^stage_log2w[s] waves (f110_scan_plan.h explains the choice).  Read through `rare`, not held in registers.
    int n_stages;
    int stage_cars[8];          // SCAN_MAX_STAGES
    int stage_log2w[8];         // each 0..SCAN_MAX_LOG2W
    // pose source: pose = (src[car*stride], src[car*stride+1], src[car*stride+yaw_off])
    const double *pose_src;
    int pose_stride, yaw_off;
    // full-step extras (all NULL for the function-level scan)
    const double *state;         // [N,7]: velocity for the iTTC test
    const int32_t *noise_step;   // [N]
    // The noise table (one 8-B gather per beam taken): [noise_slots][noise_cap][nb], a ring of noise_cap = noise_mask + 1 rows
    // per slot.  Base and size travel BY VALUE -- through the device-resident
    // descriptor every wave started with a chain of two dependent scalar loads, 0.9 % of the launch (profiles/r04_noise.txt)
    // -- so they only change when the table is re-allocated (f110_launch_epoch moves then; a ring that follows the cars
    // never is).  The window of rows that are present moves all the time: it stays behind the descriptor and is checked
    // by dynamics_kernel, off this kernel's path.
    const double *noise_base;
    int noise_mask, noise_cap, noise_slots;
    const double *side;          // [nb] side distances (base_classes.py:123-156), read only for iTTC candidates
    double side_max;             // their largest finite value: scan values at or above side_max + margin cannot be candidates
    const int32_t *env_noise;    // [B] noise slot (= seed) of every env, or NULL (all envs on slot 0)
    uint32_t *dev_err;           // device error word (f110_device_errors): F110_DEVERR_* bits, or NULL
    const double *beam_cosines;  // [nb]
    double ttc_thresh;
    uint8_t *in_collision;       // [N]
    const uint8_t *pending_reset;// [B]
    int reset_only;              // 1: only envs with pending_reset are processed
    const uint16_t *chunk_beam0; // [ceil(nb/64)] first beam of the k-th 64-beam chunk to be marched (long rays first)
    // Launch order (or NULL = car order): the wave that would march car i marches car order[i].  A permutation of the shard's
    // cars that only changes WHICH wave marches WHICH car -- results are indexed by the car -- so that cars standing on the
    // same noise row can be launched next to each other (f110_set_scan_order; Engine keeps it sorted by the envs' row counters:
    // in a batch whose envs were reset at different times every env reads its own row, 566 MB per step at 65 536 envs, and the
    // rows of neighbouring waves then come from the L1 / L2 instead of HBM).  Single-map handles only (a workgroup stages ONE LUT).
    const int32_t *order;
    // 1: workgroups of ONE wave (block = 64 threads) -- every car stages its own map's LUT, so neighbouring cars may stand on
    // different maps (f110_assign_maps with a map per env); 0: SCAN_WAVES cars per workgroup share one LUT copy.
    int wg_single;
    int n_maps;             // slots of `maps` (bounds build)
    // Side distances per VEHICLE (f110_set_side_distance_slots), or NULL = the handle's one table `side`: [side_n_slots][nb], the
    // car's row is that of its env's params slot (env_params[env], NULL: slot 0).  Both belong to the rarely needed arguments:
    // read through the kernarg pointer inside the iTTC candidate branch only; side_max then spans every installed row.
    const double *side_slots;
    const int32_t *env_params;
    int side_n_slots;       // rows of side_slots (bounds build)
    // outputs
    float *out_f32;              // [N,nb] or NULL
    double *out_f64;             // [N,nb] or NULL
    uint32_t *lookups;           // [N] or NULL (accumulated)
};

// scan_kernel re-reads its argument block through the kernarg segment pointer, which is only the same block
// if ScanArgs is the kernel's ONLY argument, passed by value at offset 0, and trivially copyable (the launch
// memcpy's it).  The stage list is a fixed array inside it: plan_scan checks the count and the exponents.
static_assert(__is_trivially_copyable(ScanArgs), "ScanArgs is copied into the kernarg segment byte for byte");
static_assert(offsetof(ScanArgs, maps) == 0, "kernarg re-read assumes the argument block starts with ScanArgs");
static_assert(sizeof(((ScanArgs *)0)->stage_cars) == SCAN_MAX_STAGES * sizeof(int) &&
              sizeof(((ScanArgs *)0)->stage_log2w) == SCAN_MAX_STAGES * sizeof(int), "stage list capacity");
static_assert(sizeof(ScanArgs) <= 4096, "kernarg segment size");

// One wavefront per car.  Lanes own rays; a finished ray idles (its lookups return 0.0) until at least REFILL_MIN_IDLE lanes are idle, then every idle
// lane (a) finishes its previous beam -- noise, iTTC candidate test, fp32/fp64 store --
// and (b) takes the next beam of the car.  No LDS staging of the scan but ROWBUF's (below): the only other LDS
// use is the distance LUT shared by the workgroup (8 KiB in the classic form), so occupancy is register-bound.
// STEP: full env step (noise + iTTC + state update); false: ScanSimulator2D.scan(pose, None).
// SM 0: ScanSimulator2D.scan(pose, None); 1: the scan of a step (noise, iTTC flag; env_kernel follows); 2: the same with
// ordinary instead of streaming stores for the fp32 scan (launches of more than ~300 000 cars, see emit).
constexpr int SCAN_MIN_WAVES = 8; // waves per SIMD: the kernel is held to their 80-SGPR budget (see the wave -> car mapping)
// LUTN: slots of the LDS image.  LUT_LDS is the classic form; LUT_COMPACT[i] the compact one (f110_scan_plan.h): always
// launched as workgroups of one wave, reading the map's compact cell table and image.  The march statements are the same:
// they see another descriptor and a shorter LUT at LDS address 0.
static_assert(N_COMPACT == SCAN_COMPACT_N && LUT_COMPACT[0] == SCAN_COMPACT_S[0] && LUT_COMPACT[1] == SCAN_COMPACT_S[1],
              "the plan's compact sizes are the map tables'");
// ROWBUF (LUTN == 256 only): the fp32 results of the wave's last SCAN_ROWBUF_CHUNKS chunk positions are staged in LDS behind
// the LUT and the chunk table and written out as whole chunks when the march has ended (f110_scan_plan.h: scan_rowbuf_plan).
template <int LUTN> struct __attribute__((aligned(16))) ScanLds { double lut[LUTN]; int chunk0[MAX_CHUNKS]; };
template <int LUTN> struct __attribute__((aligned(16))) ScanLdsRows { double lut[LUTN]; int chunk0[MAX_CHUNKS]; float rows[SCAN_ROWBUF_CHUNKS * 64]; };
static_assert(sizeof(ScanLds<SCAN_ROWBUF_LUT>) == SCAN_ROWBUF_BASE && sizeof(ScanLdsRows<SCAN_ROWBUF_LUT>) <= SCAN_LDS_PER_GROUP,
              "32 one-wave workgroups with a row buffer each fit a CU's LDS");
template <bool DIRECT> struct EmitTag { static constexpr bool direct = DIRECT; };
// BYTES (LUTN == 256 only): the march reads the map's byte table (f110_map.h: cell_elem_b) instead of cells_c[0].
template <bool IDENT, bool POW2, int SM, int LUTN = LUT_LDS, bool ROWBUF = false, bool BYTES = false>
__global__ __launch_bounds__(SCAN_THREADS, SCAN_MIN_WAVES) void scan_kernel(ScanArgs a)
{
    constexpr bool STEP = SM >= 1;
    constexpr bool COMPACT = LUTN != LUT_LDS;
    static_assert(!COMPACT || (compact_index(LUTN) >= 0 && STEP && IDENT && POW2), "compact forms: the step's scan, kind 3");
    static_assert(!ROWBUF || LUTN == SCAN_ROWBUF_LUT, "the row buffer: the compact form of 256 slots");
    static_assert(!BYTES || LUTN == LUT_COMPACT[0], "byte cell codes: the compact form of 256 slots");
    // ONE LDS object, the LUT first: march_ident_pow2 addresses the LUT by the cell codes alone, i.e. the LUT sits at LDS
    // address 0 (the kernel has no other LDS variable; every parity test would fail otherwise)
    __shared__ typename std::conditional<ROWBUF, ScanLdsRows<LUTN>, ScanLds<LUTN>>::type s_mem;
    double *const s_lut = s_mem.lut;
    int *const s_chunk0 = s_mem.chunk0;
    float *s_rows = nullptr;
    if constexpr (ROWBUF) s_rows = s_mem.rows;
    // the same argument block addressed through the kernarg segment (ScanArgs is the only kernel argument): rarely
    // needed fields are re-read through it where they are used instead of being held in SGPRs for the whole kernel
#if defined(__HIP_DEVICE_COMPILE__)
    const ScanArgs *rare = (const ScanArgs *)__builtin_amdgcn_kernarg_segment_ptr();
#else
    const ScanArgs *rare = &a; // host pass of the single-source compile: never executed
#endif
    const int nb = a.scan.nb;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int wg_single = COMPACT ? 1 : rare->wg_single;
    const int wid = wg_single ? (int)blockIdx.x : (int)blockIdx.x * SCAN_WAVES + wave; // wave-uniform (scalar)
    // wave -> (car, part of its beam queue).  Kept to one extra argument and shifts: this kernel sits at
    // the 80-SGPR budget of 8 waves/SIMD, and a scalar spilled inside the refill loop costs ~3 % of the launch.
    int wpc, car, part, lg; // (wpc = 2^lg: the divisions by it below are shifts -- a scalar integer division is ~25 dependent instructions)
    {
        // (the stage list read from the kernel arguments with constant indices instead -- no dependent loads -- measured no better)
        int t = wid, c = 0, st = 0;
        const int ns = rare->n_stages;
        for (; st < ns; st++) {
            const int cars_s = rare->stage_cars[st], w = cars_s << rare->stage_log2w[st];
            if (t < w) break;
            t -= w; c += cars_s;
        }
        lg = st < ns ? rare->stage_log2w[st] : 0;
        wpc = 1 << lg; car = st < ns ? c + (t >> lg) : a.n_cars; part = t & (wpc - 1);
    }
    // the car's map (wave-uniform: scalar loads); waves past the last car still help to stage the LUT
    int car_c = rare->car_base + min(car, a.n_cars - 1);
    if (rare->order) car_c = rare->order[car_c]; // (launch position -> car; wave-uniform: a scalar load)
    const int env_c = a.agents == 1 ? car_c : car_c / a.agents; // (one agent: no division at run time)
    F110_BCHK(rare->n_stages >= 1 && rare->n_stages <= SCAN_MAX_STAGES, BT_STAGE_LIST, rare->dev_err);
    int map_slot = a.env_map ? a.env_map[env_c] : 0;
#if defined(F110_BOUNDS)
    F110_BCHK((unsigned)map_slot < (unsigned)rare->n_maps, BT_MAP_SLOT, rare->dev_err);
    if ((unsigned)map_slot >= (unsigned)rare->n_maps) map_slot = 0;
#endif
    const MapDev &md = a.maps[map_slot];
    {   // LDS image of the LUT prepared by the host (slot 0 = dt[-1,-1], last slot = the far marker): 16-B copies
        const double2 *src = reinterpret_cast<const double2 *>(COMPACT ? md.lut_lds_c[compact_index(LUTN) & 1] : md.lut_lds);
        double2 *dst = reinterpret_cast<double2 *>(s_lut);
        for (int i = threadIdx.x; i < LUTN / 2; i += SCAN_THREADS) dst[i] = src[i];
        if (SCAN_WAVES > 1 && wg_single) // (a lone wave copies the other waves' shares too)
            for (int k = 1; k < SCAN_WAVES; k++)
                for (int i = threadIdx.x + k * WAVE; i < LUTN / 2; i += SCAN_THREADS) dst[i] = src[i];
    }
    static_assert(MAX_CHUNKS <= WAVE, "one pass of one wave stages the chunk table");
    if ((int)threadIdx.x < ((nb + 63) >> 6)) s_chunk0[threadIdx.x] = a.chunk_beam0[threadIdx.x];
    __syncthreads();
    MapView mv;
    if (BYTES) mv.init_bytes(md, compact_off_far(LUTN));
    else if (COMPACT) mv.init(md, md.cells_c[compact_index(LUTN) & 1], md.cells_bytes, compact_off_far(LUTN));
    else mv.init(md, md.cells, md.cells_bytes, OFF_FAR);
    F110_BOUNDS_ONLY(mv.err = rare->dev_err;)
    if (car >= a.n_cars) return;
    car = car_c; // (from here on the car's index in the shard)
    // this wave's slice of the car's beam queue: chunk positions part, part+wpc, ...
    const int nbl = scan_rowbuf_plan(nb, lg, part).nbl; // beams of this wave
    if (a.reset_only && !a.pending_reset[env_c]) return; // (car == car_c here: the waves past the last car have left)

    const double px = a.pose_src[(size_t)car * a.pose_stride];
    const double py = a.pose_src[(size_t)car * a.pose_stride + 1];
    const double yaw = a.pose_src[(size_t)car * a.pose_stride + a.yaw_off];
    const double eps = a.scan.eps, max_range = a.scan.max_range;

    // per-car constants of the finishing stage
    const double vel = STEP ? a.state[(size_t)car * 7 + 3] : 0.0;
    const bool do_ttc = STEP && vel != 0.0;               // laser_models.py:206
    // iTTC hit needs 0 <= (v - side)/(vel*cos) < thresh, hence |v - side| < thresh*|vel|:
    // only such candidate beams pay the exact fp64 division
    const double cand = a.ttc_thresh * fabs(vel) * 1.000000001;
    // ... and only scan values below (largest side distance + cand) can be candidates at all: |v - side_i| < cand needs
    // v < side_i + cand <= side_max + cand (the margin covers the roundings of the sum and of v - side_i), so the beam's side
    // distance is read in that rare case only and the noise rows hold nothing but noise
    // (the margin is added, not multiplied in: a table of negative side distances must not pull the bound the wrong way)
    const double side_pre = do_ttc ? (rare->side_max + cand) + 1e-9 * (fabs(rare->side_max) + cand) : -__builtin_inf(); // (no iTTC test: no value is below it)
    const double *__restrict__ ns = nullptr;
    if (STEP) {
        // the car's noise row: row `scans since its reset` of its env's slot (a ring of noise_cap rows per slot)
        const int row = a.noise_step[car];
        int slot = a.env_noise ? a.env_noise[env_c] : 0;
#if defined(F110_BOUNDS)
        F110_BCHK(slot >= 0 && slot < rare->noise_slots, BT_NOISE_SLOT, rare->dev_err);
        if (!(slot >= 0 && slot < rare->noise_slots)) slot = 0;
#endif
        ns = a.noise_base + (size_t)(unsigned)(slot * a.noise_cap + (row & a.noise_mask)) * (size_t)(unsigned)nb; // (slots * cap rows < 2^31: noise_resize)
    }
    float *o32 = a.out_f32 ? a.out_f32 + (size_t)car * nb : nullptr;
    double *o64 = a.out_f64 ? a.out_f64 + (size_t)car * nb : nullptr;
    bool hit = false;

    // finishing stage of one beam: clamp (laser_models.py:143-144), noise (:450-452),
    // stores, iTTC (:189-217).  nzv: noise of the beam, loaded by the caller ahead of time.
    // ROWBUF: the refill passes `i` = beam | queue position << 12 (both below 4 096) and the beams at or behind the wave's
    // first staged position go to the row buffer; tag.direct (the d0 loop below): a plain beam, always stored directly.
    auto emit = [&](auto tag, int i, double tot, double nzv) {
        constexpr bool STAGING = ROWBUF && !decltype(tag)::direct;
        int kq = 0;
        if (STAGING) { kq = i >> 12; i &= 4095; }
#if defined(F110_BOUNDS)
        F110_BCHK((unsigned)i < (unsigned)nb, BT_SCAN_STORE, rare->dev_err);
        if ((unsigned)i >= (unsigned)nb) return;
#endif
        double v; // :143-144 min(total, max_range) (a NaN total, i.e. a NaN pose, also clamps: v_min_f64 returns the other operand)
        asm("v_min_f64 %0, %1, %2" : "=v"(v) : "v"(tot), "s"(max_range)); // (fmin() would first quieten both operands: two more instructions)
        if (STEP) v += nzv;
        // Streaming (non-temporal) stores: the scan is written once and read by later kernels only; as ordinary stores the
        // 27 scattered store instructions of a car took their turn in the L1 beside the table look-ups, which are what bounds
        // this kernel -- 0.683 -> 0.654 ms per 65 536 cars (profiles/r04_scan_stores.txt)
        // (Very large launches are the exception -- 524 288 cars: 4.78 ms with ordinary stores, 4.95 ms with streaming ones, whose
        // partial lines reach the HBM un-merged; 65 536: 0.683 / 0.654, 262 144: 2.476 / 2.459 -- so the host picks the
        // instantiation by the launch's size.  A run-time flag tested here costs 3.4 % of the launch.)
        if (o32) {
            bool staged = false;
            if (STAGING) {
                int n = nbl;
                asm volatile("" : "+s"(n)); // (the first staged position is formed here, not held in a scalar register across the march)
                const int k0 = scan_rowbuf_k0(n);
                staged = kq >= k0;
                if (staged) {
                    unsigned off = scan_rowbuf_offset(kq, k0);
#if defined(F110_BOUNDS)
                    F110_BCHK(off < (unsigned)(SCAN_ROWBUF_CHUNKS * 256) && ((kq ^ i) & 63) == 0, BT_SCAN_STORE, rare->dev_err);
                    if (off >= (unsigned)(SCAN_ROWBUF_CHUNKS * 256)) off = 0u;
#endif
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(s_rows) + off) = (float)v;
                }
            }
            if (!staged) {
                float *q = reinterpret_cast<float *>(reinterpret_cast<char *>(o32) + (size_t)((unsigned)i * 4u));
                if (SM == 2) *q = (float)v;
                else __builtin_nontemporal_store((float)v, q);
            }
        }
        if (o64) {
            double *q64 = reinterpret_cast<double *>(reinterpret_cast<char *>(o64) + (size_t)((unsigned)i * 8u));
            if (SM == 2) *q64 = v;
            else __builtin_nontemporal_store(v, q64);
        }
        if (__builtin_expect(v < side_pre, 0)) {
            const ScanArgs *ra = rare;
            asm volatile("" : "+s"(ra)); // re-read the rarely needed arguments here instead of holding them in SGPRs
            const double *side = ra->side;
            if (const double *const rows = ra->side_slots) {
                // the table of the car's own vehicle: row `params slot of its env` (wave-uniform: scalar loads and one scalar
                // division for A > 1, paid by candidates only -- the env index is not kept in a register across the march)
                const int ag = ra->agents;
                const int32_t *const ep = ra->env_params;
                int sl = ep ? ep[ag == 1 ? car : car / ag] : 0;
#if defined(F110_BOUNDS)
                F110_BCHK((unsigned)sl < (unsigned)ra->side_n_slots, BT_SIDE_SLOT, ra->dev_err);
                if ((unsigned)sl >= (unsigned)ra->side_n_slots) sl = 0;
#endif
                side = rows + (size_t)(unsigned)sl * (size_t)(unsigned)nb;
            }
            const double sd = v - side[i];
            if (fabs(sd) < cand) {
                const double proj_vel = vel * ra->beam_cosines[i];
                const double ttc = sd / proj_vel;
                if ((ttc < ra->ttc_thresh) && (ttc >= 0.0)) hit = true;
            }
        }
    };

    // ---- ray march (laser_models.py:107-186) -------------------------------------
    // The first table read of every beam is at the car itself (:129): done once.
    double d0 = dist_lookup<IDENT, POW2, BYTES>(mv, s_lut, px, py);
    if (__builtin_expect(is_far_marker(d0), 0)) d0 = dist_lookup_far<IDENT, POW2, BYTES>(mv, px, py); // (wave-uniform: every lane reads the car's own cell)
    unsigned nlook = (unsigned)nbl; // the reference reads the table once per beam before marching
    if (!(d0 > eps && d0 <= max_range)) {
        for (int k = lane; k < nbl; k += WAVE) {
            F110_BCHK((k >> 6) * wpc + part < MAX_CHUNKS, BT_CHUNK_ORDER, rare->dev_err);
            int i = s_chunk0[((k >> 6) * wpc + part) & (MAX_CHUNKS - 1)] + (k & 63);
#if defined(F110_BOUNDS)
            F110_BCHK((unsigned)i < (unsigned)nb, BT_NOISE_BEAM, rare->dev_err);
            if ((unsigned)i >= (unsigned)nb) i = 0;
#endif
            emit(EmitTag<true>(), i, d0, STEP ? ns[i] : 0.0);
        }
    } else {
        const double td = (double)a.scan.theta_dis;
        double t0w = td * (yaw - a.scan.fov / 2.) / (2. * F110_PI);
        t0w = fmod_small(t0w, td);
        while (t0w < 0) t0w += td;
        // 24.40 fixed point of t0w in [0, theta_dis); a NaN / out-of-range yaw falls to the slow path
        const bool t0_ok = t0w >= 0 && t0w < td;
        const unsigned long long T0 = t0_ok ? (unsigned long long)(t0w * 1099511627776.0) : 0ull;
        const unsigned guard2 = t0_ok ? 859u : 0xffffffffu;

        // (wave-uniform) may this car's rays take the fast march?  Every look-up lies within max_range of the car.
        bool fast = false;
        if (IDENT) {
            const double reach = max_range * mv.rinv + 2.0, lim = BYTES ? march_fast_limit_bytes(mv) : march_fast_limit(mv);
            const double q0x = POW2 ? __builtin_fma(px, mv.rinv, mv.nox) : (px - mv.ox) * mv.rinv;
            const double q0y = POW2 ? __builtin_fma(py, mv.rinv, mv.noy) : (py - mv.oy) * mv.rinv;
            fast = fabs(q0x) + reach < lim && fabs(q0y) + reach < lim;
            // the byte march clamps no row: the car's own row in -1 .. H, and the table padded for this reach (it is, by
            // construction: the install pads for the handle's max_range).  Any other car takes the clamped twin.
            if (BYTES) fast = fast && q0y >= -1.0 && q0y < (double)(mv.H + 1) && reach <= (double)md.pad_rows;
        }
        int next = 0;           // wave-uniform: next unassigned slot of the beam order
        bool active = false;
        int beam = -1;          // beam whose result `total` holds (-1: none)
        double x = px, y = py, c = 0, s = 0, total = 0;
        double d = 0;           // the lane's last table value (kept across the phases: a parked -0.0 is a cell of the second table)
        double nz = 0;          // noise of the lane's beam (fetched when the beam is taken)
        for (;;) {
            // ---- cells of the second table (rare): a lane that read the far marker stopped with an exact no-op; finish its
            // look-up here, once per phase instead of one compare per look-up
            {
                const bool farp = !active && is_far_marker(d);
                if (__builtin_expect(vote(farp) != 0ull, 0)) {
                    if (farp) {
                        d = dist_lookup_far<IDENT, POW2, BYTES>(mv, x, y);
                        total += d;
                        x += d * c;
                        y += d * s;
                        active = (d > eps) && (total <= max_range);
                    }
                }
            }
            // ---- refill phase: idle lanes finish their beam and take the next one ----
            const unsigned long long idle = vote(!active);
            const int nidle = __popcll(idle);
            if (!active) {
                // all independent loads first (one memory round trip).  The noise entry is fetched
                // for the beam being TAKEN and carried in registers until the beam is finished: idle lanes take
                // consecutive beams, so this gather touches a few cache lines, where a gather by the FINISHED beams
                // (scattered over the scan) touched a line per lane -- the L1's tag pipeline is what bounds this kernel
                const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32),
                                    __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
                const int k = next + rank;
                const bool take = k < nbl;
                const int kk = take ? k : 0;
                F110_BCHK((kk >> 6) * wpc + part < MAX_CHUNKS, BT_CHUNK_ORDER, rare->dev_err);
                int b = s_chunk0[((kk >> 6) * wpc + part) & (MAX_CHUNKS - 1)] + (kk & 63);
#if defined(F110_BOUNDS)
                F110_BCHK((unsigned)b < (unsigned)nb, BT_NOISE_BEAM, rare->dev_err);
                if ((unsigned)b >= (unsigned)nb) b = 0;
#endif
                const double nsv = STEP ? *reinterpret_cast<const double *>(reinterpret_cast<const char *>(ns) + (size_t)((unsigned)b * 8u)) : 0.0;
                const double nzv = nz;
                int ti = beam_theta_index(T0, t0w, b, a.scan, guard2);
#if defined(F110_BOUNDS)
                F110_BCHK((unsigned)ti < (unsigned)a.scan.cs_len, BT_CS_TABLE, rare->dev_err);
                if ((unsigned)ti >= (unsigned)a.scan.cs_len) ti = 0;
#endif
                const double2 cs = *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(a.scan.cs) + (size_t)((unsigned)ti * 16u)); // second round trip, overlapped with emit()
                if (beam >= 0) emit(EmitTag<false>(), beam, total, nzv);
                beam = -1;
                c = cs.x; // (every idle lane: one that takes no beam never marches again, and the far look-ups are finished above)
                s = cs.y;
                if (take) {
                    x = px + d0 * c;
                    y = py + d0 * s;
                    total = d0;
                    beam = ROWBUF ? b | (k << 12) : b;
                    nz = nsv;
                    active = true;
                }
            }
            next += nidle;
            int nact = __popcll(vote(active));
            if (nact == 0) break;
            // ---- march phase: the rays that are still marching step, under their own EXEC mask (a finished ray issues no
            // look-up and keeps its total), until enough lanes are idle again or, once no beams are left, the wave has drained ----
            const int go = next < nbl ? WAVE - REFILL_MIN_IDLE : 0; // keep marching while nact > go
#if !defined(F110_BOUNDS)
            if (IDENT && POW2) {
                unsigned long long am = vote(active);
                if (fast) march_ident_pow2_fast<BYTES>(mv, x, y, total, d, c, s, eps, max_range, am, go, nlook, nact);
                else march_ident_pow2<BYTES>(mv, x, y, total, d, c, s, eps, max_range, am, go, nlook, nact);
                active = ((am >> lane) & 1ull) != 0ull;
                continue;
            }
            if (IDENT && !POW2 && fast) {
                unsigned long long am = vote(active);
                while (march_ident_np_fast(mv, x, y, total, d, c, s, eps, max_range, am, go, nlook, nact)) {
                    // a marching ray's quotient lies within 1e-9 of an integer: this one iteration through dist_lookup, which
                    // replays the reference's own division for such lanes (cell_index)
                    nlook += (unsigned)nact;
                    bool act = __builtin_amdgcn_inverse_ballot_w64(am);
                    if (act) {
                        d = dist_lookup<IDENT, POW2, BYTES>(mv, s_lut, x, y);
                        total += d;
                        x += d * c;
                        y += d * s;
                        act = (d > eps) && (total <= max_range);
                    }
                    am = vote(act);
                    nact = __popcll(am);
                    if (nact <= go) break;
                }
                active = ((am >> lane) & 1ull) != 0ull;
                continue;
            }
#endif
            do {
                nlook += (unsigned)nact;
                if (active) {
                    d = dist_lookup<IDENT, POW2, BYTES>(mv, s_lut, x, y);
                    total += d;
                    x += d * c;
                    y += d * s;
                    active = (d > eps) && (total <= max_range);
                }
                nact = __popcll(vote(active));
            } while (nact > go);
        }
        // ---- the staged chunks, whole: slot t holds queue position j0 + t, lane l its beam chunk start + l.  Every beam of the
        // wave has been emitted (the loop ends when no ray marches and none is left to take), and a workgroup is one wave: its
        // own LDS writes are ordered before these reads without a barrier.
        if (ROWBUF && o32) {
            const ScanRowbufPlan rp = scan_rowbuf_plan(nb, lg, part);
            for (int t = 0; t < rp.n_slots; t++) {
                F110_BCHK(((rp.j0 + t) << lg) + part < MAX_CHUNKS, BT_CHUNK_ORDER, rare->dev_err);
                const int i = s_chunk0[(((rp.j0 + t) << lg) + part) & (MAX_CHUNKS - 1)] + lane;
                const float f = s_rows[t * 64 + lane];
                if (i < nb) {
                    F110_BCHK(i >= 0 && t < SCAN_ROWBUF_CHUNKS, BT_SCAN_STORE, rare->dev_err);
                    float *q = reinterpret_cast<float *>(reinterpret_cast<char *>(o32) + (size_t)((unsigned)i * 4u));
                    if (SM == 2) *q = f;
                    else __builtin_nontemporal_store(f, q);
                }
            }
        }
    }
    const ScanArgs *ra = rare;
    asm volatile("" : "+s"(ra));
    if (ra->lookups && lane == 0) atomicAdd(&ra->lookups[car], nlook);

    // ---- iTTC result: the flag only; env_kernel zeroes the state (base_classes.py:241-250)
    // once every wave of the car is done.  Plain store: all writers store the same 1.
    if (STEP) {
        if (vote(hit) != 0ull && lane == 0) ra->in_collision[car] = 1;
    }
}

} // namespace f110
