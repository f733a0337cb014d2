// f110_map.h -- the cell-table format of a map, shared by the host code that builds the tables (f110_maps.hip), the device
// pipeline that builds them (f110_mapgen.h) and the scan that reads them (f110_scan.h).  No kernels.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else // a plain host compile (tests/test_scan_bytes_cpu.py holds the layout functions): the qualifiers say nothing there
#define __host__
#define __device__
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace f110 {

// Cell table.  Each map cell stores, as a u16, the BYTE OFFSET of its distance inside the LDS copy of the LUT:
// 8 * (k + 1), k = RANK of the cell's exact squared distance d2 (in cells, to the nearest obstacle) among the distinct d2
// values of the map, for k < LDS_RANKS = 1022 (squared distances are sums of two squares, so that reaches d2 ~ 3 900 =
// 62 cells); OFF_FAR for larger ranks and for cells of a user table that are not resolution*sqrt(int) -- those re-read a
// second table (u16 rank, 65535 = "use the fp64 table") in a rarely taken branch.
// The table has a one-cell BORDER on every side holding code 0, and LDS slot 0 holds dt[-1,-1]: the reference's
// out-of-bounds read (laser_models.py:80-81,:103) becomes an ordinary lookup of a clamped index -- no bounds compare, no
// select in the march loop (the loaded value addresses the ds_read directly).
// The far marker's LDS slot holds -0.0: as a distance it is an exact no-op (total += -0.0, x += -0.0 * c) that ends the ray's
// march (-0.0 > eps is false); the wave looks at the sign of its parked lanes' last distance once per refill, not once per look-up.
// Layout: 8-column strips, map cell (r, c), r in -1..H, c in -1..W, at [(c >> 3) + 1][r + 1][c & 7] (arithmetic
// shift: the left border column is the last column of strip 0), so one 128-B cache line holds an 8x8-cell block.  The 64 rays of a wave sample neighbouring
// points, so a gather touches fewer lines than with a row-major table (which measured
// ~40 L1 accesses per 64-lane gather and made the kernel L1-tag-rate bound), and the byte
// offset is two shift-adds and one multiply-add: (c >> 3) * (strip_bytes - 16) + (c << 1) + (r << 4) + strip_bytes + 16.
// (Round 5 tried to have the address unit form an equivalent layout -- a swizzled structured descriptor, index = row, offset =
// 2 * column, the descriptor's range check as the row clamp: two VALU instructions instead of six -- and it is exact and 26 %
// slower: an `idxen` load merges at most two lanes per access, profiles/r05_swizzle_probe.txt.)
constexpr int LUT_LDS = 1024;                           // LDS LUT slots
constexpr unsigned SLOT_OOB = 0, SLOT_FAR = LUT_LDS - 1; // slot 0: dt[-1,-1]; slots 1 .. LUT_LDS-2: ranks 0 .. LDS_RANKS-1; last: far marker
constexpr unsigned LDS_RANKS = LUT_LDS - 2;
constexpr unsigned OFF_FAR = 8 * SLOT_FAR;
constexpr unsigned CODE_ESC = 65535;                    // second table: read the fp64 table instead
__host__ __device__ inline unsigned cell_code(unsigned rank) { return rank < LDS_RANKS ? 8u * (rank + 1u) : OFF_FAR; }
// Compact forms (one-wave workgroups, f110_scan_plan.h): an LDS image of S slots -- the first S - 1 slots of the classic image
// (dt[-1,-1] and ranks 0 .. S-3), then the far marker -- and a cell table of its own in which every code at or beyond the
// marker's slot IS the marker's offset.  Same strips, same border; a cell behind the marker takes the second table as ever, so
// only the share of look-ups on that rare path differs.  A map sized for its road rarely needs more than a few hundred ranks,
// and 2 KB instead of 8 KB per LUT copy is what lets every wave own one.
constexpr int N_COMPACT = 2;
constexpr int LUT_COMPACT[N_COMPACT] = {256, 512};
__host__ __device__ constexpr unsigned compact_off_far(int S) { return 8u * (unsigned)(S - 1); }
__host__ __device__ constexpr unsigned compact_code(unsigned code, int S) { return code < compact_off_far(S) ? code : compact_off_far(S); }
__host__ __device__ constexpr int compact_index(int S) { return S == 256 ? 0 : S == 512 ? 1 : -1; }
static_assert(compact_index(LUT_COMPACT[0]) == 0 && compact_index(LUT_COMPACT[1]) == 1, "compact_index names LUT_COMPACT's entries");
// geometry of the padded strip table
__host__ __device__ inline int map_rows_padded(int H) { return ((H + 2 + 7) >> 3) << 3; }
__host__ __device__ inline size_t map_cells(int H, int W) { return (size_t)((W >> 3) + 2) * map_rows_padded(H) * 8; } // strip 0 only holds the left border column
// element index of map cell (r, c), -1 <= r <= H, -1 <= c <= W
__host__ __device__ inline size_t cell_elem(int r, int c, int Hp) { return ((size_t)((c >> 3) + 1) * Hp + (size_t)(r + 1)) * 8 + (size_t)(c & 7); }
// Byte table of the compact form of 256 slots.  Its codes are multiples of 8 below 2 048 -- 8 bits of information -- so the cell
// holds the SLOT, compact_code(code, 256) >> 3 (0: the border / dt[-1,-1], 255: the far marker), and the march shifts it back
// into the LDS byte offset.  Strips of 16 columns, 16 bytes per row inside a strip, so strip_bytes = Hp * 16 is the u16
// table's and a 128-B line holds 8 rows x 16 columns: map cell (r, c) at [(c >> 4) + 1][r + 1][c & 15], byte offset
// (c >> 4) * (strip_bytes - 16) + c + (r << 4) + strip_bytes + 16.  Border and padding hold 0 as in the u16 tables.
__host__ __device__ constexpr unsigned byte_code(unsigned code) { return compact_code(code, LUT_COMPACT[0]) >> 3; }
__host__ __device__ inline size_t map_cells_b(int H, int W) { return (size_t)((W >> 4) + 2) * map_rows_padded(H) * 16; } // strip 0 only holds the left border column
__host__ __device__ inline size_t cell_elem_b(int r, int c, int Hp) { return ((size_t)((c >> 4) + 1) * Hp + (size_t)(r + 1)) * 16 + (size_t)(c & 15); }
// the u16 table's element of the cell that byte element i stands for (border, padding and the columns past W included: the u16
// table's padding holds 0 too), or (size_t)-1 where the u16 table has no such element (strips past its last one)
__host__ __device__ inline size_t cell_elem_of_byte(size_t i, int Hp, int W)
{
    const size_t strip = i / ((size_t)Hp * 16), row = i / 16 % (size_t)Hp, col = i % 16;
    const long long c = ((long long)strip - 1) * 16 + (long long)col; // -16 .. 16 * ((W >> 4) + 1) - 1
    if (c < -1 || c > W) return (size_t)-1;                           // outside the border columns: padding
    return ((size_t)((c >> 3) + 1) * Hp + row) * 8 + (size_t)(c & 7);
}

// The byte table as the device holds it: ROW-PADDED.  Every strip carries P rows of 0 above the border row -1 and at least P
// below the border row H, P = map_pad_rows(max_range / resolution): the smallest multiple of 8 that is >= ceil(reach) + 2.
// Every look-up of a ray lies within max_range of its car, so for a car standing on rows -1 .. H no row a march can form
// leaves [-1 - P, H + P] -- its own strip -- and the fast march needs no clamp of the row (f110_scan.h: march_ident_pow2_fast).
// The layout is the one above for a map of H + 2 P rows with row r stored at r + P: cell_elem_b(r + P, c, map_rows_b(H, P)).
// P is a multiple of 8, so the padded rows stay a multiple of 8 and (r + 1 + P) = (r + 1) mod 8: a 128-B line holds the very
// 8 x 16 cells it held without the padding.
constexpr size_t COMPACT_MAX_BYTES = (size_t)64 << 20;  // the largest table a compact form (and the padded byte table) may be
constexpr int MAP_PAD_ROWS_MAX = 1 << 20;
// P for reach = max_range / resolution in cells, or -1 where there is none (a reach that is not finite, negative or absurd)
__host__ __device__ inline int map_pad_rows(double reach)
{
    if (!(reach >= 0.0) || !(reach < (double)MAP_PAD_ROWS_MAX)) return -1;
    return (((int)ceil(reach) + 2 + 7) >> 3) << 3;
}
__host__ __device__ inline int map_rows_b(int H, int P) { return map_rows_padded(H + 2 * P); }
__host__ __device__ inline size_t map_cells_bp(int H, int W, int P) { return map_cells_b(H + 2 * P, W); }
__host__ __device__ inline size_t cell_elem_bp(int r, int c, int H, int P) { return cell_elem_b(r + P, c, map_rows_b(H, P)); }
// the bytes in front of strip 1, map row 0 -- where the march's descriptor starts (MapView::init_bytes)
__host__ __device__ inline size_t map_bytes_skip(int H, int P) { return (size_t)map_rows_b(H, P) * 16 + 16 * (size_t)(1 + P); }
// the size rule: the padded table counts toward the compact tables' limit, and its strip must stay a signed 24-bit operand
// of the march's multiply-add.  Where it fails no byte table is built and the launch reads word codes.
__host__ __device__ inline bool map_bytes_fit(int H, int W, int P)
{
    return P >= 0 && (long long)H + 2ll * P + 10 < (1ll << 19) && map_cells_bp(H, W, P) <= COMPACT_MAX_BYTES;
}
// cell_elem_of_byte for the padded table: byte row `row` stands for the u16 table's row `row - P` (its r + 1); the padding
// rows have no u16 element
__host__ __device__ inline size_t cell_elem_of_byte_padded(size_t i, int H, int W, int P)
{
    const int Hb = map_rows_b(H, P), Hp = map_rows_padded(H);
    const size_t strip = i / ((size_t)Hb * 16), col = i % 16;
    const long long row = (long long)(i / 16 % (size_t)Hb) - P;      // the u16 table's row index, r + 1
    const long long c = ((long long)strip - 1) * 16 + (long long)col;
    if (c < -1 || c > W || row < 0 || row >= Hp) return (size_t)-1;
    return ((size_t)((c >> 3) + 1) * Hp + (size_t)row) * 8 + (size_t)(c & 7);
}

struct MapDev {
    const uint16_t *cells;  // padded strips [(W >> 3) + 2][Hp][8] of LDS byte offsets
    const uint16_t *cells_far; // same layout: rank (<= 65534) of the cells marked OFF_FAR, 65535 = fp64 table
    unsigned cells_bytes;
    unsigned strip_bytes;   // Hp * 16, Hp = H + 2 rounded up to a multiple of 8
    const double *lut;      // [lut_len <= 65535] resolution*sqrt(d2_k), indexed by rank k
    const double *lut_lds;  // [LUT_LDS] image staged in LDS: dt[-1,-1], lut[0..LDS_RANKS-1], -0.0
    const double *dt;       // [H*W] exact fp64 distance table (escape path, rarely touched)
    int H, W;
    double res, rinv, ox, oy, oc, os, wres, hres, oob; // oob = dt[H-1][W-1]
    unsigned lut_len;       // entries of lut
    const uint16_t *cells_c[N_COMPACT];  // compact cell tables (layout and size of `cells`) for S = LUT_COMPACT[i], or NULL
    const double *lut_lds_c[N_COMPACT];  // [S] their LDS images
    const uint8_t *cells_b;              // row-padded byte table of cells_c[0] (16-column strips, map_cells_bp elements), or NULL
    unsigned cells_b_bytes;
    unsigned strip_bytes_b;              // its strip: map_rows_b(H, pad_rows) * 16 (the u16 tables keep strip_bytes)
    unsigned pad_rows;                   // its P
};

} // namespace f110
