"""The row-padded byte cell table on the CPU (red_gym_amd/csrc/f110_map.h: map_pad_rows, map_rows_b, map_cells_bp, cell_elem_bp,
map_bytes_skip, map_bytes_fit, cell_elem_of_byte_padded; f110_scan_plan.h: scan_codes_available): the table as the builder
fills it against the offset arithmetic of the clamp-free march statement (f110_scan.h: march_ident_pow2_fast<true>) replayed in
32-bit wrap-around against MapView::init_bytes' descriptor, the size rule, and the fall-back to word codes."""
import ctypes
import math

import numpy as np
import pytest

import host_build

SHIM = r'''
#include "f110_map.h"
#include "f110_scan_plan.h"
using namespace f110;

extern "C" int shim_pad_rows(double reach) { return map_pad_rows(reach); }
extern "C" int shim_rows_padded(int H) { return map_rows_padded(H); }
extern "C" int shim_rows_b(int H, int P) { return map_rows_b(H, P); }
extern "C" long long shim_cells_bp(int H, int W, int P) { return (long long)map_cells_bp(H, W, P); }
extern "C" long long shim_cells_b(int H, int W) { return (long long)map_cells_b(H, W); }
extern "C" long long shim_cells(int H, int W) { return (long long)map_cells(H, W); }
extern "C" long long shim_skip(int H, int P) { return (long long)map_bytes_skip(H, P); }
extern "C" int shim_fit(int H, int W, int P) { return map_bytes_fit(H, W, P); }
extern "C" long long shim_max_bytes() { return (long long)COMPACT_MAX_BYTES; }
// out[(r + 1) * (W + 2) + (c + 1)] for r = -1 .. H, c = -1 .. W: the padded byte table's element, the plain byte table's, the u16 table's
extern "C" void shim_layouts(int H, int W, int P, long long *bp, long long *b, long long *w)
{
    const int Hp = map_rows_padded(H);
    for (int r = -1; r <= H; r++)
        for (int c = -1; c <= W; c++) {
            const size_t k = (size_t)(r + 1) * (W + 2) + (c + 1);
            bp[k] = (long long)cell_elem_bp(r, c, H, P); b[k] = (long long)cell_elem_b(r, c, Hp); w[k] = (long long)cell_elem(r, c, Hp);
        }
}
extern "C" void shim_elem_of_byte_padded(int H, int W, int P, long long *out)
{
    const size_t n = map_cells_bp(H, W, P);
    for (size_t i = 0; i < n; i++) out[i] = (long long)cell_elem_of_byte_padded(i, H, W, P);
}
extern "C" int shim_codes_available(int has_table, int forced) { return scan_codes_available(has_table != 0, forced); }
extern "C" int shim_codes_choice(int lut, int rowbuf, int forced) { return scan_codes_choice(lut, rowbuf != 0, forced); }
'''

C_PAD = 40                      # columns swept on either side of the map
REACH = (0.5, 3.0, 37.0, 480.0)  # max_range / resolution; 480: 30 m at 2^-4 m, example_map's


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('scan_rowpad'), 'scanrowpad', host_build.FAIL_SHIM + SHIM)
    L.shim_pad_rows.argtypes = [ctypes.c_double]
    for f in (L.shim_cells_bp, L.shim_cells_b, L.shim_cells, L.shim_skip, L.shim_max_bytes):
        f.restype = ctypes.c_longlong
    L.shim_layouts.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    L.shim_elem_of_byte_padded.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    return L


def march_offset(r, c, strip_bytes):
    """The clamp-free statement's arithmetic on a row r and a column c as the hardware does it: v_ashrrev_i32 4,
    v_lshl_add_u32 (row, 4, column), v_mad_i32_i24 with strip_bytes - 16 -- 32-bit wrap-around, the multiply on the sign-extended
    low 24 bits of both operands, no v_med3 on either coordinate.  An offset against MapView::init_bytes' descriptor."""
    def s24(v):
        v = v & 0xffffff
        return v - ((v & 0x800000) << 1)
    c32 = c.astype(np.int64) & 0xffffffff
    strip = (c.astype(np.int64) >> 4) & 0xffffffff
    rc = (((r.astype(np.int64) << 4) & 0xffffffff) + c32) & 0xffffffff
    return (s24(strip) * s24(np.int64(strip_bytes - 16)) + rc) & 0xffffffff


def test_pad_rows_rule(lib):
    """P: the smallest multiple of 8 that is >= ceil(reach) + 2; none for a reach that is no number of cells."""
    for reach in REACH + (0.0, 1.0, 5.999, 6.0, 6.001, 13.9, 14.0, 14.1, 240.0, 485.9, 486.0, 486.1, 600.0, 1e5):
        P = lib.shim_pad_rows(reach)
        need = math.ceil(reach) + 2
        assert P % 8 == 0 and P >= need and P - 8 < need, (reach, P)
    assert lib.shim_pad_rows(480.0) == 488 and lib.shim_pad_rows(240.0) == 248 and lib.shim_pad_rows(40.0) == 48
    for reach in (float('nan'), float('inf'), -1.0, 1e300, float(1 << 20)):
        assert lib.shim_pad_rows(reach) == -1, reach


@pytest.mark.parametrize('reach', REACH)
def test_clamp_free_march_reads_the_cell_or_zero(lib, reach):
    """H 1..40, W 1..70; every row in [-1 - P, H + P] and column in [-40, W + 40] through the statement's arithmetic: a map cell
    reads its own element, anything else reads 0 -- out of the descriptor's range, or a byte the builder writes as 0 -- and so
    no (r, c) outside the map reads a map cell.  The table is the builder's: element i holds what its u16 element holds
    (cell_elem_of_byte_padded), 0 where it has none; the u16 table here holds a cell's own number 1 + r * W + c, 0 on its border
    and padding."""
    P = lib.shim_pad_rows(reach)
    assert P % 8 == 0 and P >= math.ceil(reach) + 2
    for H in range(1, 41):
        Hp, Hb = lib.shim_rows_padded(H), lib.shim_rows_b(H, P)
        assert Hb == ((H + 2 * P + 2 + 7) >> 3) << 3 and Hb % 8 == 0 and Hb >= H + 2 * P + 2
        S = Hb * 16
        skip = lib.shim_skip(H, P)
        assert skip == S + 16 * (1 + P)                                  # strip 1, map row 0
        r = np.arange(-1 - P, H + P + 1)[:, None]
        assert np.array_equal((r + 1 + P) % 8, (r + 1) % 8)               # a line holds the rows it held without the padding
        c_all = np.arange(-C_PAD, 70 + C_PAD + 1)[None, :]
        rel_all = march_offset(r + 0 * c_all, c_all + 0 * r, S)
        for W in range(1, 71):
            n_b, n_w = lib.shim_cells_bp(H, W, P), lib.shim_cells(H, W)
            assert n_b == ((W >> 4) + 2) * S == lib.shim_cells_b(H + 2 * P, W)
            # the layouts of the cells and border cells
            lay_bp, lay_b, lay_w = (np.zeros((H + 2, W + 2), dtype=np.int64) for _ in range(3))
            lib.shim_layouts(H, W, P, lay_bp.ctypes.data, lay_b.ctypes.data, lay_w.ctypes.data)
            rr, cc = np.arange(-1, H + 1)[:, None], np.arange(-1, W + 1)[None, :]
            assert np.array_equal(lay_bp, (((cc >> 4) + 1) * Hb + (rr + P + 1)) * 16 + (cc & 15))
            assert lay_bp.max() < n_b and len(np.unique(lay_bp)) == lay_bp.size
            # 128-byte lines: the padded table moves every cell by whole lines, so a line holds the same 8 x 16 cells
            assert ((lay_bp - lay_b) % 128 == 0).all()
            assert np.array_equal(np.unique(lay_bp // 128, return_inverse=True)[1], np.unique(lay_b // 128, return_inverse=True)[1])
            # the table as the builder fills it
            src = np.zeros(n_b, dtype=np.int64)
            lib.shim_elem_of_byte_padded(H, W, P, src.ctypes.data)
            assert src.min() >= -1 and src.max() < n_w
            assert np.array_equal(src[lay_bp], lay_w)                     # a cell's byte element reads the cell's u16 element
            tw = np.zeros(n_w, dtype=np.int64)
            own = 1 + np.arange(H)[:, None] * W + np.arange(W)[None, :]
            tw[lay_w[1:-1, 1:-1]] = own
            tb = np.where(src >= 0, tw[np.maximum(src, 0)], 0)
            assert np.count_nonzero(tb) == H * W                          # nothing but the map's cells is written non-zero
            # the statement against the descriptor (base: table + skip, n_b - skip bytes; anything else answers 0)
            c = c_all[:, :W + 2 * C_PAD + 1]
            rel = rel_all[:, :W + 2 * C_PAD + 1]
            read = rel < n_b - skip
            got = np.where(read, tb[np.where(read, rel + skip, 0)], 0)
            inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
            want = np.where(inside, 1 + r * W + c, 0)
            assert np.array_equal(got, want), (H, W, P)
            assert read[inside].all()
            assert np.array_equal(((rel + skip) & 0xffffffff)[inside], lay_bp[1:-1, 1:-1].ravel())


def test_size_rule_and_fall_back(lib):
    lim = lib.shim_max_bytes()
    assert lim == 64 << 20
    P = 488
    for H, W in ((1, 1), (40, 70), (800, 800), (1600, 1600), (46, 65519), (46, 65520), (100, 200000), (2000, 40000)):
        fit = lib.shim_cells_bp(H, W, P) <= lim
        assert lib.shim_fit(H, W, P) == int(fit), (H, W)
    assert lib.shim_cells_bp(46, 65519, P) == lim and lib.shim_fit(46, 65519, P) == 1 and lib.shim_fit(46, 65520, P) == 0
    # a map whose u16 tables fit and whose padded byte table does not: compact forms without the byte table
    assert lib.shim_cells(100, 200000) * 2 <= lim and lib.shim_fit(100, 200000, P) == 0 and lib.shim_fit(100, 200000, 8) == 1
    # no P (a reach that is no number of cells): no table; a strip beyond the multiply-add's signed 24 bits: no table
    assert lib.shim_fit(40, 70, -1) == 0
    assert lib.shim_fit(1, 1, 262000) == 1 and lib.shim_fit(1, 1, 262200) == 0
    assert lib.shim_rows_b(1, 262000) * 16 - 16 < 1 << 23
    # the fall-back: without the table the rule sees "word", whatever the override says; with it, the override as it is
    for forced in (-1, 0, 1):
        assert lib.shim_codes_available(1, forced) == forced and lib.shim_codes_available(0, forced) == 0
        for lut in (0, 256, 512):
            for rowbuf in (0, 1):
                assert lib.shim_codes_choice(lut, rowbuf, lib.shim_codes_available(0, forced)) == 0
                assert lib.shim_codes_choice(lut, rowbuf, lib.shim_codes_available(1, forced)) == int(lut == 256 and rowbuf == 1 and forced != 0)
