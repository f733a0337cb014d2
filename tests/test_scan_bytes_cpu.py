"""The byte cell table of the compact scan form of 256 slots on the CPU (red_gym_amd/csrc/f110_map.h: map_cells_b, cell_elem_b,
cell_elem_of_byte, byte_code; f110_scan_plan.h: scan_codes_override, scan_codes_choice): the layout against the offset
arithmetic of the march statements replayed in 32-bit wrap-around, the element, and the routing."""
import ctypes

import numpy as np
import pytest

import host_build

SHIM = r'''
#include "f110_map.h"
#include "f110_scan_plan.h"
using namespace f110;

extern "C" int shim_rows_padded(int H) { return map_rows_padded(H); }
extern "C" long long shim_cells_b(int H, int W) { return (long long)map_cells_b(H, W); }
extern "C" long long shim_cells(int H, int W) { return (long long)map_cells(H, W); }
// out[(r + 1) * n_cols + (c - c_lo)] = cell_elem_b(r, c, Hp) for r = -1 .. H, c = c_lo .. c_lo + n_cols - 1
extern "C" void shim_layout_b(int H, int c_lo, int n_cols, long long *out)
{
    const int Hp = map_rows_padded(H);
    for (int r = -1; r <= H; r++)
        for (int k = 0; k < n_cols; k++) out[(size_t)(r + 1) * n_cols + k] = (long long)cell_elem_b(r, c_lo + k, Hp);
}
// the same for the u16 table's cell_elem, c = -1 .. W
extern "C" void shim_layout_w(int H, int W, long long *out)
{
    const int Hp = map_rows_padded(H);
    for (int r = -1; r <= H; r++)
        for (int c = -1; c <= W; c++) out[(size_t)(r + 1) * (W + 2) + (c + 1)] = (long long)cell_elem(r, c, Hp);
}
extern "C" void shim_elem_of_byte(int H, int W, long long *out)
{
    const int Hp = map_rows_padded(H);
    const size_t n = map_cells_b(H, W);
    for (size_t i = 0; i < n; i++) out[i] = (long long)cell_elem_of_byte(i, Hp, W);
}
extern "C" unsigned shim_byte_code(unsigned code) { return byte_code(code); }
extern "C" unsigned shim_compact_code(unsigned code, int S) { return compact_code(code, S); }
extern "C" int shim_codes_override(const char *v) { return scan_codes_override(v); }
extern "C" int shim_codes_choice(int lut, int rowbuf, int forced) { return scan_codes_choice(lut, rowbuf != 0, forced); }
// through plan_scan: bytes | rowbuf << 1 | lut << 2 of the one launch
extern "C" int shim_plan_codes(int n_cars, int compact, int f32, int rows, int codes, int step, int kind)
{
    std::vector<StageSpec> st;
    ScanPlanIn in;
    in.n_cars = n_cars; in.agents = 1; in.num_beams = 1080; in.stages = &st; in.step = step != 0; in.stores = nullptr;
    in.multi = false; in.wg_single = false; in.kind = kind; in.compact = compact; in.out_f32 = f32 != 0; in.rows = rows;
    if (codes >= -1) in.codes = codes;
    std::vector<ScanLaunch> plan;
    if (plan_scan(in, [&](int) { return kind; }, plan) || plan.size() != 1) return -1;
    return plan[0].bytes | plan[0].rowbuf << 1 | plan[0].lut << 2;
}
'''

C_PAD = 40      # columns swept on either side of the map


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('scan_bytes'), 'scanbytes', host_build.FAIL_SHIM + SHIM)
    L.shim_cells_b.restype = L.shim_cells.restype = ctypes.c_longlong
    L.shim_layout_b.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    L.shim_layout_w.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p]
    L.shim_elem_of_byte.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p]
    L.shim_byte_code.restype = L.shim_compact_code.restype = ctypes.c_uint
    L.shim_byte_code.argtypes = [ctypes.c_uint]
    L.shim_compact_code.argtypes = [ctypes.c_uint, ctypes.c_int]
    L.shim_codes_override.argtypes = [ctypes.c_char_p]
    return L


def march_offset(r, c, strip_bytes):
    """The march statements' arithmetic on a clamped row r and a column c as the hardware does it: v_ashrrev_i32 4,
    v_lshl_add_u32 (row, 4, column), v_mad_i32_i24 with strip_bytes - 16 -- 32-bit wrap-around, the multiply on the
    sign-extended low 24 bits of both operands.  The result is an offset against MapView::init_bytes' descriptor, which starts
    strip_bytes + 16 bytes into the table: the constant of the layout's offset is in its base."""
    def s24(v):
        v = v & 0xffffff
        return v - ((v & 0x800000) << 1)
    c32 = c.astype(np.int64) & 0xffffffff
    strip = (c.astype(np.int64) >> 4) & 0xffffffff                # arithmetic shift of the 32-bit column
    rc = (((r.astype(np.int64) << 4) & 0xffffffff) + c32) & 0xffffffff
    return (s24(strip) * s24(np.int64(strip_bytes - 16)) + rc) & 0xffffffff


def test_layout_sweep(lib):
    """H 1..40, W 1..70, rows -1..H, columns -40..W + 40."""
    for H in range(1, 41):
        Hp = lib.shim_rows_padded(H)
        assert Hp == ((H + 2 + 7) >> 3) << 3
        S = Hp * 16
        r = np.arange(-1, H + 1)[:, None]
        for W in range(1, 71):
            n_b = lib.shim_cells_b(H, W)
            assert n_b == ((W >> 4) + 2) * S
            c = np.arange(-C_PAD, W + C_PAD + 1)[None, :]
            # what the hardware does with the march's offset: inside the descriptor's n_b - skip bytes it reads table byte
            # skip + offset; anywhere else (a negative offset wraps to 2^31 or more) it answers 0.  `off`: the table byte, or
            # n_b + offset where nothing is read
            skip = S + 16
            rel = march_offset(r + 0 * c, c + 0 * r, S)
            read = rel < n_b - skip
            off = np.where(read, rel + skip, n_b + rel)
            lay = np.zeros(off.shape, dtype=np.int64)
            lib.shim_layout_b(H, -C_PAD, off.shape[1], lay.ctypes.data)
            # the layout function is the issue's formula ...
            assert np.array_equal(lay, (((c >> 4) + 1) * Hp + (r + 1)) * 16 + (c & 15))
            # ... and the march forms it wherever the cell or a border cell exists
            # -- as a table byte that is read, or, in front of the descriptor, a border cell's (it holds 0, and 0 is the answer)
            cell = ((c >= -1) & (c <= W)) & (r == r)
            assert np.array_equal(((rel + skip) & 0xffffffff)[cell], lay[cell])
            front = cell & ~read
            assert np.array_equal(front, cell & (lay < skip)) and ((c < 0) | (r < 0))[front].all()
            assert read[(c >= 0) & (c <= W) & (r >= 0)].all()                 # every map cell (and the far borders) is read
            # distinct cells, distinct offsets, all inside the table
            oc = lay[cell]
            assert oc.max() < n_b and len(np.unique(oc)) == oc.size
            # a column outside the strips: an offset at or beyond the table's bytes (negative ones wrap)
            outside = ((c < -16) | (c >= 16 * ((W >> 4) + 1))) & (r == r)
            assert outside.any() and off[outside].min() >= n_b
            # the columns in between that are no cell: inside the table, on none of the cells' elements (padding, which holds 0)
            pad = ~cell & ~outside
            assert not np.isin(off[pad & read], oc).any() and (off[pad & read] < n_b).all()


def test_every_byte_element_names_its_u16_element_or_padding(lib):
    for H, W in [(1, 1), (6, 15), (7, 16), (9, 17), (23, 31), (23, 33), (40, 70), (14, 32), (15, 47), (5, 64)]:
        Hp = lib.shim_rows_padded(H)
        n_b, n_w = lib.shim_cells_b(H, W), lib.shim_cells(H, W)
        src = np.zeros(n_b, dtype=np.int64)
        lib.shim_elem_of_byte(H, W, src.ctypes.data)
        lay_b = np.zeros((H + 2, W + 2), dtype=np.int64)
        lay_w = np.zeros((H + 2, W + 2), dtype=np.int64)
        lib.shim_layout_b(H, -1, W + 2, lay_b.ctypes.data)
        lib.shim_layout_w(H, W, lay_w.ctypes.data)
        assert np.array_equal(src[lay_b], lay_w)                     # a cell's byte element reads the cell's u16 element
        assert src.max() < n_w and src.min() >= -1
        # every other element is the u16 table's padding (rows past H + 1 of the cells' columns: 0 there too) or nothing at all
        other = np.ones(n_b, dtype=bool)
        other[lay_b.ravel()] = False
        named = src[other & (src >= 0)]
        assert not np.isin(named, lay_w.ravel()).any()
        rows = np.arange(n_b) // 16 % Hp
        assert (rows[other & (src >= 0)] >= H + 2).all()


def test_the_element_is_the_slot(lib):
    """compact_code(code, 256) >> 3 for every u16 code 0 .. 8 184 in steps of 8: slot 0 the border, 255 the far marker."""
    for code in range(0, 8185, 8):
        b = lib.shim_byte_code(code)
        assert b == lib.shim_compact_code(code, 256) >> 3 == min(code >> 3, 255)
        assert 0 <= b <= 255 and b << 3 == lib.shim_compact_code(code, 256)      # the march's shift gives the u16 table's code back
    assert lib.shim_byte_code(0) == 0 and lib.shim_byte_code(8 * 255) == 255 and lib.shim_byte_code(8 * 254) == 254


def test_routing(lib):
    assert [lib.shim_codes_override(v) for v in (None, b'byte', b'word', b'', b'BYTE', b'bytes', b'u8')] == [-1, 1, 0, -1, -1, -1, -1]
    for lut in (0, 256, 512):
        for rowbuf in (0, 1):
            for forced in (-1, 0, 1):
                assert lib.shim_codes_choice(lut, rowbuf, forced) == int(lut == 256 and rowbuf == 1 and forced != 0), (lut, rowbuf, forced)
    # through plan_scan (bytes | rowbuf << 1 | lut << 2): bytes exactly where the row buffer is launched
    P = lib.shim_plan_codes
    for codes in (-2, -1, 1):                                                      # -2: the field's default
        assert P(65536, 256, 1, -1, codes, 1, 3) == 1 | 2 | 256 << 2
        assert P(65536, 256, 1, 1, codes, 1, 3) == 1 | 2 | 256 << 2
        assert P(65536, 256, 1, 0, codes, 1, 3) == 256 << 2                        # rows direct: the u16 table
        assert P(65536, 256, 0, -1, codes, 1, 3) == 256 << 2                       # no fp32 output: no row buffer, no bytes
        assert P(65536, 512, 1, 1, codes, 1, 3) == 512 << 2 and P(65536, 0, 1, 1, codes, 1, 3) == 0
        assert P(65536, 256, 1, 1, codes, 0, 3) == 0 and P(65536, 256, 1, 1, codes, 1, 1) == 0   # f110_scan; kind 1
    assert P(65536, 256, 1, -1, 0, 1, 3) == 2 | 256 << 2 and P(65536, 256, 1, 1, 0, 1, 3) == 2 | 256 << 2   # word: the row buffer stays
