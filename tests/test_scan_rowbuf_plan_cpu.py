"""The row buffer of the compact scan form (red_gym_amd/csrc/f110_scan_plan.h: scan_rowbuf_plan, scan_rowbuf_k0,
scan_rowbuf_offset -- the copies scan_kernel itself calls) on the CPU, for every beam count, split and part: what emit stages
and where, against the write-out's (slot, lane) walk, both replayed here on a shuffled chunk order."""
import ctypes

import numpy as np
import pytest

import host_build

SHIM = r'''
#include "f110_scan_plan.h"
using namespace f110;

extern "C" void shim_rowbuf_plan(int nb, int lg, int part, int *out)
{
    const ScanRowbufPlan p = scan_rowbuf_plan(nb, lg, part);
    out[0] = p.my_chunks; out[1] = p.nbl; out[2] = p.j0; out[3] = p.n_slots;
}
// emit's side, as the kernel has it: from the wave's beam count and a beam's queue position alone.  off[k] = byte offset in
// the row buffer of queue position k, or -1 where the beam is stored directly
extern "C" void shim_rowbuf_emit(int nbl, int *off)
{
    const int k0 = scan_rowbuf_k0(nbl);
    for (int k = 0; k < nbl; k++) off[k] = k >= k0 ? (int)scan_rowbuf_offset(k, k0) : -1;
}
extern "C" int shim_rowbuf_chunks(void) { return SCAN_ROWBUF_CHUNKS; }
extern "C" int shim_rowbuf_lds(void) { return SCAN_ROWBUF_BASE + SCAN_ROWBUF_CHUNKS * 256; }
extern "C" int shim_rowbuf_group(void) { return SCAN_LDS_PER_GROUP; }
extern "C" int shim_rows_override(const char *v) { return scan_rows_override(v); }
extern "C" int shim_rows_choice(int lut, int f32, int forced) { return scan_rowbuf_choice(lut, f32 != 0, forced); }
extern "C" int shim_plan_rowbuf(int n_cars, int compact, int f32, int rows, int step, int kind)
{
    std::vector<StageSpec> st;
    ScanPlanIn in;
    in.n_cars = n_cars; in.agents = 1; in.num_beams = 1080; in.stages = &st; in.step = step != 0; in.stores = nullptr;
    in.multi = false; in.wg_single = false; in.kind = kind; in.compact = compact;
    if (f32 >= 0) in.out_f32 = f32 != 0;
    if (rows >= -1) in.rows = rows;
    std::vector<ScanLaunch> plan;
    if (plan_scan(in, [&](int) { return kind; }, plan) || plan.size() != 1) return -1;
    return plan[0].rowbuf | plan[0].lut << 1;
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('scan_rowbuf_plan'), 'scanrowbuf', host_build.FAIL_SHIM + SHIM)
    L.shim_rowbuf_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
    L.shim_rowbuf_emit.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.shim_rows_override.argtypes = [ctypes.c_char_p]
    return L


def plan(L, nb, lg, part):
    out = np.zeros(4, dtype=np.int32)
    L.shim_rowbuf_plan(nb, lg, part, out.ctypes.data)
    return out.tolist()


def test_the_buffer_is_what_a_group_of_32_has_left(lib):
    C = lib.shim_rowbuf_chunks()
    assert lib.shim_rowbuf_group() == 163840 // 32 == 5120
    assert lib.shim_rowbuf_lds() == 256 * 8 + 64 * 4 + C * 256 <= 5120 < lib.shim_rowbuf_lds() + 256   # the largest count that fits
    assert C == 11


@pytest.mark.parametrize('lg', [0, 1, 2, 3])
def test_every_beam_is_direct_or_in_one_slot_and_the_write_out_walks_exactly_the_staged_ones(lib, lg):
    C = lib.shim_rowbuf_chunks()
    wpc = 1 << lg
    rng = np.random.default_rng(lg)
    off = np.zeros(4096, dtype=np.int32)
    lanes = np.arange(64)
    for nb in range(1, 4097):
        nch = (nb + 63) // 64
        # the chunk order: a permutation of the chunk starts (multiples of 64) with the car's last, possibly short, chunk last
        chunk0 = np.r_[rng.permutation(nch - 1), nch - 1] * 64
        seen = np.zeros(nb, dtype=np.int32)
        for part in range(wpc):
            my_chunks, nbl, j0, n_slots = plan(lib, nb, lg, part)
            # the slice: chunk positions part, part + wpc, ... of the car's queue; the last chunk of the car may be short
            mine = chunk0[part::wpc]
            assert my_chunks == len(mine) and nbl == int(np.minimum(64, nb - mine).sum())
            assert j0 == max(0, my_chunks - C) and n_slots == min(my_chunks, C)
            if nbl == 0:
                continue
            k = np.arange(nbl)
            j = k >> 6
            beam = mine[j] + (k & 63)                 # what the refill hands out at queue position k
            assert beam.max() < nb
            seen[beam] += 1
            lib.shim_rowbuf_emit(nbl, off.ctypes.data)
            o = off[:nbl]
            staged = o >= 0
            assert np.array_equal(staged, j >= j0)                               # the last min(my_chunks, C) positions, no other
            so = o[staged]
            assert np.array_equal(so, (j[staged] - j0) * 256 + (beam[staged] & 63) * 4)   # slot j - j0, dword (beam & 63)
            assert so.size == 0 or (so.min() >= 0 and so.max() + 4 <= C * 256 and len(np.unique(so)) == so.size)
            # the write-out: slot t, lane l reads float t * 64 + l and stores it to beam chunk start + l where that is a beam
            wb = (mine[j0:j0 + n_slots, None] + lanes[None, :]).ravel()
            wf = (np.arange(n_slots)[:, None] * 64 + lanes[None, :]).ravel()
            keep = wb < nb
            assert wf.size == 0 or wf.max() < C * 64
            want = dict(zip((so // 4).tolist(), beam[staged].tolist()))
            assert dict(zip(wf[keep].tolist(), wb[keep].tolist())) == want
            if wpc == 1:
                assert staged.all() == (nb <= 64 * C)                            # up to capacity everything is staged ...
                if 64 * C < nb <= 64 * (C + 1):
                    assert j0 == 1 and np.array_equal(~staged, j == 0)           # ... one chunk more: exactly one chunk direct
        assert (seen == 1).all()                                                 # the parts share the car's beams out, once each


def test_the_shapes_the_issue_names(lib):
    assert plan(lib, 1080, 0, 0) == [17, 1080, 6, 11]                            # a whole car: 11 chunks staged (696 beams), 6 direct
    for part in range(4):
        assert plan(lib, 1080, 2, part)[2] == 0                                  # the tail's split cars stage everything
    assert max(plan(lib, 4096, 3, p)[0] for p in range(8)) == 8
    assert plan(lib, 704, 0, 0) == [11, 704, 0, 11] and plan(lib, 705, 0, 0) == [12, 705, 1, 11]


def test_override_names_and_the_rule(lib):
    assert [lib.shim_rows_override(v) for v in (None, b'lds', b'direct', b'', b'LDS', b'ldss')] == [-1, 1, 0, -1, -1, -1]
    for forced in (-1, 1):
        assert lib.shim_rows_choice(256, 1, forced) == 1
        assert lib.shim_rows_choice(256, 0, forced) == 0 and lib.shim_rows_choice(512, 1, forced) == 0
        assert lib.shim_rows_choice(0, 1, forced) == 0
    assert lib.shim_rows_choice(256, 1, 0) == 0
    # through plan_scan: (rowbuf | lut << 1) of the one launch; f32 = -1 / rows = -2 leave the fields at their defaults
    assert lib.shim_plan_rowbuf(65536, 256, 1, -1, 1, 3) == 513 and lib.shim_plan_rowbuf(65536, 256, 1, 1, 1, 3) == 513
    assert lib.shim_plan_rowbuf(65536, 256, 1, 0, 1, 3) == 512 and lib.shim_plan_rowbuf(65536, 256, 0, -1, 1, 3) == 512
    assert lib.shim_plan_rowbuf(65536, 256, -1, -2, 1, 3) == 512                 # no fp32 row unless the caller says so
    assert lib.shim_plan_rowbuf(65536, 512, 1, 1, 1, 3) == 1024 and lib.shim_plan_rowbuf(65536, 0, 1, 1, 1, 3) == 0
    assert lib.shim_plan_rowbuf(65536, 256, 1, 1, 0, 3) == 0 and lib.shim_plan_rowbuf(65536, 256, 1, 1, 1, 1) == 0   # f110_scan; kind 1
