"""The compact form in the scan's launch plan (red_gym_amd/csrc/f110_scan_plan.h) on the CPU: ScanPlanIn::compact at its
default gives the plan tests/test_scan_plan_cpu.py pins, a non-zero S gives one-wave workgroups with the same stages where the
form applies and nothing else anywhere, and the eligibility rule is held to hand-made shares at, under and over its cap."""
import ctypes
import itertools

import numpy as np
import pytest

import host_build
import test_scan_plan_cpu as base

ROW = 28

SHIM = r'''
#include "f110_scan_plan.h"
using namespace f110;

// compact < 0: the field is left at its default member initialiser
extern "C" int shim_plan_c(int n_cars, int agents, int nb, const int *spec, int n_spec, int step, int stores, int multi,
                           int wg_single, int kind, int compact, int *out, int cap, int *n_out)
{
    std::vector<StageSpec> st;
    for (int i = 0; i < n_spec; i++) st.push_back({spec[2 * i], spec[2 * i + 1]});
    ScanPlanIn in;
    in.n_cars = n_cars; in.agents = agents; in.num_beams = nb; in.stages = &st; in.step = step != 0;
    in.stores = stores == 0 ? nullptr : stores == 1 ? "plain" : "stream";
    in.multi = step && multi; in.wg_single = wg_single != 0; in.kind = kind;
    if (compact >= 0) in.compact = compact;
    std::vector<ScanLaunch> plan;
    const int rc = plan_scan(in, [&](int) { return kind; }, plan);
    *n_out = (int)plan.size();
    if (rc) return rc;
    for (size_t i = 0; i < plan.size() && (int)i < cap; i++) {
        const ScanLaunch &l = plan[i];
        int *r = out + 28 * i;
        memset(r, 0, 28 * sizeof(int));
        r[0] = l.car_base; r[1] = l.n_cars; r[2] = l.kind & 1; r[3] = l.kind >> 1; r[4] = l.sm; r[5] = l.n_stages;
        for (int s = 0; s < l.n_stages; s++) { r[6 + 2 * s] = l.stage_cars[s]; r[7 + 2 * s] = l.stage_log2w[s]; }
        r[22] = l.grid; r[23] = l.block; r[24] = l.wg_single; r[25] = l.order; r[26] = l.events; r[27] = l.lut;
    }
    return rc;
}

extern "C" int shim_choice(const double *share, int n_cars, int agents, double cap, int min_cars)
{
    return cap < 0 ? scan_compact_choice(share, n_cars, agents) : scan_compact_choice(share, n_cars, agents, cap, min_cars);
}
extern "C" void shim_reach(int H, int W, const uint16_t *codes, unsigned code_zero, unsigned off0, unsigned off1, const double *poses,
                           int stride, int n, double ox, double oy, double rinv, double *share)
{
    const unsigned off_far[2] = {off0, off1};
    scan_reach_shares(H, W, [&](int r, int c) { return (unsigned)codes[(size_t)r * W + c]; }, code_zero, off_far, poses, stride, n, ox,
                      oy, rinv, share);
}
extern "C" int shim_override(const char *v) { return scan_form_override(v); }
extern "C" double shim_cap(void) { return SCAN_COMPACT_CAP; }
extern "C" int shim_min_cars(void) { return SCAN_COMPACT_MIN_CARS; }
extern "C" int shim_default_compact(void) { ScanPlanIn in = {}; ScanPlanIn in2; in2.n_cars = 0; return in.compact * 2 + in2.compact; }
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('scan_compact_plan'), 'scancompact', host_build.FAIL_SHIM + SHIM)
    ip = ctypes.POINTER(ctypes.c_int)
    L.shim_plan_c.argtypes = [ctypes.c_int] * 3 + [ip, ctypes.c_int] + [ctypes.c_int] * 6 + [ip, ctypes.c_int, ip]
    L.shim_choice.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    L.shim_override.argtypes = [ctypes.c_char_p]
    L.shim_reach.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_uint] * 3 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_double] * 3 + [ctypes.c_void_p]
    L.shim_reach.restype = None
    L.shim_cap.restype = ctypes.c_double
    return L


def run(L, n, A, nb, spec, step, stores, multi, wg_single, kind, compact):
    sp = [v for c, lg in spec for v in ((-1 if c is None else c), lg)]
    spa = (ctypes.c_int * max(1, len(sp)))(*sp)
    out = np.zeros(64 * ROW, dtype=np.int32)
    n_out = ctypes.c_int(0)
    rc = L.shim_plan_c(n, A, nb, spa, len(spec), int(step), base.STORES[stores], int(multi), int(wg_single), kind, compact,
                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 64, ctypes.byref(n_out))
    if rc:
        return rc
    assert n_out.value <= 64
    res = []
    for r in out[:n_out.value * ROW].reshape(-1, ROW).tolist():
        res.append(dict(car_base=r[0], n_cars=r[1], ident=r[2], pow2=r[3], sm=r[4],
                        stages=[(r[6 + 2 * s], r[7 + 2 * s]) for s in range(r[5])], grid=r[22], block=r[23],
                        wg_single=r[24], order=r[25], events=r[26], lut=r[27]))
    return res


def pinned_inputs():
    """The single-kind inputs of the pinned test's sweep (its kind-split cases need a map per env, where the form never applies)."""
    for n, A, nb, spec, step, stores in itertools.product(base.CARS, base.AGENTS, [64, 1080, 4096], [None, '*:2', '8:0,*:2'],
                                                          [False, True], [None, 'plain']):
        B, n = base.shard(n, A)
        yield n, A, nb, base.parse(spec), step, stores


def test_default_field_is_classic_and_gives_the_pinned_plan(lib):
    assert lib.shim_default_compact() == 0
    for n, A, nb, spec, step, stores in pinned_inputs():
        for multi, wgs, kind in [(False, False, 3), (False, False, 1), (True, True, 3), (True, False, 3)]:
            want = base.plan(n, A, nb, spec, step, stores, multi, wgs, kind, None)
            for compact in (-1, 0):
                got = run(lib, n, A, nb, spec, step, stores, multi, wgs, kind, compact)
                if want == base.E_INVALID:
                    assert got == base.E_INVALID
                    continue
                assert [{k: v for k, v in la.items() if k != 'lut'} for la in got] == want, (n, A, nb, spec, step, stores, multi)
                assert all(la['lut'] == 0 for la in got)


@pytest.mark.parametrize('S', [256, 512])
def test_a_compact_form_gives_one_wave_workgroups_with_the_same_stages(lib, S):
    for n, A, nb, spec, step, stores in pinned_inputs():
        for multi, wgs, kind in [(False, False, 3), (False, False, 1), (False, False, 2), (True, True, 3), (True, False, 3)]:
            classic = run(lib, n, A, nb, spec, step, stores, multi, wgs, kind, 0)
            got = run(lib, n, A, nb, spec, step, stores, multi, wgs, kind, S)
            if classic == base.E_INVALID:
                assert got == base.E_INVALID
                continue
            applies = step and not multi and kind == 3   # the step's scan, a single map, origin unrotated, resolution 2^k
            if not applies:
                assert got == classic
                continue
            assert len(got) == len(classic) == 1
            g, c = got[0], classic[0]
            waves = sum(cars << lg for cars, lg in c['stages'])
            assert g['stages'] == c['stages'] and g['lut'] == S and g['block'] == 64 and g['grid'] == waves and g['wg_single'] == 1
            for k in ('car_base', 'n_cars', 'ident', 'pow2', 'sm', 'order', 'events'):
                assert g[k] == c[k], k


def choice(L, share, n, A=1, cap=-1.0, min_cars=0):
    return L.shim_choice((ctypes.c_double * 2)(*share), n, A, cap, min_cars)


def test_eligibility_rule(lib):
    cap, lo = 0.125, 0.125 - 2.0 ** -20    # hand-made shares: at the cap, one step under it, one over it (exact in binary)
    hi = 0.125 + 2.0 ** -20
    N = 1 << 20
    assert choice(lib, (lo, lo), N, 1, cap, 1) == 256            # the smallest S that qualifies
    assert choice(lib, (cap, lo), N, 1, cap, 1) == 512           # AT the cap does not qualify: the comparison is strict
    assert choice(lib, (hi, lo), N, 1, cap, 1) == 512
    assert choice(lib, (hi, cap), N, 1, cap, 1) == 0
    assert choice(lib, (hi, hi), N, 1, cap, 1) == 0
    assert choice(lib, (lo, hi), N, 1, cap, 1) == 256
    assert choice(lib, (0.0, 0.0), N, 1, 0.0, 1) == 0            # a cap of 0 admits nothing
    # shares from a histogram of ranks: cells of rank >= S - 2 lie behind the S-slot marker (slot 0 is dt[-1,-1], the last the marker)
    ranks = np.r_[np.full(8000, 10), np.full(1000, 253), np.full(999, 254), np.full(1, 510)]
    share = [float((ranks >= S - 2).mean()) for S in (256, 512)]
    assert share == [0.1, 0.0001]
    assert choice(lib, share, N, 1, 0.1, 1) == 512 and choice(lib, share, N, 1, 0.1001, 1) == 256
    assert choice(lib, share, N, 1, 0.0001, 1) == 0
    # the car count and the agents
    assert choice(lib, (0.0, 0.0), 999, 1, cap, 1000) == 0 and choice(lib, (0.0, 0.0), 1000, 1, cap, 1000) == 256
    assert choice(lib, (0.0, 0.0), N, 2, cap, 1) == 0
    # the shipped constants: example_map's corridor (no cell behind either marker) is routed at the benchmark's size, not below
    assert 0.0 < lib.shim_cap() < 0.01 and lib.shim_min_cars() == 32768
    assert choice(lib, (0.0, 0.0), 65536) == 256 and choice(lib, (0.0, 0.0), 32767) == 0
    assert choice(lib, (lib.shim_cap(), 0.0), 65536) == 512 and choice(lib, (1.0, 1.0), 65536) == 0


def test_override_names(lib):
    assert [lib.shim_override(v) for v in (None, b'classic', b'compact256', b'compact512', b'', b'compact', b'Classic')] == \
        [-1, 0, 256, 512, -1, -1, -1]


# ---------------------------------------------------------------- the shares the rule reads
CODE0, OFF256, OFF512 = 8, 8 * 255, 8 * 511     # cell_code(0) and the two markers' offsets (f110_map.h)


def code(rank):
    return 8 * (rank + 1)


def reach(L, codes, cars, ox=-1.0, oy=2.0, res=0.25):
    """cars: [(row, col, fraction inside the cell)] -> (share256, share512) of scan_reach_shares."""
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    H, W = codes.shape
    poses = np.array([[ox + (c + f) * res, oy + (r + f) * res, 0.3] for r, c, f in cars], dtype=np.float64).reshape(-1, 3)
    share = np.zeros(2)
    L.shim_reach(H, W, codes.ctypes.data, CODE0, OFF256, OFF512, poses.ctypes.data, 3, len(cars), ox, oy, 1.0 / res, share.ctypes.data)
    return share.tolist()


def hand_made_map():
    """20 x 30: a wall (code of rank 0) round everything and down column 12; left of it a corridor of 18 x 11 cells with no
    cell behind either marker, right of it open ground of 18 x 16 cells: 100 of them behind the 256-slot marker, 36 of those
    behind the 512-slot one too.  The two touch only through the wall."""
    m = np.full((20, 30), code(0), dtype=np.uint16)
    m[1:19, 1:12] = code(5)
    m[1:19, 13:29] = code(100)
    m[2:12, 14:24] = code(254)        # rank 254 = S - 2 for S = 256: the first rank behind its marker
    m[3:9, 15:21] = code(510)
    m[5, 5] = code(253)               # the last rank inside the 256-slot image, in the corridor
    return m


def test_reach_shares_on_a_hand_made_map(lib):
    m = hand_made_map()
    ground = 18 * 16
    corridor, open_ground = [0.0, 0.0], [100 / ground, 36 / ground]
    assert reach(lib, m, [(3, 3, 0.5)]) == corridor
    assert reach(lib, m, [(3, 20, 0.5)]) == open_ground
    assert reach(lib, m, [(18, 11, 0.01), (1, 1, 0.99)]) == corridor              # the corners of the corridor: cell = floor(...)
    # the mean over the cars: three in the corridor, one on open ground, one inside the wall, one off the map, one NaN
    cars = [(3, 3, 0.5), (10, 8, 0.2), (17, 2, 0.7), (6, 26, 0.5), (0, 0, 0.5), (4, 12, 0.5)]
    want = [open_ground[0] / 6, open_ground[1] / 6]
    assert reach(lib, m, cars) == want
    assert reach(lib, m, cars + [(-3, 4, 0.5), (4, 31, 0.5)]) == [open_ground[0] / 8, open_ground[1] / 8]
    assert reach(lib, m, [(0, 0, 0.5)]) == [0.0, 0.0] and reach(lib, m, [(40, 40, 0.5)]) == [0.0, 0.0]
    codes = np.ascontiguousarray(m)
    poses = np.array([[np.nan, 0.0, 0.0], [-1.0 + 20.5 * 0.25, 2.0 + 3.5 * 0.25, 0.0]])
    share = np.zeros(2)
    lib.shim_reach(20, 30, codes.ctypes.data, CODE0, OFF256, OFF512, poses.ctypes.data, 3, 2, -1.0, 2.0, 4.0, share.ctypes.data)
    assert share.tolist() == [open_ground[0] / 2, open_ground[1] / 2]
    # 8-connected: a diagonal gap in the wall joins the two sides, and the order of the cars does not matter
    m2 = m.copy()
    m2[9, 12] = code(7)
    both = 18 * 11 + ground + 1
    assert reach(lib, m2, [(3, 3, 0.5)]) == reach(lib, m2, [(3, 20, 0.5)]) == [100 / both, 36 / both]
    # ... and so does a gap that is only diagonal: the wall steps from column 12 to column 13 between rows 9 and 10, so that
    # (10, 12) and (9, 13) touch at a corner and nowhere else
    m3 = m.copy()
    m3[10:19, 12] = code(5)
    m3[10:19, 13] = code(0)
    n3 = 18 * 11 + 9 + ground - 9
    out256 = 100 - int((m[10:19, 13] >= OFF256).sum())
    assert reach(lib, m3, [(3, 3, 0.5)]) == reach(lib, m3, [(3, 20, 0.5)]) == [out256 / n3, 36 / n3]
    # with the rule: the corridor's cars are routed, the open ground's are not, and six strays among 65 536 do not change it
    assert choice(lib, reach(lib, m, [(3, 3, 0.5)]), 65536) == 256
    assert choice(lib, reach(lib, m, [(3, 20, 0.5)]), 65536) == 0
    many = [(3, 3, 0.5)] * 5000 + [(3, 20, 0.5)] * 6
    got = reach(lib, m, many)
    assert abs(got[0] - 6 * open_ground[0] / 5006) < 1e-15 and choice(lib, got, 65536) == 256
