"""The scan's launch plan (red_gym_amd/csrc/f110_scan_plan.h) on the CPU: the header and a small extern "C" shim are
compiled for the host and loaded with ctypes.  Results of the scan do not depend on the plan (the GPU tests hold every
launch shape to `==`), so a plan that drifts from the measured launch shapes would only cost speed, silently: here every
launch the plan makes is compared, field by field, with a restatement of its rules in Python."""
import ctypes
import functools

import numpy as np
import pytest

import host_build

E_INVALID = -1
MAX_MAPS = 4096
ROW = 27   # ints per launch in the shim's output

SHIM = r'''
#include "f110_scan_plan.h"
using namespace f110;

extern "C" int shim_parse(const char *s, int *out, int cap, const char **why)
{
    std::vector<StageSpec> spec;
    *why = "";
    if (!parse_stage_spec(s, spec, why)) return -1;
    for (size_t i = 0; i < spec.size() && (int)i < cap; i++) { out[2 * i] = spec[i].cars; out[2 * i + 1] = spec[i].lg; }
    return (int)spec.size();
}

// slot_kind: per slot ident | pow2 << 1; multi: the handle's map per env (f110_assign_maps), which only the step's scan reads
extern "C" int shim_plan(int n_cars, int agents, int nb, const int *spec, int n_spec, int step, int stores, int multi,
                         int wg_single, int ident, int pow2, const int32_t *env_map, const uint8_t *slot_kind, int *out,
                         int cap, int *n_out)
{
    std::vector<StageSpec> st;
    for (int i = 0; i < n_spec; i++) st.push_back({spec[2 * i], spec[2 * i + 1]});
    ScanPlanIn in;
    in.n_cars = n_cars; in.agents = agents; in.num_beams = nb; in.stages = &st; in.step = step != 0;
    in.stores = stores == 0 ? nullptr : stores == 1 ? "plain" : "stream";
    in.multi = step && multi; in.wg_single = wg_single != 0; in.kind = ident | pow2 << 1;
    g_msg[0] = 0;
    std::vector<ScanLaunch> plan;
    const int rc = plan_scan(in, [&](int env) { return (int)slot_kind[env_map[env]]; }, plan);
    *n_out = (int)plan.size();
    if (rc) return rc;
    for (size_t i = 0; i < plan.size() && (int)i < cap; i++) {
        const ScanLaunch &l = plan[i];
        int *r = out + 27 * i;
        memset(r, 0, 27 * sizeof(int));
        r[0] = l.car_base; r[1] = l.n_cars; r[2] = l.kind & 1; r[3] = l.kind >> 1; r[4] = l.sm; r[5] = l.n_stages;
        for (int s = 0; s < l.n_stages; s++) { r[6 + 2 * s] = l.stage_cars[s]; r[7 + 2 * s] = l.stage_log2w[s]; }
        r[22] = l.grid; r[23] = l.block; r[24] = l.wg_single; r[25] = l.order; r[26] = l.events;
    }
    return rc;
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('scan_plan'), 'scanplan', host_build.FAIL_SHIM + SHIM)
    L.shim_message.restype = ctypes.c_char_p
    L.shim_parse.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                             ctypes.POINTER(ctypes.c_char_p)]
    ip = ctypes.POINTER(ctypes.c_int)
    L.shim_plan.argtypes = [ctypes.c_int] * 3 + [ip, ctypes.c_int] + [ctypes.c_int] * 6 + [
        ctypes.c_void_p, ctypes.c_void_p, ip, ctypes.c_int, ip]
    return L


# ---------------------------------------------------------------- the rules, restated
STORES = {None: 0, 'plain': 1, 'stream': 2}


def parse(spec):
    """A valid "cars:lg,..." list as [(cars or None for "*", lg)]; None or '' -> []."""
    out = []
    for part in (spec or '').split(',') if spec else []:
        c, _, lg = part.partition(':')
        out.append((None if c == '*' else int(c), int(lg or 0)))
    return out


@functools.lru_cache(maxsize=None)
def stage_list(spec, n, A, nb):
    """spec: a tuple of parse()."""
    if not spec:
        nch = -(-nb // 64)
        wpc = 8 if n <= 1024 else 4 if n <= 2048 else 1
        while wpc > 1 and wpc > nch:
            wpc //= 2
        if wpc > 1 or nch < 8:
            return [(n, wpc.bit_length() - 1)]      # the default single stage is not normalised
        spec = [(None, 0), (min(4096 if A >= 2 else 2048, n // 2), 2)]
    st = [(None if c is None else c - c % 2, lg) for c, lg in spec]
    fixed = sum(c for c, _ in st if c is not None)
    if fixed > n:
        st, fixed = [(None, 0)], 0
    if any(c is None for c, _ in st):
        st = [(n - fixed if c is None else c, lg) for c, lg in st]
    else:
        st.append((n - fixed, 0))
    st = [(c, lg) for c, lg in st if c > 0]
    if any(c % 2 for c, _ in st[:-1]) or len(st) > 8:
        return [(n, 0)]
    return st


def kind_runs(kinds):
    """Maximal runs of equal values: [(first env, end env)]."""
    cuts = np.r_[0, np.flatnonzero(kinds[1:] != kinds[:-1]) + 1, len(kinds)]
    return list(zip(cuts[:-1].tolist(), cuts[1:].tolist()))


def plan(n, A, nb, spec, step, stores, multi, wg_single, kind_and, env_kinds):
    """[dict per launch], or E_INVALID."""
    multi = step and multi
    wgs = multi and wg_single
    if multi and kind_and != 3:
        shape = [(e0 * A, (e1 - e0) * A, int(env_kinds[e0])) for e0, e1 in kind_runs(env_kinds)]
    else:
        shape = [(0, n, kind_and)]
    out = []
    for i, (base, m, kind) in enumerate(shape):
        stages = stage_list(tuple(spec), m, A, nb)
        if multi and not wgs and any((base + sum(c for c, _ in stages[:j])) % 2 for j in range(len(stages))):
            return E_INVALID
        plain = stores == 'plain' if stores else m > 327680
        waves = sum(c << lg for c, lg in stages)
        out.append(dict(car_base=base, n_cars=m, ident=kind & 1, pow2=kind >> 1, sm=0 if not step else 2 if plain else 1,
                        stages=stages, grid=waves if wgs else -(-waves // 2), block=64 if wgs else 128, wg_single=int(wgs),
                        order=int(step and not multi), events=int(step and i == 0)))
    return out


# ---------------------------------------------------------------- the plan, through the shim
def run_plan(L, n, A, nb, spec, step, stores, multi=False, wg_single=False, kind_and=3, env_map=None, slot_kind=None):
    sp = [v for c, lg in spec for v in ((-1 if c is None else c), lg)]
    spa = (ctypes.c_int * max(1, len(sp)))(*sp)
    if env_map is None:
        env_map = np.zeros(max(1, n // A), dtype=np.int32)
    env_map = np.ascontiguousarray(env_map, dtype=np.int32)
    sk = np.zeros(MAX_MAPS, dtype=np.uint8)
    if slot_kind is not None:
        sk[:len(slot_kind)] = slot_kind
    cap, n_out = 0, ctypes.c_int(16)
    while n_out.value > cap:   # (the shim reports every launch, writes those that fit)
        cap = n_out.value
        out = np.zeros(cap * ROW, dtype=np.int32)
        rc = L.shim_plan(n, A, nb, spa, len(spec), int(step), STORES[stores], int(multi), int(wg_single), kind_and & 1,
                         kind_and >> 1, env_map.ctypes.data, sk.ctypes.data,
                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), cap, ctypes.byref(n_out))
        if rc:
            return rc
    res = []
    for r in out[:n_out.value * ROW].reshape(-1, ROW).tolist():
        res.append(dict(car_base=r[0], n_cars=r[1], ident=r[2], pow2=r[3], sm=r[4],
                        stages=[(r[6 + 2 * s], r[7 + 2 * s]) for s in range(r[5])], grid=r[22], block=r[23],
                        wg_single=r[24], order=r[25], events=r[26]))
    return res


def check(L, n, A, nb, spec, step, stores, multi=False, wg_single=False, kind_and=3, env_map=None, slot_kind=None):
    """The plan == the restatement, and its invariants."""
    got = run_plan(L, n, A, nb, spec, step, stores, multi, wg_single, kind_and, env_map, slot_kind)
    env_kinds = None
    if env_map is not None:
        env_kinds = np.asarray(slot_kind, dtype=np.uint8)[np.asarray(env_map)]
    want = plan(n, A, nb, spec, step, stores, multi, wg_single, kind_and, env_kinds)
    assert got == want, (n, A, nb, spec, step, stores, multi, wg_single, kind_and)
    assert got != E_INVALID, L.shim_message()
    c0 = 0
    for la in got:
        assert la['car_base'] == c0                           # the runs cover every car, in order
        assert sum(c for c, _ in la['stages']) == la['n_cars']
        assert 1 <= len(la['stages']) <= 8
        assert all(c >= 1 and 0 <= lg <= 3 for c, lg in la['stages'])
        if step and multi and not wg_single:                  # two-wave workgroups on a map per env: even stage starts
            s = la['car_base']
            for c, _ in la['stages']:
                assert s % 2 == 0, (la, s)
                s += c
        c0 += la['n_cars']
    assert c0 == n
    return got


CARS = [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 65536, 327680, 327681, 524288]
AGENTS = [1, 2, 3, 12]
BEAMS = [2, 64, 271, 511, 512, 1080, 4096]
# test_gpu_step.py::test_scan_stage_lists_give_identical_results and test_gpu_map_per_env.py
SPECS = [None, '*:0', '*:1', '*:3', '8:0,*:2', '6:2,*:0,10:1', '20:3,*:0,4:2', '*:1,32:0', '*:2,16:0,8:1', '*:3,2:0']


def random_specs(rng, k):
    out = []
    for _ in range(k):
        parts = ['%d:%d' % (rng.integers(0, 5000), rng.integers(0, 4)) for _ in range(rng.integers(0, 6))]
        if rng.random() < 0.7:
            parts.insert(int(rng.integers(0, len(parts) + 1)), '*:%d' % rng.integers(0, 4))
        out.append(','.join(parts) if parts else '*:0')
    return out


def shard(cars, A):
    """The envs and cars of a shard near `cars` cars."""
    B = max(1, cars // A)
    return B, B * A


def specs_for(n, rng):
    """The fixed list plus random valid ones, without those f110_set_scan_stages refuses for a handle of n cars."""
    return [s for s in SPECS + random_specs(rng, 4) if sum(c for c, _ in parse(s) if c is not None) <= n]


# ---------------------------------------------------------------- one map
@pytest.mark.parametrize('A', AGENTS)
def test_one_map_plans(lib, A):
    """The step's scan and f110_scan on one map: every car count, beam count, stage list and store mode."""
    rng = np.random.default_rng(A)
    cars = CARS + rng.integers(1, 600000, 6).tolist()
    for cars_ in cars:
        B, n = shard(cars_, A)
        for nb in BEAMS:
            for spec in specs_for(n, rng):
                for stores in (None, 'plain', 'stream'):
                    got = check(lib, n, A, nb, parse(spec), True, stores, kind_and=int(rng.integers(0, 4)))
                    assert len(got) == 1 and got[0]['order'] == 1 and got[0]['events'] == 1
                # f110_scan: any pose count, one agent, SM 0; the step's list may not fit (whole cars then)
                got = check(lib, cars_, 1, nb, parse(spec), False, None)
                assert len(got) == 1 and got[0]['sm'] == 0 and got[0]['order'] == 0 and got[0]['events'] == 0


def test_default_list_pins(lib):
    """A few launch shapes by hand: 8 / 4 / 1 waves per car by size, the four-wave tail of big launches."""
    def stages(n, A=1, nb=1080, spec=None, step=True):
        return run_plan(lib, n, A, nb, parse(spec), step, None)[0]['stages']
    assert stages(1024) == [(1024, 3)]
    assert stages(1025) == [(1025, 2)] and stages(2048) == [(2048, 2)]
    assert stages(2049) == [(2049, 0)]                  # "*" of 1 025 cars in front of the tail is odd: whole cars
    assert stages(65536) == [(63488, 0), (2048, 2)]
    assert stages(65536, A=2) == [(61440, 0), (4096, 2)]
    assert stages(4097) == [(4097, 0)]                  # "*" of 2 049 cars is odd: one stage of whole cars
    assert stages(1024, nb=64) == [(1024, 0)]           # one chunk of beams: one wave per car
    assert stages(1024, nb=200) == [(1024, 2)]          # four chunks: at most 4 waves per car
    assert stages(97, spec='*:1,32:0') == [(97, 0)]     # an odd "*" in front of other stages: whole cars
    assert stages(98, spec='*:1,32:0') == [(66, 1), (32, 0)]
    big = run_plan(lib, 327681, 1, 1080, [], True, None)[0]
    assert big['sm'] == 2 and run_plan(lib, 327680, 1, 1080, [], True, None)[0]['sm'] == 1


# ---------------------------------------------------------------- a map per env
# slot -> kind (ident | pow2 << 1), as the matrix of test_gpu_map_per_env.py: every kind, (ident, pow2) twice
SLOT_KIND = [3, 3, 1, 1, 2, 0]


def layout(name, B, rng):
    e = np.arange(B)
    if name == 'uniform':
        return np.zeros(B, dtype=np.int32)
    if name == 'one_kind':
        return np.asarray([0, 1], dtype=np.int32)[(e // 5) % 2]
    if name == 'blocks':
        out = np.zeros(B, dtype=np.int32)
        for k, s in enumerate([0, 2, 4, 5, 1, 3]):
            out[B * k // 6:] = s
        return out
    if name == 'odd_blocks':
        blk = np.repeat(np.arange(B), np.resize([7, 13, 5, 11, 9, 3], B))[:B]
        return np.asarray([3, 2, 0, 5, 4, 1], dtype=np.int32)[blk % 6]
    if name == 'interleaved':
        return np.asarray([0, 2, 4, 5, 1, 3], dtype=np.int32)[e % 6]
    if name == 'random':
        blk = np.repeat(np.arange(B), rng.integers(1, 9, B))[:B]
        return rng.integers(0, 6, B).astype(np.int32)[blk]
    raise ValueError(name)


def assign_flags(env_map, A):
    """multi, wg_single as f110_assign_maps sets them, and the AND of the kinds over the used slots (slot 0 always)."""
    multi = bool((env_map != 0).any())
    cars = np.repeat(env_map, A)
    single = multi and bool((cars[1::2] != cars[:-1:2][:len(cars[1::2])]).any())
    kind_and = 3
    for s in set(env_map.tolist()) | {0}:
        kind_and &= SLOT_KIND[s]
    return multi, single, kind_and


@pytest.mark.parametrize('name', ['uniform', 'one_kind', 'blocks', 'odd_blocks', 'interleaved', 'random'])
@pytest.mark.parametrize('A', AGENTS)
def test_map_per_env_plans(lib, name, A):
    """Kind runs, wg_single, events and orders of the step's scan on the layouts of test_gpu_map_per_env.py."""
    rng = np.random.default_rng(A * 100 + len(name))
    many_runs = name in ('interleaved', 'random', 'odd_blocks')
    for cars_ in CARS + rng.integers(1, 20000, 4).tolist():
        B, n = shard(cars_, A)
        if many_runs and B > 2100:
            continue   # (runs of a few envs each: more envs add launches, not shapes)
        env_map = layout(name, B, rng)
        multi, single, kind_and = assign_flags(env_map, A)
        for nb in (1080,) if many_runs else (64, 271, 1080):
            for spec in specs_for(n, rng):
                for stores in (None, 'plain', 'stream'):
                    got = check(lib, n, A, nb, parse(spec), True, stores, multi, single, kind_and, env_map, SLOT_KIND)
                    assert sum(la['events'] for la in got) == 1 and got[0]['events'] == 1
                    assert all(la['order'] == int(not multi) for la in got)
                # f110_scan ignores the map per env: one launch, the AND kind
                got = check(lib, cars_, 1, nb, parse(spec), False, None, multi, single, kind_and, env_map, SLOT_KIND)
                assert len(got) == 1 and (got[0]['ident'] | got[0]['pow2'] << 1) == kind_and


def test_ce522ba_shape_stays_at_even_cars(lib):
    """A map per env in two-wave workgroups (blocks of (ident, pow2) maps at even cars: one launch) with a "*" stage of an
    odd car count in front of other stages: the plan falls back to whole cars, never starts a stage at an odd car."""
    for B, A, spec in [(97, 1, '*:1,32:0'), (97, 1, '*:2,16:0,8:1'), (97, 1, '*:3,2:0'), (33, 3, '*:1,32:0'),
                       (33, 3, '*:3,2:0')]:
        env_map = np.zeros(B, dtype=np.int32)
        env_map[(B // 2) & ~1:] = 1
        multi, single, kind_and = assign_flags(env_map, A)
        assert multi and not single and kind_and == 3
        got = check(lib, B * A, A, 1080, parse(spec), True, None, multi, single, kind_and, env_map, SLOT_KIND)
        assert got[0]['stages'] == [(B * A, 0)], got


def test_inconsistent_inputs_are_refused(lib):
    """A kind run that starts at an odd car without wg_single (f110_assign_maps would have set it) is an error code."""
    env_map = np.r_[np.full(3, 2), np.zeros(7)].astype(np.int32)   # cars 0..2 on an (ident) map, a run from car 3
    rc = run_plan(lib, 10, 1, 1080, [], True, None, True, False, 1, env_map, SLOT_KIND)
    assert rc == E_INVALID
    assert b'starts at car 3' in lib.shim_message()
    got = check(lib, 10, 1, 1080, [], True, None, True, True, 1, env_map, SLOT_KIND)
    assert [(la['car_base'], la['n_cars'], la['block']) for la in got] == [(0, 3, 64), (3, 7, 64)]


# ---------------------------------------------------------------- the parser (f110_set_scan_stages)
def test_parse_stage_spec(lib):
    """The lists of test_gpu_step.py::test_set_scan_stages_refuses_malformed_lists against the parser itself ("100:0,*:1"
    parses: f110_set_scan_stages refuses it for naming more cars than its handle has)."""
    def parsed(s):
        out = (ctypes.c_int * 32)()
        why = ctypes.c_char_p()
        k = lib.shim_parse(s.encode(), out, 16, ctypes.byref(why))
        return None if k < 0 else [(out[2 * i], out[2 * i + 1]) for i in range(k)]
    for bad in ('x', '*:9', '*:0,*:1', '4:0:1', '1:0,1:0,1:0,1:0,1:0,1:0,*:0', '*:-1', '2:0,', '', '1073741824:0', ':1', '*:'):
        assert parsed(bad) is None, bad
    assert parsed('4') == [(4, 0)]
    assert parsed('4:1,*:0') == [(4, 1), (-1, 0)]
    assert parsed('100:0,*:1') == [(100, 0), (-1, 1)]
    assert parsed('1:0,1:1,1:2,1:3,*:0,0:0') == [(1, 0), (1, 1), (1, 2), (1, 3), (-1, 0), (0, 0)]
    for s in SPECS[1:]:
        assert parsed(s) == [(-1 if c is None else c, lg) for c, lg in parse(s)], s
