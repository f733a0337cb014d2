"""A map per env (f110_assign_maps) against the fp64 oracle at every launch shape the scan takes for it.

With several maps the step's scan is launched once per run of envs whose maps are of one KIND (resolution a power of two or
not, origin rotated or not), each launch with its own first car and its own stage list; where neighbouring cars stand on
different maps it runs one wave per workgroup (wg_single), otherwise the two waves of a workgroup each stage HALF of the
look-up table, each from its own car's map, and f110_set_scan_order is ignored.  Every test here builds its maps from crops
of the shipped maps (walled in, so that rays stay short and 4 096 slots stay small), compares sampled envs with one oracle
Env each (a Scanner built from the same mask, resolution, origin and angle) or two engines with `==`, and ends with a clean
device error word (the bounds-checked build then covers the map slot index, tests/test_gpu_bounds.py)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402

T = 8          # steps of every oracle run; a masked reset after step MASK_AT
MASK_AT = 3


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _source(name):
    from red_gym_amd import maps, workload
    y = workload.EXAMPLE_MAP + '.yaml' if name == 'example' else maps.builtin_map_yaml(name)
    return maps.load_map(y, '.png').free


def _crop(name, r0, c0, h, w, res, theta, ox, oy):
    """A walled-in crop of a shipped map as a slot spec (free mask, resolution, origin x, origin y, origin angle)."""
    free = np.ascontiguousarray(_source(name)[r0:r0 + h, c0:c0 + w], dtype=np.uint8)
    free[0, :] = free[-1, :] = 0
    free[:, 0] = free[:, -1] = 0
    return (free, float(res), float(ox), float(oy), float(theta))


def _kind(spec):
    res, theta = spec[1], spec[4]
    return (float(np.cos(theta)) == 1.0 and float(np.sin(theta)) == 0.0, np.frexp(res)[0] == 0.5)


# The matrix's slots: every kind twice, the two maps of a kind at different resolutions (so that every entry of their
# look-up tables differs and a table staged half from one and half from the other shows in the scans).
POOL = {
    0: ('example', 330, 180, 160, 200, 0.0625, 0.0, -3.0, -2.0),    # ident, pow2
    1: ('example', 900, 1100, 150, 170, 0.125, 0.0, 1.5, -9.0),     # ident, pow2
    2: ('berlin', 120, 200, 170, 150, 0.05, 0.0, -4.0, 3.0),        # ident
    3: ('skirk', 200, 100, 160, 160, 0.07, 0.0, 2.0, 2.0),          # ident
    4: ('example', 1200, 400, 150, 180, 0.0625, 0.4, -1.0, 5.0),    # pow2
    5: ('berlin', 300, 250, 160, 170, 0.05, 0.3, 6.0, -3.0),        # neither: the rotated 0.05 m slot
    6: ('skirk', 300, 300, 128, 128, 0.0625, 0.0, -7.0, -6.0),      # ident, pow2
    7: ('example', 600, 700, 140, 160, 0.25, 0.0, 4.0, 0.5),        # ident, pow2
}


def _pool(slot):
    return _crop(*POOL[slot])


_DT = {}


def _dt(spec):
    """The slot's distance table as oracle.load_map builds it: res * scipy's EDT of the free mask."""
    from scipy.ndimage import distance_transform_edt
    free, res = spec[:2]
    k = (free.tobytes(), free.shape, res)
    if k not in _DT:
        _DT[k] = np.ascontiguousarray(res * distance_transform_edt(free))
    return _DT[k]


def _scanner(spec):
    """oracle.Scanner on the slot's map: dt = res * EDT(mask) as oracle.load_map, orig_c / orig_s as set_map_occupancy."""
    free, res, ox, oy, theta = spec
    sc = oracle.Scanner(1080, 2 * np.pi)
    sc.set_map_dict({'height': free.shape[0], 'width': free.shape[1], 'resolution': res, 'orig_x': ox, 'orig_y': oy,
                     'orig_c': float(np.cos(theta)), 'orig_s': float(np.sin(theta)), 'dt': _dt(spec)})
    return sc


def _poses(specs, assign, A, rng, overlap_every=7):
    """Random poses on free cells at least 0.35 m from a wall of every env's own map (the cell centre taken to the world
    through the map's origin); in every overlap_every-th env of several agents agent 1 sits on agent 0 (GJK hit, done,
    autoreset)."""
    B = len(assign)
    poses = np.zeros((B, A, 3))
    for slot in np.unique(assign):
        free, res, ox, oy, theta = specs[slot]
        cells = np.argwhere(_dt(specs[slot]) > 0.35)
        envs = np.nonzero(assign == slot)[0]
        pick = cells[rng.integers(0, len(cells), (len(envs), A))]
        xr, yr = (pick[..., 1] + 0.5) * res, (pick[..., 0] + 0.5) * res
        c, s = np.cos(theta), np.sin(theta)
        poses[envs, :, 0] = ox + xr * c - yr * s
        poses[envs, :, 1] = oy + xr * s + yr * c
        poses[envs, :, 2] = rng.uniform(-np.pi, np.pi, (len(envs), A))
    if A > 1:
        poses[::overlap_every, 1, :2] = poses[::overlap_every, 0, :2] + 0.1
    return poses


def _kind_runs(specs, assign):
    """The scan launches of a step (f110_step.hip run_step): one for all envs when every used slot is of the
    (ident, pow2) kind, else one per run of envs of one kind.  [(first env, end env)]."""
    kinds = [_kind(specs[s]) for s in assign]
    if all(_kind(sp) == (True, True) for sp in specs.values()):
        return [(0, len(assign))]
    runs, e0 = [], 0
    for e in range(1, len(assign) + 1):
        if e == len(assign) or kinds[e] != kinds[e0]:
            runs.append((e0, e))
            e0 = e
    return runs


def _sample(specs, assign, A, rng, n_random=24):
    """Random envs plus the envs at the edges of launches, map blocks and the default list's tail stage."""
    B = len(assign)
    runs = _kind_runs(specs, assign)
    edges = [0, B - 1]
    for e0, e1 in (runs if len(runs) <= 48 else [runs[i] for i in rng.choice(len(runs), 48, replace=False)]):
        edges += [e0, e1 - 1]
        n = (e1 - e0) * A
        if n > 2048:                                  # one wave per car: "*:0,<tail>:2" (scan_stage_list)
            star = n - min(4096 if A >= 2 else 2048, n // 2)
            if star % 2 == 0:                         # (an odd first stage falls back to one stage)
                t0 = e0 + star // A
                edges += [t0 - 1, t0, t0 + 1]
    blocks = np.nonzero(np.diff(assign))[0]
    if len(blocks) > 48:
        blocks = rng.choice(blocks, 48, replace=False)
    for b in blocks:
        edges += [b, b + 1]
    extra = rng.choice(B, size=min(n_random, B), replace=False)
    s = np.unique(np.clip(np.r_[edges, extra], 0, B - 1))
    return s


def _engine(B, A, specs, assign, **kw):
    from red_gym_amd import F110VecEnv, workload
    kw.setdefault('autoreset', True)
    env = F110VecEnv(B, map=workload.EXAMPLE_MAP, map_ext='.png', num_agents=A, keep_f64_scans=True, count_lookups=True, **kw)
    for slot, spec in specs.items():
        env.eng.set_map_occupancy(*spec, slot=slot)
    env.eng.assign_maps(assign)
    return env


def _run_vs_oracle(env, specs, assign, poses, acts, sample, seeds=None, env_params=None):
    """T autoreset steps with a masked reset after step MASK_AT; every sampled env against its own oracle Env:
    state and scans_f64 to 1e-9, scans to 1e-5, collisions and done `==`, distance-table reads `==` at the end.  Returns the
    number of done flags the sampled envs raised."""
    A = poses.shape[1]
    scanners = {}
    ors = {}
    for b in sample:
        b = int(b)
        slot = int(assign[b])
        if slot not in scanners:
            scanners[slot] = _scanner(specs[slot])
        noise = oracle.noise_table(12345 if seeds is None else seeds[b], T + 4)
        ors[b] = oracle.Env(scanners[slot], A, params=None if env_params is None else env_params[b], noise=noise)
    B = len(assign)
    mask = np.zeros(B, dtype=np.uint8)
    mask[1::3] = 1
    env.reset(torch.as_tensor(poses, device=env.device))
    oo = {b: ors[b].reset(poses[b]) for b in ors}
    pending = {b: oo[b]['done'] for b in ors}

    def compare(tag):
        st, s64, s32 = _np(env.state[sample]), _np(env.eng.t['scans_f64'][sample]), _np(env.eng.t['scans'][sample])
        col, dn = _np(env.eng.t['collisions'][sample]), _np(env.eng.t['done'][sample])
        for j, b in enumerate(ors):
            assert np.allclose(st[j], oo[b]['state'], rtol=0, atol=1e-9), (tag, b)
            assert np.allclose(s64[j], oo[b]['scans'], rtol=0, atol=1e-9), (tag, b)
            assert np.allclose(s32[j], oo[b]['scans'], rtol=0, atol=1e-5), (tag, b)
            assert np.array_equal(col[j].astype(np.float64), oo[b]['collisions']), (tag, b)
            assert bool(dn[j]) == oo[b]['done'], (tag, b)

    compare('reset')
    dones = 0
    for k in range(T):
        env.step(torch.as_tensor(acts[k], device=env.device))
        for b in ors:
            oo[b] = ors[b].reset(poses[b]) if pending[b] else ors[b].step(acts[k][b])
            pending[b] = oo[b]['done']
            dones += int(oo[b]['done'])
        compare(k)
        if k == MASK_AT:
            # only the masked envs and those waiting for their autoreset take part in this reset's step
            env.reset(torch.as_tensor(poses, device=env.device), torch.as_tensor(mask, device=env.device))
            for b in ors:
                if mask[b] or pending[b]:
                    oo[b] = ors[b].reset(poses[b])
                    pending[b] = oo[b]['done']
            compare('masked reset')
    lk = _np(env.eng.t['lookups'][sample]).sum(axis=1)
    assert np.array_equal(lk, [oo[b]['lookups'] for b in ors])
    assert env.eng.device_errors() == 0
    return dones


def _layout(name, B, A):
    """env -> slot of the matrix's layouts."""
    e = np.arange(B)
    if name == 'even_blocks':        # (a) blocks of an even car count, several kind runs: two-wave workgroups
        order = [0, 2, 4, 5, 1, 3]
        cuts = [(B * k // len(order)) & ~1 for k in range(len(order) + 1)]
        cuts[-1] = B
        out = np.zeros(B, dtype=np.int32)
        for k, s in enumerate(order):
            out[cuts[k]:cuts[k + 1]] = s
        return out
    if name == 'interleaved':        # (b) e % K: neighbours differ, wg_single
        return np.asarray([0, 2, 4, 5, 1, 3], dtype=np.int32)[e % 6]
    if name == 'odd_blocks':         # (c) blocks of odd env counts
        sizes = np.resize([7, 13, 5, 11, 9, 3], B)
        blk = np.repeat(np.arange(B), sizes)[:B]
        return np.asarray([3, 2, 0, 5, 4, 1], dtype=np.int32)[blk % 6]
    if name == 'one_kind':           # (d) every used slot (ident, pow2): one launch that reads env_map
        sizes = np.resize([16, 1, 1, 9, 30, 2, 5], B)
        blk = np.repeat(np.arange(B), sizes)[:B]
        return np.asarray([0, 1, 6, 7], dtype=np.int32)[blk % 4]
    if name == 'two_slots':          # (e) a rotated 0.05 m slot and an unrotated 2^-4 m slot
        return np.where(e < (B * 2) // 5, 0, 5).astype(np.int32)
    raise ValueError(name)


LAYOUTS = ['even_blocks', 'interleaved', 'odd_blocks', 'one_kind', 'two_slots']


def _specs_for(assign):
    return {int(s): _pool(int(s)) for s in np.unique(np.r_[assign, 0])}


# 8, 4, 4 and 1 waves per car (waves_per_car: up to 1 024 cars 8, up to 2 048 cars 4, 1 beyond); odd car counts
@pytest.mark.parametrize('B,A', [(97, 1), (700, 3), (611, 3), (4099, 1), (3001, 2)])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_launch_shapes_vs_oracle(B, A, layout):
    from red_gym_amd import workload
    rng = np.random.default_rng(B * 10 + A)
    assign = _layout(layout, B, A)
    specs = _specs_for(assign)
    env = _engine(B, A, specs, assign)
    poses = _poses(specs, assign, A, rng)
    acts = workload.action_pool(T, B, A)
    dones = _run_vs_oracle(env, specs, assign, poses, acts, _sample(specs, assign, A, rng))
    assert dones > 0 or A == 1      # (overlapping cars: GJK hit, done, autoreset)
    env.close()


def _fullsize_specs(n_slots, rng, h=48, w=64):
    """n_slots small walled-in crops of the three shipped maps at random places, every kind (by slot quarter)."""
    srcs = ['example', 'berlin', 'skirk']
    kinds = [(0.0625, 0.0), (0.05, 0.0), (0.125, 0.35), (0.07, 0.6)]   # (ident, pow2), (ident), (pow2), (neither)
    specs = {}
    for s in range(n_slots):
        name = srcs[s % 3]
        H, W = _source(name).shape
        while True:
            r0, c0 = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            res, theta = kinds[(s * 4) // n_slots]
            sp = _crop(name, r0, c0, h, w, res, theta, rng.uniform(-20, 20), rng.uniform(-20, 20))
            if (_dt(sp) > 0.35).sum() >= 40:    # room for cars (_poses)
                break
        specs[s] = sp
    return specs


def test_fullsize_two_maps_interleaved_vs_oracle():
    """The profiled configuration: 65 536 envs x 1 agent on two (ident, pow2) maps, env e on map e % 2 -- one launch of
    one-wave workgroups with the default tail stage (2 048 cars of four waves each)."""
    from red_gym_amd import workload
    B, A = 65536, 1
    rng = np.random.default_rng(65536)
    specs = {0: _pool(0), 1: _pool(1)}
    assign = (np.arange(B) % 2).astype(np.int32)
    env = _engine(B, A, specs, assign)
    sample = _sample(specs, assign, A, rng, n_random=40)
    assert B - 2048 in sample
    _run_vs_oracle(env, specs, assign, _poses(specs, assign, A, rng), workload.action_pool(T, B, A), sample)
    env.close()


def test_fullsize_four_kinds_in_blocks_vs_oracle():
    """16 384 envs x 2 agents, four maps of the four kinds in equal blocks: four launches of two-wave workgroups."""
    from red_gym_amd import workload
    B, A = 16384, 2
    rng = np.random.default_rng(16384)
    specs = {0: _pool(0), 2: _pool(2), 4: _pool(4), 5: _pool(5)}
    assign = np.asarray([0, 2, 4, 5], dtype=np.int32)[(np.arange(B) * 4) // B]
    env = _engine(B, A, specs, assign)
    assert _run_vs_oracle(env, specs, assign, _poses(specs, assign, A, rng), workload.action_pool(T, B, A),
                          _sample(specs, assign, A, rng, n_random=32)) > 0
    env.close()


def test_every_slot_used_4096_maps_x_16_envs_vs_oracle():
    """All F110_MAX_MAPS slots hold a map of their own and every one is used: 65 536 envs, 16 per slot in blocks, the
    four kinds in four quarters of the slots; the envs of slot 4 095 are sampled."""
    from red_gym_amd import _lib, workload
    n_slots = _lib.F110_MAX_MAPS
    B, A = 16 * n_slots, 1
    rng = np.random.default_rng(4096)
    specs = _fullsize_specs(n_slots, rng)
    assign = (np.arange(B) // 16).astype(np.int32)
    env = _engine(B, A, specs, assign)
    sample = np.unique(np.r_[_sample(specs, assign, A, rng, n_random=32), B - 16, B - 9, B - 1])
    _run_vs_oracle(env, specs, assign, _poses(specs, assign, A, rng), workload.action_pool(T, B, A), sample)
    env.close()


def test_every_env_its_own_world_vs_oracle():
    """4 096 envs x 2 agents, each with its own map slot pattern (e % 61 over 61 slots of all four kinds), its own noise
    generator (noise_source='per_env', seed per env) and its own params slot (mass and friction: the beam tables follow env
    0's width / lf / lr, a documented limit), sampled envs against oracle Envs built the same way."""
    from red_gym_amd import workload
    from red_gym_amd.engine import DEFAULT_PARAMS
    B, A = 4096, 2
    rng = np.random.default_rng(61)
    specs = _fullsize_specs(61, rng, h=64, w=80)
    assign = (np.arange(B) % 61).astype(np.int32)
    seeds = [5000 + 13 * e for e in range(B)]
    pars = [dict(DEFAULT_PARAMS, m=3.0 + 1.5 * (e % 97) / 97, mu=0.8 + 0.5 * ((e * 7) % 89) / 89) for e in range(B)]
    env = _engine(B, A, specs, assign, seed=seeds, params=pars, noise_source='per_env')
    assert env.eng._noise_per_env
    assert _run_vs_oracle(env, specs, assign, _poses(specs, assign, A, rng), workload.action_pool(T, B, A),
                          _sample(specs, assign, A, rng, n_random=32), seeds=seeds, env_params=pars) > 0
    env.close()


# ---------------------------------------------------------------- stage lists under a map per env
def _same_steps(e1, e2, poses, acts, steps=T, check_every=1):
    keys = ('scans_f64', 'scans', 'state', 'lookups', 'collisions', 'in_collision', 'toggles', 'done', 'noise_step')
    B = poses.shape[0]
    mask = torch.zeros(B, dtype=torch.uint8, device='cuda')
    mask[::3] = 1
    p = torch.as_tensor(poses, device='cuda')
    e1.reset(p); e2.reset(p)
    for k in range(steps):
        a = torch.as_tensor(acts[k % len(acts)], device='cuda')
        e1.step(a); e2.step(a)
        if k == MASK_AT:
            e1.reset(p, mask); e2.reset(p, mask)
        if k % check_every == 0 or k == steps - 1:
            for key in keys:
                assert torch.equal(e1.eng.t[key], e2.eng.t[key]), (k, key)


def _stage_boundaries(B, A, spec):
    """Env -> slot with block boundaries at even cars inside every stage after the first (where a stage list that starts
    a stage at an odd car would pair two cars of two maps in one workgroup).  Slots 0, 7 and 1 are all (ident, pow2), at
    0.0625, 0.25 and 0.125 m (every entry of their tables differs): ONE launch, whose stages start where the list says."""
    n = B * A
    stages = [s.split(':') for s in spec.split(',')]
    fixed = sum(int(c) - int(c) % 2 for c, _ in stages if c != '*')
    cars = [n - fixed if c == '*' else int(c) - int(c) % 2 for c, _ in stages]
    out = np.zeros(B, dtype=np.int32)
    c0 = 0
    for k, c in enumerate(cars[:-1]):
        c0 += c
        # the first env after the start of the next stage whose first car is even
        e = [e for e in range(c0 // A, B) if (e * A) % 2 == 0 and e * A > c0]
        if e:
            out[e[0]:] = [7, 1][k % 2]
    return out


@pytest.mark.parametrize('spec', ['*:1,32:0', '*:2,16:0,8:1', '*:3,2:0', '8:0,*:2', '6:2,*:0,10:1'])
@pytest.mark.parametrize('B,A', [(97, 1), (33, 3)])
def test_stage_lists_under_a_map_per_env_give_identical_results(spec, B, A):
    """f110_set_scan_stages(spec) on a map-per-env engine `==` the same engine on the default stage list: scans, lookups,
    state, collisions, done (include/f110_hip.h: results do not depend on the stage list).  The stage lists put a "*"
    stage of an odd car count and 2 / 4 / 8 waves per car in front of other stages; map blocks begin at even cars inside
    the later stages."""
    from red_gym_amd import workload
    rng = np.random.default_rng(len(spec) * 7 + A)
    assign = _stage_boundaries(B, A, spec)
    specs = _specs_for(assign)
    e1, e2 = _engine(B, A, specs, assign), _engine(B, A, specs, assign)
    e2.eng.set_scan_stages(spec)
    poses = _poses(specs, assign, A, rng)
    _same_steps(e1, e2, poses, workload.action_pool(T, B, A))
    assert e1.eng.device_errors() == 0 and e2.eng.device_errors() == 0
    e1.close(); e2.close()


@pytest.mark.parametrize('spec', ['*:1,32:0', '*:2,16:0,8:1', '*:3,2:0'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_stage_lists_on_the_matrix_layouts(spec, layout):
    """The same `==` on the layouts of test_launch_shapes_vs_oracle (701 envs x 1 agent: odd car counts in most launches)."""
    from red_gym_amd import workload
    B, A = 701, 1
    rng = np.random.default_rng(701)
    assign = _layout(layout, B, A)
    specs = _specs_for(assign)
    e1, e2 = _engine(B, A, specs, assign), _engine(B, A, specs, assign)
    e2.eng.set_scan_stages(spec)
    _same_steps(e1, e2, _poses(specs, assign, A, rng), workload.action_pool(T, B, A))
    assert e1.eng.device_errors() == 0 and e2.eng.device_errors() == 0
    e1.close(); e2.close()


# ---------------------------------------------------------------- graphs
def _graph_setup(B, A):
    from red_gym_amd import workload
    assign = _layout('even_blocks', B, A)
    specs = _specs_for(assign)
    rng = np.random.default_rng(B)
    return assign, specs, _poses(specs, assign, A, rng), torch.as_tensor(workload.action_pool(8, B, A), device='cuda')


@pytest.mark.parametrize('how', ['nodes', 'capture'])
def test_library_graph_with_kind_runs_equals_eager(how):
    """f110_graph_create of a step that holds one scan launch per kind run: 20 replays `==` eager steps; assign_maps with
    another pattern moves the launch epoch, the old graph is refused (F110_E_INVALID) and step_lib_graph re-builds it."""
    from red_gym_amd import _lib
    B, A = 301, 1
    assign, specs, poses, acts = _graph_setup(B, A)
    e1, e2 = _engine(B, A, specs, assign), _engine(B, A, specs, assign)
    e1.reset(poses); e2.reset(poses)
    buf = e2.build_step_graph(how)
    assert e2.lib_graph_info() == 2 + len(_kind_runs(specs, assign))    # dynamics, the scans, env bookkeeping
    keys = [k for k in e1.eng.t if e1.eng.t[k] is not None]
    for k in range(40):
        e1.step(acts[k % 8])
        buf.copy_(acts[k % 8])
        e2.step_lib_graph()
        if k == 19:
            torch.cuda.synchronize()
            for key in keys:
                assert torch.equal(e1.eng.t[key], e2.eng.t[key]), key
            other = _layout('odd_blocks', B, A)
            ep = e2.eng.launch_epoch()
            e1.eng.assign_maps(other); e2.eng.assign_maps(other)
            assert e2.eng.launch_epoch() > ep
            assert e2.eng.lib.f110_graph_launch(e2._lg, e2.eng._stream()) == _lib.E_INVALID
    torch.cuda.synchronize()
    for key in keys:
        assert torch.equal(e1.eng.t[key], e2.eng.t[key]), key
    assert e1.eng.device_errors() == 0 and e2.eng.device_errors() == 0
    e1.close(); e2.close()


def test_captured_step_with_kind_runs_equals_eager():
    """F110VecEnv.capture_step / step_graph (a torch stream capture) across several scan launches, and its re-capture after
    assign_maps with another pattern: `==` eager stepping."""
    B, A = 301, 2
    assign, specs, poses, acts = _graph_setup(B, A)
    e1, e2 = _engine(B, A, specs, assign), _engine(B, A, specs, assign)
    e1.reset(poses); e2.reset(poses)
    buf = e2.capture_step()
    keys = [k for k in e1.eng.t if e1.eng.t[k] is not None]
    for k in range(40):
        e1.step(acts[k % 8])
        buf.copy_(acts[k % 8])
        e2.step_graph()
        if k == 19:
            torch.cuda.synchronize()
            for key in keys:
                assert torch.equal(e1.eng.t[key], e2.eng.t[key]), key
            ep = e2.eng.launch_epoch()
            other = _layout('interleaved', B, A)
            e1.eng.assign_maps(other); e2.eng.assign_maps(other)
            assert e2.eng.launch_epoch() > ep
    torch.cuda.synchronize()
    for key in keys:
        assert torch.equal(e1.eng.t[key], e2.eng.t[key]), key
    assert e2._g_epoch == e2.eng.launch_epoch()                         # re-captured
    assert e1.eng.device_errors() == 0 and e2.eng.device_errors() == 0
    e1.close(); e2.close()


# ---------------------------------------------------------------- scan order
def test_scan_order_is_ignored_with_several_maps_and_applies_again_after():
    """A random launch order set through the ABI (and Engine's own sorting, REORDER_MIN_CARS lowered) on a multi-map
    handle: `==` the car-order run; after assign_maps(None) the order applies again and the results stay `==`."""
    from red_gym_amd import workload
    from red_gym_amd.engine import _lib, _ptr
    B, A = 2051, 1
    assign = _layout('interleaved', B, A)
    specs = _specs_for(assign)
    rng = np.random.default_rng(2051)
    poses = _poses(specs, assign, A, rng)
    acts = workload.action_pool(8, B, A)
    e0, e1 = _engine(B, A, specs, assign), _engine(B, A, specs, assign)
    e0.eng.scan_reorder = False
    e1.eng.REORDER_MIN_CARS = 1024
    perm = torch.randperm(B * A, generator=torch.Generator().manual_seed(5)).to(dtype=torch.int32, device=e1.device)
    _lib.check(e1.eng.lib.f110_set_scan_order(e1.eng._h, _ptr(perm)))
    _same_steps(e0, e1, poses, acts, steps=24, check_every=4)
    # back to one map: the order is used again
    p0 = _poses({0: specs[0]}, np.zeros(B, dtype=np.int32), A, rng)
    for e in (e0, e1):
        e.eng.assign_maps(None)
    _same_steps(e0, e1, p0, acts, steps=24, check_every=4)
    assert e0.eng.device_errors() == 0 and e1.eng.device_errors() == 0
    e0.close(); e1.close()
