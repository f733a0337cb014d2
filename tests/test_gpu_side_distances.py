"""Side distances per vehicle (f110_set_side_distance_slots, side_distances='per_env'): every env's iTTC wall test uses the
outline of its OWN car.  One handle against one oracle Env per env whose oracle.Scanner was built from that env's params
(base_classes.py:116-156 run per independently constructed env), next to the default mode against oracle envs that all
share env 0's scanner (one process's class-level statics).  tests/test_side_distances_cpu.py checks that the two oracle
readings really differ in this scenario."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from side_distance_cases import VEHICLES, Scanners, batch, differs, oracle_history  # noqa: E402

TESTS = os.path.dirname(os.path.abspath(__file__))


def _np(t):
    return t.detach().cpu().numpy()


def _env(assets, B, A, env_par, mode, map_name=None, **kw):
    from red_gym_amd import F110VecEnv
    return F110VecEnv(B, map=map_name or os.path.join(assets, 'example_map'), num_agents=A, params=env_par, autoreset=True,
                      keep_f64_scans=True, side_distances=mode, **kw)


def _compare(env, hist, poses, acts, T, envs=None, step=None, tag=''):
    """reset + T steps of `env` against the oracle histories: state / fp64 scans 1e-9, the rest `==`, every step"""
    import torch
    envs = list(hist) if envs is None else envs
    step = step or env.step
    env.reset(poses)
    for k in range(T):
        obs, _, done, info = step(torch.as_tensor(acts[k % acts.shape[0]], device='cuda'))
        st, sc, col = _np(env.state), _np(obs['scans_f64']), _np(obs['collisions'])
        idx, tg, dn = _np(info['collision_idx']), _np(info['toggles']), _np(done)
        for e in envs:
            h = hist[e]
            assert np.array_equal(col[e].astype(np.float64), h['collisions'][k]), (tag, k, e, 'collisions')
            assert bool(dn[e]) == bool(h['done'][k]), (tag, k, e, 'done')
            assert np.allclose(st[e], h['state'][k], rtol=0, atol=1e-9), (tag, k, e, 'state')
            assert np.allclose(sc[e], h['scans'][k], rtol=0, atol=1e-9), (tag, k, e, 'scans')
            assert np.array_equal(idx[e].astype(np.float64), h['collision_idx'][k]), (tag, k, e, 'collision_idx')
            assert np.array_equal(tg[e].astype(np.float64), h['toggles'][k]), (tag, k, e, 'toggles')
    assert env.eng.device_errors() == 0, tag


def _histories(assets, B, A, T, which=('own', 'shared')):
    env_par, poses, acts = batch(B, A)
    scs = Scanners(assets)
    noise = oracle.noise_table(12345, T + 4)
    h = {}
    if 'own' in which:
        h['own'] = oracle_history(lambda e: scs.of(env_par[e]), env_par, poses, acts, T, A, noise)
    if 'shared' in which:
        h['shared'] = oracle_history(lambda e: scs.of(env_par[0]), env_par, poses, acts, T, A, noise)
    return env_par, poses, acts, h


def _slot_tables(eng, env_par):
    """[slots, num_beams] side tables in the engine's slot order, built like Engine does"""
    from red_gym_amd.engine import beam_tables
    assign = eng.env_params_assign
    first = {int(s): int(np.argmax(assign == s)) for s in np.unique(assign)}
    return np.stack([beam_tables(eng.num_beams, eng.fov, env_par[first[s]])[2] for s in range(len(first))]), first


@pytest.mark.parametrize('A', [1, 2])
def test_every_env_is_the_reference_env_built_from_its_own_params(assets, A):
    """12 envs on three vehicles (default, larger, smaller), autoreset, six envs driven into the wall, 90 steps: env e `==`
    the oracle env whose scanner was built from env e's params.  The scenario can tell the two semantics apart: for an env of
    each non-default vehicle the oracle history on env 0's scanner differs in `collisions` / `done`."""
    B, T = 12, 90
    env_par, poses, acts, h = _histories(assets, B, A, T)
    for v in (1, 2):
        assert any(differs(h['own'][e], h['shared'][e]) is not None for e in range(B) if e % 3 == v), v
    env = _env(assets, B, A, env_par, 'per_env')
    from red_gym_amd.engine import beam_tables
    for e in range(B):
        assert np.array_equal(env.eng.side_distances_of(e), beam_tables(1080, 2 * np.pi, env_par[e])[2])
    _compare(env, h['own'], poses, acts, T, tag='per_env')
    assert sum(int(h['own'][e]['done'].any()) for e in range(B)) >= 4
    env.close()


@pytest.mark.parametrize('A', [1, 2])
def test_shared_mode_is_env_0s_table_for_every_env(assets, A):
    """The default: the same batch `==` oracle envs that all hold env 0's scanner; no table is installed (the launch epoch is
    that of a handle built without the keyword) and side_distances_of answers env 0's table for every env.  A single params
    dict with 'per_env' is the same thing."""
    from red_gym_amd import F110VecEnv
    from red_gym_amd.engine import beam_tables
    B, T = 12, 90
    env_par, poses, acts, h = _histories(assets, B, A, T, which=('shared',))
    env = _env(assets, B, A, env_par, 'shared')
    plain = F110VecEnv(B, map=os.path.join(assets, 'example_map'), num_agents=A, params=env_par, autoreset=True, keep_f64_scans=True)
    assert env.eng.launch_epoch() == plain.eng.launch_epoch() and env.eng._side_slots is None
    plain.close()
    t0 = beam_tables(1080, 2 * np.pi, env_par[0])[2]
    assert all(np.array_equal(env.eng.side_distances_of(e), t0) for e in range(B))
    _compare(env, h['shared'], poses, acts, T, tag='shared')
    env.close()
    one = _env(assets, 2, 1, VEHICLES[1], 'per_env')
    assert one.eng._side_slots is None
    assert np.array_equal(one.eng.side_distances_of(1), beam_tables(1080, 2 * np.pi, VEHICLES[1])[2])
    one.close()
    with pytest.raises(ValueError):
        _env(assets, 2, 1, VEHICLES[1], 'per_car')


def test_check_ttc_slots_row_by_row(assets):
    """f110_check_ttc_slots on 24 000 rows `==` oracle.Scanner(params=p).check_ttc: scan rows of stepped envs, shifted so that
    one beam lies within thresh*|vel| of its side distance in the row's slot (or just outside), velocities of both signs
    and zero, slots at random.  At least 10 % of the rows hit, and at least 10 % of the hits are misses under another
    slot's table.  Then custom tables with negative, inf and NaN entries against orc_check_ttc holding the same rows."""
    import torch
    B, A, n = 12, 1, 24000
    env_par, poses, acts = batch(B, A)
    env = _env(assets, B, A, env_par, 'per_env')
    eng = env.eng
    env.reset(poses)
    rows = []
    for k in range(40):
        obs = env.step(torch.as_tensor(acts[k % 8], device='cuda'))[0]
        rows.append(_np(obs['scans_f64']).reshape(-1, 1080))
    rows = np.concatenate(rows)
    tables, first = _slot_tables(eng, env_par)
    S = tables.shape[0]
    scs = [oracle.Scanner(1080, 2 * np.pi, params=env_par[first[s]]) for s in range(S)]
    rng = np.random.default_rng(7)
    pick, slot, beam = rng.integers(0, rows.shape[0], n), rng.integers(0, S, n), rng.integers(0, 1080, n)
    vel = rng.uniform(-8., 8., n)
    vel[rng.random(n) < 0.1] = 0.
    u = rng.uniform(-1., 2., n)              # the chosen beam's ttc = u * thresh: a hit for u in [0, 1)
    thresh = 0.005
    scans = rows[pick]
    proj = vel * scs[0].beam_cosines[beam]
    scans = scans - (scans[np.arange(n), beam] - tables[slot, beam])[:, None] + (u * thresh * proj)[:, None]
    got = _np(eng.check_ttc_slots(scans, vel, slot)).astype(bool)
    want = np.array([scs[slot[r]].check_ttc(scans[r], vel[r]) for r in range(n)])
    other = np.array([scs[(slot[r] + 1) % S].check_ttc(scans[r], vel[r]) for r in range(n)])
    hits, flips = int(want.sum()), int((want & ~other).sum())
    print('rows %d hits %d (%.1f %%), hits that miss under another slot %d (%.1f %%)' % (n, hits, 100. * hits / n, flips, 100. * flips / max(hits, 1)))
    assert np.array_equal(got, want), int((got != want).sum())
    assert hits >= 0.1 * n and flips >= 0.1 * hits
    assert np.array_equal(_np(eng.check_ttc_slots(scans, vel, (slot + 1) % S)).astype(bool), other)
    # custom tables: negative, infinite and NaN entries, per slot
    custom = tables.copy()
    custom[0, ::7] = -custom[0, ::7]
    custom[1, 3::11] = np.inf
    custom[1, 5::13] = -np.inf
    custom[2, 2::5] = np.nan
    custom[2, ::9] *= -0.5
    eng.set_side_distance_slots(custom)
    for s in range(S):
        scs[s].side_distances[:] = custom[s]
    got = _np(eng.check_ttc_slots(scans, vel, slot)).astype(bool)
    want2 = np.array([scs[slot[r]].check_ttc(scans[r], vel[r]) for r in range(n)])
    assert np.array_equal(got, want2) and want2.sum() > 0 and (want2 != want).any()
    assert eng.device_errors() == 0
    eng.set_side_distance_slots(None)
    with pytest.raises(ValueError):
        eng.check_ttc_slots(scans[:4], vel[:4], slot[:4])          # no tables installed
    env.close()


def test_every_env_its_own_outline_at_batch_scale(assets):
    """4 096 envs, 4 096 distinct vehicles (dynamics AND width / lf / lr / length drawn), 'per_env': 72 sampled envs -- the
    ones driven into the wall among them -- `==` their own oracle envs, 70 steps; sampled envs do hit walls."""
    from red_gym_amd.engine import DEFAULT_PARAMS
    from red_gym_amd import workload
    B, A, T = 4096, 1, 70
    rng = np.random.default_rng(99)
    pars = []
    for e in range(B):
        p = dict(DEFAULT_PARAMS)
        lf, lr = float(rng.uniform(0.09, 0.27)), float(rng.uniform(0.10, 0.29))
        p.update(mu=float(rng.uniform(0.6, 1.3)), C_Sf=float(rng.uniform(3.5, 5.5)), C_Sr=float(rng.uniform(4.0, 6.0)),
                 m=float(rng.uniform(3.0, 4.5)), I=float(rng.uniform(0.035, 0.06)), a_max=float(rng.uniform(6.0, 10.0)),
                 width=float(rng.uniform(0.2, 0.48)), lf=lf, lr=lr, length=float((lf + lr) * rng.uniform(1.5, 1.8)))
        pars.append(p)
    pars[0] = dict(DEFAULT_PARAMS)
    poses = workload.spawn_poses(B, A)
    acts = workload.action_pool(8, B, A)
    wall = np.arange(100, 600)
    poses[wall, :, 2] += np.linspace(0.9, 1.4, wall.size)[:, None]
    acts[:, wall, :, 0] = 0.05
    acts[:, wall, :, 1] = 7.0
    sample = sorted(set([0, 1, 63, 64, 65, 1000, 2047, 2048, 3000, 4095] + list(range(100, 600, 8))))
    assert len(sample) >= 64
    scs = Scanners(assets)
    noise = oracle.noise_table(12345, T + 4)
    hist = oracle_history(lambda e: scs.of(pars[e]), pars, poses, acts, T, A, noise, envs=sample)
    assert sum(int(hist[e]['done'].any()) for e in sample) >= 20
    env = _env(assets, B, A, pars, 'per_env')
    assert env.eng._side_slots.shape == (B, 1080)
    _compare(env, hist, poses, acts, T, envs=sample, tag='4096')
    env.close()


def test_slot_count_invariant_extension_and_removal(assets):
    """No call leaves an env on a params slot without a side table: a table count other than the slot count is refused,
    f110_set_params_slots with another count is refused while tables are installed (neither moves the epoch nor changes what
    the next steps compute), f110_set_params_slot beyond the count extends the tables with slot 0's, removal restores the
    shared table."""
    import torch
    from red_gym_amd import _lib
    from red_gym_amd.engine import _np_ptr, params_vec
    B, A, T = 12, 1, 60
    env_par, poses, acts, h = _histories(assets, B, A, T)
    env = _env(assets, B, A, env_par, 'per_env')
    eng = env.eng
    tables, _ = _slot_tables(eng, env_par)
    ep = eng.launch_epoch()
    with torch.cuda.device(eng.device):
        assert eng.lib.f110_set_side_distance_slots(eng._h, _np_ptr(tables), 2) == _lib.E_INVALID
        assert eng.lib.f110_set_side_distance_slots(eng._h, _np_ptr(tables), -1) == _lib.E_INVALID
        two = np.ascontiguousarray(np.stack([params_vec(VEHICLES[0]), params_vec(VEHICLES[1])]))
        assert eng.lib.f110_set_params_slots(eng._h, _np_ptr(two), 2) == _lib.E_INVALID
        assert b'side' in eng.lib.f110_last_error()
    assert eng.launch_epoch() == ep
    _compare(env, h['own'], poses, acts, T, tag='after refusals')
    # extension: slot 3 = the larger vehicle's params with a copy of slot 0's side table; the two wall envs of the larger
    # vehicle move there -> they behave as under the shared table, every other env as before
    big = int(eng.env_params_assign[1])
    assign = eng.env_params_assign.copy()
    moved = [e for e in range(B) if assign[e] == big and 3 <= e < 9]
    assign[moved] = 3
    pv = params_vec(VEHICLES[1])
    with torch.cuda.device(eng.device):
        _lib.check(eng.lib.f110_set_params_slot(eng._h, 3, _np_ptr(pv), -1))
        assert eng.launch_epoch() > ep
        _lib.check(eng.lib.f110_assign_params(eng._h, _np_ptr(np.ascontiguousarray(assign, dtype=np.int32))))
    mixed = {e: (h['shared'][e] if e in moved else h['own'][e]) for e in range(B)}
    assert any(differs(h['own'][e], h['shared'][e]) is not None for e in moved)
    _compare(env, mixed, poses, acts, T, tag='extended')
    # the tables now count 4: three are refused, four accepted
    with torch.cuda.device(eng.device):
        assert eng.lib.f110_set_side_distance_slots(eng._h, _np_ptr(tables), 3) == _lib.E_INVALID
    # removal: back on the handle's one table (env 0's)
    ep = eng.launch_epoch()
    eng.set_side_distance_slots(None)
    assert eng.launch_epoch() > ep
    _compare(env, h['shared'], poses, acts, T, tag='removed')
    ep = eng.launch_epoch()
    eng.set_side_distance_slots(None)                 # nothing installed: nothing changes
    assert eng.launch_epoch() == ep
    env.close()


@pytest.mark.parametrize('how', ['torch', 'nodes'])
def test_graphs_captured_before_an_install_recapture(assets, how):
    """A torch-captured step and a library graph, built while the handle is on the shared table, notice the install (launch
    epoch), re-capture by themselves and then `==` the oracle envs on their own tables."""
    B, A, T = 12, 1, 60
    env_par, poses, acts, h = _histories(assets, B, A, T)
    env = _env(assets, B, A, env_par, 'shared')
    if how == 'torch':
        env.capture_step()
        step = env.step_graph
    else:
        env.build_step_graph('nodes')
        step = env.step_lib_graph
    _compare(env, h['shared'], poses, acts, 12, step=step, tag='before install')
    ep = env.eng.launch_epoch()
    env.eng.set_side_distance_slots(_slot_tables(env.eng, env_par)[0])
    assert env.eng.launch_epoch() > ep
    _compare(env, h['own'], poses, acts, T, step=step, tag='after install')
    env.close()


def test_update_params_changes_dynamics_not_side_tables(assets):
    """update_params replaces every car's RaceCar.params (base_classes.py:158-169) and nothing else: afterwards all envs
    drive the new dynamics, each still with the side table of the vehicle it was constructed with."""
    B, A, T = 12, 1, 60
    env_par, poses, acts = batch(B, A)
    env = _env(assets, B, A, env_par, 'per_env')
    before = [env.eng.side_distances_of(e).copy() for e in range(B)]
    ep = env.eng.launch_epoch()
    new = dict(VEHICLES[0], mu=0.8, m=4.2, a_max=8.0, width=0.6, lf=0.3, lr=0.3, length=1.0)
    env.update_params(new)
    assert all(np.array_equal(env.eng.side_distances_of(e), before[e]) for e in range(B))
    assert env.eng.launch_epoch() == ep
    scs = Scanners(assets)
    noise = oracle.noise_table(12345, T + 4)
    hist = oracle_history(lambda e: scs.of(env_par[e]), [new] * B, poses, acts, T, A, noise)
    old = oracle_history(lambda e: scs.of(env_par[e]), env_par, poses, acts, T, A, noise, envs=[0])
    assert not np.allclose(hist[0]['state'], old[0]['state'], rtol=0, atol=1e-6)      # the dynamics did change
    _compare(env, hist, poses, acts, T, tag='update_params')
    env.close()


def _berlin_batch(B):
    env_par = [VEHICLES[e % 3] for e in range(B)]
    poses = np.zeros((B, 1, 3))
    poses[:, 0, 0] = np.linspace(-1., 1., B)
    poses[:, 0, 1] = 0.3 * np.sin(np.arange(B))
    poses[:, 0, 2] = 0.1 * (np.arange(B) % 5 - 2)
    side = np.array([1, -1, 1, -1, 1, -1])
    poses[3:9, 0, 2] = np.linspace(0.9, 1.4, 6) * side       # turned towards the nearer wall of the corridor ...
    poses[3:9, 0, 1] = 0.9 * side                            # ... from about a metre in front of it
    from red_gym_amd import workload
    acts = workload.action_pool(8, B, 1)
    acts[:, 3:9, :, 0] = 0.0
    acts[:, 3:9, :, 1] = 7.0
    return env_par, poses, acts


@pytest.mark.parametrize('shape', ['berlin', 'map_per_env', 'scan_order', 'four_waves_per_car'])
def test_other_launch_shapes(assets, shape):
    """The per-slot read in every scan instantiation a step can launch: a 0.05 m map, a map per env (one-wave workgroups),
    a non-trivial launch order, several waves per car -- each `==` the oracle envs on their own tables."""
    import torch
    from red_gym_amd import _lib
    from red_gym_amd.engine import _np_ptr
    B, A, T = 12, 1, 60
    if shape == 'berlin':
        env_par, poses, acts = _berlin_batch(B)
        yaml_path = os.path.join(assets, 'maps', 'berlin.yaml')
        scs = Scanners(assets, yaml_path=yaml_path)
        noise = oracle.noise_table(12345, T + 4)
        own = oracle_history(lambda e: scs.of(env_par[e]), env_par, poses, acts, T, A, noise)
        shared = oracle_history(lambda e: scs.of(env_par[0]), env_par, poses, acts, T, A, noise)
        assert any(differs(own[e], shared[e]) is not None for e in range(B))
        env = _env(assets, B, A, env_par, 'per_env', map_name='berlin')
    else:
        env_par, poses, acts, h = _histories(assets, B, A, T, which=('own',))
        own = h['own']
        env = _env(assets, B, A, env_par, 'per_env')
    eng = env.eng
    keep = None
    if shape == 'map_per_env':
        m = eng.map
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_set_map_slot_occupancy(eng._h, 1, _np_ptr(m.free), m.height, m.width, m.resolution,
                                                           m.orig_x, m.orig_y, m.orig_c, m.orig_s))
        eng.assign_maps(np.arange(B) % 2)            # neighbouring cars on different slots: one wave per workgroup
    elif shape == 'scan_order':
        keep = torch.as_tensor(np.roll(np.arange(B, dtype=np.int32)[::-1], 5).copy(), device='cuda')   # a permutation of the cars
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_set_scan_order(eng._h, C.c_void_p(keep.data_ptr())))
    elif shape == 'four_waves_per_car':
        eng.set_scan_stages('*:2')
    _compare(env, own, poses, acts, T, tag=shape)
    env.close()


def test_plain_store_instantiation(assets, tmp_path):
    """scan_kernel<.., 2> (F110_SCAN_STORES=plain, read once per process: a child process) with per-vehicle tables `==` the
    oracle envs on their own tables."""
    B, A, T = 12, 1, 60
    env_par, poses, acts, h = _histories(assets, B, A, T, which=('own',))
    out = str(tmp_path / 'plain.npz')
    script = (
        "import sys, os, numpy as np, torch\n"
        "sys.path[:0] = [%r, %r]\n"
        "from side_distance_cases import batch\n"
        "from red_gym_amd import F110VecEnv\n"
        "B, A, T = 12, 1, 60\n"
        "env_par, poses, acts = batch(B, A)\n"
        "env = F110VecEnv(B, map=%r, num_agents=A, params=env_par, autoreset=True, keep_f64_scans=True, side_distances='per_env')\n"
        "env.reset(poses)\n"
        "st, sc, col, dn = [], [], [], []\n"
        "for k in range(T):\n"
        "    obs, _, done, info = env.step(torch.as_tensor(acts[k %% 8], device='cuda'))\n"
        "    st.append(env.state.cpu().numpy().copy()); sc.append(obs['scans_f64'].cpu().numpy().copy())\n"
        "    col.append(obs['collisions'].cpu().numpy().copy()); dn.append(done.cpu().numpy().copy())\n"
        "err = env.eng.device_errors()\n"
        "np.savez(sys.argv[1], st=np.stack(st), sc=np.stack(sc), col=np.stack(col), dn=np.stack(dn), err=err)\n"
        "env.close()\n" % (os.path.dirname(TESTS), TESTS, os.path.join(assets, 'example_map')))
    r = subprocess.run([sys.executable, '-c', script, out], env=dict(os.environ, F110_SCAN_STORES='plain'), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    g = np.load(out)
    assert int(g['err']) == 0
    for e in range(B):
        o = h['own'][e]
        assert np.array_equal(g['col'][:, e].astype(np.float64), o['collisions']), e
        assert np.array_equal(g['dn'][:, e].astype(bool), o['done'].astype(bool)), e
        assert np.allclose(g['st'][:, e], o['state'], rtol=0, atol=1e-9), e
        assert np.allclose(g['sc'][:, e], o['scans'], rtol=0, atol=1e-9), e
