"""Path follower on the GPU (csrc/f110_pathfollow.h) against the reference's recorded results (g17) and the NumPy checker of
tests/path_cases.py: integers `==`, everything else within 1e-9 * max(1, |value|) (device sin / cos /
atan2 and another order of operations enter); the QP against the enumerator's optimum, |u - u*| <= 1e-9."""
import os

import numpy as np
import pytest

import path_cases as pc

pytestmark = pytest.mark.gpu

SPLITS = (1, 63, 65, 130)
WORST = {}


def _env(assets, B, A=1, **kw):
    from red_gym_amd import F110VecEnv
    return F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=A, timestep=0.015, **kw)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _close(what, got, want, rel=1e-9):
    ok, worst = pc.close(got, want, rel)
    WORST[what] = max(WORST.get(what, 0.0), worst)
    print('%-28s largest |got - want| / max(1, |want|) = %.3g' % (what, worst))
    assert ok, (what, worst)


def _chunks(n):
    """Consecutive chunks of 1, 63, 65, 130, 1, ... cases: lanes idle either side of a wave boundary (two lanes per case)."""
    lo, k = 0, 0
    while lo < n:
        hi = min(n, lo + SPLITS[k % len(SPLITS)])
        yield slice(lo, hi)
        lo, k = hi, k + 1


def _built_cases(g, n, seed):
    """Cases built to make some, all or no bounds bind: g17's paths with a velocity around the first reference state's."""
    rng = np.random.default_rng(seed)
    paths = g['paths'][:n]
    _, ref = pc.reference_states(paths)
    vels = ref[:, 0, 2:4] + rng.normal(0.0, 1.0, (n, 2)) * rng.choice([0.02, 0.3, 0.5, 0.8], (n, 1))
    return paths, vels


def test_g17_through_the_function_level_entries(golden):
    from red_gym_amd import pathfollow
    g = golden('g17_paths.npz')
    n = g['raw'].shape[0]
    paths, dists, ref, acts, idx = (np.zeros_like(g[k]) for k in ('paths', 'dists', 'ref_traj', 'vels', 'index_out'))
    for m in _chunks(n):
        paths[m] = pathfollow.decode_paths(_dev(g['raw'][m]), _dev(g['poses'][m])).cpu().numpy()
        out = pathfollow.mpc_controls(_dev(g['paths'][m]), _dev(g['vels'][m]), horizon=8)       # ref_traj's nine recorded rows
        dists[m], ref[m] = out['dists'].cpu().numpy(), out['ref_traj'].cpu().numpy()
        out = pathfollow.mpc_controls(_dev(g['paths'][m]), _dev(g['vels'][m]))
        acts[m] = out['actions'].cpu().numpy()
        assert out['errors'] == 0
        idx[m] = pathfollow.advance_index(_dev(g['paths'][m]), _dev(g['index'][m]), _dev(g['xy'][m])).cpu().numpy()
    assert np.array_equal(idx, g['index_out'])
    _close('g17 paths', paths, g['paths'])
    _close('g17 dists', dists, g['dists'])
    _close('g17 ref_traj', ref, g['ref_traj'])
    _close('g17 (steer, speed)', acts, g['conv_out'][:n])     # the reference's converter on the enumerator's optimum of the case
    path = os.environ.get('F110_PATHFOLLOW_REPORT')
    if path:
        with open(path, 'w') as f:
            f.writelines('%-28s %.3g\n' % kv for kv in sorted(WORST.items()))


@pytest.mark.parametrize('cfg', pc.QP_CONFIGS)              # every horizon 1..8; the first four are the first tests' own
def test_qp_equals_the_enumerators_optimum(golden, cfg):
    from red_gym_amd import pathfollow
    g = golden('g17_paths.npz')
    c = pc.config(**cfg)
    H = c['horizon']
    n17, nb = (780, 600) if H <= 5 else (40, 40)               # (3^8 patterns per axis: fewer cases)
    bp, bv = _built_cases(g, nb, 1710 + H)
    paths, vels = np.concatenate([g['paths'][:n17], bp]), np.concatenate([g['vels'][:n17], bv])
    want, active, _, ref = pc.mpc_accel(paths, vels, c)
    # coverage, on the enumerator's results: per axis no bound active / some but not all / all H
    none, some, every = (active == 0).mean(), ((active > 0) & (active < H)).mean(), (active == H).mean()
    print('H = %d, %d cases: no bound active %.1f %%, some %.1f %%, all %.1f %%' % (H, paths.shape[0], 100 * none, 100 * some, 100 * every))
    if not cfg:
        assert none >= 0.20 and some >= 0.20 and every >= 0.05
    else:
        assert none > 0 and every > 0 and (some > 0 or H == 1)
    got, steps = np.zeros_like(want), np.zeros(want.shape, dtype=np.int32)
    for m in _chunks(paths.shape[0]):
        out = pathfollow.mpc_controls(_dev(paths[m]), _dev(vels[m]), **cfg)
        got[m], steps[m] = out['accel'].cpu().numpy(), out['qp_steps'].cpu().numpy()
        assert out['errors'] == 0
    print('active-set walk: at most %d steps, %.2f on average' % (steps.max(), steps.mean()))
    err = np.abs(got - want).max()
    WORST['qp H=%d' % H] = err
    print('largest |u - u*| = %.3g' % err)
    assert err <= 1e-9
    assert steps.min() >= 1 and steps.max() <= 4 * H + 2
    # the device's own answer against the KKT conditions of the first variable's QP needs the whole u: the walk's u_0 with the
    # enumerator's u_1.. is THE optimum iff u_0 is, so the check is made on the full vector rebuilt with u_0 = the device's
    for axis in range(2):
        Hm, f = pc.qp_terms(ref, paths[:, 0, axis], vels[:, axis], axis, c)
        u, _, _ = pc.solve_box_qp(Hm, f)
        u[:, 0] = got[:, axis]
        assert (np.abs(u) <= 1.0).all()
        assert (pc.kkt_violation(Hm, f, u) <= 1e-9 * np.maximum(1.0, np.abs(f).max(axis=1))).all()


def _snapshot(env):
    import torch
    b = env.eng.follower.buf
    torch.cuda.synchronize()
    return {k: b[k].cpu().numpy().copy() for k in ('path_points', 'path_index', 'path_replanned', 'mpc_accel')}


# the third: short chords and a fast reference, so that the end clamp and the late spline pieces run through act (has_vy = 0, the
# engine's strides)
@pytest.mark.parametrize('B,A,agent,cfg,steps', [(65, 1, 0, dict(dist_threshold=1.29, replan_at=2), 70), (33, 2, 1, dict(), 30),
                                                 (33, 1, 0, dict(vector_length=0.25, desired_velocity=4.7, horizon=8, replan_at=3, dist_threshold=1.29), 20)])
def test_closed_loop_equals_checker_through_resets(assets, B, A, agent, cfg, steps):
    """Seeded raw actions that change every step; the checker is fed the device's poses and velocities step by step.  A quarter
    of the envs of the first configuration is spawned across the track and driven at the wall (the follower's action is
    computed and checked, then overridden) so that autoresets happen; a masked reset of half the envs mid-way."""
    import torch
    from red_gym_amd import workload
    env = _env(assets, B, A, autoreset=True)
    env.follow_paths(agent=agent, **cfg)
    ck = pc.FollowChecker(B, env.timestep, agent=agent, **cfg)
    spawn = workload.spawn_poses(B, A)
    crash = (np.arange(B) % 4 == 1) & (A == 1)
    spawn[crash, 0, 2] += np.pi / 2
    crash_dev = torch.as_tensor(crash, device=env.device)
    rng = np.random.default_rng(1720 + B)
    _, _, _, info = env.reset(spawn)
    assert set(env.eng.follower.INFO) <= set(info) and info['path_points'].shape == (B, 8, 2)
    ck.update(env.state[:, agent, :2].cpu().numpy(), info['current_time'].cpu().numpy())
    assert (info['path_index'].cpu().numpy() == -1).all()
    resets, pending = 0, np.zeros(B, dtype=bool)
    sentinel = 7.5
    for k in range(steps):
        if k == steps // 2:
            mask = (np.arange(B) % 2 == 0).astype(np.uint8)
            _, _, _, info = env.reset(spawn, torch.as_tensor(mask))
        else:
            raw = rng.uniform(-1.0, 1.0, (B, 16))
            st = env.state[:, agent].cpu().numpy()
            want_act, want_acc, want_rep = ck.act(raw, st[:, [0, 1, 4]], st[:, 3])
            out = torch.full((B, A, 2), sentinel, dtype=torch.float64, device=env.device)
            acts = env.path_actions(_dev(raw), out=out)
            got = _snapshot(env)
            assert np.array_equal(got['path_replanned'], want_rep) and np.array_equal(got['path_index'], ck.index), k
            assert want_rep[pending].all(), 'a reset env did not replan at its next act'
            pending[:] = False
            _close('loop paths', got['path_points'], ck.paths)
            _close('loop mpc_accel', got['mpc_accel'], want_acc)
            _close('loop (steer, speed)', acts[:, agent].cpu().numpy(), want_act)
            assert (acts.cpu().numpy()[:, [a for a in range(A) if a != agent]] == sentinel).all()
            assert np.abs(want_act[:, 1]).max() <= 1.0
            acts = torch.where(acts == sentinel, 0.0, acts)
            acts[:, 0, 0] = torch.where(crash_dev, 0.0, acts[:, 0, 0])
            acts[:, 0, 1] = torch.where(crash_dev, 8.0, acts[:, 0, 1])
            _, _, _, info = env.step(acts)
        clock = info['current_time'].cpu().numpy()
        was_reset = ck.update(env.state[:, agent, :2].cpu().numpy(), clock)
        assert np.array_equal(info['path_index'].cpu().numpy(), ck.index), k
        assert (ck.index[was_reset] == -1).all()
        pending |= was_reset
        if k != steps // 2:
            resets += int(was_reset.sum())
    print('autoresets: %d; envs that advanced: %d of %d; envs that replanned after their first path: %d'
          % (resets, (ck.advances > 0).sum(), B, (ck.reached > 0).sum()))
    if cfg:
        assert resets > 0, 'no autoreset happened'
        assert (ck.advances > 0).mean() >= 0.5
        assert (ck.reached > 0).mean() >= 0.25                 # replans because the index reached replan_at, not because of a reset
    assert env.eng.device_errors() == 0
    env.close()


def _run(env, how, pool, raw, sd, lo, hi):
    import torch
    env.load_state_dict(sd)
    outs = []
    for k in range(lo, hi):
        raw.copy_(pool[k])
        if how == 'eager':
            env.step(env.path_actions(raw))
        elif how == 'graph':
            env.step_graph()
        else:
            env.path_actions(raw, out=env._g_actions)
            env.step_lib_graph()
        b = env.eng.follower.buf
        o = {key: b[key].clone() for key in ('path_points', 'path_index', 'path_replanned', 'mpc_accel')}
        o['state'] = env.state.clone()
        outs.append(o)
    torch.cuda.synchronize()
    return outs


def _equal_runs(a, b, what):
    import torch
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for key in x:
            assert torch.equal(x[key], y[key]), (what, k, key)


def test_graphs_and_checkpoint_equal_eager(assets):
    """The same run through step, step_graph (the follower as the captured policy) and step_lib_graph (the follower in front of
    the library's graph) gives `==` tensors; a state_dict round trip mid-run continues `==`."""
    import torch
    from red_gym_amd import workload
    B, A = 64, 1
    env = _env(assets, B, A, autoreset=True)
    env.follow_paths(dist_threshold=1.29, replan_at=2)
    env.reset(workload.spawn_poses(B, A))
    rng = np.random.default_rng(1730)
    pool = _dev(rng.uniform(-1.0, 1.0, (24, B, 16)))
    raw = torch.zeros((B, 16), dtype=torch.float64, device=env.device)
    for k in range(4):
        env.step(env.path_actions(pool[k]))
    sd = env.state_dict()
    assert {'path_points', 'path_index', 'path_t_seen'} <= set(sd)
    eager = _run(env, 'eager', pool, raw, sd, 4, 24)
    assert int(sum(o['path_replanned'].sum() for o in eager)) > 0 and int(eager[-1]['path_index'].max()) >= 1
    env.capture_step(policy=lambda e, out: e.path_actions(raw, out=out))
    _equal_runs(eager, _run(env, 'graph', pool, raw, sd, 4, 24), 'step_graph')
    env.build_step_graph()
    _equal_runs(eager, _run(env, 'lib', pool, raw, sd, 4, 24), 'step_lib_graph')
    first = _run(env, 'eager', pool, raw, sd, 4, 14)
    mid = env.state_dict()
    rest = _run(env, 'eager', pool, raw, mid, 14, 24)
    _equal_runs(eager, first + rest, 'uninterrupted')
    _equal_runs(rest, _run(env, 'eager', pool, raw, mid, 14, 24), 'resumed')
    # a checkpoint taken without the follower's state restarts it: every env decodes a new path
    plain = {k: v for k, v in mid.items() if k not in ('path_points', 'path_index', 'path_t_seen')}
    o = _run(env, 'eager', pool, raw, plain, 14, 15)[0]
    assert bool(o['path_replanned'].all())
    assert env.eng.device_errors() == 0
    env.close()


def test_switching_off_removes_everything_and_the_step_is_unchanged(assets):
    import torch
    from red_gym_amd import workload
    B, A = 32, 2
    pool = workload.action_pool(12, B, A)
    raw = _dev(np.random.default_rng(1740).uniform(-1.0, 1.0, (B, 16)))
    runs = []
    for on in (False, True):
        env = _env(assets, B, A, autoreset=True)
        if on:
            env.follow_paths(agent=1)
            env.follow_paths(False)
        res = [env.reset(workload.spawn_poses(B, A))] + [env.step(pool[k]) for k in range(12)]
        obs, reward, done, info = res[-1]
        torch.cuda.synchronize()
        snap = {'done': done.clone(), 'reward': reward.clone(), **{'obs_' + k: v.clone() for k, v in obs.items() if torch.is_tensor(v)},
                **{'info_' + k: v.clone() for k, v in info.items() if torch.is_tensor(v)}}
        runs.append((snap, set(info), set(env.state_dict())))
        if on:
            env.follow_paths(agent=1)
            info = env.step(env.path_actions(raw))[3]
            assert set(info) - runs[0][1] == {'path_points', 'path_index', 'path_replanned', 'mpc_accel'}
            assert set(env.state_dict()) - runs[0][2] == {'path_points', 'path_index', 'path_t_seen'}
            env.follow_paths(False)
            assert set(env.step(pool[0])[3]) == runs[0][1] and set(env.state_dict()) == runs[0][2]
            with pytest.raises(ValueError):
                env.eng.follower.kernel()                           # F110_E_INVALID: no follower
            with pytest.raises(ValueError):
                env.path_actions(raw)
        assert env.eng.device_errors() == 0
        env.close()
    (off, keys_off, sd_off), (on_, keys_on, sd_on) = runs
    assert keys_on == keys_off and sd_on == sd_off and not {'path_points', 'path_index'} & keys_off
    for k in off:
        assert torch.equal(off[k], on_[k]), k
    # nothing is allocated before the first install
    env = _env(assets, 4, 1)
    assert env.eng.follower.buf is None and not env.eng.follower.on
    env.close()


def test_indices_stay_in_bounds(assets, golden):
    """Every index the new kernels form from data -- the waypoint index, the free set of the QP's table, the spline piece -- is
    checked in the bounds-checked build of the library (-DF110_BOUNDS, tests/test_gpu_bounds.py): the device error word stays
    clean over a closed loop with resets, and indices outside 0..7 given to the advance entry are copied, not used."""
    import torch
    from red_gym_amd import pathfollow, workload
    g = golden('g17_paths.npz')
    idx = np.array([-1, 0, 7, 8, 100, -2147483648, 2147483647, 3], dtype=np.int32)
    xy = g['paths'][:8, 3]
    new = pathfollow.advance_index(_dev(g['paths'][:8]), _dev(idx), _dev(xy)).cpu().numpy()
    assert new.tolist() == [-1, 0, 7, 8, 100, -2147483648, 2147483647, 4]
    B = 65
    env = _env(assets, B, 2, autoreset=True)
    env.follow_paths(agent=1, dist_threshold=1.29, replan_at=3, horizon=8)
    env.reset(workload.spawn_poses(B, 2))
    rng = np.random.default_rng(1750)
    for k in range(12):
        if k == 6:
            env.reset(workload.spawn_poses(B, 2), torch.as_tensor((np.arange(B) % 3 == 0).astype(np.uint8)))
        env.step(env.path_actions(_dev(rng.uniform(-1.0, 1.0, (B, 16)))))
    i = env.eng.follower.buf['path_index']
    assert int(i.min()) >= -1 and int(i.max()) <= 3
    assert env.eng.device_errors() == 0
    env.close()


# ---------------------------------------------------------------- off the defaults (tests/path_cases.py: CONFIGS and the case families)
def _mpc(paths, vels, **cfg):
    """mpc_controls in the chunks of _chunks: dict of NumPy arrays, `errors` or-ed."""
    from red_gym_amd import pathfollow
    H = pc.config(**cfg)['horizon']
    n = paths.shape[0]
    out = dict(dists=np.zeros((n, 8)), ref_traj=np.zeros((n, H + 1, 4)), accel=np.zeros((n, 2)), actions=np.zeros((n, 2)),
               qp_steps=np.zeros((n, 2), dtype=np.int32), errors=0)
    for m in _chunks(n):
        o = pathfollow.mpc_controls(_dev(paths[m]), _dev(vels[m]), **cfg)
        for k in out:
            if k == 'errors':
                out[k] |= o[k]
            else:
                out[k][m] = o[k].cpu().numpy()
    return out


def _decode(raw, poses, **cfg):
    from red_gym_amd import pathfollow
    out = np.zeros((raw.shape[0], 8, 2))
    for m in _chunks(raw.shape[0]):
        out[m] = pathfollow.decode_paths(_dev(raw[m]), _dev(poses[m]), **cfg).cpu().numpy()
    return out


@pytest.mark.parametrize('name', list(pc.CONFIGS))
def test_g19_through_the_function_level_entries(golden, name):
    g = golden('g19_path_configs.npz')
    cfg = pc.CONFIGS[name]['cfg']
    raw, poses, vels = pc.g19_inputs(name)
    rec = {k: g['%s/%s' % (name, k)] for k in ('paths', 'dists', 'ref_traj', 'conv_out')}
    _close(name + ' paths', _decode(raw, poses, **cfg), rec['paths'])
    out = _mpc(rec['paths'], vels, **cfg)
    assert out['errors'] == 0
    _close(name + ' dists', out['dists'], rec['dists'])
    _close(name + ' ref_traj', out['ref_traj'], rec['ref_traj'])
    _close(name + ' (steer, speed)', out['actions'], rec['conv_out'])


def _same_steps(what, steps, info):
    """Where the transcribed walk's step counts do not hang on rounding (path_cases.step_stable) the device takes as many steps:
    the same faces in the same order.  (u is never compared with the transcription, only with the enumerator.)"""
    m = info['stable']
    print('%s: %d of %d walks step-stable; device steps == transcription on %d of them' % (what, m.sum(), m.size, (steps[m] == info['steps'][m]).sum()))
    assert np.array_equal(steps[m], info['steps'][m])


@pytest.mark.parametrize('name', ['bound2', 'bound5', 'bound8'])
def test_optimum_on_the_edge_of_a_bound(name):
    """No cycling and no wrong face at the walk's tolerances: the unconstrained optimum or a multiplier within 0, 1e-13, 1e-11, 1e-8
    of a bound, either side."""
    f = pc.family(name)
    H = f['cfg']['horizon']
    out = _mpc(f['paths'], f['vels'], horizon=H)
    err = np.abs(out['accel'] - f['info']['u'][:, :, 0]).max()
    agree = (out['qp_steps'] == f['info']['steps']).mean()
    print('%s: %d cases, largest |u_0 - u*_0| = %.3g, steps <= %d (%.0f %% as the transcribed walk)' % (name, f['paths'].shape[0], err, out['qp_steps'].max(), 100 * agree))
    WORST[name] = err
    assert err <= 1e-9 and out['errors'] == 0
    assert out['qp_steps'].min() >= 1 and out['qp_steps'].max() <= 4 * H + 2
    _same_steps(name, out['qp_steps'], f['info'])


def test_weights_at_the_edge_of_validate():
    """r = 1e-6 with q = p = 0 (a diagonal Hessian) and r = 1e-6 with p = 1e4 at horizon 8 (condition ~ 1e9): the device is allowed
    max(1e-9, 16 * e_ref), e_ref the enumerator's own fp64-against-longdouble difference (tests/path_cases.py stiff_cases; 16 for
    the device's table inversion and order of sums).  `errors` is the whole device error word of the call: no step limit reached,
    and in the bounds-checked build no index reported."""
    dg = pc.family('diagonal')
    out = _mpc(dg['paths'], dg['vels'], **pc.EDGE_DIAGONAL)
    assert out['errors'] == 0 and np.array_equal(out['accel'], dg['info']['u'][:, :, 0]) and (out['qp_steps'] == 1).all()
    st = pc.family('stiff')
    out = _mpc(st['paths'], st['vels'], **pc.EDGE_STIFF)
    tol = max(1e-9, 16 * st['e_ref'])
    err = np.abs(out['accel'] - st['want']).max()
    print('stiff: e_ref %.3g, allowed %.3g, device %.3g; steps <= %d (transcribed walk <= %d)' % (st['e_ref'], tol, err, out['qp_steps'].max(), st['info']['steps'].max()))
    WORST['stiff'] = err
    assert out['errors'] == 0 and err <= tol
    assert out['qp_steps'].min() >= 1 and out['qp_steps'].max() <= 4 * 8 + 2
    _same_steps('stiff', out['qp_steps'], st['info'])
    # the order of the releases: cases on which releasing the first wrong-signed multiplier instead of the worst takes another
    # number of steps to the same optimum
    ro = pc.family('release_order')
    out = _mpc(ro['paths'], ro['vels'], **pc.EDGE_STIFF)
    err = np.abs(out['accel'] - ro['info']['u'][:, :, 0]).max()
    print('release order: %d cases, device %.3g; worst-first steps %s, first-first %s, device %s'
          % (ro['paths'].shape[0], err, ro['info']['steps'][ro['tells']].tolist(), ro['first'][ro['tells']].tolist(), out['qp_steps'][ro['tells']].tolist()))
    WORST['release order'] = err
    assert out['errors'] == 0 and err <= tol and ro['tells'].sum() >= 6
    _same_steps('release order', out['qp_steps'], ro['info'])


def test_nonuniform_chords_and_a_stationary_point():
    """mpc_controls takes any path: chords in ratios of 1 : 4 and 4 : 1 (the elimination has no pivoting), against the dense solve of
    reference_states; and a path that turns back on itself, with a reference state on the spline's stationary point: rv = (0, 0)."""
    paths = pc.nonuniform_paths(pc.g17_paths())
    for cfg in (dict(horizon=8), dict(horizon=8, desired_velocity=4.7)):   # the second: pieces 4..6 and the clamp, the far not-a-knot row's slopes themselves
        c = pc.config(**cfg)
        vels = pc.built_cases(paths, c, 2120)
        out = _mpc(paths, vels, **cfg)
        x, ref = pc.reference_states(paths, c)
        assert out['errors'] == 0 and all(np.isfinite(out[k]).all() for k in ('dists', 'ref_traj', 'accel', 'actions'))
        _close('non-uniform dists', out['dists'], x)
        _close('non-uniform ref_traj', out['ref_traj'], ref)
        _close('non-uniform accel', out['accel'], pc.mpc_accel(paths, vels, c)[0])
    paths, c, k = pc.stationary_case()
    cfg = {key: c[key] for key in ('desired_velocity', 'timestep', 'horizon')}
    vels = np.array([[1.0, 0.0], [0.0, -0.5]])
    out = _mpc(paths, vels, **cfg)
    x, ref = pc.reference_states(paths, c)
    assert out['errors'] == 0 and all(np.isfinite(out[key]).all() for key in ('dists', 'ref_traj', 'accel', 'actions'))
    assert (out['ref_traj'][:, k, 2:] == 0.0).all()
    _close('stationary ref_traj', out['ref_traj'], ref)
    _close('stationary accel', out['accel'], pc.mpc_accel(paths, vels, c)[0])


def test_exact_directions_and_negative_lengths():
    """Rows exactly behind the car, (-a, +0.0) and (-a, -0.0), zero rows and poses beyond 2 pi: the wrap's argument is exactly 0 or
    2 pi and the turn direction is the checker's.  And the two options validate lets be negative."""
    raw, poses = pc.exact_direction_cases()
    want = pc.decode(raw, poses)
    got = _decode(raw, poses)
    _close('exact directions', got, want)
    # the direction of the turn, read off the paths: the sign of the cross product of neighbouring chords
    def turns(p):
        d = np.diff(np.concatenate([np.zeros((p.shape[0], 1, 2)), p], axis=1), axis=1)[:, 1:]
        cross = d[:, :-1, 0] * d[:, 1:, 1] - d[:, :-1, 1] * d[:, 1:, 0]
        return np.sign(np.where(np.abs(cross) > 1e-6, cross, 0.0))
    assert np.array_equal(turns(got), turns(want)) and (turns(want) < 0).any()
    g = pc.g17_paths()[:65]
    cfg = dict(car_length=-0.3, desired_velocity=-2.0)
    raw, poses, vels = pc.designed_raw(65, 2300), pc.designed_poses(65, 2301), pc.designed_vels(65, 2302)
    _close('negative car_length', _decode(raw, poses, **cfg), pc.decode(raw, poses, pc.config(**cfg)))
    out = _mpc(g, vels, **cfg)
    x, ref = pc.reference_states(g, pc.config(**cfg))
    assert out['errors'] == 0
    _close('negative velocity ref_traj', out['ref_traj'], ref)
    _close('negative velocity accel', out['accel'], pc.mpc_accel(g, vels, pc.config(**cfg))[0])


def test_nonfinite_inputs_stay_in_their_env():
    """A diverged policy: NaN raw actions in envs 7 and 64 of 130, NaN / inf velocities in envs 8 and 65.  Every other env's outputs
    are `==` to the same batch without them (the lane exchange never crosses envs), the walks end within the step limit and the
    error word holds at most DEVERR_QP_LIMIT -- in the bounds-checked build too: every index comes from bit masks and selects."""
    from red_gym_amd import pathfollow
    n = 130
    raw, poses, vels = pc.designed_raw(n, 2400), pc.designed_poses(n, 2401), pc.designed_vels(n, 2402)
    clean_paths = pathfollow.decode_paths(_dev(raw), _dev(poses)).cpu().numpy()
    bad_raw = raw.copy()
    bad_raw[7, 5], bad_raw[64] = np.nan, np.nan
    paths = pathfollow.decode_paths(_dev(bad_raw), _dev(poses)).cpu().numpy()
    others = np.ones(n, dtype=bool)
    others[[7, 64]] = False
    assert np.array_equal(paths[others], clean_paths[others])
    # the points in front of the first NaN row are untouched (row 0 of the action is never read), the others are NaN
    assert np.array_equal(paths[7, :2], clean_paths[7, :2]) and np.isnan(paths[7, 2:]).all()
    assert np.array_equal(paths[64, :1], clean_paths[64, :1]) and np.isnan(paths[64, 1:]).all()
    for H in (5, 8):
        clean = pathfollow.mpc_controls(_dev(clean_paths), _dev(vels), horizon=H)
        assert clean['errors'] == 0
        bad_vels = vels.copy()
        bad_vels[8, 0], bad_vels[65] = np.nan, (np.inf, -np.inf)
        out = pathfollow.mpc_controls(_dev(paths), _dev(bad_vels), horizon=H)     # NaN paths in 7 and 64, non-finite velocities in 8 and 65
        others[[8, 65]] = False
        for k in ('dists', 'ref_traj', 'accel', 'actions', 'qp_steps'):
            assert np.array_equal(out[k].cpu().numpy()[others], clean[k].cpu().numpy()[others]), k
        steps = out['qp_steps'].cpu().numpy()
        print('H = %d: steps of the non-finite envs %s, error word %d' % (H, steps[~others].tolist(), out['errors']))
        assert steps.min() >= 1 and steps.max() <= pc.QP_LIMIT
        assert out['errors'] & ~pc.DEVERR_QP_LIMIT == 0
