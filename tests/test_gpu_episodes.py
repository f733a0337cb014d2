"""Episode tracker on the GPU (csrc/f110_episodes.h): the kernels alone and the tracker behind the step, every array `==` the
Python mirror of tests/episodes_cases.py."""
import os

import numpy as np
import pytest

import episodes_cases as ec
import gpu_checks as gk

pytestmark = pytest.mark.gpu

DT = 0.01
TLAD, VGAIN = 0.82461887897713965, 1.375
BUF_KEYS = ec.STATE + ('limit',) + ec.LOG + ('count',)
INFO_KEYS = {'episode_return': 'ep_return', 'episode_length': 'ep_length', 'truncated': 'truncated', 'episodes_finished': 'count'}
INFO_OFF = {'checkpoint_done', 'collision_idx', 'current_time', 'toggles'}
STATE_OFF = {'state', 'steer_buf', 'steer_cnt', 'noise_step', 'spawn', 'start_rot', 'near_start', 'toggles', 'current_time',
             'pending_reset', 'collisions', 'collision_idx', 'in_collision', 'lap_counts', 'lap_times', 'done', 'checkpoint_done',
             'scans'}


_eq = gk.equal      # `==` at the array's own width: bit patterns for fp64, values and dtype for the integers


def _env(assets, B, **kw):
    from red_gym_amd import F110VecEnv
    return F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, **kw)


def _waypoints(env):
    import torch
    from red_gym_amd import workload
    rl = workload.load_waypoints(workload.RACELINE)
    return torch.as_tensor(np.ascontiguousarray(rl[:, [1, 2, 5]]), device=env.device)


def _tracker_arrays(env):
    return {k: gk.to_host(env.episodes.buf[k]) for k in BUF_KEYS}


def _assert_tracker(env, ck, what, info=None):
    got, want = _tracker_arrays(env), ck.arrays()
    bad = [k for k in BUF_KEYS if not _eq(got[k], want[k])]
    assert not bad, (what, bad)
    if info is not None:
        for key, name in INFO_KEYS.items():
            assert _eq(gk.to_host(info[key]), want[name]), (what, key)


def _feed(env, ck, reward, done, info, obs):
    """The checker takes what step() returned; pending_reset as the step left it is `done` (autoreset) or 0."""
    done_h = gk.to_host(done)
    pend = done_h.astype(np.uint8) if env.eng.autoreset else np.zeros(env.num_envs, np.uint8)
    closed = ck.update(gk.to_host(reward), done_h, gk.to_host(info['current_time']), gk.to_host(obs['lap_counts'])[:, 0], pend)
    return closed, pend


# ---------------------------------------------------------------- 1. the kernels alone
PATTERNS = ('none', 'all', 'third', 'lane0', 'last')


def _pattern(name, n):
    e = np.arange(n)
    return {'none': e < 0, 'all': e >= 0, 'third': e % 3 == 0, 'lane0': e % 64 == 0, 'last': e == n - 1}[name]


def _schedule(n, M, k, rng, clock):
    """Update k of five for the closing set M: (reward, done, clock, laps).  M closes at update 0 (DONE), is reset at 1, steps at 2
    (its envs with limit 1 close: LIMIT), is reset at 3 (the ones still open close: RESET) and closes at 4 (DONE); the other envs
    step on, every 5th of them left alone at update 3."""
    done = np.zeros(n, np.uint8)
    clock = clock.copy()
    if k in (0, 4):
        done[M] = 1
    if k in (1, 3):
        idle = ~M & (np.arange(n) % 5 == 2) & (k == 3)
        clock[M] = DT
        clock[~M & ~idle] += DT
    else:
        clock += DT
    reward = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
    return reward, done, clock, rng.integers(0, 3, n).astype(np.int32)


class _Raw(object):
    """The tracker's arrays between guards, and the struct of pointers to them."""

    def __init__(self, n, L, limit):
        import torch
        from red_gym_amd import episodes
        tt = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}
        self.g = {}
        for k in ec.STATE + ('limit',):
            self.g[k] = gk.Guarded(n, dtype=tt[ec.DTYPES[k]], fill=7)
        for k in ec.LOG:
            self.g[k] = gk.Guarded(L, dtype=tt[ec.DTYPES[k]], fill=7)
        self.g['count'] = gk.Guarded(1, dtype=torch.int64, fill=7)
        self.g['block_counts'] = gk.Guarded(episodes.blocks(n), dtype=torch.int32, fill=7)
        self.g['pending_reset'] = gk.Guarded(n, dtype=torch.uint8, fill=7)
        for k in ec.STATE + ec.LOG + ('count', 'pending_reset'):
            self.g[k].data.zero_()
        self.g['ep_open'].data.fill_(1)
        self.g['t_seen'].data.fill_(-1.0)
        self.g['limit'].data.copy_(gk.to_device(limit))
        self.buf = {k: v.data for k, v in self.g.items()}

    def read(self):
        return {k: v.read() for k, v in self.g.items()}


def _run_case(n, name, L, autoreset, order=None):
    """Five updates of one case through f110_episodes_apply and through the checker; returns the keys that differ anywhere."""
    import torch
    from red_gym_amd import episodes
    rng = np.random.default_rng(1000 * n + 10 * L + PATTERNS.index(name))
    M = _pattern(name, n)
    limit = np.where(M & (np.arange(n) % 2 == 0), 1, 0).astype(np.int32)
    ck = ec.EpisodeChecker(n, DT, limit, L, autoreset, order=order)
    raw = _Raw(n, L, limit)
    clock = np.full(n, DT)
    bad, most = set(), 0
    for k in range(5):
        reward, done, clock, laps = _schedule(n, M, k, rng, clock)
        pend = np.zeros(n, np.uint8)
        closed = ck.update(reward, done, clock, laps, pend)
        most = max(most, len(closed))
        raw.g['pending_reset'].data.zero_()
        dev = [gk.to_device(a) for a in (clock, done, reward, laps)]
        episodes.apply(raw.buf, dev[0], dev[1], DT, reward=dev[2], laps=dev[3], pending_reset=raw.buf['pending_reset'] if autoreset else None)
        torch.cuda.synchronize()
        got, want = raw.read(), ck.arrays()          # (read() asserts the guards)
        bad |= {key for key in BUF_KEYS if not _eq(got[key], want[key])}
        if not _eq(got['pending_reset'], pend if autoreset else np.zeros(n, np.uint8)):
            bad.add('pending_reset')
    return bad, ck, most


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_kernels_equal_the_checker(n):
    """Every closing pattern and log size, five updates in a row: state, every log slot (untouched ones included), the counter,
    pending_reset and the guards `==` the checker."""
    wrapped = many = False
    for name in PATTERNS:
        for i, L in enumerate((1, 7, 64, n + 3)):
            bad, ck, most = _run_case(n, name, L, autoreset=bool((i + PATTERNS.index(name)) % 2))
            assert not bad, (n, name, L, sorted(bad))
            assert ck.count == {'none': 0}.get(name, 3 * int(_pattern(name, n).sum())), (name, ck.count)
            wrapped |= ck.count >= 2 * L
            many |= most > L
    assert wrapped and (many or n == 1)          # the counter passed the ring's end more than once; one update closed more than L


def test_another_order_than_env_order_is_told_apart():
    """A log written in another order than ascending env order differs from the kernels' on these patterns: the checker with its
    closing order reversed no longer compares equal."""
    n = 257
    for name in ('all', 'third', 'lane0'):
        bad, _, _ = _run_case(n, name, 64, True)
        assert not bad
        bad, _, _ = _run_case(n, name, 64, True, order=range(n - 1, -1, -1))
        assert 'log_env' in bad and 'log_return' in bad and 'count' not in bad and 'ep_return' not in bad, (name, sorted(bad))


def test_apply_with_the_configs_limit_and_the_constant_reward():
    """No limit array (cfg.limit for every env), no reward array (the constant timestep), no laps."""
    import torch
    from red_gym_amd import episodes
    n, L = 70, 16
    ck = ec.EpisodeChecker(n, DT, 3, L, False)
    buf = episodes.new_buffers(n, L, 'cuda')
    clock = np.zeros(n)
    done = np.zeros(n, np.uint8)
    for k in range(6):
        clock = clock + DT
        ck.update(None, done, clock)
        episodes.apply(buf, gk.to_device(clock), gk.to_device(done), DT, limit=3)
        torch.cuda.synchronize()
        want = ck.arrays()
        assert all(_eq(gk.to_host(buf[key]), want[key]) for key in BUF_KEYS if key != 'limit'), k
    assert ck.count == n and (ck.log_reason == ec.LIMIT).all() and (ck.log_length == 3).all()


# ---------------------------------------------------------------- 2. closed loop
def test_closed_loop_equals_checker(assets):
    """256 envs, autoreset, lidar noise, the shaper's reward, planner actions with a quarter of the envs driven at the wall, limits
    30..45, 150 steps and a masked reset of half the envs: info, state, log and counter `==` the checker after every step, and
    every env closed by LIMIT is respawned by the next step."""
    import torch
    from red_gym_amd import workload
    B = 256
    env = _env(assets, B, autoreset=True)
    assert env.eng._noise_on
    wp = _waypoints(env)
    env.shape_rewards()
    limits = (30 + np.arange(B) % 16).astype(np.int32)
    env.track_episodes(torch.as_tensor(limits), log=300)
    assert env.consumers[-1] is env.episodes
    ck = ec.EpisodeChecker(B, env.timestep, limits, 300, True)
    spawn = workload.spawn_poses(B, 1)
    crash = np.arange(B) % 4 == 1
    spawn[crash, 0, 2] += np.pi / 2
    crash_dev = torch.as_tensor(crash, device=env.device)
    obs, reward, done, info = env.reset(spawn)
    _feed(env, ck, reward, done, info, obs)
    _assert_tracker(env, ck, 'reset', info)
    limit_closed = []
    for k in range(150):
        if k == 75:
            mask = (np.arange(B) % 2 == 0).astype(np.uint8)
            obs, reward, done, info = env.reset(spawn, torch.as_tensor(mask))
        else:
            acts = env.pure_pursuit(wp, TLAD, VGAIN)
            acts[:, 0, 0] = torch.where(crash_dev, 0.0, acts[:, 0, 0])
            acts[:, 0, 1] = torch.where(crash_dev, 8.0, acts[:, 0, 1])
            obs, reward, done, info = env.step(acts)
        clock, done_h = gk.to_host(info['current_time']), gk.to_host(done)
        if limit_closed:   # closed by LIMIT in the step before: respawned now
            e = np.array(limit_closed)
            xy = gk.to_host(env.state)[e, 0, :2]
            assert (clock[e] == env.timestep).all() and not done_h[e].any(), k
            assert (np.abs(xy - spawn[e, 0, :2]).max(axis=1) < 2e-3).all(), k    # (one step from rest moves a car less than a millimetre)
        n0 = len(ck.records)
        _, pend = _feed(env, ck, reward, done, info, obs)
        _assert_tracker(env, ck, 'step %d' % k, info)
        assert _eq(gk.to_host(env.eng.t['pending_reset']), pend), k
        limit_closed = [r[0] for r in ck.records[n0:] if r[3] == ec.LIMIT]
        assert not done_h[limit_closed].any()
    reasons = {r[3] for r in ck.records}
    print('episodes closed: %d (done %d, limit %d, reset %d)' % ((ck.count,) + tuple(sum(r[3] == c for r in ck.records) for c in (1, 2, 3))))
    assert reasons == {ec.DONE, ec.LIMIT, ec.RESET}         # a condition of the inputs
    assert ck.count > ck.L                                  # the ring wrapped
    fin, want = env.episodes.finished(), ck.finished()
    assert all(_eq(gk.to_host(fin[key]), want[key]) for key in want)
    fin, want = env.episodes.finished(last=10), ck.finished(last=10)
    assert all(_eq(gk.to_host(fin[key]), want[key]) for key in want)
    s = env.episodes.summary(last=100)
    assert s['count'] == ck.count and s['n'] == 100 and abs(s['done'] + s['limit'] + s['reset'] - 1.0) < 1e-12
    assert s['mean_length'] == float(np.mean(ck.finished(100)['length']))
    assert env.eng.device_errors() == 0
    env.close()


# ---------------------------------------------------------------- 3. the case that motivates this
def test_a_standing_car_ends_its_episode_at_the_limit(assets):
    """64 envs, zero actions: without the tracker no env is ever reset; with track_episodes(20) every env closes five episodes of
    length 20 with reason LIMIT, logged in env order step by step.  (The respawn step behind a LIMIT counts no step -- it is the
    reference's env.reset() -- so five episodes take 5 * 20 + 4 = 104 steps, not 100.)"""
    import torch
    from red_gym_amd import workload
    B, steps = 64, 104
    spawn = workload.spawn_poses(B, 1)
    zero = torch.zeros((B, 1, 2), dtype=torch.float64, device='cuda')
    env = _env(assets, B, autoreset=True)
    env.reset(spawn)
    for k in range(steps):
        _, _, done, info = env.step(zero)
        assert not bool(done.any()) and not bool(env.eng.t['pending_reset'].any())
        assert not bool((info['current_time'] == env.timestep).any())                          # never respawned
    env.close()
    env = _env(assets, B, autoreset=True)
    env.track_episodes(20)
    env.reset(spawn)
    closes = []
    for k in range(steps):
        _, reward, done, info = env.step(zero)
        assert not bool(done.any())
        n = int(info['episodes_finished'].item())
        if n != (closes[-1][1] if closes else 0):
            closes.append((k, n))
    assert closes == [(19, 64), (40, 128), (61, 192), (82, 256), (103, 320)], closes
    fin = {k: gk.to_host(v) for k, v in env.episodes.finished().items()}
    ret = t = 0.0
    for _ in range(20):
        ret += env.timestep
    t = env.timestep
    for _ in range(20):
        t = t + env.timestep
    assert _eq(fin['env'], np.tile(np.arange(B, dtype=np.int32), 5))
    assert (fin['length'] == 20).all() and (fin['reason'] == ec.LIMIT).all() and (fin['laps'] == 0).all()
    assert _eq(fin['ret'], np.full(5 * B, ret)) and _eq(fin['time'], np.full(5 * B, t))
    assert bool(info['truncated'].all()) and env.episodes.summary()['limit'] == 1.0
    env.close()


# ---------------------------------------------------------------- 4. autoreset off
def test_without_autoreset_only_the_flag_is_raised(assets):
    import torch
    from red_gym_amd import workload
    B = 32
    spawn = workload.spawn_poses(B, 1)
    zero = torch.zeros((B, 1, 2), dtype=torch.float64, device='cuda')
    env = _env(assets, B, autoreset=False)
    env.track_episodes(10, log=64)
    ck = ec.EpisodeChecker(B, env.timestep, 10, 64, False)
    obs, reward, done, info = env.reset(spawn)
    _feed(env, ck, reward, done, info, obs)
    rose = None
    for k in range(25):
        obs, reward, done, info = env.step(zero)
        _feed(env, ck, reward, done, info, obs)
        _assert_tracker(env, ck, 'step %d' % k, info)
        assert not bool(env.eng.t['pending_reset'].any()) and not bool(done.any())
        tr = gk.to_host(info['truncated'])
        assert tr.all() or not tr.any()
        if tr.all() and rose is None:
            rose = k
        assert rose is None or tr.all()                                   # it rises once and stays
        assert (gk.to_host(info['current_time']) > env.timestep).all()    # the env keeps stepping
    assert rose == 9 and ck.count == B and int(info['episodes_finished'].item()) == B      # exactly one record per env
    assert _eq(gk.to_host(info['episode_length']), np.full(B, 10, np.int32))               # frozen
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    obs, reward, done, info = env.reset(spawn, torch.as_tensor(mask))
    _feed(env, ck, reward, done, info, obs)
    _assert_tracker(env, ck, 'masked reset', info)
    hit = mask.astype(bool)
    assert ck.count == B and not ck.truncated[hit].any() and ck.truncated[~hit].all() and ck.ep_open[hit].all()
    for k in range(10):
        obs, reward, done, info = env.step(zero)
        _feed(env, ck, reward, done, info, obs)
        _assert_tracker(env, ck, 'second episode, step %d' % k, info)
    assert ck.count == B + hit.sum() and [r[0] for r in ck.records[B:]] == list(np.flatnonzero(hit))
    assert {r[3] for r in ck.records} == {ec.LIMIT}
    env.close()


# ---------------------------------------------------------------- 5. replay
def test_the_limit_step_is_a_valid_transition_with_d_0(assets):
    import torch
    from red_gym_amd import workload
    B, T = 16, 8
    spawn = workload.spawn_poses(B, 1)
    zero = torch.zeros((B, 1, 2), dtype=torch.float64, device='cuda')
    env = _env(assets, B, autoreset=True)
    env.shape_rewards()
    env.record_replay(steps=T, action_dim=2)
    limits = (5 + np.arange(B) % 3).astype(np.int32)
    env.track_episodes(limits)
    env.reset(spawn)
    seen = 0
    was_limit = np.zeros(B, bool)
    for k in range(20):
        _, reward, done, info = env.step(zero)
        valid, trunc = gk.to_host(info['replay_valid']), gk.to_host(info['truncated']).astype(bool)
        clock = gk.to_host(info['current_time'])
        slot = (int(info['replay_count'].item()) - 1) % T
        d = gk.to_host(env.replay.buf['dones'])[slot]
        now_limit = trunc & ~was_limit & (clock != env.timestep)
        assert (valid[now_limit] == 1).all() and (d[now_limit] == 0).all(), k       # the LIMIT step: valid, d = 0
        assert (clock[was_limit] == env.timestep).all() and (valid[was_limit] == 0).all(), k   # the respawn step behind it: invalid
        assert not trunc[was_limit].any()
        seen += int(now_limit.sum())
        was_limit = now_limit
    assert seen >= 2 * B
    env.close()


# ---------------------------------------------------------------- 6. graphs
def test_graph_replays_equal_eager_steps(assets):
    """The same 60 steps eagerly, through capture_step / step_graph and through step_lib_graph: state, log and counter `==` after
    every step."""
    import torch
    from red_gym_amd import workload
    B, steps = 64, 60
    spawn = workload.spawn_poses(B, 1)
    spawn[np.arange(B) % 4 == 1, 0, 2] += np.pi / 2
    pool = torch.as_tensor(workload.action_pool(steps, B, 1), device='cuda')
    limits = (7 + np.arange(B) % 5).astype(np.int32)
    runs = {}
    for how in ('eager', 'graph', 'lib_graph'):
        env = _env(assets, B, autoreset=True)
        env.shape_rewards()
        env.track_episodes(limits, log=50)
        env.reset(spawn)
        if how == 'graph':
            env.capture_step()
        elif how == 'lib_graph':
            env.build_step_graph()
        stepper = {'eager': env.step, 'graph': env.step_graph, 'lib_graph': env.step_lib_graph}[how]
        out = []
        for k in range(steps):
            _, reward, done, info = stepper(pool[k])
            out.append({key: env.episodes.buf[key].clone() for key in BUF_KEYS})
            out[-1]['reward'], out[-1]['pending_reset'] = reward.clone(), env.eng.t['pending_reset'].clone()
        torch.cuda.synchronize()
        runs[how] = [{key: gk.to_host(v) for key, v in o.items()} for o in out]
        assert env.eng.device_errors() == 0
        env.close()
    count = int(runs['eager'][-1]['count'][0])
    assert count > 2 * 50 and ec.LIMIT in set(runs['eager'][-1]['log_reason'])
    for how in ('graph', 'lib_graph'):
        for k in range(steps):
            bad = [key for key in runs['eager'][k] if not _eq(runs[how][k][key], runs['eager'][k][key])]
            assert not bad, (how, k, bad)


# ---------------------------------------------------------------- 7. checkpoint
def test_checkpoint_restores_and_restarts(assets):
    import torch
    from red_gym_amd import workload
    B = 32
    spawn = workload.spawn_poses(B, 1)
    spawn[np.arange(B) % 4 == 1, 0, 2] += np.pi / 2
    pool = torch.as_tensor(workload.action_pool(65, B, 1), device='cuda')
    limits = (9 + np.arange(B) % 4).astype(np.int32)

    def make(track=True):
        env = _env(assets, B, autoreset=True)
        if track:
            env.track_episodes(limits, log=40)
        return env
    a = make()
    a.reset(spawn)
    for k in range(25):
        a.step(pool[k])
    sd = a.state_dict()
    assert int(sd['episodes_finished'].item()) > 0 and set(sd) - STATE_OFF == set(a.episodes.STATE)
    b = make()
    b.reset(spawn)
    b.load_state_dict(sd)
    for k in range(25, 65):
        ra, rb = a.step(pool[k]), b.step(pool[k])
        ta, tb = _tracker_arrays(a), _tracker_arrays(b)
        assert all(_eq(tb[key], ta[key]) for key in BUF_KEYS), k
        assert _eq(gk.to_host(rb[2]), gk.to_host(ra[2])) and _eq(gk.to_host(b.state), gk.to_host(a.state)), k
    assert int(a.episodes.buf['count'].item()) > 40
    # a checkpoint taken without the tracker restarts it: nothing is logged, the lengths start at 0
    plain = {k: v for k, v in sd.items() if k in STATE_OFF}
    before = _tracker_arrays(b)
    b.load_state_dict(plain)
    after = _tracker_arrays(b)
    assert all(_eq(after[key], before[key]) for key in ec.LOG + ('count', 'limit'))
    assert not after['ep_length'].any() and not after['ep_return'].any() and after['ep_open'].all() and not after['truncated'].any()
    _, _, _, info = b.step(pool[0])
    length, clock = gk.to_host(info['episode_length']), gk.to_host(info['current_time'])
    assert _eq(length, (clock != b.timestep).astype(np.int32))
    assert int(info['episodes_finished'].item()) - int(before['count'][0]) == int(gk.to_host(b.eng.t['done'])[clock != b.timestep].sum())
    a.close()
    b.close()


# ---------------------------------------------------------------- 8. opt-in
def test_off_leaves_no_key_and_statistics_only_changes_no_state(assets):
    import torch
    from red_gym_amd import workload
    B = 32
    spawn = workload.spawn_poses(B, 1)
    spawn[np.arange(B) % 4 == 1, 0, 2] += np.pi / 2
    pool = workload.action_pool(50, B, 1)
    pool[:, np.arange(B) % 4 == 1, 0] = (0.0, 8.0)          # a quarter of the envs drive straight at the wall
    pool = torch.as_tensor(pool, device='cuda')
    plain, stats = _env(assets, B, autoreset=True), _env(assets, B, autoreset=True)
    _, _, _, info = plain.reset(spawn)
    assert set(info) == INFO_OFF and set(plain.state_dict()) == STATE_OFF
    stats.track_episodes(0)
    _, _, _, info = stats.reset(spawn)
    assert set(info) == INFO_OFF | set(INFO_KEYS) and set(stats.state_dict()) == STATE_OFF | set(stats.episodes.STATE)
    for k in range(50):
        plain.step(pool[k])
        _, _, _, info = stats.step(pool[k])
        sp, ss = plain.state_dict(), stats.state_dict()
        bad = [key for key in STATE_OFF if not torch.equal(sp[key], ss[key])]
        assert not bad, (k, bad)
    for k in range(100):                                      # (on until the envs driven at the wall have reached it)
        _, _, _, info = stats.step(pool[k % 50])
    n = int(info['episodes_finished'].item())
    print('statistics only: %d episodes closed' % n)
    assert n > 0 and set(gk.to_host(stats.episodes.finished()['reason'])) == {ec.DONE} and not bool(info['truncated'].any())
    stats.track_episodes(None)
    _, _, _, info = stats.step(pool[0])
    assert set(info) == INFO_OFF and set(stats.state_dict()) == STATE_OFF
    with pytest.raises(ValueError):
        stats.episodes.finished()
    for bad in (dict(max_steps=-1), dict(log=0), dict(max_steps=torch.zeros(B + 1, dtype=torch.int32)), dict(max_steps=torch.full((B,), -1))):
        with pytest.raises(ValueError):
            stats.track_episodes(**bad)
        assert not stats.episodes.on and set(stats.step(pool[1])[3]) == INFO_OFF
    stats.track_episodes(False)
    plain.close()
    stats.close()
