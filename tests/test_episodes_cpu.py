"""The episode tracker without a GPU: its Python mirror (tests/episodes_cases.py) equals the reference's loop written down
literally, and the new entry points are exported, refuse NULL arguments and refuse a bad config before any device call."""
import ctypes as C

import numpy as np
import pytest

import episodes_cases as ec
from red_gym_amd import _lib, build

DT = 0.01


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _lib.load()


def _scripts():
    """(rewards, dones, max_steps) per env: no done at all, dones before, exactly at and right behind the limit, a done on the
    first step, rewards whose sum depends on the order of the adds."""
    rng = np.random.default_rng(21)
    out = []
    for limit, n, every in ((7, 60, 0), (7, 60, 5), (7, 63, 7), (7, 64, 8), (5, 40, 1), (1, 9, 0), (13, 200, 11), (2000, 60, 17)):
        rewards = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)).tolist()
        dones = [bool(every) and (k + 1) % every == 0 for k in range(n)]
        out.append((rewards, dones, limit))
    return out


def _drive(ck, env, rewards, dones):
    """Feeds env `env` of the checker what an autoreset engine would return for the script: a reset step first and behind
    every closed episode (clock == timestep, nothing paid), then one step per script entry."""
    B = ck.B
    clock = np.array(ck.t_seen)
    clock[env] = DT
    ck.update(np.zeros(B), np.zeros(B, bool), clock)
    for r, d in zip(rewards, dones):
        clock = np.array(ck.t_seen)
        clock[env] = ck.t_seen[env] + DT
        rew, dn = np.zeros(B), np.zeros(B, bool)
        rew[env], dn[env] = r, d
        if ck.update(rew, dn, clock):
            clock = np.array(ck.t_seen)
            clock[env] = DT                      # the respawn
            ck.update(np.full(B, 123.0), np.zeros(B, bool), clock)


def test_checker_equals_the_reference_loop():
    scripts = _scripts()
    B = len(scripts)
    ck = ec.EpisodeChecker(B, DT, [s[2] for s in scripts], 4096, True)
    for env, (rewards, dones, limit) in enumerate(scripts):
        _drive(ck, env, rewards, dones)
    seen = set()
    for env, (rewards, dones, limit) in enumerate(scripts):
        want = ec.reference_loop(rewards, dones, limit)
        got = [(r[2], r[1], r[3]) for r in ck.records if r[0] == env]
        assert len(want) >= 3, env
        assert [w[1:] for w in want] == [g[1:] for g in got], env        # lengths and reasons
        assert all(w[0] == g[0] for w, g in zip(want, got)), env          # returns `==`
        seen |= {w[2] for w in want}
    assert seen == {ec.DONE, ec.LIMIT}
    # an episode that ends by done exactly at the limit is DONE
    rewards, dones, limit = scripts[2]
    assert dones[limit - 1] and [r[3] for r in ck.records if r[0] == 2][0] == ec.DONE
    assert ck.count == len(ck.records) and ck.count < ck.L
    # the log holds the records in closing order
    fin = ck.finished()
    assert [tuple(fin[k][i] for k in ('env', 'length', 'ret', 'reason')) for i in range(ck.count)] == [r[:4] for r in ck.records]


def test_checker_rules_reset_idle_and_closed_episode():
    """The rules the loop does not have: a masked reset cuts an open episode (RESET), an env left alone changes nothing, an episode
    closed with autoreset off stays frozen and logs once, more than L closes keep the last L in env order."""
    ck = ec.EpisodeChecker(4, DT, 3, 2, False)
    z, f = np.zeros(4), np.zeros(4, bool)
    ck.update(z, f, np.full(4, DT))
    before = {k: v.copy() for k, v in ck.arrays().items()}
    ck.update(z + 9.0, f, np.full(4, DT))                                   # not stepped: idempotent
    assert all(np.array_equal(before[k], v) for k, v in ck.arrays().items())
    ck.update(z + 1.0, f, np.full(4, 2 * DT))
    ck.update(z + 1.0, f, np.array([3 * DT, 3 * DT, DT, 2 * DT]))          # env 2 reset by the user, env 3 left alone
    assert ck.records == [(2, 1, 1.0, ec.RESET, DT, 0)] and ck.ep_length.tolist() == [2, 2, 0, 1]
    pend = np.zeros(4, np.uint8)
    ck.update(z + 1.0, f, np.array([4 * DT, 4 * DT, 2 * DT, 3 * DT]), pending_reset=pend)   # envs 0, 1 reach the limit
    assert [r[0] for r in ck.records[1:]] == [0, 1] and ck.truncated.tolist() == [1, 1, 0, 0] and not pend.any()
    ck.update(z + 1.0, f, np.array([5 * DT, 5 * DT, 3 * DT, 4 * DT]))      # closed episodes step on: frozen; env 3 reaches it
    assert ck.ep_return.tolist() == [3.0, 3.0, 2.0, 3.0] and ck.count == 4 and ck.records[-1][0] == 3
    assert ck.log_env.tolist() == [1, 3]                                    # slots 3 % 2 and 2 % 2 ... record k in slot k % L
    ck2 = ec.EpisodeChecker(5, DT, 1, 2, True)
    ck2.update(None, np.zeros(5, bool), np.full(5, DT))
    pend = np.zeros(5, np.uint8)
    ck2.update(None, np.zeros(5, bool), np.full(5, 2 * DT), pending_reset=pend)          # five close, the log holds two
    assert ck2.count == 5 and pend.all()
    assert ck2.log_env[3 % 2] == 3 and ck2.log_env[4 % 2] == 4 and (ck2.log_return == DT).all()


def test_symbols_exported():
    """What the package re-exports (the library's own exports and their prototypes: tests/test_abi_cpu.py)."""
    from red_gym_amd import episodes
    assert (episodes.DONE, episodes.LIMIT, episodes.RESET) == (ec.DONE, ec.LIMIT, ec.RESET)
    import red_gym_amd
    assert (red_gym_amd.DONE, red_gym_amd.LIMIT, red_gym_amd.RESET) == (1, 2, 3) and red_gym_amd.EpisodeTracker is episodes.EpisodeTracker
    # block_counts is sized by the header's constant, one entry per workgroup of the kernels
    assert [episodes.blocks(n) for n in (1, 256, 257)] == [-(-n // _lib.F110_EPISODES_BLOCK) for n in (1, 256, 257)] == [1, 1, 2]


def test_null_arguments_are_refused_without_a_gpu(lib):
    cfg = _lib.EpisodesConfig(limit=10, log=16)
    bufs = _lib.EpisodesBuffers()
    fake = C.c_void_p(4096)
    assert lib.f110_episodes_validate(None) == _lib.E_INVALID and b'null' in lib.f110_last_error()
    assert lib.f110_episodes_install(None, C.byref(cfg)) == _lib.E_INVALID and b'null' in lib.f110_last_error()
    assert lib.f110_episodes_install(None, None) == _lib.E_INVALID
    assert lib.f110_episodes_bind(None, C.byref(bufs)) == _lib.E_INVALID
    assert lib.f110_episodes_bind(fake, None) == _lib.E_INVALID
    assert lib.f110_episodes_update(None, None) == _lib.E_INVALID and b'null' in lib.f110_last_error()
    assert lib.f110_episodes_apply(None, 4, DT, None, fake, fake, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID
    assert lib.f110_episodes_apply(C.byref(cfg), 4, DT, None, fake, fake, None, 1, None, None, None) == _lib.E_INVALID
    assert lib.f110_episodes_apply(C.byref(cfg), 4, DT, None, None, fake, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID
    assert lib.f110_episodes_apply(C.byref(cfg), 4, DT, None, fake, None, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID
    # every array of the struct but `limit` is required
    for name in _lib.EPISODES_FIELDS:
        setattr(bufs, name, 4096)
    assert lib.f110_episodes_apply(C.byref(cfg), -1, DT, None, fake, fake, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID
    assert lib.f110_episodes_apply(C.byref(cfg), 4, 0.0, None, fake, fake, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID
    for name in _lib.EPISODES_FIELDS:
        if name == 'limit':
            continue
        setattr(bufs, name, None)
        assert lib.f110_episodes_apply(C.byref(cfg), 4, DT, None, fake, fake, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID, name
        setattr(bufs, name, 4096)
    with pytest.raises(ValueError):
        _lib.check(lib.f110_episodes_update(None, None))


def test_config_is_refused(lib):
    from red_gym_amd import episodes
    episodes.validate()
    episodes.validate(limit=0, log=1)
    episodes.validate(limit=2 ** 31 - 1, log=2 ** 24)
    for kw in (dict(limit=-1), dict(log=0), dict(log=-5), dict(log=2 ** 24 + 1), dict(limit=-2 ** 40), dict(log=2 ** 40)):
        with pytest.raises(ValueError):
            episodes.validate(**kw)
    # the function-level entry refuses the same configs before it looks at anything else
    bufs = _lib.EpisodesBuffers()
    for limit, log in ((-1, 16), (10, 0)):
        cfg = _lib.EpisodesConfig(limit=limit, log=log)
        assert lib.f110_episodes_apply(C.byref(cfg), 4, DT, None, None, None, None, 1, None, C.byref(bufs), None) == _lib.E_INVALID
