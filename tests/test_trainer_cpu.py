"""The composed checker of tests/trainer_cases.py on a scripted run, no GPU: it agrees with the definitions it overlaps with
(episodes_cases.reference_loop, replay_cases.fifo, and the ring holds the shaper's own reward and images), and every mistake of the
composition it exists to find -- another order of the consumers, the image drawn too early, the wrong car, a reset seen late --
changes what it expects on this input.  The script plays the env: hand-built images, replay_cases.scripted_pushes' actions and
dones, and a clock that respawns an env behind a done, behind a LIMIT raised by the checker itself and at a masked reset."""
import numpy as np
import pytest

import episodes_cases as ec
import progress_cases as gc
import replay_cases as rc
import shaping_cases as sc
import trainer_cases as tc

B, A, AGENT, DT, T, AD = 6, 2, 1, 0.01, 3, 16
ROWS, COLS = 12, 70
LIMITS = np.array([4, 5, 0, 6, 4, 5], np.int32)
MASKED_AT, MASK = 9, np.arange(B) % 3 == 0
PUSHES = rc.scripted_pushes(ROWS, COLS, B, 8, AD, DT)                  # 19 pushes: env 4 done at 1, env 2 at 4, env 0 at 17
HAND = sc.hand_images(ROWS, COLS)
SHAPING = dict(scale=1.0, origin_x=0.0, origin_y=0.0)                  # a pixel per metre: the poses below lie inside the image
FOLLOW = dict(dist_threshold=50.0, replan_at=2)                        # every update advances the index: replans at replan_at


def _checker(**kw):
    kw.setdefault('agent', AGENT)
    return tc.LoopChecker(B, A, timestep=DT, raceline=gc.circle_raceline(6.0, 200, (30.0, 5.0)), rows=ROWS, cols=COLS, steps=T,
                          action_dim=AD, limits=LIMITS, log=64, shaping=SHAPING, follow=FOLLOW, render=lambda scans: scans.copy(), **kw)


def _state(k, fresh):
    """[B, A, 7]: every car somewhere else at every step, inside the image; an env reset by the step stands at its spawn pose."""
    e, a = np.meshgrid(np.arange(B), np.arange(A), indexing='ij')
    kk = np.where(fresh[:, None], 0, k + 1)
    st = np.zeros((B, A, 7))
    st[..., 0] = (3.0 + 7.0 * e + 2.3 * kk + 11.0 * a) % (COLS - 2) + 0.5
    st[..., 1] = 1.2 + (0.9 * kk + 1.7 * e + 3.0 * a) % 8.5
    st[..., 3] = 0.5 + 0.1 * e + 0.05 * a
    st[..., 4] = 0.1 * kk - 0.3 * a
    return st


def _images(k, q):
    """[B, A, rows, cols]: the hand-built images in turn for car 1, the script's own frames for car 0 (every third step the two
    are swapped, so that either car sees both kinds)."""
    hand = np.stack([HAND[(k + 2 * e) % HAND.shape[0]] for e in range(B)])
    cars = [rc.binary(q['frame']), hand]
    return np.stack(cars[::-1] if k % 3 == 2 else cars, axis=1)


def _play(ck):
    """The scripted run through `ck`; returns what every step expected -- `info`, the reward, pending_reset and the ring's newest step
    slot as it reads back -- and what the run fed it."""
    clock, pending = np.zeros(B), np.zeros(B, bool)
    steps, fed = [], []
    for k, q in enumerate(PUSHES):
        stood = np.zeros(B, bool)
        if k == 0:
            mask = np.ones(B, bool)
            clock = np.full(B, DT)
        elif k == MASKED_AT:
            mask = MASK
            stood = ~(mask | pending)                                  # outside the mask and not pending: not stepped
            clock = np.where(stood, clock, DT)
        else:
            mask = None
            ck.act(q['action'].astype(np.float64))
            clock = np.where(pending, DT, clock + DT)
        fresh = clock == DT
        done = q['done'].astype(bool) & ~fresh & ~stood
        images = _images(k, q)
        info, reward = ck.after_step(_state(k, fresh), clock, done, (k + np.arange(B)) // 7, pending, images, mask)
        pending = ck.pending_reset.astype(bool)
        slot = ck.newest_slot()[0]
        ring = dict(zip(('ring_s', 'ring_a', 'ring_r', 'ring_ns', 'ring_d', 'ring_ok'), ck.mirror.at(range(slot * B, slot * B + B))))
        steps.append(dict(info, reward=reward, pending_reset=ck.pending_reset.copy(), **ring))
        fed.append(dict(clock=clock.copy(), done=done, fresh=fresh, stood=stood, images=images))
    return steps, fed


def _everything(ck, steps):
    """One flat list of arrays: every step's expectations, what the ring holds at the end, the episode records."""
    out = [np.asarray(s[key]) for s in steps for key in sorted(s)]
    out += [np.asarray(x) for x in ck.mirror.at(range(T * B))]
    out.append(np.array(ck.episodes.records, dtype=np.float64).reshape(-1, 6))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and bool(np.all(sc.same(x, y))) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def base():
    ck = _checker()
    steps, fed = _play(ck)
    return ck, steps, fed


def test_the_script_holds_what_it_is_for(base):
    ck, steps, fed = base
    reasons = {r[3] for r in ck.episodes.records}
    assert reasons == {ec.DONE, ec.LIMIT, ec.RESET}
    assert any(f['stood'].any() for f in fed) and ck.mirror.count == len(PUSHES) > 2 * T
    assert (ck.follower.reached > 0).all() and (ck.follower.replans > ck.follower.reached).all()    # replans at replan_at and behind resets
    assert {k for k in steps[0] if not k.startswith('ring_')} == {
        'reward', 'pending_reset', 'lidar_bitmap', 'reward_collision', 'reward_progress', 'reward_centering', 'bitmap_collided',
        'frenet_s', 'frenet_d', 'heading_error', 'progress', 'progress_delta', 'lap_length', 'path_points', 'path_index',
        'path_replanned', 'mpc_accel', 'replay_count', 'replay_valid', 'episode_return', 'episode_length', 'truncated', 'episodes_finished'}
    # the shaper's terms depend on the image: collided takes both values, the centering term several
    for key, values in (('bitmap_collided', 2), ('reward_centering', 4), ('reward_progress', 4)):
        assert len({float(v) for s in steps for v in s[key]}) >= values, key
    # the same script is the same run
    again = _checker()
    assert _same(_everything(ck, steps), _everything(again, _play(again)[0]))


def test_episodes_agree_with_the_reference_loop(base):
    """For every env with a limit that the masked reset leaves alone: the rewards and dones its steps returned, through
    src/SAL.py's loop as episodes_cases.reference_loop writes it down, give the records the composed checker logged."""
    ck, steps, fed = base
    checked = 0
    for e in np.flatnonzero((LIMITS > 0) & ~MASK):
        stepped = [k for k, f in enumerate(fed) if not f['fresh'][e] and not f['stood'][e]]
        want = ec.reference_loop([steps[k]['reward'][e] for k in stepped], [fed[k]['done'][e] for k in stepped], int(LIMITS[e]))
        got = [(r[2], r[1], r[3]) for r in ck.episodes.records if r[0] == e]
        assert len(want) >= 2 and got == want, (e, got, want)
        checked += len(want)
    assert checked >= 8


def test_the_ring_agrees_with_fifo_and_holds_the_shapers_values(base):
    """After every push the ring's pushes are deque(maxlen=T)'s; a valid transition holds the reward the shaper paid in that step,
    the image drawn in the step before and the one drawn in this step, the raw action handed to act() and the step's done.  (The
    base run's inputs through a second checker, looked at after each step.)"""
    _, steps, fed = base
    ck = _checker()
    valid_total = limit_valid = 0
    pending = np.zeros(B, bool)
    for k, (s, f) in enumerate(zip(steps, fed)):
        if k not in (0, MASKED_AT):
            ck.act(PUSHES[k]['action'].astype(np.float64))
        mask = np.ones(B, bool) if k == 0 else MASK if k == MASKED_AT else None
        info, reward = ck.after_step(_state(k, f['fresh']), f['clock'], f['done'], (k + np.arange(B)) // 7, pending, f['images'], mask)
        pending = ck.pending_reset.astype(bool)
        held, ids = rc.fifo(T, k + 1)
        assert len(ck.mirror.steps) == held and [c for c, _ in ck.mirror.steps] == ids
        count, rec = ck.mirror.steps[-1]
        assert count == k
        for e in range(B):
            ok = k > 0 and not f['fresh'][e] and not f['stood'][e]
            assert (rec[e] is not None) == ok == bool(info['replay_valid'][e]), (k, e)
            if ok:
                s0, a, r, s1, d = rec[e]
                assert r == reward[e] == s['reward'][e] and d == int(f['done'][e])
                assert np.array_equal(s0, fed[k - 1]['images'][e, AGENT]) and np.array_equal(s1, f['images'][e, AGENT])
                assert np.array_equal(a, PUSHES[k]['action'][e])
                valid_total += 1
                limit_valid += int(info['truncated'][e] and not f['done'][e])
    assert valid_total > 3 * B and limit_valid >= 3                    # LIMIT steps are stored, valid, with d = 0


VARIANTS = {
    'shaper and ring swapped': dict(order=('progress', 'replay', 'follow', 'shaping', 'episodes')),
    'episodes before the shaper': dict(order=('progress', 'episodes', 'shaping', 'follow', 'replay')),
    'image rendered before the shaper reads it': dict(render_first=True),
    'agent 0 instead of 1': dict(agent=0),
    'reset seen late by the tracker': dict(late='progress'),
    'reset seen late by the shaper': dict(late='shaping'),
    'reset seen late by the follower': dict(late='follow'),
    'reset seen late by the ring': dict(late='replay'),
    'reset seen late by the episodes': dict(late='episodes'),
}


@pytest.mark.parametrize('name', list(VARIANTS))
def test_every_variant_is_told_apart(base, name):
    ck, steps, _ = base
    other = _checker(**VARIANTS[name])
    other_steps, _ = _play(other)
    want, got = _everything(ck, steps), _everything(other, other_steps)
    assert not _same(want, got), name
    # and it shows in what the GPU test compares after a step, not only at the end of the run
    first = next((k for k, (x, y) in enumerate(zip(steps, other_steps)) if not _same([x[key] for key in sorted(x)], [y[key] for key in sorted(y)])), None)
    print('%s: first differing step %s' % (name, first))
    assert first is not None, name
