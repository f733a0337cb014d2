"""Replay buffer without a GPU: the checker of tests/replay_cases.py against the reference's recorded ReplayBuffer (g18) and
against itself, and the library's host-only validate entry."""
import numpy as np
import pytest

import replay_cases as rc


def test_mirror_fifo_reproduces_the_reference(golden):
    g = golden('g18_replay.npz')
    assert set(g['capacity'].tolist()) == set(rc.FIFO_CAPACITIES) and len(g['capacity']) == sum(3 * c + 1 for c in rc.FIFO_CAPACITIES)
    for k, (cap, n) in enumerate(zip(g['capacity'], g['pushes'])):
        length, ids = rc.fifo(int(cap), int(n))
        assert length == int(g['length'][k]) and ids == g['ids'][g['offsets'][k]:g['offsets'][k + 1]].tolist(), (cap, n)
    # the Mirror keeps its pushes in the same deque: one env, every transition valid after the first push
    for cap in rc.FIFO_CAPACITIES[1:]:
        for n in (0, 1, cap, cap + 1, 3 * cap):
            m = rc.Mirror(cap, 1, 1, 1, 1, 0.01)
            for i in range(n + 1):
                m.push(np.zeros((1, 1, 1), np.uint8), [[float(i)]], [float(i)], [False], [1.0 + i])
            assert [c - 1 for c, rec in m.steps if rec[0] is not None] == rc.fifo(cap, n)[1], (cap, n)


def test_validate_accepts_and_refuses():
    from red_gym_amd import replay
    replay.validate(6, shaping={}, steps=4, action_dim=16)
    replay.validate(65536, shaping={}, capacity=1000000)
    replay.validate(3, shaping=dict(rows=75, cols=100), steps=2, action_dim=1)
    with pytest.raises(ValueError, match='shaping is off'):
        replay.validate(6, steps=4)
    with pytest.raises(ValueError, match='step slots'):
        replay.validate(6, shaping={}, steps=1)
    with pytest.raises(ValueError, match='step slots'):
        replay.validate(65536, shaping={}, capacity=65536)          # capacity // num_envs = 1
    with pytest.raises(ValueError, match='action_dim'):
        replay.validate(6, shaping={}, steps=4, action_dim=0)
    with pytest.raises(ValueError, match='overflows'):
        replay.validate(2 ** 31 - 1, shaping=dict(rows=16384, cols=16384), steps=2 ** 31 - 2)
    with pytest.raises(ValueError, match='pixels'):
        replay.validate(6, shaping=dict(rows=20000, cols=64), steps=4)


def test_config_errors():
    from red_gym_amd import replay
    with pytest.raises(TypeError, match='unknown replay option'):
        replay.make_config(4, prioritised=True)
    c = replay.make_config(4, capacity=103)
    assert (c.steps, c.action_dim) == (25, 16)
    assert replay.make_config(4, capacity=103, steps=7, action_dim=3).steps == 7
    assert replay.make_config(65536).steps == 1000000 // 65536


@pytest.mark.parametrize('cols', [64, 100, 300, 1])
def test_pack_round_trip(cols):
    rows = 5
    imgs = rc.edge_images(rows, cols)
    p = rc.pack(imgs)
    assert p.shape == (imgs.shape[0], rows, rc.words(cols)) and p.dtype == np.uint64
    assert np.array_equal(rc.unpack(p, cols), np.where(imgs == 255, 255, 0).astype(np.uint8))
    # bit k of word w is pixel 64 w + k; the tail bits are 0
    for c in {0, min(63, cols - 1), min(64, cols - 1), cols - 1}:
        one = np.zeros((1, 1, cols), np.uint8)
        one[0, 0, c] = 255
        w = rc.pack(one)[0, 0]
        assert int(w[c // 64]) == 1 << (c % 64) and int(w.sum()) == 1 << (c % 64)
    full = rc.pack(np.full((1, 1, cols), 255, np.uint8))[0, 0]
    assert sum(bin(int(v)).count('1') for v in full) == cols


def test_draw_stays_inside_its_domain():
    rng = np.random.default_rng(3)
    for T, B, count in ((4, 6, 0), (4, 6, 1), (4, 6, 3), (4, 6, 4), (4, 6, 61), (5, 7, 13), (2, 1, 9), (15, 65536, 40)):
        valid = (rng.uniform(size=(T, B)) < 0.5).astype(np.uint8)
        stored = min(count, T)
        idx, ok, cands = rc.draw(valid, count, 987654321, 17, 64)
        assert all(0 <= c < stored * B for c in cands)
        assert ((idx >= 0) == (ok == 1)).all() and (idx < T * B).all()
        assert all(valid[i // B, i % B] for i in idx[idx >= 0])
        if stored == 0:
            assert (ok == 0).all() and (idx == -1).all() and not cands
        # only step slots that hold a push are drawn
        assert all((i // B) in {(count - 1 - a) % T for a in range(stored)} for i in idx[idx >= 0])
    assert rc.splitmix64(0) == 0 and rc.splitmix64(rc.GOLDEN) == 0xE220A8397B1DCDAF   # the first output of splitmix64 seeded with 0


def test_redraw_finds_a_transition_for_every_draw_of_the_gpu_test():
    c = rc.DRAW_CASE
    valid = rc.draw_case_valid()
    assert valid.shape == (c['T'], c['B']) and 0.2 < 1.0 - valid.mean() < 0.5     # a good share of candidates is refused
    for first in (0, c['n']):                                                    # the GPU test samples twice
        idx, ok, cands = rc.draw(valid, c['count'], c['seed'], first, c['n'])
        assert (ok == 1).all() and len(cands) > c['n']                            # some draws needed a second candidate
    a = rc.draw(valid, c['count'], c['seed'], 0, c['n'])[0]
    b = rc.draw(valid, c['count'], c['seed'], c['n'], c['n'])[0]
    assert not np.array_equal(a, b) and len(set(a.tolist())) > 15
