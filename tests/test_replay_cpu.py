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


def test_shape_table_covers_every_size_selected_path():
    """SHAPES (what the GPU tests run) against paths(), the header's arithmetic restated: every pack branch with one pass and
    with several whose last is partial, both unpack forms with one pass and with at least two, the rows either side of a gather
    block (REPLAY_ROWS = 16) and several blocks."""
    assert len(set(rc.SHAPES)) == len(rc.SHAPES)
    p = {s: rc.paths(*s) for s in rc.SHAPES}
    for branch in ('dense', 'aligned', 'bytewise'):
        mine = [v for v in p.values() if v['pack'] == branch]
        assert any(v['pack_passes'] == 1 for v in mine), branch
        assert any(v['pack_passes'] > 1 and v['pack_last_partial'] for v in mine), branch
    for form in ('vec4', 'scalar'):
        mine = [v for v in p.values() if v['unpack'] == form]
        assert any(v['unpack_passes'] == 1 for v in mine) and any(v['unpack_passes'] >= 2 for v in mine), form
    rows = {r for r, _ in rc.SHAPES}
    assert {1, 15, 16, 17} <= rows and max(rows) > 32
    assert {p[s]['row_blocks'] for s in ((15, 15), (16, 96), (17, 16), (33, 48))} == {1, 2, 3}
    # paths() on sizes worked out by hand from csrc/f110_replay.h
    assert rc.paths(256, 256) == dict(pack='dense', pack_passes=4, pack_last_partial=False, unpack='vec4', unpack_passes=1, row_blocks=16)
    assert rc.paths(224, 224) == dict(pack='aligned', pack_passes=4, pack_last_partial=True, unpack='vec4', unpack_passes=1, row_blocks=14)
    assert rc.paths(75, 320) == dict(pack='dense', pack_passes=2, pack_last_partial=True, unpack='vec4', unpack_passes=2, row_blocks=5)
    assert rc.paths(9, 257) == dict(pack='bytewise', pack_passes=1, pack_last_partial=True, unpack='scalar', unpack_passes=5, row_blocks=1)
    assert rc.paths(84, 84) == dict(pack='bytewise', pack_passes=3, pack_last_partial=True, unpack='vec4', unpack_passes=1, row_blocks=6)
    assert rc.paths(40, 1028)['unpack_passes'] == 5 and rc.paths(20, 272)['pack'] == 'aligned' and rc.paths(20, 272)['unpack_passes'] == 2


def test_scripted_pushes_exercise_the_ring():
    """The ring's run on frames the test writes (test_gpu_replay.py), on the mirror alone: its sizes cover every pack branch and
    both unpack forms with one pass and with several, every frame holds both values, no env repeats a frame, and the ring comes
    to hold invalid transitions (a clock that stands still, a reset) and terminal ones."""
    assert set(rc.RING_SHAPES) <= set(rc.SHAPES) and {(224, 224), (20, 272), (84, 84), (9, 257), (40, 1028)} <= set(rc.RING_SHAPES)
    p = [rc.paths(*s) for s in rc.RING_SHAPES]
    assert {(v['pack'], v['pack_passes'] > 1) for v in p} == {(b, m) for b in ('dense', 'aligned', 'bytewise') for m in (False, True)}
    assert {(v['unpack'], v['unpack_passes'] > 1) for v in p} == {(f, m) for f in ('vec4', 'scalar') for m in (False, True)}
    assert {1, 15, 16, 17} <= {r for r, _ in rc.RING_SHAPES}
    B, T, dt = 5, 3, 0.01
    for rows, cols in rc.RING_SHAPES:
        m = rc.Mirror(T, B, rows, cols, 16, dt)
        pushes = rc.scripted_pushes(rows, cols, B, T, 16, dt)
        assert len(pushes) == 2 * T + 3
        prev, invalid, terminal = None, 0, 0
        for k, q in enumerate(pushes):
            f = rc.binary(q['frame'])
            assert all((f[e] == 0).any() and (f[e] == 255).any() for e in range(B))
            assert prev is None or all((f[e] != prev[e]).any() for e in range(B))
            v = m.push(f, q['action'], q['reward'], q['done'], q['clock'])
            assert not v.any() if k == 0 else v.sum() >= B - 1
            if k:
                invalid += int((v == 0).sum())
                terminal += int((v & q['done']).sum())
            prev = f
        assert invalid == 2 and terminal == 3 and m.count == 2 * T + 3
        assert all(((q['frame'] != 0) & (q['frame'] != 255)).any() for q in pushes)   # raw bytes: only 255 is a set bit
    a = np.stack([q['action'] for q in rc.scripted_pushes(3, 64, B, T, 300, dt)])
    assert a.dtype == np.float32 and np.unique(a).size == a.size                  # arange-distinct, exact in fp32


@pytest.mark.parametrize('rows,cols', rc.SHAPES)
def test_pack_round_trip_at_every_shape(rows, cols):
    for imgs in (rc.edge_images(rows, cols), rc.random_images(rows, cols)):
        p = rc.pack(imgs)
        assert p.shape == (imgs.shape[0], rows, rc.words(cols))
        assert np.array_equal(rc.unpack(p, cols), np.where(imgs == 255, 255, 0).astype(np.uint8))
        # the padding bits of a row's last word are 0
        if cols % 64:
            assert not (p[:, :, -1] >> np.uint64(cols % 64)).any()
    r = rc.random_images(rows, cols)
    assert r.shape[0] == 7 and all((im == 254).any() and (im == 127).any() and (im == 255).any() for im in r)
    assert 0.2 < (r == 255).mean() < 0.4


def test_draw_is_uniform_over_the_valid_transitions():
    """sample() promises a uniform draw over the valid transitions.  The GPU's draw `==` this checker bit for bit
    (test_gpu_replay.py), so the distribution is checked here: 20 000 draws on DRAW_CASE's pattern, Pearson's statistic over its
    26 valid transitions inside the central 99.8 % of chi-square with 25 degrees of freedom (8.65 .. 52.62)."""
    from scipy.stats import chi2
    c = rc.DRAW_CASE
    valid = rc.draw_case_valid()
    n = 20000
    idx, ok, _ = rc.draw(valid, c['count'], c['seed'], 0, n)
    assert (ok == 1).all()
    hist = np.bincount(idx, minlength=valid.size).reshape(valid.shape)
    assert not hist[valid == 0].any()                                             # no invalid index is drawn
    k = int(valid.sum())
    assert k == 26
    expected = n / k
    stat = float(((hist[valid == 1] - expected) ** 2 / expected).sum())
    lo, hi = chi2.ppf(0.001, k - 1), chi2.ppf(0.999, k - 1)
    print('Pearson statistic %.2f over %d cells, bounds %.2f .. %.2f' % (stat, k, lo, hi))
    assert lo < stat < hi
