"""The n-step walk's checker (tests/nstep_cases.py) without a GPU: the contract over the ring's arrays `==` the brute-force statement over
per-env episodes, on scripted rings and on a replay_cases.Mirror fed scripted_pushes; nstep = 1 `==` the one-step quantities; and the
census of the base ring -- every way a span ends, both seams -- counted from the checker alone, before anything is compared with it
(tests/test_gpu_nstep.py runs the kernels on the same rings).  Then the ABI's refusals, which need no device."""
import collections
import ctypes as C

import numpy as np
import pytest

import nstep_cases as nc
import qhead_cases as qc
import replay_cases as rc

F = ('ns_frame', 'ret', 'd', 'discount', 'span')


def _same(a, b):
    """Raw bits (a NaN or a signed zero would show)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_census_of_the_base_ring():
    """From walk() alone, at nstep = 3: at least three transitions for each way a span ends, a span across the step-slot seam T - 1 -> 0
    and one whose frame after lies across the frame-slot seam T -> 0."""
    valid, dones, rewards, count = nc.census_ring()
    T, B = valid.shape
    assert (T, B, count) == (rc.DRAW_CASE['T'], rc.DRAW_CASE['B'], rc.DRAW_CASE['count']) and count > T
    w = nc.walk(valid, dones, rewards, count, np.arange(T * B), 3, nc.GAMMA)
    ends = collections.Counter(e for e in w['end'] if e)
    print(dict(ends))
    assert set(ends) == set(nc.ENDS) and all(ends[e] >= 3 for e in nc.ENDS), ends
    assert sum(ends.values()) == int(valid.sum()) == int((w['span'] > 0).sum())
    live = w['span'] > 0
    c0, last = w['c0'][live], w['c0'][live] + w['span'][live] - 1
    assert ((c0 % T) > (last % T)).any()                              # a span that leaves step slot T - 1 for 0
    assert ((c0 % (T + 1)) > (last % (T + 1))).any()                  # a frame after that lies behind frame slot T, in 0
    assert not np.array_equal(c0 % T > last % T, c0 % (T + 1) > last % (T + 1))   # the two seams lie apart: the moduli differ
    assert set(w['span'][live].tolist()) == {1, 2, 3} and set(w['d'][live].tolist()) == {0, 1}
    # the running product: gamma, gamma * gamma, (gamma * gamma) * gamma
    g = np.float64(nc.GAMMA)
    assert set(w['discount'].tolist()) == {g, g * g, g * g * g}


@pytest.mark.parametrize('name', sorted(nc.rings()))
def test_walk_equals_brute_force_on_scripted_rings(name):
    valid, dones, rewards, count = nc.rings()[name]
    T, B = valid.shape
    assert {'census': count > T, 'not_wrapped': count < T, 'two_wraps': count == 2 * T + 1}[name]
    idx = nc.all_indices(T, B)
    pushes = nc.pushes_of_arrays(valid, dones, rewards, count)
    for nstep in nc.NSTEPS:
        w = nc.walk(valid, dones, rewards, count, idx, nstep, nc.GAMMA)
        b = nc.brute(pushes, T, B, idx, nstep, nc.GAMMA)
        assert all(_same(w[k], b[k]) for k in F), (name, nstep, [k for k in F if not _same(w[k], b[k])])
        assert w['span'][0] == 0 and w['span'][-1] == 0 and (w['span'] <= nstep).all()
        assert (w['span'][1:-1] > 0).any() and ((w['span'] > 0) == (w['ns_frame'] >= 0)).all()
        # a refused row is the zero transition with discount = gamma
        dead = w['span'] == 0
        assert (w['ns_frame'][dead] == -1).all() and not w['ret'][dead].any() and not w['d'][dead].any() and _same(w['discount'][dead], np.full(dead.sum(), nc.GAMMA))
    longest = nc.walk(valid, dones, rewards, count, idx, 64, nc.GAMMA)['span'].max()
    assert longest <= min(count, T) and (name != 'census' or longest == T)


@pytest.mark.parametrize('name', sorted(nc.rings()))
def test_nstep_1_is_the_one_step_transition(name):
    valid, dones, rewards, count = nc.rings()[name]
    T, B = valid.shape
    idx = nc.all_indices(T, B)
    w = nc.walk(valid, dones, rewards, count, idx, 1, nc.GAMMA)
    o = nc.one_step(valid, dones, rewards, count, idx)
    assert _same(w['ns_frame'], o['ns_frame']) and _same(w['ret'], o['r']) and _same(w['d'], o['d']) and _same((w['span'] > 0).astype(np.uint8), o['ok'])
    assert _same(w['discount'], np.full(len(idx), nc.GAMMA)) and set(w['span'].tolist()) == {0, 1}


@pytest.mark.parametrize('pushes', [3, 6, 9, 13])
def test_walk_equals_brute_force_on_the_mirror(pushes):
    """The ring as the reference would keep it (a deque of pushes) after 3, 6, 9 and 2 T + 3 scripted pushes of T = 5, B = 6: the arrays
    the device holds are rebuilt from the pushes' own valid flags; the brute force reads the deque."""
    T, B, ts = 5, 6, 0.01
    m = rc.Mirror(T, B, 4, 5, 3, ts)
    valid, dones, rewards = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8), np.zeros((T, B))
    script = rc.scripted_pushes(4, 5, B, T, 3, ts)
    assert len(script) == 2 * T + 3
    for k, p in enumerate(script[:pushes]):
        slot = m.count % T
        valid[slot] = m.push(p['frame'], p['action'], p['reward'], p['done'], p['clock'])
        dones[slot], rewards[slot] = p['done'], p['reward']
    assert np.array_equal(valid, m.valid_array()) and valid.any() and (pushes == 13 or not valid.all())   # (the scripted invalid pushes are 0, 3 and 5)
    idx = nc.all_indices(T, B)
    for nstep in nc.NSTEPS:
        w = nc.walk(valid, dones, rewards, m.count, idx, nstep, nc.GAMMA)
        b = nc.brute(nc.pushes_of_mirror(m), T, B, idx, nstep, nc.GAMMA)
        assert all(_same(w[k], b[k]) for k in F), (pushes, nstep)
        # and the mirror's own one-step answer where the span is one
        _, _, r, _, d, ok = m.at(idx)
        one = w['span'] == 1
        assert _same((w['span'] > 0).astype(np.uint8), ok) and _same(w['ret'][one], r[one]) and _same(w['d'][one], d[one])


def test_target_rows_with_gamma_is_the_one_step_target():
    """target_rows with discount[b] = gamma `==` qc.forward's target; another discount changes the rows that are not done, and only those."""
    for shape in qc.FORWARD_SHAPES[:5]:
        inp = qc.inputs(*shape)
        n = shape[0]
        for fp32 in (False, True):
            want = qc.forward(inp, fp32_action=fp32, gamma=nc.GAMMA, alpha=0.2)['target']
            got, _ = nc.target_rows(inp, np.full(n, nc.GAMMA), 0.2, fp32_action=fp32)
            assert _same(got, want), shape
        other, _ = nc.target_rows(inp, np.full(n, nc.GAMMA) ** 3, 0.2)
        moved = other != qc.forward(inp, gamma=nc.GAMMA, alpha=0.2)['target']
        assert not moved[inp['done'] == 1].any() and (n < 2 or moved[inp['done'] == 0].any())


def test_mirror_and_constants():
    from red_gym_amd import _lib, replay
    assert _lib.F110_REPLAY_MAX_NSTEP == nc.MAX_NSTEP == replay.MAX_NSTEP == max(nc.NSTEPS)
    for name in ('f110_replay_nstep', 'f110_replay_sample_nstep', 'f110_qhead_forward_rows'):
        assert name in _lib.SYMBOLS


def test_refusals_need_no_device():
    """A null handle, and for the critic head what is refused on the arguments alone, come back as F110_E_INVALID without a launch."""
    from red_gym_amd import _lib, build, qhead
    build.build()
    lib = _lib.load()
    one = 4096                                   # never dereferenced
    assert lib.f110_replay_nstep(None, one, 4, 3, 0.99, one, one, one, one, one, None) == _lib.E_INVALID and b'null handle' in lib.f110_last_error()
    assert lib.f110_replay_sample_nstep(None, 0, one, 4, 3, 0.99, one, one, one, one, one, one, one, one, one, None) == _lib.E_INVALID
    cfg = qhead.make_config(8, 2, 2)
    p = _lib.QheadCritics()
    for c in range(2):
        p.pre[c], p.w_act[c], p.w2[c] = one, one, one
    rows = lambda discount, alpha, alpha_dev, target=one: lib.f110_qhead_forward_rows(  # noqa: E731
        C.byref(cfg), C.byref(p), one, 4, one, one, one, discount, alpha, alpha_dev, one, None, target, None)
    assert rows(None, 0.2, None) == _lib.E_INVALID and b'null discount' in lib.f110_last_error()
    assert rows(one, float('nan'), None) == _lib.E_INVALID and b'not finite' in lib.f110_last_error()
