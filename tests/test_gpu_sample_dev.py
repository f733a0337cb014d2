"""Device-side batch sampling (f110_replay_sample, ReplayBuffer.sample_frames_dev): the draw counter lives on the device, so every
output is compared with the host-counter path at the same draw numbers -- the indices `==` tests/replay_cases.py draw(), everything else
`==` frames_at(indices) -- and a captured sample replays with fresh draws."""
import os

import numpy as np
import pytest

import gpu_checks as gk
import replay_cases as rc

pytestmark = pytest.mark.gpu

NAMES = ('s_idx', 'ns_idx', 'a', 'r', 'd', 'ok')


def _ring(assets, rows=40, cols=30):
    """A ring of DRAW_CASE's shape (T = 5, B = 7) after 13 pushes -- the counter is past one wrap -- with distinct stored actions and
    DRAW_CASE's pattern of invalid slots."""
    import torch
    from red_gym_amd import F110VecEnv, workload
    c = rc.DRAW_CASE
    env = F110VecEnv(c['B'], map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, autoreset=True)
    env.shape_rewards(rows=rows, cols=cols)
    env.record_replay(steps=c['T'])
    env.reset(workload.spawn_poses(c['B'], 1))
    acts = torch.zeros((c['B'], 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for k in range(c['count'] - 1):
        env.replay_action.copy_(torch.arange(c['B'] * 16, device=env.device).reshape(c['B'], 16) + 1000.0 * k)
        env.step(acts)
    pattern = rc.draw_case_valid()
    env.replay.buf['valid'].copy_(torch.as_tensor(pattern))
    assert int(env.replay.buf['count']) == c['count'] > c['T'] and not pattern.all() and pattern.any()
    return env, pattern


def _assert_is_frames_at(rp, got, want_idx):
    """got: sample_frames_dev's result; every output but the indices `==` frames_at(indices)."""
    import torch
    frames, idx = got['frames'], got['indices']
    assert np.array_equal(gk.to_host(idx), want_idx)
    want = rp.frames_at(idx)
    assert frames.data_ptr() == want['frames'].data_ptr() and frames.shape == want['frames'].shape
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), name


def test_two_calls_continue_one_stream_of_draws(assets):
    import torch
    env, pattern = _ring(assets)
    c, rp = rc.DRAW_CASE, env.replay
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    host_before = rp._draws
    first = rp.sample_frames_dev(5, counter, seed=c['seed'])
    second = rp.sample_frames_dev(7, counter, seed=c['seed'])
    _assert_is_frames_at(rp, first, rc.draw(pattern, c['count'], c['seed'], 0, 5)[0])
    _assert_is_frames_at(rp, second, rc.draw(pattern, c['count'], c['seed'], 5, 7)[0])
    assert int(counter) == 12
    assert gk.to_host(first['ok']).all() and gk.to_host(second['ok']).all() and (gk.to_host(first['s_idx']) >= 0).all() and gk.to_host(second['a']).any()
    idx = np.concatenate([gk.to_host(first['indices']), gk.to_host(second['indices'])])
    assert pattern[idx // c['B'], idx % c['B']].all()                                  # no drawn index is invalid
    # the stored action names its env: a[., 0] = 16 env + 1000 k
    assert np.array_equal(gk.to_host(second['a'])[:, 0] % 1000, 16.0 * (gk.to_host(second['indices']) % c['B']))
    # the host counter of draw() has not moved, and draw() does not move the device counter
    assert rp._draws == host_before
    again, _ = rp.draw(5, seed=c['seed'])
    assert np.array_equal(gk.to_host(again), rc.draw(pattern, c['count'], c['seed'], host_before, 5)[0]) and rp._draws == host_before + 5 and int(counter) == 12
    # out=: the static tensors are written and returned; a counter past 2^63 draws on (the bits of a uint64)
    out = rp.sample_out(7)
    counter.fill_(-3)
    got = rp.sample_frames_dev(7, counter, seed=c['seed'], out=out)
    assert all(got[name] is out[name] for name in NAMES) and got['indices'] is out['indices'] and 'frames' not in out
    _assert_is_frames_at(rp, got, rc.draw(pattern, c['count'], c['seed'], 2 ** 64 - 3, 7)[0])
    assert int(counter) == 4
    for bad in (lambda: rp.sample_frames_dev(5, counter.int()), lambda: rp.sample_frames_dev(5, counter.cpu()),
                lambda: rp.sample_frames_dev(5, counter, out=out), lambda: rp.sample_frames_dev(5, torch.zeros(2, dtype=torch.int64, device=env.device))):
        with pytest.raises(ValueError):
            bad()
    assert int(counter) == 4 and env.eng.device_errors() == 0
    env.close()


def test_the_empty_ring(assets):
    import torch
    env, _ = _ring(assets)
    c = rc.DRAW_CASE
    env.record_replay(steps=c['T'])                                                     # a new, empty ring
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    out = env.replay.sample_out(9)
    for t in out.values():
        t.fill_(3)
    got = env.replay.sample_frames_dev(9, counter, out=out)
    s_idx, ns_idx, a, r, d, ok, idx = (got[k] for k in NAMES + ('indices',))
    assert (gk.to_host(idx) == -1).all() and (gk.to_host(s_idx) == -1).all() and (gk.to_host(ns_idx) == -1).all()
    assert not gk.to_host(ok).any() and not gk.to_host(a).any() and not gk.to_host(r).any() and not gk.to_host(d).any() and int(counter) == 9
    env.step(torch.zeros((c['B'], 1, 2), dtype=torch.float64, device=env.device))      # one frame, no transition yet
    assert not gk.to_host(env.replay.sample_frames_dev(9, counter)['ok']).any() and int(counter) == 18
    assert env.eng.device_errors() == 0
    env.close()


def test_a_captured_sample_draws_afresh_at_every_replay(assets):
    """Captured once, replayed three times with n = 256: the batches are the checker's draws at first = 0, 256 and 512 (a counter
    baked into the graph would give the first batch three times), each `==` frames_at; the capture itself draws nothing."""
    import torch
    env, pattern = _ring(assets)
    c, rp = rc.DRAW_CASE, env.replay
    n = c['n']
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    out = rp.sample_out(n)
    out['indices'].fill_(-5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        got = rp.sample_frames_dev(n, counter, seed=c['seed'], out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(counter) == 0 and (gk.to_host(out['indices']) == -5).all()
    batches = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_ok, _ = rc.draw(pattern, c['count'], c['seed'], k * n, n)
        assert want_ok.all()
        _assert_is_frames_at(rp, got, want_idx)
        assert int(counter) == (k + 1) * n
        batches.append(gk.to_host(out['indices']).copy())
    assert not np.array_equal(batches[0], batches[1]) and not np.array_equal(batches[1], batches[2])
    assert env.eng.device_errors() == 0
    env.close()
