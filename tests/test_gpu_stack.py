"""Frame stacks on the device (f110_replay_stack, ReplayBuffer.stack_rows / stack_latest and the stack= option of the sampling calls):
rows and depth `==` the checker of tests/stack_cases.py at every frame row of the scripted rings test_stack_cpu.py takes its census on,
between guards; the latest mode; the refusals; a closed loop in which the newest stacks follow a Python mirror fed what step returned --
through a done, a masked reset, the wrap, restart() and a loaded checkpoint, eager and through both step graphs; a captured walk behind
a captured sample; and the stacks the n-step and the prioritized sample return."""
import os

import numpy as np
import pytest

import gpu_checks as gk
import nstep_cases as nc
import replay_cases as rc
import stack_cases as sc
from test_gpu_nstep import _ring

pytestmark = pytest.mark.gpu

G = nc.GAMMA
BASE = ('frames', 'indices', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok')  # of every batch
STACKED = ('pair', 'stacks', 's_stack', 'ns_stack', 'depth')            # what stack > 1 adds


def _raw_stack(env, rows, n, k):
    """f110_replay_stack itself on guarded outputs -> (rc, rows_out [n, k], depth [n]) as host arrays (the guards are checked)."""
    import torch
    eng = env.eng
    out = gk.Guarded(n * k, dtype=torch.int64, fill=-77)
    depth = gk.Guarded(n, dtype=torch.int32, fill=-77)
    code = eng.lib.f110_replay_stack(eng._h, None if rows is None else rows.data_ptr(), n, k, out.ptr, depth.ptr, eng._stream())
    torch.cuda.synchronize()
    return code, out.read().reshape(n, k), depth.read()


@pytest.mark.parametrize('name', sorted(sc.rings()))
def test_stack_rows_equal_the_checker_at_every_row(assets, name):
    import torch
    valid, dones, rewards, count = sc.rings()[name]
    T, B = valid.shape
    env = _ring(assets, (valid, dones, rewards, count))
    rp = env.replay
    rows = sc.all_rows(T, B)
    dev = gk.to_device(rows)
    for k in sc.STACKS:
        want = sc.stack(valid, count, rows, k)
        code, got_rows, got_depth = _raw_stack(env, dev, len(rows), k)
        assert code == 0 and np.array_equal(got_rows, want['rows']) and np.array_equal(got_depth, want['depth']), (name, k)
        s_rows, depth = rp.stack_rows(rows, k)
        assert s_rows.dtype == torch.int64 and depth.dtype == torch.int32 and tuple(s_rows.shape) == (len(rows), k)
        assert np.array_equal(gk.to_host(s_rows), want['rows']) and np.array_equal(gk.to_host(depth), want['depth'])
        # the latest mode: the checker's, and the stack of the newest frame's row
        code, got_rows, got_depth = _raw_stack(env, None, B, k)
        latest = sc.stack(valid, count, None, k)
        assert code == 0 and np.array_equal(got_rows, latest['rows']) and np.array_equal(got_depth, latest['depth']), (name, k, 'latest')
        l_rows, l_depth = rp.stack_latest(k)
        assert np.array_equal(gk.to_host(l_rows), latest['rows']) and np.array_equal(gk.to_host(l_depth), latest['depth'])
    # the invariant, on the device's own locate: stack(ns)[1:] == stack(s)[:-1] where the stack of s is full
    plain = rp.frames_at(nc.all_indices(T, B))
    frames, s_idx, ns_idx, ok = (plain[f] for f in ('frames', 's_idx', 'ns_idx', 'ok'))
    keep = ok.bool()
    s4, ds = rp.stack_rows(s_idx[keep], 4)
    ns4, dns = rp.stack_rows(ns_idx[keep], 4)
    full = ds == 4
    assert torch.equal(ns4[full][:, 1:], s4[full][:, :-1]) and torch.equal(dns, torch.clamp(ds + 1, max=4)) and bool(keep.any())
    # frames_at(stack=k): the stacks of its own s_idx / ns_idx, everything else unchanged
    got = rp.frames_at(nc.all_indices(T, B), stack=3)
    assert sorted(got) == sorted(BASE + STACKED) and got['frames'].data_ptr() == frames.data_ptr()
    assert all(torch.equal(got[f], plain[f]) for f in ('a', 'r', 'd', 'ok'))
    for pos, (name, col0, idx) in enumerate((('s_stack', 's_idx', s_idx), ('ns_stack', 'ns_idx', ns_idx))):
        want_rows, want_depth = rp.stack_rows(idx, 3)
        assert torch.equal(got[name], want_rows) and torch.equal(got[name][:, 0], idx) and torch.equal(got['depth'][pos], want_depth)
        assert torch.equal(got[col0], idx) and torch.equal(got[col0], got[name][:, 0])
    assert env.eng.device_errors() == 0
    env.close()


def test_refusals_move_nothing(assets):
    import torch
    from red_gym_amd import _lib
    valid, dones, rewards, count = sc.base_ring()
    T, B = valid.shape
    env = _ring(assets, (valid, dones, rewards, count))
    rp, eng = env.replay, env.eng
    rows = torch.arange(5, device=env.device)
    for bad in (lambda: rp.stack_rows(rows, 0), lambda: rp.stack_rows(rows, 9), lambda: rp.stack_rows(rows, 2.0), lambda: rp.stack_rows(rows, True),
                lambda: rp.stack_latest(0), lambda: rp.stack_latest(9), lambda: rp.frames_at(rows, stack=9),
                lambda: rp.stack_latest(3, out=(torch.zeros((B, 2), dtype=torch.int64, device=env.device), torch.zeros((B,), dtype=torch.int32, device=env.device))),
                lambda: rp.sample_frames_dev(5, torch.zeros((1,), dtype=torch.int64, device=env.device), out=rp.sample_out(5), stack=3),
                lambda: rp.sample_out(5, stack=0)):
        with pytest.raises(ValueError):
            bad()
    # the library's own checks, behind the host's: no launch, nothing written
    out = gk.Guarded(5 * 8, dtype=torch.int64, fill=-77)
    depth = gk.Guarded(8, dtype=torch.int32, fill=-77)
    call = lambda r, n, k, o=out.ptr, d=depth.ptr: eng.lib.f110_replay_stack(eng._h, r, n, k, o, d, eng._stream())  # noqa: E731
    for args in ((rows.data_ptr(), 5, 0), (rows.data_ptr(), 5, 9), (rows.data_ptr(), -1, 3), (None, B - 1, 3), (None, B + 1, 3)):
        assert call(*args) == _lib.E_INVALID, args
    assert call(rows.data_ptr(), 5, 3, o=None) == _lib.E_INVALID and call(rows.data_ptr(), 5, 3, d=None) == _lib.E_INVALID
    assert call(rows.data_ptr(), 0, 3) == 0                                       # nothing to do is no error
    torch.cuda.synchronize()
    assert out.untouched() and depth.untouched()
    out.read(), depth.read()
    # without a ring
    env.replay.remove()
    assert call(rows.data_ptr(), 5, 3) != 0
    torch.cuda.synchronize()
    assert out.untouched() and depth.untouched() and env.eng.device_errors() == 0
    env.close()


def test_the_empty_ring_gives_empty_stacks(assets):
    valid, dones, rewards, count = nc.census_ring()
    env = _ring(assets, (valid, dones, rewards, count))
    env.record_replay(steps=valid.shape[0])                                            # a new, empty ring
    rows, depth = env.replay.stack_latest(4)
    assert (gk.to_host(rows) == -1).all() and not gk.to_host(depth).any()
    rows, depth = env.replay.stack_rows(np.arange(-1, 10), 4)
    assert (gk.to_host(rows) == -1).all() and not gk.to_host(depth).any() and env.eng.device_errors() == 0
    env.close()


# ---------------------------------------------------------------------------------------------- the closed loop
class _Mirror:
    """Per env the frames of its running episode as step returned them, newest last: a push that step reports valid continues the
    episode, any other starts one with its own frame; the ring keeps T + 1 frames."""

    def __init__(self, B, T):
        self.T, self.hist = T, [[] for _ in range(B)]

    def push(self, frames, valid):
        for e, h in enumerate(self.hist):
            self.hist[e] = ((h if valid[e] else []) + [frames[e]])[-(self.T + 1):]

    def latest(self, k):
        """(frames [B, k, ...] newest first with the oldest repeated, depth [B])"""
        out, depth = [], []
        for h in self.hist:
            f = h[::-1][:k]
            depth.append(len(f))
            out.append(f + [f[-1]] * (k - len(f)))
        return np.array(out), np.array(depth, np.int32)


@pytest.mark.parametrize('how', ['eager', 'step_graph', 'step_lib_graph'])
def test_the_newest_stacks_follow_a_mirror_through_a_scripted_run(assets, how):
    """6 envs (two spawned across the track and driven at the wall, so that they finish and are reset by the step), T = 5, 60 steps with a
    masked reset, a restart() of the chain and a loaded checkpoint on the way.  After every push, resets included: frames[stack_latest(k)
    [:, 0]] `==` the packed bitmap the step returned, and the whole stack and its depth `==` the mirror's, for k = 1, 4 and 8 (8 > T + 1:
    those stacks end at the ring's oldest frame)."""
    import torch
    from red_gym_amd import F110VecEnv, workload
    B, T, rows, cols = 6, 5, 40, 30
    env = F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, autoreset=True, timestep=0.025)
    env.shape_rewards(rows=rows, cols=cols)
    env.record_replay(steps=T)
    rp = env.replay
    spawn = workload.spawn_poses(B, 1)
    crash = np.arange(B) % 4 == 1
    spawn[crash, 0, 2] += np.pi / 2
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = torch.as_tensor(np.where(crash, 8.0, 2.0), device=env.device)
    mirror = _Mirror(B, T)
    seen = dict(done=0, invalid=0, depths=set(), pushes=0)

    def pushed(res, what):
        _, _, done, info = res
        torch.cuda.synchronize()
        bitmap = info['lidar_bitmap']
        packed = rc.pack(gk.to_host(bitmap)) if bitmap.dtype == torch.uint8 else gk.to_host(bitmap).view(np.uint64)
        valid = gk.to_host(info['replay_valid'])
        mirror.push(packed, valid)
        seen['done'] += int(gk.to_host(done).sum())
        seen['invalid'] += int((valid == 0).sum())
        seen['pushes'] += 1
        frames = gk.to_host(rp.frame_view()).view(np.uint64)
        for k in (1, 4, 8):
            s_rows, depth = rp.stack_latest(k)
            s_rows, depth = gk.to_host(s_rows), gk.to_host(depth)
            want, want_depth = mirror.latest(k)
            assert np.array_equal(frames[s_rows[:, 0]], packed), (what, k)
            assert np.array_equal(depth, want_depth) and np.array_equal(frames[s_rows], want), (what, k, depth, want_depth)
            seen['depths'].update(depth.tolist())

    def graphs():
        if how == 'step_graph':
            env.capture_step()
        elif how == 'step_lib_graph':
            env.build_step_graph()

    pushed(env.reset(spawn), 'reset')
    graphs()
    stepper = env.step if how == 'eager' else getattr(env, how)
    sd = None
    for k in range(60):
        if k == 10:
            sd = env.state_dict()
        if k == 20:
            pushed(env.reset(spawn, torch.as_tensor((np.arange(B) % 2 == 0).astype(np.uint8))), 'masked reset')
        if k == 30:
            rp.restart()
        if k == 40:
            env.load_state_dict(sd)                                                     # (the chain of frames breaks: restart())
            graphs()
        pushed(stepper(acts), 'step %d' % k)
    print(how, seen)
    assert seen['done'] > 0 and seen['pushes'] == 62 and seen['invalid'] >= 4 * B and seen['depths'] == {1, 2, 3, 4, 5, 6}
    assert int(rp.buf['count']) == 62 and env.eng.device_errors() == 0
    env.close()


# ---------------------------------------------------------------------------------------------- behind the samples
def _assert_stacks(rp, ring, got, k, nstep):
    """got: a sampling call's batch with stack = k: 's_stack' and 'ns_stack' `==` the checker's stacks of the rows the plain call gives for
    the same indices, and `==` stack_rows of them; 's_idx' and 'ns_idx' are those rows, column 0 of the stacks; 'depth' is beside them."""
    import torch
    valid, dones, rewards, count = ring
    idx = got['indices']
    plain = rp.frames_at(idx, nstep=nstep, gamma=G if nstep > 1 else None)
    depth = got['depth']
    for pos, (name, col0) in enumerate((('s_stack', 's_idx'), ('ns_stack', 'ns_idx'))):
        want = sc.stack(valid, count, gk.to_host(plain[col0]), k)
        assert np.array_equal(gk.to_host(got[name]), want['rows']) and np.array_equal(gk.to_host(depth[pos]), want['depth'])
        again = rp.stack_rows(plain[col0], k)
        assert torch.equal(got[name], again[0]) and torch.equal(depth[pos], again[1]) and torch.equal(got[name][:, 0], plain[col0])
        assert torch.equal(got[col0], plain[col0]) and torch.equal(got[col0], got[name][:, 0])
    assert all(torch.equal(got[f], plain[f]) for f in ('a', 'r', 'd', 'ok'))


def test_a_captured_walk_behind_a_captured_sample(assets):
    """Captured once, replayed three times with n = 256 at stack = 4: the batches are the checker's draws at first = 0, 256 and 512 and the
    stacks of each `==` the checker; the capture itself draws nothing."""
    import torch
    ring = sc.base_ring()
    valid, count = ring[0], ring[3]
    env = _ring(assets, ring)
    rp, seed, n, k = env.replay, rc.DRAW_CASE['seed'], 256, 4
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    out = rp.sample_out(n, stack=k)
    assert sorted(out) == sorted(list(rp.sample_out(n)) + ['pair', 'stacks', 's_stack', 'ns_stack', 'depth'])
    out['indices'].fill_(-5)
    out['stacks'].fill_(-5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        got = rp.sample_frames_dev(n, counter, seed=seed, out=out, stack=k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(counter) == 0 and (gk.to_host(out['indices']) == -5).all() and (gk.to_host(out['stacks']) == -5).all()
    assert sorted(got) == sorted(BASE + STACKED) and 'frames' not in out and all(got[f] is out[f] for f in out)
    depths = set()
    for u in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_ok, _ = rc.draw(valid, count, seed, u * n, n)
        assert want_ok.all() and np.array_equal(gk.to_host(got['indices']), want_idx) and int(counter) == (u + 1) * n
        _assert_stacks(rp, ring, got, k, 1)
        assert torch.equal(out['s_idx'], out['s_stack'][:, 0]) and torch.equal(out['ns_idx'], out['ns_stack'][:, 0])
        depths.update(gk.to_host(got['depth']).reshape(-1).tolist())
    assert depths == {1, 2, 3, 4} and env.eng.device_errors() == 0
    # uncaptured, without out=: the same draws at the same counter
    counter.zero_()
    fresh = rp.sample_frames_dev(n, counter, seed=seed, stack=k)
    assert np.array_equal(gk.to_host(fresh['indices']), rc.draw(valid, count, seed, 0, n)[0])
    _assert_stacks(rp, ring, fresh, k, 1)
    env.close()


def test_the_stacks_of_the_nstep_and_the_prioritized_sample(assets):
    """With nstep = 3 the stack of ns_idx is the stack of the span's end; with priorities the same behind f110_priority_sample."""
    import torch
    ring = sc.base_ring()
    env = _ring(assets, ring)
    rp, seed, n, k = env.replay, rc.DRAW_CASE['seed'], 64, 3
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    got = rp.sample_frames_dev(n, counter, seed=seed, nstep=3, gamma=G, stack=k)
    assert sorted(got) == sorted(BASE + ('discount', 'span') + STACKED) and int(counter) == n and bool((got['span'] > 1).any())
    _assert_stacks(rp, ring, got, k, 3)
    at = rp.frames_at(got['indices'], nstep=3, gamma=G, stack=k)
    assert sorted(at) == sorted(got) and all(torch.equal(at[f], got[f]) for f in ('s_stack', 'ns_stack', 'depth', 's_idx', 'ns_idx'))
    rp.set_priorities(True)
    for nstep in (1, 3):
        got = rp.sample_priority_dev(n, counter, seed=seed, nstep=nstep, gamma=G, stack=k)
        assert sorted(got) == sorted(BASE + ('discount', 'span', 'prio', 'weight') + STACKED) and bool(got['ok'].all())
        _assert_stacks(rp, ring, got, k, nstep)
        plain = rp.sample_out(n, nstep, priorities=True, stack=k)
        assert sorted(plain) == sorted(list(rp.sample_out(n, nstep, priorities=True)) + ['pair', 'stacks', 's_stack', 'ns_stack', 'depth'])
    assert env.eng.device_errors() == 0
    env.close()
