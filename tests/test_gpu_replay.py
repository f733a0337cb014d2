"""Replay buffer on the GPU (csrc/f110_replay.h): every output `==` the checker of tests/replay_cases.py -- NumPy's packbits,
the splitmix64 draw in Python ints, and a mirror of the ring on collections.deque fed what step() returned."""
import os

import numpy as np
import pytest

import gpu_checks as gk
import replay_cases as rc
import shaping_cases as sc

pytestmark = pytest.mark.gpu

def _env(assets, B, A=1, **kw):
    from red_gym_amd import F110VecEnv
    return F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=A, **kw)


def _packed_u64(t):
    return np.ascontiguousarray(gk.to_host(t)).view(np.uint64)


@pytest.mark.parametrize('rows,cols,group', [(256, 256, 'a'), (75, 100, 'b'), (40, 300, 'c'), (3, 1, None)] + [s + (None,) for s in rc.SHAPES])
def test_pack_and_unpack_equal_numpy(golden, rows, cols, group):
    """f110_replay_pack / _unpack `==` np.packbits(bitorder='little') on 5 FILL images of g16, on the edge images and on 7
    images of arbitrary bytes (a batch that is neither one image nor a multiple of 4), at the sizes of g16 and at every size of
    rc.SHAPES: each branch of replay_pack_image and each form of replay_unpack_row with one pass and with several."""
    import torch
    from red_gym_amd import replay
    batches = [rc.edge_images(rows, cols), rc.random_images(rows, cols)]
    assert batches[1].shape[0] == 7
    if group is not None:
        imgs = sc.unpack_images(golden('g16_shaping.npz'), group)
        assert imgs.shape[1:] == (rows, cols)
        filled = (imgs.reshape(imgs.shape[0], -1) == 255).sum(axis=1)
        batches.append(imgs[np.argsort(-filled, kind='stable')[:5]])          # the five fullest (many of 40 x 300's are empty)
        assert batches[-1].shape[0] == 5 and all(im.max() == 255 for im in batches[-1])
    for imgs in batches:
        dev = torch.as_tensor(imgs, device='cuda')
        packed = replay.pack_bitmaps(dev)
        want = rc.pack(imgs)
        assert packed.shape == want.shape
        bad = int((_packed_u64(packed) != want).sum())
        print('%d x %d, %d images: %d differing words' % (rows, cols, imgs.shape[0], bad))
        assert bad == 0
        back = gk.to_host(replay.unpack_bitmaps(packed, cols))
        assert np.array_equal(back, rc.unpack(want, cols)) and np.array_equal(back, np.where(imgs == 255, 255, 0).astype(np.uint8))


def _assert_batch(got, want, what):
    names = ('s', 'a', 'r', 'ns', 'd', 'ok')
    bad = {k: int((gk.to_host(g) != w).sum()) for k, g, w in zip(names, got, want)}
    print(what, 'differing elements:', bad, 'valid:', int(want[5].sum()))
    assert not any(bad.values()), (what, bad)


@pytest.mark.parametrize('rows,cols', [(256, 256), (75, 100)])
def test_closed_loop_equals_mirror_through_resets(assets, rows, cols):
    """6 envs (every fourth spawned across the track and driven at the wall), T = 4, 60 steps with autoreset, random raw
    actions through path_actions and a masked reset of half the envs in the middle: after every step replay_valid `==` the
    mirror's decision, every 7 steps sample_at(all T * B indices) `==` the mirror -- and what is compared there holds something:
    every stored s has pixels of both values, and s != ns for at least half of the valid transitions.  (Time step 0.025 s: from
    a standing start a car needs about a second to reach the wall across the track, and the run has 60 steps.)"""
    import torch
    from red_gym_amd import workload
    B, T, AD = 6, 4, 16
    env = _env(assets, B, autoreset=True, timestep=0.025)
    env.shape_rewards(rows=rows, cols=cols)
    env.follow_paths()
    env.record_replay(capacity=T * B + 3, action_dim=AD)
    assert env.replay.steps == T and len(env.replay) == 0
    mirror = rc.Mirror(T, B, rows, cols, AD, env.timestep)
    spawn = workload.spawn_poses(B, 1)
    crash = np.arange(B) % 4 == 1
    spawn[crash, 0, 2] += np.pi / 2
    crash_dev = torch.as_tensor(crash, device=env.device)
    rng = np.random.default_rng(18)
    all_idx = torch.arange(T * B, device=env.device)
    raw = np.zeros((B, AD))
    autoresets, checks = 0, 0

    def pushed(res, what):
        _, reward, done, info = res
        torch.cuda.synchronize()
        clock = gk.to_host(info['current_time'])
        want = mirror.push(gk.to_host(info['lidar_bitmap']), raw.astype(np.float32), gk.to_host(reward), gk.to_host(done), clock)
        assert info['lidar_bitmap'].shape == (B, rows, cols)
        assert np.array_equal(gk.to_host(info['replay_valid']), want), (what, gk.to_host(info['replay_valid']), want)
        assert int(info['replay_count']) == mirror.count
        return clock, want

    clock, valid = pushed(env.reset(spawn), 'reset')
    assert not valid.any()
    for k in range(60):
        if k == 30:
            mask = (np.arange(B) % 2 == 0).astype(np.uint8)
            before = clock
            clock, valid = pushed(env.reset(spawn, torch.as_tensor(mask)), 'masked reset')
            assert not valid[mask == 1].any() and not valid[clock == before].any()
        else:
            raw = rng.uniform(-1.0, 1.0, (B, AD))
            acts = env.path_actions(torch.as_tensor(raw, device=env.device))
            acts[:, 0, 0] = torch.where(crash_dev, 0.0, acts[:, 0, 0])
            acts[:, 0, 1] = torch.where(crash_dev, 8.0, acts[:, 0, 1])
            clock, valid = pushed(env.step(acts), 'step %d' % k)
            autoresets += int((clock == env.timestep).sum())
            assert not valid[clock == env.timestep].any()
        if k % 7 == 6 or k == 59:
            want = mirror.at(range(T * B))
            _assert_batch(env.replay.sample_at(all_idx), want, 'after step %d' % k)
            assert len(env.replay) == len(mirror)
            # what is compared holds something: every stored s has both values, and most transitions change the image
            held = np.flatnonzero(want[5])
            moved = sum(bool((want[0][i] != want[3][i]).any()) for i in held)
            both = sum(bool((want[0][i] == 0).any() and (want[0][i] == 255).any()) for i in held)
            print('after step %d: %d valid, s != ns in %d, s holds 0 and 255 in %d' % (k, held.size, moved, both))
            assert held.size > 0 and 2 * moved >= held.size and both == held.size
            checks += 1
    print('autoresets: %d, pushes: %d, valid held: %d, terminal transitions held: %d'
          % (autoresets, mirror.count, len(mirror), int(mirror.at(range(T * B))[4].sum())))
    assert autoresets > 0, 'no autoreset happened'
    assert mirror.count > 2 * T and checks >= 8                                    # the ring wrapped many times
    # -1 and indices beyond the ring: zeros and ok = 0
    odd = [-1, T * B, 2 ** 40, -7]
    _assert_batch(env.replay.sample_at(torch.as_tensor(odd)), mirror.at(odd), 'odd indices')
    assert env.eng.device_errors() == 0
    env.close()


def _filled_env(assets, B=6, T=4, steps=9, **kw):
    """An env with shaper and replay on after `steps` zero-action steps with distinct stored actions."""
    import torch
    from red_gym_amd import workload
    env = _env(assets, B, autoreset=True)
    env.shape_rewards(**kw)
    env.record_replay(steps=T)
    env.reset(workload.spawn_poses(B, 1))
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for k in range(steps):
        env.replay_action.copy_(torch.arange(B * 16, device=env.device).reshape(B, 16) + 1000.0 * k)
        env.step(acts)
    return env, acts


def test_sample_equals_the_checkers_draw(assets):
    import torch
    env, _ = _filled_env(assets)
    rp = env.replay
    B, T = 6, 4
    # (a) the ring as the run left it: every transition of the last T steps is valid
    valid = gk.to_host(rp.buf['valid'])
    count = int(rp.buf['count'])
    assert count == 10 and valid.all()
    idx, ok = rp.draw(256, seed=77)
    want_idx, want_ok, _ = rc.draw(valid, count, 77, 0, 256)
    assert np.array_equal(gk.to_host(idx), want_idx) and np.array_equal(gk.to_host(ok), want_ok) and want_ok.all()
    # (b) the synthetic pattern whose redraw condition the CPU suite has checked: a ring of DRAW_CASE's shape
    env.close()
    c = rc.DRAW_CASE
    env, _ = _filled_env(assets, B=c['B'], T=c['T'], steps=c['count'] - 1)
    rp = env.replay
    assert int(rp.buf['count']) == c['count']
    pattern = rc.draw_case_valid()
    rp.buf['valid'].copy_(torch.as_tensor(pattern))
    s, a, r, ns, d, ok = rp.sample(c['n'], seed=c['seed'])
    first = gk.to_host(rp._keep)
    want_idx, want_ok, _ = rc.draw(pattern, c['count'], c['seed'], 0, c['n'])
    assert np.array_equal(first, want_idx) and gk.to_host(ok).all() and want_ok.all()
    assert pattern[first // c['B'], first % c['B']].all()                            # no drawn index is invalid
    assert s.shape == (c['n'], 256, 256) and s.dtype == torch.uint8 and a.shape == (c['n'], 16) and r.dtype == torch.float64
    # the stored action names its env and step: a[., 0] = 16 env + 1000 k
    slot, e = first // c['B'], first % c['B']
    assert np.array_equal(gk.to_host(a)[:, 0] % 1000, 16.0 * e)
    rp.sample(c['n'], seed=c['seed'])
    second = gk.to_host(rp._keep)
    assert np.array_equal(second, rc.draw(pattern, c['count'], c['seed'], c['n'], c['n'])[0]) and not np.array_equal(first, second)
    # (c) an empty buffer: every draw reports ok = 0
    env.record_replay(steps=c['T'])
    s, a, r, ns, d, ok = env.replay.sample(64)
    assert not gk.to_host(ok).any() and (gk.to_host(env.replay._keep) == -1).all() and not gk.to_host(s).any() and not gk.to_host(ns).any()
    env.step(torch.zeros((c['B'], 1, 2), dtype=torch.float64, device=env.device))     # one frame, no transition yet
    assert not gk.to_host(env.replay.sample(64)[5]).any() and len(env.replay) == 0
    assert env.eng.device_errors() == 0
    env.close()


@pytest.mark.parametrize('rows,cols', [(256, 256), (75, 100), (40, 30)])
def test_fp32_output(assets, rows, cols):
    import torch
    env, _ = _filled_env(assets, rows=rows, cols=cols)
    idx = torch.as_tensor([0, 5, 23, -1, 11, 17], device=env.device)
    s8, a8, r8, ns8, d8, ok8 = env.replay.sample_at(idx)
    for scale in (1.0, 1.0 / 255.0, 0.3):
        s, a, r, ns, d, ok = env.replay.sample_at(idx, dtype=torch.float32, scale=scale)
        assert s.shape == ns.shape == (6, 1, rows, cols) and s.dtype == torch.float32
        assert torch.equal(s, (s8.float() * scale).unsqueeze(1)) and torch.equal(ns, (ns8.float() * scale).unsqueeze(1))
        assert torch.equal(a, a8) and torch.equal(r, r8) and torch.equal(d, d8) and torch.equal(ok, ok8)
    assert gk.to_host(ok8).tolist() == [1, 1, 1, 0, 1, 1] and int(s8.max()) == 255 and not gk.to_host(s8[3]).any()
    env.close()


def test_graph_replays_leave_the_same_ring_as_eager_steps(assets):
    """capture_step + step_graph and build_step_graph + step_lib_graph over 12 steps: the same ring and counter as eager
    stepping -- the slot comes from the device-side counter, not from the host."""
    import torch
    from red_gym_amd import workload
    B, A, T = 8, 2, 5
    env = _env(assets, B, A, autoreset=True)
    env.shape_rewards()
    env.reset(workload.spawn_poses(B, A))
    pool = workload.action_pool(16, B, A)
    for k in range(3):
        env.step(pool[k])
    sd = env.state_dict()
    rings = {}
    for how in ('eager', 'step_graph', 'step_lib_graph'):
        env.load_state_dict(sd)
        env.record_replay(steps=T, action_dim=3)
        if how == 'step_graph':
            env.capture_step()
        elif how == 'step_lib_graph':
            env.build_step_graph()
        stepper = env.step if how == 'eager' else getattr(env, how)
        for k in range(3, 15):
            env.replay_action.fill_(float(k))
            _, _, _, info = stepper(pool[k])
            assert 'replay_count' in info
        torch.cuda.synchronize()
        rings[how] = env.replay.save()
        assert int(rings[how]['count']) == 12 and len(env.replay) > 0
    for how in ('step_graph', 'step_lib_graph'):
        for k, v in rings['eager'].items():
            assert torch.equal(v, rings[how][k]), (how, k)
    assert env.eng.device_errors() == 0
    env.close()


def test_switching_off_save_load_and_checkpoints(assets):
    import torch
    from red_gym_amd import workload
    B, A = 8, 2
    pool = workload.action_pool(20, B, A)
    runs = []
    for had_it in (False, True):
        env = _env(assets, B, A, autoreset=True)
        if had_it:
            with pytest.raises(ValueError, match='shaper is off'):
                env.record_replay(steps=4)
        env.shape_rewards()
        if had_it:
            env.record_replay(steps=4)
            assert env.replay.on and env.replay.buf['frames'].shape == (5, B, 256, 4)
            env.record_replay(None)
            assert env.replay.buf is None and not env.replay.on
            with pytest.raises(ValueError):
                env.eng.replay.kernel()                                              # F110_E_INVALID: no buffer
        snaps = []
        for k in range(21):
            obs, reward, done, info = env.reset(workload.spawn_poses(B, A)) if k == 0 else env.step(pool[k - 1])
            snaps.append({'reward': reward.clone(), 'done': done.clone(), **{'obs_' + n: v.clone() for n, v in obs.items() if torch.is_tensor(v)},
                          **{'info_' + n: v.clone() for n, v in info.items() if torch.is_tensor(v)}})
        torch.cuda.synchronize()
        runs.append((snaps, set(info), set(env.state_dict())))
        if had_it:
            keep = env
        else:
            env.close()
    (off, keys_off, sd_off), (on_, keys_on, sd_on) = runs
    assert keys_on == keys_off and sd_on == sd_off and 'replay_count' not in keys_on
    for step, (x, y) in enumerate(zip(off, on_)):
        for k in x:
            assert torch.equal(torch.nan_to_num(x[k].double(), nan=-1.0), torch.nan_to_num(y[k].double(), nan=-1.0)), (step, k)
    env = keep
    env.record_replay(steps=4)
    _, _, _, info = env.step(pool[0])
    assert set(info) - keys_off == {'replay_count', 'replay_valid'} and set(env.state_dict()) == sd_off
    # removing the shaper, or another image size, removes the buffer too
    env.shape_rewards(rows=75, cols=100)
    assert not env.replay.on and 'replay_count' not in env.step(pool[0])[3]
    env.record_replay(steps=4)
    assert env.replay.buf['frames'].shape == (5, B, 75, 2)
    env.shape_rewards(False)
    assert not env.replay.on and env.replay.buf is None
    # save / load round trip, and a checkpoint breaks the chain but keeps what is stored
    env.shape_rewards()
    env.record_replay(steps=4)
    env.reset(workload.spawn_poses(B, A))
    for k in range(6):
        env.step(pool[k])
    saved = env.replay.save()
    sd = env.state_dict()
    assert not {'frames', 'actions', 'rewards', 'dones', 'valid', 'count', 'chain_start'} & set(sd) and int(saved['count']) == 7
    idx = torch.arange(4 * B, device=env.device)
    before = [t.clone() for t in env.replay.sample_at(idx)]
    for k in range(6, 9):
        env.step(pool[k])
    assert not all(torch.equal(x, y) for x, y in zip(before, env.replay.sample_at(idx)))
    env.replay.load(saved)
    for x, y in zip(before, env.replay.sample_at(idx)):
        assert torch.equal(x, y)
    for k, v in env.replay.save().items():
        assert torch.equal(v, saved[k]), k
    with pytest.raises(ValueError, match='does not fit'):
        env.replay.load({k: v[:1] for k, v in saved.items()})
    env.load_state_dict(sd)
    n_before = len(env.replay)
    _, _, _, info = env.step(pool[6])
    assert not gk.to_host(info['replay_valid']).any()                                       # the chain was broken: a frame, no transition
    assert len(env.replay) == n_before - int(gk.to_host(saved['valid'])[7 % 4].sum())       # only the evicted step slot's are gone
    _, _, _, info = env.step(pool[7])
    assert gk.to_host(info['replay_valid']).any()
    assert env.eng.device_errors() == 0
    env.close()


@pytest.mark.parametrize('rows,cols,action_dim', [s + (16,) for s in rc.RING_SHAPES] + [(3, 64, 300)])
def test_ring_equals_mirror_on_scripted_frames(assets, rows, cols, action_dim):
    """The push itself (env.eng.replay.kernel()) on inputs the test writes into the buffers it reads -- the shaper's bitmap and
    total, the engine's clock and done, replay_action -- at the sizes of rc.RING_SHAPES: 5 envs, T = 3, 2 T + 3 pushes of
    rc.scripted_pushes (frames of arbitrary bytes that differ per env and push, a clock that stands still, a reset, terminal
    steps).  After every push last_valid, the counter and sample_at(all T * B indices) as uint8 and as fp32 at scales 1 and
    1 / 255 `==` the mirror.  action_dim = 300 runs the action loops of push and gather beyond one pass of the workgroup."""
    import torch
    B, T = 5, 3
    env = _env(assets, B, autoreset=True)
    env.shape_rewards(rows=rows, cols=cols)
    env.record_replay(steps=T, action_dim=action_dim)
    rp, sh, t = env.replay, env.eng.shaper.buf, env.eng.t
    assert tuple(sh['bitmap'].shape) == (B, rows, cols) and tuple(env.replay_action.shape) == (B, action_dim)
    mirror = rc.Mirror(T, B, rows, cols, action_dim, env.timestep)
    pushes = rc.scripted_pushes(rows, cols, B, T, action_dim, env.timestep)
    assert len(pushes) == 2 * T + 3
    all_idx = torch.arange(T * B, device=env.device)
    prev, invalid, terminal = None, 0, 0
    for k, q in enumerate(pushes):
        frame = rc.binary(q['frame'])
        assert all((frame[e] == 0).any() and (frame[e] == 255).any() for e in range(B))
        assert prev is None or all((frame[e] != prev[e]).any() for e in range(B))
        prev = frame
        sh['bitmap'].copy_(torch.as_tensor(q['frame']))
        sh['total'].copy_(torch.as_tensor(q['reward']))
        t['current_time'].copy_(torch.as_tensor(q['clock']))
        t['done'].copy_(torch.as_tensor(q['done'].astype(bool)))
        env.replay_action.copy_(torch.as_tensor(q['action']))
        rp.kernel()
        torch.cuda.synchronize()
        valid = mirror.push(frame, q['action'], q['reward'], q['done'], q['clock'])
        assert np.array_equal(gk.to_host(rp.buf['last_valid']), valid), (k, gk.to_host(rp.buf['last_valid']), valid)
        assert int(rp.buf['count']) == mirror.count
        if k:
            invalid += int((valid == 0).sum())
            terminal += int((valid & q['done']).sum())
        want = mirror.at(range(T * B))
        _assert_batch(rp.sample_at(all_idx), want, '%d x %d, push %d, uint8' % (rows, cols, k))
        for scale in (1.0, 1.0 / 255.0):
            on = np.float32(255.0) * np.float32(scale)
            got = rp.sample_at(all_idx, dtype=torch.float32, scale=scale)
            assert got[0].shape == got[3].shape == (T * B, 1, rows, cols) and got[0].dtype == torch.float32
            want32 = tuple(np.where(w == 255, on, np.float32(0.0)).astype(np.float32)[:, None] if i in (0, 3) else w for i, w in enumerate(want))
            _assert_batch(got, want32, '%d x %d, push %d, fp32 * %g' % (rows, cols, k, scale))
    assert invalid >= 1 and terminal >= 1 and len(mirror) == len(rp) > 0
    assert np.array_equal(gk.to_host(rp.buf['valid']), mirror.valid_array())
    assert env.eng.device_errors() == 0
    env.close()


def _draw_direct(env, seed, first, n):
    """f110_replay_draw itself (the wrapper keeps its own draw counter) into arrays longer than the launch has lanes: what lies
    beyond the n draws must stay as it was."""
    import torch
    from red_gym_amd import _lib
    eng = env.eng
    m = (n + 255) // 256 * 256 + 300
    idx = torch.full((m,), -7, dtype=torch.int64, device=env.device)
    ok = torch.full((m,), 9, dtype=torch.uint8, device=env.device)
    with torch.cuda.device(env.device):
        _lib.check(eng.lib.f110_replay_draw(eng._h, seed, first, n, idx.data_ptr(), ok.data_ptr(), eng._stream()))
    torch.cuda.synchronize()
    idx, ok = gk.to_host(idx), gk.to_host(ok)
    assert (idx[n:] == -7).all() and (ok[n:] == 9).all(), 'the draw wrote beyond its n = %d outputs' % n
    return idx[:n], ok[:n]


def test_draw_at_every_launch_shape_and_a_wrapping_draw_number(assets):
    """n = 1, 255, 257 and 1000 draws (a partial last workgroup, several workgroups) on DRAW_CASE's pattern, from draw number 0
    and from 2 ** 64 - 3, where the draw number wraps inside the launch: `==` the checker, nothing written beyond n."""
    import torch
    c = rc.DRAW_CASE
    env, _ = _filled_env(assets, B=c['B'], T=c['T'], steps=c['count'] - 1, rows=40, cols=30)
    pattern = rc.draw_case_valid()
    env.replay.buf['valid'].copy_(torch.as_tensor(pattern))
    assert int(env.replay.buf['count']) == c['count']
    for first in (0, 2 ** 64 - 3):
        for n in (1, 255, 257, 1000):
            idx, ok = _draw_direct(env, c['seed'], first, n)
            want_idx, want_ok, _ = rc.draw(pattern, c['count'], c['seed'], first, n)
            assert np.array_equal(idx, want_idx) and np.array_equal(ok, want_ok), (first, n)
            assert pattern[idx[idx >= 0] // c['B'], idx[idx >= 0] % c['B']].all()
    # the draws either side of the wrap are those of draw numbers 2 ** 64 - 3 .. 2 ** 64 - 1 and 0 ..: another stream than 0 ..
    assert np.array_equal(_draw_direct(env, c['seed'], 2 ** 64 - 3, 257)[0][3:], _draw_direct(env, c['seed'], 0, 254)[0])
    assert env.eng.device_errors() == 0
    env.close()


@pytest.mark.parametrize('start', [2 ** 31 - 3, 2 ** 40 + 1])
def test_counter_beyond_32_bits(assets, start):
    """A ring of T = 4, B = 6 whose counter starts at 2 ** 31 - 3 (the run crosses 2 ** 31) and at 2 ** 40 + 1 (save(), edit
    count and chain_start, load()), 2 T + 3 pushes through the eager step and through step_graph: replay_count, replay_valid,
    sample_at(all T * B indices) and draw(257) `==` the mirror started at the same count after every push.  A kernel or a
    binding that kept 32 bits of `count` would report another replay_count and take other slots."""
    import torch
    from red_gym_amd import workload
    B, T, AD = 6, 4, 16
    env = _env(assets, B, autoreset=True)
    env.shape_rewards()
    env.reset(workload.spawn_poses(B, 1))
    pool = workload.action_pool(3 + 2 * T + 3, B, 1)
    for k in range(3):
        env.step(pool[k])
    sd = env.state_dict()
    env.record_replay(steps=T, action_dim=AD)
    rp = env.replay
    blank = rp.save()
    blank['count'].fill_(start)
    blank['chain_start'].fill_(start)
    all_idx = torch.arange(T * B, device=env.device)
    for how in ('eager', 'step_graph'):
        env.load_state_dict(sd)
        rp.load(blank)
        assert int(rp.buf['count']) == start and len(rp) == 0
        mirror = rc.Mirror(T, B, 256, 256, AD, env.timestep)
        mirror.count = mirror.chain_start = start
        if how == 'step_graph':
            env.capture_step()
        stepper = env.step if how == 'eager' else env.step_graph
        for k in range(2 * T + 3):
            action = (np.arange(B * AD).reshape(B, AD) + 1000.0 * k).astype(np.float32)
            env.replay_action.copy_(torch.as_tensor(action))
            _, reward, done, info = stepper(pool[3 + k])
            torch.cuda.synchronize()
            valid = mirror.push(gk.to_host(info['lidar_bitmap']), action, gk.to_host(reward), gk.to_host(done), gk.to_host(info['current_time']))
            assert np.array_equal(gk.to_host(info['replay_valid']), valid), (how, k)
            assert int(info['replay_count']) == mirror.count == start + k + 1
            assert not valid.any() if k == 0 else valid.any()
            _assert_batch(rp.sample_at(all_idx), mirror.at(range(T * B)), '%s from %d, push %d' % (how, start, k))
            first = rp._draws
            idx, ok = rp.draw(257, seed=5)
            want_idx, want_ok, _ = rc.draw(mirror.valid_array(), mirror.count, 5, first, 257)
            assert np.array_equal(gk.to_host(idx), want_idx) and np.array_equal(gk.to_host(ok), want_ok), (how, k)
            assert want_ok.all() == (k > 0)
        idx, ok = _draw_direct(env, 5, 2 ** 64 - 3, 257)
        want_idx, want_ok, _ = rc.draw(mirror.valid_array(), mirror.count, 5, 2 ** 64 - 3, 257)
        assert np.array_equal(idx, want_idx) and np.array_equal(ok, want_ok) and want_ok.all()
        assert len(rp) == len(mirror) > 2 * B and mirror.count > 2 ** 31
    assert env.eng.device_errors() == 0
    env.close()
