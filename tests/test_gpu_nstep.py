"""N-step returns on the device (f110_replay_nstep, f110_replay_sample_nstep, f110_qhead_forward_rows, SACAgent(nstep=k)): every output of
the walk `==` the checker of tests/nstep_cases.py as raw bits at every index of the scripted rings test_nstep_cpu.py takes its census
on; the fused sample against the draw checker, nstep_at and frames_at; a captured sample that draws afresh; the refusals; the target
with a discount per row `==` the checker at tests/qhead_cases.py's forward shapes; and the agent: nstep = 1 is the agent without the
option, nstep = 3 is update_batch on a batch assembled by hand, replays are eager updates, and nstep is part of the graph key."""
import os

import numpy as np
import pytest

import gpu_checks as gk
import nstep_cases as nc
import qhead_cases as qc
import replay_cases as rc
import update_cases as uc
from test_gpu_sac_agent import SEED, SMALL, _differing, _kw, _ring_env, _snapshot

pytestmark = pytest.mark.gpu

G = nc.GAMMA
WALK = ('ns_frame', 'ret', 'd', 'discount', 'span')
FIELDS = ('s_idx', 'ns_idx', 'a', 'r', 'd', 'ok')                    # of every batch, beside 'frames' and 'indices'


def _ring(assets, ring, rows=40, cols=30):
    """A ring of DRAW_CASE's shape (T = 5, B = 7) built as tests/test_gpu_sample_dev.py builds its own -- `count` pushes of real steps with
    distinct stored actions -- with the scripted valid, dones and rewards of `ring` written over what the steps stored."""
    import torch
    from red_gym_amd import F110VecEnv, workload
    valid, dones, rewards, count = ring
    T, B = valid.shape
    env = F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, autoreset=True)
    env.shape_rewards(rows=rows, cols=cols)
    env.record_replay(steps=T)
    env.reset(workload.spawn_poses(B, 1))
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for k in range(count - 1):
        env.replay_action.copy_(torch.arange(B * 16, device=env.device).reshape(B, 16) + 1000.0 * k)
        env.step(acts)
    buf = env.replay.buf
    buf['valid'].copy_(torch.as_tensor(valid))
    buf['dones'].copy_(torch.as_tensor(dones))
    buf['rewards'].copy_(torch.as_tensor(rewards))
    assert int(buf['count']) == count
    return env


def _bits_equal(got, want):
    got, want = gk.to_host(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _assert_walk(got, want, what):
    """got: (ns_idx, ret, d, discount, span) device tensors; want: nc.walk()'s dict."""
    bad = [k for k, g in zip(WALK, got) if not _bits_equal(g, want[k])]
    assert not bad, (what, bad)


@pytest.mark.parametrize('name', sorted(nc.rings()))
def test_nstep_at_equals_the_checker_at_every_index(assets, name):
    import torch
    ring = nc.rings()[name]
    valid, dones, rewards, count = ring
    T, B = valid.shape
    env = _ring(assets, ring)
    rp = env.replay
    idx = nc.all_indices(T, B)
    assert idx[0] == -1 and idx[-1] == T * B and len(idx) == T * B + 2
    for nstep in nc.NSTEPS:
        want = nc.walk(valid, dones, rewards, count, idx, nstep, G)
        got = rp.nstep_at(idx, nstep, G)
        assert [t.dtype for t in got] == [torch.int64, torch.float64, torch.uint8, torch.float64, torch.int32]
        _assert_walk(got, want, (name, nstep))
    # nstep = 1: what frames_at gives, and gamma's bits in every row
    plain = rp.frames_at(idx)
    assert sorted(plain) == sorted(('frames', 'indices') + FIELDS)
    frames, s_idx, ns_idx, a, r, d, ok = (plain[k] for k in ('frames',) + FIELDS)
    one = rp.nstep_at(idx, 1, G)
    assert torch.equal(one[0], ns_idx) and _bits_equal(one[1], gk.to_host(r)) and torch.equal(one[2], d) and torch.equal((one[4] > 0).to(torch.uint8), ok)
    assert _bits_equal(one[3], np.full(len(idx), G))
    # frames_at(nstep=3): frames_at's frame before, action and ok beside nstep_at's walk
    got = rp.frames_at(idx, nstep=3, gamma=G)
    assert sorted(got) == sorted(('frames', 'indices', 'discount', 'span') + FIELDS)
    assert got['frames'].data_ptr() == frames.data_ptr() and torch.equal(got['s_idx'], s_idx) and torch.equal(got['a'], a) and torch.equal(got['ok'], ok)
    _assert_walk((got['ns_idx'], got['r'], got['d'], got['discount'], got['span']), nc.walk(valid, dones, rewards, count, idx, 3, G), (name, 'frames_at'))
    assert env.eng.device_errors() == 0
    env.close()


def _assert_sample(rp, ring, got, want_idx, nstep):
    """got: sample_frames_dev(nstep > 1)'s result: the indices `==` the draw checker's, the walk `==` nstep_at(indices) and the checker,
    the rest `==` frames_at(indices)."""
    import torch
    valid, dones, rewards, count = ring
    frames, s_idx, ns_idx, a, r, d, ok, idx, discount, span = (got[k] for k in ('frames',) + FIELDS + ('indices', 'discount', 'span'))
    assert np.array_equal(gk.to_host(idx), want_idx)
    _assert_walk((ns_idx, r, d, discount, span), nc.walk(valid, dones, rewards, count, want_idx, nstep, G), 'sample')
    again = rp.nstep_at(idx, nstep, G)
    assert all(torch.equal(x, y) for x, y in zip((ns_idx, r, d, discount, span), again))
    one = rp.frames_at(idx)
    assert frames.data_ptr() == one['frames'].data_ptr() and torch.equal(s_idx, one['s_idx']) and torch.equal(a, one['a']) and torch.equal(ok, one['ok'])


def test_sample_nstep_continues_one_stream_of_draws(assets):
    import torch
    ring = nc.census_ring()
    valid, count = ring[0], ring[3]
    env = _ring(assets, ring)
    rp, seed = env.replay, rc.DRAW_CASE['seed']
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    first = rp.sample_frames_dev(5, counter, seed=seed, nstep=3, gamma=G)
    second = rp.sample_frames_dev(7, counter, seed=seed, nstep=3, gamma=G)
    assert sorted(first) == sorted(('frames', 'indices', 'discount', 'span') + FIELDS) and int(counter) == 12
    _assert_sample(rp, ring, first, rc.draw(valid, count, seed, 0, 5)[0], 3)
    _assert_sample(rp, ring, second, rc.draw(valid, count, seed, 5, 7)[0], 3)
    # the one-step call at the same draw numbers draws the same transitions, and returns its seven fields and the indices as before
    counter.zero_()
    plain = rp.sample_frames_dev(5, counter, seed=seed)
    assert sorted(plain) == sorted(('frames', 'indices') + FIELDS) and torch.equal(plain['indices'], first['indices']) and torch.equal(plain['s_idx'], first['s_idx']) and int(counter) == 5
    # out=: with nstep > 1 the two extra tensors are required, written and returned
    out = rp.sample_out(7, 3)
    assert sorted(out) == sorted(list(rp.sample_out(7)) + ['discount', 'span']) and 'discount' not in rp.sample_out(7, 1)
    got = rp.sample_frames_dev(7, counter, seed=seed, out=out, nstep=3, gamma=G)
    assert got['discount'] is out['discount'] and got['span'] is out['span'] and got['r'] is out['r'] and 'frames' not in out and int(counter) == 12
    _assert_sample(rp, ring, got, rc.draw(valid, count, seed, 5, 7)[0], 3)
    assert env.eng.device_errors() == 0
    env.close()


def test_refusals_move_nothing(assets):
    import torch
    ring = nc.census_ring()
    env = _ring(assets, ring)
    rp = env.replay
    counter = torch.full((1,), 4, dtype=torch.int64, device=env.device)
    idx = torch.arange(5, device=env.device)
    out3, out1 = rp.sample_out(5, 3), rp.sample_out(5)
    for t in out3.values():
        t.fill_(3)
    short = dict(out3, span=out3['span'].long())
    for bad in (lambda: rp.nstep_at(idx, 0, G), lambda: rp.nstep_at(idx, 65, G), lambda: rp.nstep_at(idx, 3, float('nan')), lambda: rp.nstep_at(idx, 3, None),
                lambda: rp.nstep_at(idx, 2.0, G), lambda: rp.frames_at(idx, nstep=3), lambda: rp.frames_at(idx, nstep=65, gamma=G),
                lambda: rp.sample_frames_dev(5, counter, out=out3, nstep=0, gamma=G), lambda: rp.sample_frames_dev(5, counter, out=out3, nstep=65, gamma=G),
                lambda: rp.sample_frames_dev(5, counter, out=out3, nstep=3, gamma=float('nan')), lambda: rp.sample_frames_dev(5, counter, out=out3, nstep=3),
                lambda: rp.sample_frames_dev(5, counter, out=out1, nstep=3, gamma=G), lambda: rp.sample_frames_dev(5, counter, out=short, nstep=3, gamma=G),
                lambda: rp.sample_frames_dev(4, counter, out=out3, nstep=3, gamma=G)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert int(counter) == 4 and all(bool((t == 3).all()) for t in out3.values())
    # the library's own checks, behind the host's: the raw entries refuse the same without a launch
    from red_gym_amd import _lib
    eng, o = env.eng, out3
    for nstep, gamma in ((0, G), (65, G), (3, float('inf'))):
        assert eng.lib.f110_replay_nstep(eng._h, idx.data_ptr(), 5, nstep, gamma, o['ns_idx'].data_ptr(), o['r'].data_ptr(), o['d'].data_ptr(),
                                         o['discount'].data_ptr(), o['span'].data_ptr(), eng._stream()) == _lib.E_INVALID
        assert eng.lib.f110_replay_sample_nstep(eng._h, 1, counter.data_ptr(), 5, nstep, gamma, o['indices'].data_ptr(), o['s_idx'].data_ptr(), o['ns_idx'].data_ptr(),
                                                o['a'].data_ptr(), o['r'].data_ptr(), o['d'].data_ptr(), o['ok'].data_ptr(), o['discount'].data_ptr(),
                                                o['span'].data_ptr(), eng._stream()) == _lib.E_INVALID
    assert eng.lib.f110_replay_nstep(eng._h, idx.data_ptr(), 5, 3, G, o['ns_idx'].data_ptr(), o['r'].data_ptr(), o['d'].data_ptr(), o['discount'].data_ptr(), None,
                                     eng._stream()) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert int(counter) == 4 and all(bool((t == 3).all()) for t in out3.values()) and env.eng.device_errors() == 0
    env.close()


def test_the_empty_ring_gives_zero_transitions(assets):
    import torch
    env = _ring(assets, nc.census_ring())
    env.record_replay(steps=rc.DRAW_CASE['T'])                                          # a new, empty ring
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    out = env.replay.sample_out(9, 3)
    for t in out.values():
        t.fill_(3)
    got = env.replay.sample_frames_dev(9, counter, out=out, nstep=3, gamma=G)
    s_idx, ns_idx, a, r, d, ok, idx, discount, span = (got[k] for k in FIELDS + ('indices', 'discount', 'span'))
    assert all((gk.to_host(t) == -1).all() for t in (idx, s_idx, ns_idx)) and not any(gk.to_host(t).any() for t in (a, r, d, ok, span))
    assert _bits_equal(discount, np.full(9, G)) and int(counter) == 9 and env.eng.device_errors() == 0
    env.close()


def test_a_captured_sample_draws_afresh_at_every_replay(assets):
    """Captured once, replayed three times with n = 256 at nstep = 3: the batches are the checker's draws at first = 0, 256 and 512, the
    walk of each `==` the checker; the capture itself draws nothing."""
    import torch
    ring = nc.census_ring()
    valid, dones, rewards, count = ring
    env = _ring(assets, ring)
    rp, seed, n = env.replay, rc.DRAW_CASE['seed'], rc.DRAW_CASE['n']
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    out = rp.sample_out(n, 3)
    out['indices'].fill_(-5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        got = rp.sample_frames_dev(n, counter, seed=seed, out=out, nstep=3, gamma=G)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(counter) == 0 and (gk.to_host(out['indices']) == -5).all()
    batches = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_ok, _ = rc.draw(valid, count, seed, k * n, n)
        assert want_ok.all()
        _assert_sample(rp, ring, got, want_idx, 3)
        assert int(counter) == (k + 1) * n
        batches.append(gk.to_host(out['indices']).copy())
    assert not np.array_equal(batches[0], batches[1]) and not np.array_equal(batches[1], batches[2])
    assert set(gk.to_host(out['span']).tolist()) == {1, 2, 3} and env.eng.device_errors() == 0
    env.close()


# ---------------------------------------------------------------------------------------------- the target with a discount per row
FEATURES = 24


def _discounts(n, seed):
    """gamma, gamma^2 and gamma^3 by running products, mixed over the rows (row 0, which is not done, takes gamma^3 where n > 1)."""
    g = np.float64(G)
    table = np.array([g, g * g, g * g * g])
    pick = np.random.default_rng([n, seed]).integers(0, 3, n)
    if n > 1:
        pick[0] = 2
    return table[pick]


@pytest.mark.parametrize('shape', qc.FORWARD_SHAPES)
def test_td_target_takes_a_discount_per_row(shape):
    """td_target with an [n] fp64 gamma `==` the checker (qc.forward's q and qmin from the `pre` the module's own feature GEMM gives, then
    the target's two lines with discount[b]); with a tensor filled with gamma `==` the by-value call, bit for bit; dense on and off, alpha
    by value and as Temperature.alpha."""
    import torch
    from red_gym_amd import dense as dn
    from red_gym_amd import qhead
    from red_gym_amd.temperature import Temperature
    n, H, A = shape
    F = FEATURES
    inp = qc.inputs(n, H, A)
    torch.manual_seed(n + H + A)
    fc1s = [torch.nn.Linear(F + A, H).cuda() for _ in range(2)]
    fc2s = [torch.nn.Linear(H, 1).cuda() for _ in range(2)]
    feats = [torch.randn((n, F), device='cuda').relu_() for _ in range(2)]
    action, nlp = gk.to_device(inp['action']), gk.to_device(inp['nlp'])
    reward, done = gk.to_device(inp['reward']), gk.to_device(inp['done'])
    disc = _discounts(n, 5)
    disc_dev, flat = gk.to_device(disc), torch.full((n,), G, dtype=torch.float64, device='cuda')
    temp = Temperature(init_alpha=0.37)
    assert float(temp.alpha.item()) == 0.37
    for dense in (True, False):
        w1s = [l.weight.detach() for l in fc1s]
        if dense:
            _, pres = qhead._feature_pre([f.contiguous() for f in feats], w1s, F, A, dn.DEFAULT_SEGMENT)
        else:
            pres = [torch.mm(f, w[:, :F].t()) for f, w in zip(feats, w1s)]
        host = dict(inp, pre=[gk.to_host(p) for p in pres], w_act=[gk.to_host(l.weight)[:, F:] for l in fc1s], b1=[gk.to_host(l.bias) for l in fc1s],
                    w2=[gk.to_host(l.weight).reshape(-1) for l in fc2s], b2=[gk.to_host(l.bias) for l in fc2s])
        for alpha, value in ((0.2, 0.2), (temp.alpha, 0.37)):
            want, _ = nc.target_rows(host, disc, value)
            got = qhead.td_target(feats, action, nlp, reward, done, fc1s, fc2s, disc_dev, alpha, dense=dense)
            bad = gk.differing(got, want)
            print('%s dense=%s alpha=%s: %d of %d targets differ' % (shape, dense, value, bad, n))
            assert got.dtype == torch.float32 and bad == 0, (shape, dense, value)
            by_value = qhead.td_target(feats, action, nlp, reward, done, fc1s, fc2s, G, alpha, dense=dense)
            per_row = qhead.td_target(feats, action, nlp, reward, done, fc1s, fc2s, flat, alpha, dense=dense)
            assert torch.equal(per_row.view(torch.int32), by_value.view(torch.int32))
            if n > 1:
                assert not torch.equal(got, by_value)                        # (row 0 is not done: its discount shows)
    for bad_gamma in (disc_dev.float(), disc_dev[:-1] if n > 1 else disc_dev.repeat(2), disc_dev.cpu(), disc_dev.reshape(n, 1)):
        with pytest.raises(ValueError):
            qhead.td_target(feats, action, nlp, reward, done, fc1s, fc2s, bad_gamma, 0.2)


# ---------------------------------------------------------------------------------------------- the agent
def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _eps(gen, n, A):
    import torch
    return tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))


def _agent(c, nstep=None):
    """A SACAgent on the tensors of a new fp32 mirror on the GPU (the same seed: the same networks); nstep=None: built without the option."""
    import torch
    from red_gym_amd import SACAgent
    m = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=SEED, **_kw(c))
    kw = {} if nstep is None else dict(nstep=nstep)
    return SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, **kw, **_kw(c))


def test_nstep_1_is_the_agent_without_the_option(assets):
    """Three updates of SACAgent(nstep=1) and of an agent built without the option: every parameter, moment, loss and index `==`, the
    same graph key, the same tensors in the sample."""
    import torch
    from red_gym_amd import SACAgent
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    plain, one = _agent(c), _agent(c, 1)
    assert one.nstep == 1 == plain.nstep and _differing(_snapshot(one), _snapshot(plain)) == []
    assert one._graph_key(env.replay, n) == plain._graph_key(env.replay, n) and 'nstep' not in str(plain._graph_key(env.replay, n))
    gen = torch.Generator(device='cuda').manual_seed(11)
    for u in range(3):
        eps = _eps(gen, n, A)
        lp, lo = plain.update(env.replay, n, eps=eps), one.update(env.replay, n, eps=eps)
        assert _same_bits(lp, lo) and _differing(_snapshot(one), _snapshot(plain)) == [], u
        assert sorted(one.sample) == sorted(plain.sample) and 'span' not in one.sample
        assert all(torch.equal(one.sample[k], plain.sample[k]) for k in plain.sample) and int(one.draws) == int(plain.draws) == (u + 1) * n
    assert 'nstep' not in one.state_dict()
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            SACAgent(nstep=bad, **_kw(c))
    assert env.eng.device_errors() == 0
    env.close()


def test_nstep_3_is_update_batch_on_a_batch_assembled_by_hand(assets):
    """One update(nstep = 3) `==` update_batch on frames_at's frame before and action and nstep_at's walk of the same indices, with the
    same eps; the spans are not all one, and a one-step agent on the same draws ends elsewhere."""
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    three, by_hand, one = _agent(c, 3), _agent(c), _agent(c)
    assert three.nstep == 3 and three._graph_key(env.replay, n) != one._graph_key(env.replay, n)
    eps = _eps(torch.Generator(device='cuda').manual_seed(12), n, A)
    l3 = three.update(env.replay, n, eps=eps)
    s = three.sample
    assert sorted(s) == sorted(list(env.replay.sample_out(n)) + ['discount', 'span'])
    one_step = env.replay.frames_at(s['indices'])
    frames, s_idx, a, ok = (one_step[k] for k in ('frames', 's_idx', 'a', 'ok'))
    ns_idx, ret, d, discount, span = env.replay.nstep_at(s['indices'], 3, three.gamma)
    assert bool(ok.all()) and bool((span > 1).any()) and torch.equal(span, s['span']) and torch.equal(ret, s['r']) and torch.equal(discount, s['discount'])
    lh = by_hand.update_batch(dict(frames=frames, s_idx=s_idx, ns_idx=ns_idx, a=a, r=ret, d=d, discount=discount), eps=eps)
    assert _same_bits(l3, lh) and bool(torch.isfinite(l3).all()) and _differing(_snapshot(three), _snapshot(by_hand)) == []
    l1 = one.update(env.replay, n, eps=eps)
    assert torch.equal(one.sample['indices'], s['indices']) and not _same_bits(l1, l3) and _differing(_snapshot(one), _snapshot(three)) != []
    assert env.eng.device_errors() == 0
    env.close()


def test_nstep_3_replays_equal_eager_updates_and_nstep_is_in_the_graph_key(assets):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    eager, graph = _agent(c, 3), _agent(c, 3)
    start = _snapshot(graph)
    losses = graph.capture_update(env.replay, n, draws=False)
    torch.cuda.synchronize()
    assert _differing(_snapshot(graph), start) == [] and int(graph.draws) == 0 and graph.captures == 1
    gen = torch.Generator(device='cuda').manual_seed(13)
    for u in range(3):
        eps = _eps(gen, n, A)
        want = eager.update(env.replay, n, eps=eps)
        got = graph.update_graph(eps=eps)
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert _same_bits(got, want) and bool(torch.isfinite(got).all()) and _differing(_snapshot(graph), _snapshot(eager)) == [], u
        assert sorted(graph.sample) == sorted(eager.sample) and all(torch.equal(graph.sample[k], eager.sample[k]) for k in eager.sample)
        assert int(graph.draws) == int(eager.draws) == (u + 1) * n and bool((graph.sample['span'] > 1).any())
    # nstep is part of the key: another nstep is another capture, with a sample of the other form
    key3 = graph._graph_key(env.replay, n)
    graph.nstep = 1
    assert graph._graph_key(env.replay, n) != key3
    graph.update_graph(eps=eps)
    assert graph.recaptured and graph.captures == 2 and 'span' not in graph.sample
    graph.update_graph(eps=eps)
    assert not graph.recaptured and graph.captures == 2
    graph.nstep = 3
    graph.update_graph(eps=eps)
    torch.cuda.synchronize()
    assert graph.recaptured and graph.captures == 3 and 'span' in graph.sample and env.eng.device_errors() == 0
    env.close()
