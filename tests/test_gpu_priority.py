"""Prioritized replay on the device (csrc/f110_priority.h): the tree alone at every level count -- rebuild, pick and set `==` the checker
of tests/priority_cases.py -- then on an engine: the push hook after every step of a scripted run, eager and through both graphs; the
sample against the checker's pick, nstep_at and frames_at, captured and replayed; the importance weights; the quantisation and the
write-back.  Words cross as int32 / int64 bits and are compared as uint32 / uint64."""
import ctypes as C
import os

import numpy as np
import pytest

import gpu_checks as gk
import priority_cases as pc

pytestmark = pytest.mark.gpu

PICKS = 4096
SEED = 0x1234567890ABCDEF
G = 0.97


def _dev_words(a):
    """A uint32 host array as the int32 tensor that holds its bits."""
    return gk.to_device(np.ascontiguousarray(a, np.uint32).view(np.int32))


def _u32(t):
    return np.ascontiguousarray(gk.to_host(t)).view(np.uint32)


def _u64(t, words=None):
    a = np.ascontiguousarray(gk.to_host(t)).view(np.uint64)
    return a if words is None else a[:words]


def _tree(leaf):
    """(leaf, node) on the device for the host leaves, the nodes rebuilt over words of garbage."""
    from red_gym_amd import priority
    dev = _dev_words(leaf)
    node = priority.new_nodes(dev)
    node.fill_(-7)
    priority.rebuild(dev, node)
    return dev, node


def _cases(L):
    last = np.zeros(L, np.uint32)
    last[-1] = 12345
    return dict(random=pc.random_leaves(L), sparse=pc.sparse_leaves(L), last=last, zero=np.zeros(L, np.uint32))


@pytest.mark.parametrize('L', pc.GPU_L)
def test_rebuild_and_pick_equal_the_checker(L):
    from red_gym_amd import priority
    lay = pc.layout(L)
    assert priority.node_words(L) == lay['words']
    for name, leaf in _cases(L).items():
        want_node = pc.rebuild(leaf)
        want_idx, want_q, path = pc.pick(leaf, want_node, SEED, 3, PICKS)
        if name == 'random':                     # from the checker alone: the draws reach every child of the top and the last node of every level
            top = lay['count'][-1] if lay['levels'] else L
            assert set(path[:, 0].tolist()) == set(range(top)), (L, sorted(set(range(top)) - set(path[:, 0].tolist())))
            if L >= 4097:
                for k in range(lay['levels']):
                    assert lay['count'][k] - 1 in path[:, lay['levels'] - 1 - k], (L, k)
                assert L - 1 in path[:, -1]
        if name == 'zero':
            assert (want_idx == -1).all() and not want_q.any()
        if name == 'last':
            assert (want_idx == L - 1).all()
        dev, node = _tree(leaf)
        assert np.array_equal(_u64(node, lay['words']), want_node), (L, name)
        idx, q = priority.pick(dev, node, SEED, 3, PICKS)
        bad = int((gk.to_host(idx) != want_idx).sum()), int((_u32(q) != want_q).sum())
        print('L %d %s: %d nodes, %d of %d picks differ (q: %d)' % (L, name, lay['words'], bad[0], PICKS, bad[1]))
        assert bad == (0, 0), (L, name)
        assert np.array_equal(_u32(dev), leaf)                      # (neither entry writes a leaf)


def _set_rows(L, n, seed):
    """n rows for a set: the last quarter names the leaves of the first quarter again (with other words), some rows lie outside the tree
    and some carry q = 0."""
    rng = np.random.default_rng([L, n, seed])
    idx = rng.integers(0, L, n).astype(np.int64)
    idx[n - n // 4:] = idx[:n // 4]
    out = np.arange(5, n, 17)
    idx[out] = np.where(out % 2 == 0, -1 - out, L + out // 2)
    q = rng.integers(1, 1 << 32, n).astype(np.uint32)
    q[3::11] = 0
    return idx, q


def _shared(idx, L):
    """Rows inside the tree whose leaf another row names as well."""
    inside = idx[(idx >= 0) & (idx < L)]
    _, inverse, counts = np.unique(inside, return_inverse=True, return_counts=True)
    return int((counts[inverse] > 1).sum())


@pytest.mark.parametrize('L', pc.GPU_L)
def test_set_equals_the_checker(L):
    """f110_ptree_set with 64 and with 4 096 rows.  Asserted first: the 4 096 rows hold at least 100 rows that name a leaf another row
    names (64 rows cannot hold 100; a quarter of them, 16 pairs, are made to), rows outside the tree and rows with q = 0."""
    from red_gym_amd import priority
    lay = pc.layout(L)
    leaf = pc.random_leaves(L, seed=1)
    dev, node = _tree(leaf)
    for n in (64, 4096):
        idx, q = _set_rows(L, n, 2)
        outside = int(((idx < 0) | (idx >= L)).sum())
        assert _shared(idx, L) >= (100 if n == 4096 else 28) and outside >= 3 and int((q == 0).sum()) >= 5 and (idx < 0).any() and (idx >= L).any()
        priority.set_words(dev, node, gk.to_device(idx), _dev_words(q))
        leaf = pc.set_max(leaf, idx, q)
        got_leaf, got_node = _u32(dev), _u64(node, lay['words']).copy()
        bad = int((got_leaf != leaf).sum()), int((got_node != pc.rebuild(leaf)).sum())
        print('L %d, %d rows (%d share a leaf, %d outside): %d leaves and %d nodes differ' % (L, n, _shared(idx, L), outside, bad[0], bad[1]))
        assert bad == (0, 0), (L, n)
        priority.rebuild(dev, node)                                 # the invariant held: a rebuild changes nothing
        assert np.array_equal(_u64(node, lay['words']), got_node)


# ---------------------------------------------------------------------------------------------- on an engine
SHAPES = ((5, 7), (96, 3), (16, 300))          # (B, T): one level only, rows that straddle level-1 nodes, three levels


def _env(assets, B, T, priorities=True, rows=20, cols=24):
    from red_gym_amd import F110VecEnv, workload
    env = F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, autoreset=True)
    env.shape_rewards(rows=rows, cols=cols)
    env.record_replay(steps=T, action_dim=4, priorities=priorities)
    env.reset(workload.spawn_poses(B, 1))
    return env


def _read(env):
    """(leaf uint32, node uint64, state fields, valid [L]) as the device holds them."""
    p = env.replay.priorities
    L = p.leaf.numel()
    return _u32(p.leaf), _u64(p.node, pc.layout(L)['words']), pc.state_words(gk.to_host(p.state)), gk.to_host(env.replay.buf['valid']).reshape(-1)


def _assert_fresh_tree(env, what):
    leaf, node, state, valid = _read(env)
    want = np.where(valid != 0, state['qmax'], 0).astype(np.uint32)
    assert np.array_equal(leaf, want) and np.array_equal(node, pc.rebuild(want)), what
    return leaf


def _scripted_run(env, how, T, check):
    """T + 6 pushes: steps, a whole reset, a masked reset of every second env, a restart() of the chain, and the wrap of the ring.  -> the
    (leaf, node) pairs as they stood after every push (device clones)."""
    import torch
    from red_gym_amd import workload
    B = env.num_envs
    pool = workload.action_pool(8, B, 1)
    spawn = workload.spawn_poses(B, 1)
    if how == 'step_graph':
        env.capture_step()
    elif how == 'step_lib_graph':
        env.build_step_graph()
    stepper = env.step if how == 'eager' else getattr(env, how)
    p, seen = env.replay.priorities, []
    for k in range(T + 3):
        if k == 2:
            env.reset(spawn)
        elif k == 4:
            env.reset(spawn, torch.as_tensor((np.arange(B) % 2 == 0).astype(np.uint8)))
        if k == 6:
            env.replay.restart()
        if k in (2, 4):
            seen.append((p.leaf.clone(), p.node.clone()))
            if check:
                _assert_fresh_tree(env, (how, k, 'reset'))
        stepper(pool[k % 8])
        seen.append((p.leaf.clone(), p.node.clone()))
        if check:
            _assert_fresh_tree(env, (how, k))
    return seen


@pytest.mark.parametrize('B,T', SHAPES)
def test_push_hook_keeps_the_tree_through_a_scripted_run(assets, B, T):
    import torch
    lay = pc.layout(B * T)
    assert lay['levels'] == {35: 0, 288: 1, 4800: 2}[B * T] and (B % 64 != 0)
    runs = {}
    for how in ('eager', 'step_graph', 'step_lib_graph'):
        env = _env(assets, B, T)
        _assert_fresh_tree(env, 'installed')
        runs[how] = _scripted_run(env, how, T, check=(how == 'eager'))
        leaf = _assert_fresh_tree(env, (how, 'end'))
        _, _, state, valid = _read(env)
        assert int(env.replay.buf['count']) == T + 6 and state['qmax'] == pc.ONE and valid.any() and not valid.all() and (leaf > 0).any()
        assert env.eng.device_errors() == 0
        env.close()
    for how in ('step_graph', 'step_lib_graph'):
        assert len(runs[how]) == len(runs['eager']) == T + 5
        for k, ((l0, n0), (l1, n1)) in enumerate(zip(runs['eager'], runs[how])):
            assert torch.equal(l0, l1) and torch.equal(n0, n1), (how, k)


def _filled_env(assets, B=16, T=12, priorities=True, steps=20):
    """A ring that has wrapped, with resets in it, and words of many magnitudes on its valid transitions."""
    import torch
    from red_gym_amd import workload
    env = _env(assets, B, T, priorities)
    pool = workload.action_pool(8, B, 1)
    gen = torch.Generator(device=env.device).manual_seed(5)
    for k in range(steps):
        if k in (12, 16):                        # (two masked resets the ring still holds at the end: rows of invalid transitions)
            env.reset(workload.spawn_poses(B, 1), torch.as_tensor((np.arange(B) % 3 == 0).astype(np.uint8)))
        env.replay_action.copy_(torch.rand((B, 4), device=env.device, generator=gen))
        env.step(pool[k % 8])
    return env


def _spread_words(env, seed=9):
    """Random words on every transition through f110_priority_set (the invalid ones are skipped) -> the leaves read back."""
    L = env.replay.priorities.leaf.numel()
    rng = np.random.default_rng(seed)
    q = (rng.integers(1, 1 << 16, L) << rng.integers(0, 16, L)).astype(np.uint32)
    env.replay.priorities.set(gk.to_device(np.arange(L, dtype=np.int64)), _dev_words(q))
    leaf, node, state, valid = _read(env)
    assert np.array_equal(leaf, np.where(valid != 0, q, 0)) and np.array_equal(node, pc.rebuild(leaf)) and state['qmax'] == max(pc.ONE, int(q[valid != 0].max()))
    return leaf, node


BATCH = ('frames', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok', 'indices', 'discount', 'span', 'prio', 'weight')   # the priority draw's, whatever nstep is


def _assert_sample(env, got, leaf, node, first, n, nstep):
    import torch
    rp = env.replay
    frames, s_idx, ns_idx, a, r, d, ok, idx, discount, span, prio, weight = (got[k] for k in BATCH)
    want_idx, want_q, _ = pc.pick(leaf, node, SEED, first, n)
    assert np.array_equal(gk.to_host(idx), want_idx) and np.array_equal(_u32(prio), want_q)
    walk = rp.nstep_at(idx, nstep, G)
    assert all(torch.equal(x, y) for x, y in zip((ns_idx, r, d, discount, span), walk))
    one = rp.frames_at(idx)
    assert frames.data_ptr() == one['frames'].data_ptr() and torch.equal(s_idx, one['s_idx']) and torch.equal(a, one['a']) and torch.equal(ok, one['ok'])
    if nstep == 1:
        assert torch.equal(ns_idx, one['ns_idx']) and torch.equal(r.view(torch.int64), one['r'].view(torch.int64)) and torch.equal(d, one['d'])
    return want_q


@pytest.mark.parametrize('nstep', (1, 3))
def test_sample_equals_the_checkers_pick_and_the_ring(assets, nstep):
    import torch
    env = _filled_env(assets)
    rp = env.replay
    leaf, node = _spread_words(env)
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    first = rp.sample_priority_dev(64, counter, seed=SEED, nstep=nstep, gamma=G)
    second = rp.sample_priority_dev(200, counter, seed=SEED, nstep=nstep, gamma=G)
    assert sorted(first) == sorted(BATCH) and int(counter) == 264 and first['prio'].dtype == torch.int32 and first['weight'].dtype == torch.float32
    _assert_sample(env, first, leaf, node, 0, 64, nstep)
    _assert_sample(env, second, leaf, node, 64, 200, nstep)
    assert bool(first['ok'].all()) and (nstep == 1 or bool((first['span'] > 1).any()))
    assert sorted(rp.sample_out(8, nstep, priorities=True)) == sorted(list(rp.sample_out(8, 3)) + ['prio', 'weight'])
    with pytest.raises(ValueError):
        rp.sample_priority_dev(8, counter, out=rp.sample_out(8, 3))
    rp.set_priorities(None)
    with pytest.raises(ValueError):
        rp.sample_priority_dev(8, counter)
    assert env.eng.device_errors() == 0
    env.close()


def _betas(beta, step, end, k):
    out = []
    for _ in range(k):
        beta = min(end, beta + step)
        out.append(beta)
    return out


def test_a_captured_sample_replays_as_three_eager_ones(assets):
    import torch
    env = _filled_env(assets, priorities=dict(beta=0.4, beta_end=1.0, beta_updates=2))
    rp, p = env.replay, env.replay.priorities
    leaf, node = _spread_words(env)
    n = 96
    want_beta = _betas(0.4, p.beta_step, 1.0, 3)
    assert want_beta[1] == want_beta[2] == 1.0 and 0.4 < want_beta[0] < 1.0
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    eager = []
    for k in range(3):
        got = rp.sample_priority_dev(n, counter, seed=SEED, nstep=3, gamma=G)
        eager.append({k: got[k].clone() for k in BATCH[1:]})
        assert int(counter) == (k + 1) * n and p.beta == want_beta[k]
    counter.zero_()
    p.set_beta(0.4)
    out = rp.sample_out(n, 3, priorities=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        got = rp.sample_priority_dev(n, counter, seed=SEED, out=out, nstep=3, gamma=G)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(counter) == 0 and p.beta == 0.4                       # the capture itself draws nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert sorted(got) == sorted(BATCH) and all(torch.equal(got[f], eager[k][f]) for f in BATCH[1:]), k
        assert int(counter) == (k + 1) * n and p.beta == want_beta[k]
        _assert_sample(env, got, leaf, node, k * n, n, 3)
    assert not torch.equal(eager[0]['indices'], eager[1]['indices']) and not torch.equal(eager[0]['weight'], eager[1]['weight'])     # other draws, other weights
    assert env.eng.device_errors() == 0
    env.close()


def test_importance_weights(assets):
    """1.0f exactly where prio == qmin, 0 where ok == 0, ones at beta = 0, elsewhere within one fp32 ulp of float32(NumPy's fp64 pow): the
    device's fp64 pow errs by a few 2^-53, far below half an fp32 ulp, so only a rounding tie can move the result."""
    import torch
    from red_gym_amd import priority
    env = _filled_env(assets, priorities=dict(beta=0.4, beta_end=1.0, beta_updates=1000))
    rp, p = env.replay, env.replay.priorities
    _spread_words(env)
    # a stale leaf: a heavy word on an invalid transition, written past the handle's valid check -> rows the ring refuses (ok = 0)
    valid = gk.to_host(rp.buf['valid']).reshape(-1)
    stale = int(np.flatnonzero(valid == 0)[0])
    priority.set_words(p.leaf, p.node, gk.to_device(np.array([stale], np.int64)), _dev_words(np.array([1 << 31], np.uint32)))
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    n = 512
    for beta in (0.4, 1.0, 0.0):
        p.set_beta(beta)
        got = rp.sample_priority_dev(n, counter, seed=SEED, nstep=1, gamma=G)
        ok, idx, prio, w = gk.to_host(got['ok']), gk.to_host(got['indices']), _u32(got['prio']), gk.to_host(got['weight'])
        assert (ok == 0).sum() >= 5 and (idx[ok == 0] == stale).all() and (ok != 0).sum() >= 100
        qmin = prio[ok != 0].min()
        assert w.dtype == np.float32 and (w[ok == 0] == 0.0).all() and (w[(ok != 0) & (prio == qmin)] == 1.0).all() and ((ok != 0) & (prio == qmin)).any()
        want = pc.weights(prio, ok, beta)
        if beta == 0.0:
            assert (w[ok != 0] == 1.0).all()
        ulps = np.abs(w.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        print('beta %.1f: %d rows, %d without ok, %d differ from NumPy by one ulp, worst %d' % (beta, n, (ok == 0).sum(), (ulps == 1).sum(), ulps.max()))
        assert ulps.max() <= 1 and (w[ok != 0] > 0).all() and (w <= 1.0).all()
        assert beta == 0.0 or len(set(w.tolist())) > 10
    assert env.eng.device_errors() == 0
    env.close()


def _update(env, idx, ok, td):
    """PriorityTree.update on host rows -> q_out uint32."""
    import torch
    q_out = torch.full((len(idx),), -1, dtype=torch.int32, device=env.device)
    env.replay.priorities.update(gk.to_device(np.asarray(idx, np.int64)), gk.to_device(np.asarray(ok, np.uint8)), gk.to_device(np.asarray(td, np.float32)), q_out)
    return _u32(q_out)


def test_quantisation_and_write_back(assets):
    env = _filled_env(assets)
    rp = env.replay
    valid = gk.to_host(rp.buf['valid']).reshape(-1)
    L = len(valid)
    live = np.flatnonzero(valid != 0)
    assert len(live) >= 100 and len(live) < L
    rng = np.random.default_rng(21)

    def rows(n):
        return live[rng.integers(0, len(live), n)]

    # exponent 1, eps 0: the word is rint(td * 2^16) exactly
    rp.set_priorities(dict(exponent=1.0, eps=0.0))
    td = np.concatenate([rng.uniform(0.0, 40.0, 500), rng.uniform(0.0, 1e-3, 100), [0.5, 1.0, 1.5 / 65536, 2.5 / 65536, 3.0]]).astype(np.float32)
    got = _update(env, rows(len(td)), np.ones(len(td)), td)
    want = np.clip(np.rint(td.astype(np.float64) * 65536.0), 1, pc.QMAX_WORD).astype(np.uint64).astype(np.uint32)
    assert np.array_equal(got, want) and np.array_equal(got, pc.quantise(td, 1.0, 0.0)[0]) and got[-3] == 2 and got[-2] == 2
    # the edges: NaN and inf, a huge td clamps, a tiny one gives 1
    edge = np.array([np.nan, np.inf, 3e38, 70000.0, 65535.99, 1e-30, 0.0], np.float32)
    got = _update(env, rows(len(edge)), np.ones(len(edge)), edge)
    assert got.tolist() == [pc.QMAX_WORD] * 4 + [int(np.rint(np.float64(np.float32(65535.99)) * 65536.0)), 1, 1]
    assert _read(env)[2]['qmax'] == pc.QMAX_WORD
    # exponent 0.6: `==` NumPy where NumPy's p * 2^16 lies clear of a rounding boundary, within one word anywhere
    rp.set_priorities(dict(exponent=0.6, eps=1e-6))
    td = np.concatenate([rng.uniform(0.0, 30.0, 3000), rng.uniform(0.0, 0.01, 1000)]).astype(np.float32)
    want, x = pc.quantise(td, 0.6, 1e-6)
    frac = x - np.floor(x)
    clear = ((frac >= 0.05) & (frac <= 0.45)) | ((frac >= 0.55) & (frac <= 0.95))
    assert clear.sum() >= 3000 and (~clear).sum() >= 100
    idx = rows(len(td))
    before = _read(env)
    assert before[2]['qmax'] == pc.ONE and np.array_equal(before[0], np.where(valid != 0, pc.ONE, 0))       # (the install reset the tree)
    got = _update(env, idx, np.ones(len(td)), td)
    delta = got.astype(np.int64) - want.astype(np.int64)
    print('exponent 0.6: %d rows, %d clear of a boundary; %d words differ from NumPy, worst by %d' % (len(td), clear.sum(), (delta != 0).sum(), np.abs(delta).max()))
    assert np.array_equal(got[clear], want[clear]) and np.abs(delta).max() <= 1
    # the tree after the update is the checker's set fed with q_out; several rows named one leaf
    leaf, node, state, _ = _read(env)
    want_leaf = pc.set_max(before[0], idx, got)
    assert _shared(idx, L) >= 100 and np.array_equal(leaf, want_leaf) and np.array_equal(node, pc.rebuild(want_leaf)) and state['qmax'] == max(pc.ONE, int(got.max()))
    # rows without ok, invalid transitions and indices outside the ring leave the tree alone and have q_out = 0
    dead = np.flatnonzero(valid == 0)
    idx2 = np.concatenate([rows(50), dead[:20], [-1, L, L + 5], rows(30)])
    ok2 = np.concatenate([np.zeros(50), np.ones(20), np.ones(3), np.ones(30)])
    td2 = rng.uniform(50.0, 60.0, len(idx2)).astype(np.float32)
    got2 = _update(env, idx2, ok2, td2)
    assert not got2[:73].any() and np.array_equal(got2[73:], pc.quantise(td2[73:], 0.6, 1e-6)[0])
    leaf2, node2, state2, _ = _read(env)
    want2 = pc.set_max(leaf, idx2[73:], got2[73:])
    assert np.array_equal(leaf2, want2) and np.array_equal(node2, pc.rebuild(want2)) and state2['qmax'] == int(got2.max()) > state['qmax']
    assert not leaf2[dead].any()
    # the next push enters with the raised qmax
    from red_gym_amd import workload
    env.step(workload.action_pool(1, env.num_envs, 1)[0])
    leaf3, node3, state3, valid3 = _read(env)
    slot = (int(rp.buf['count']) - 1) % rp.steps
    row = slice(slot * env.num_envs, (slot + 1) * env.num_envs)
    assert np.array_equal(leaf3[row], np.where(valid3[row] != 0, state2['qmax'], 0)) and valid3[row].any() and np.array_equal(node3, pc.rebuild(leaf3))
    assert env.eng.device_errors() == 0
    env.close()


def test_refusals_and_removal(assets):
    import torch
    from red_gym_amd import _lib
    env = _filled_env(assets, priorities=None, steps=3)
    rp, eng = env.replay, env.eng
    assert rp.priorities is None
    epoch = eng.launch_epoch()
    for bad in (dict(exponent=-0.5), dict(exponent=9.0), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            rp.set_priorities(bad)
        assert rp.priorities is None
    assert eng.launch_epoch() == epoch                               # a refused install moves nothing
    rp.set_priorities(True)
    p = rp.priorities
    assert eng.launch_epoch() > epoch and p.qmax == pc.ONE and p.beta == 0.4
    _assert_fresh_tree(env, 'switched on over a filled ring')
    A, n = p.leaf.data_ptr(), 4
    lib, h, s = eng.lib, eng._h, eng._stream()
    for call, word in ((lambda: lib.f110_priority_update(h, None, A, A, n, None, s), 'null idx'), (lambda: lib.f110_priority_update(h, A, None, A, n, None, s), 'null ok'),
                       (lambda: lib.f110_priority_update(h, A, A, None, n, None, s), 'null td'), (lambda: lib.f110_priority_update(h, A, A, A, -1, None, s), 'n=-1'),
                       (lambda: lib.f110_priority_set(h, A, None, n, s), 'null q'),
                       (lambda: lib.f110_priority_sample(h, 1, A + 4, n, 1, G, A, A, A, A, A, A, A, A, A, A, A, s), 'not 8-byte aligned'),
                       (lambda: lib.f110_priority_sample(h, 1, A, -1, 1, G, A, A, A, A, A, A, A, A, A, A, A, s), 'n=-1'),
                       (lambda: lib.f110_priority_sample(h, 1, A, n, 1, G, A, A, A, A, A, A, A, A, A, A, None, s), 'null argument')):
        assert call() == _lib.E_INVALID and word.encode() in lib.f110_last_error(), (word, lib.f110_last_error())
    b = _lib.PriorityBuffers()
    b.leaf, b.node, b.state = A, p.node.data_ptr(), p.state.data_ptr() + 4
    assert lib.f110_priority_bind(h, C.byref(b)) == _lib.E_INVALID and b'state is not 8-byte aligned' in lib.f110_last_error()
    torch.cuda.synchronize()
    _assert_fresh_tree(env, 'after the refusals')
    # a new ring drops the priorities; record_replay(priorities=None) launches nothing of them
    env.record_replay(steps=5, action_dim=4)
    assert rp.priorities is None and lib.f110_priority_reset(h, s) == _lib.E_INVALID and b'no priorities are installed' in lib.f110_last_error()
    assert env.eng.device_errors() == 0
    env.close()
