"""SACAgent(per=True) (red_gym_amd/sac.py) on a small ring with priorities: the first update is update_batch on a batch assembled by hand
from sample_priority_dev, and the tree behind it is the checker's; replays of the captured update are eager updates, the tree included;
equal priorities are the unweighted update; per=False ignores a ring's priorities; a saved ring continues to the same tree."""
import numpy as np
import pytest

import gpu_checks as gk
import priority_cases as pc
import update_cases as uc
from test_gpu_sac_agent import SEED, SMALL, _differing, _kw, _ring_env, _snapshot

pytestmark = pytest.mark.gpu

EXACT = dict(exponent=1.0, eps=0.0, beta=0.5, beta_end=1.0, beta_updates=4)      # (at exponent 1 the word of a td is NumPy's, exactly)


def _agent(c, **kw):
    import torch
    from red_gym_amd import SACAgent
    m = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=SEED, **_kw(c))
    return SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, **kw, **_kw(c))


def _eps(gen, n, A):
    import torch
    return tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _per_env(assets, c, priorities=EXACT, spread=True):
    """test_gpu_sac_agent's ring with priorities switched on over it and (spread) words of many magnitudes on its transitions."""
    env = _ring_env(assets, c)
    env.replay.set_priorities(priorities)
    if spread:
        L = env.replay.priorities.leaf.numel()
        q = (np.random.default_rng(4).integers(1 << 10, 1 << 20, L)).astype(np.uint32)
        env.replay.priorities.set(gk.to_device(np.arange(L, dtype=np.int64)), gk.to_device(q.view(np.int32)))
    return env


def _tree(env):
    p = env.replay.priorities
    L = p.leaf.numel()
    return (np.ascontiguousarray(gk.to_host(p.leaf)).view(np.uint32), np.ascontiguousarray(gk.to_host(p.node)).view(np.uint64)[:pc.layout(L)['words']],
            pc.state_words(gk.to_host(p.state)))


def _same_tree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize('nstep', (1, 3))
def test_first_update_is_update_batch_by_hand_and_the_tree_is_the_checkers(assets, nstep):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _per_env(assets, c)
    rp, p = env.replay, env.replay.priorities
    per, by_hand = _agent(c, per=True, nstep=nstep), _agent(c)
    eps = _eps(torch.Generator(device='cuda').manual_seed(31), n, A)
    before = _tree(env)
    kept = p.leaf.clone(), p.state.clone()
    seen = []
    update = p.update
    p.update = lambda indices, ok, td, q_out=None: (seen.append(td.clone()), update(indices, ok, td, q_out))[1]
    lp = per.update(rp, n, eps=eps)
    s = per.sample
    assert sorted(s) == sorted(rp.sample_out(n, nstep, priorities=True)) and int(per.draws) == n and len(seen) == 1
    after = _tree(env)
    # the tree: the checker's set fed with the words of the TD errors the update handed over
    idx, ok, td = gk.to_host(s['indices']), gk.to_host(s['ok']), gk.to_host(seen[0])
    q = pc.quantise(td, 1.0, 0.0)[0]
    assert ok.all() and (td > 0).all() and len(set(q.tolist())) > n // 2
    want_leaf = pc.set_max(before[0], idx, q)
    assert np.array_equal(after[0], want_leaf) and np.array_equal(after[1], pc.rebuild(want_leaf)) and not np.array_equal(after[0], before[0])
    assert after[2] == dict(before[2], qmax=max(before[2]['qmax'], int(q.max())), beta=min(1.0, 0.5 + p.beta_step))
    w = gk.to_host(s['weight'])
    assert np.abs(w.view(np.int32).astype(np.int64) - pc.weights(gk.to_host(s['prio']).view(np.uint32), ok, 0.5).view(np.int32)).max() <= 1 and len(set(w.tolist())) > 4
    # by hand: the tree put back, the same draw, update_batch with the weight and the write-back
    p.leaf.copy_(kept[0])
    p.state.copy_(kept[1])
    p.rebuild()
    assert _same_tree(_tree(env), before)
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    got = rp.sample_priority_dev(n, counter, nstep=nstep, gamma=per.gamma)
    frames, s_idx, ns_idx, a, r, d, ok_t, indices, discount, span, prio, weight = (
        got[k] for k in ('frames', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok', 'indices', 'discount', 'span', 'prio', 'weight'))
    assert all(torch.equal(x, s[k]) for k, x in dict(indices=indices, s_idx=s_idx, ns_idx=ns_idx, a=a, r=r, d=d, weight=weight, prio=prio, span=span).items())
    batch = dict(frames=frames, s_idx=s_idx, ns_idx=ns_idx, a=a, r=r, d=d, weight=weight, indices=indices, ok=ok_t)
    if nstep > 1:
        batch['discount'] = discount
        assert bool((span > 1).any())
    lh = by_hand.update_batch(batch, eps=eps, replay=rp)
    assert _same_bits(lp, lh) and bool(torch.isfinite(lp).all()) and _differing(_snapshot(per), _snapshot(by_hand)) == []
    assert _same_tree(_tree(env), after) and len(seen) == 2 and torch.equal(seen[0], seen[1])
    # without the rows' names nothing is written back
    third = _agent(c)
    third.update_batch({k: v for k, v in batch.items() if k not in ('indices', 'ok')}, eps=eps, replay=rp)
    assert len(seen) == 2 and _same_tree(_tree(env), after) and _differing(_snapshot(third), _snapshot(per)) == []
    assert env.eng.device_errors() == 0
    env.close()


def test_three_replays_equal_three_eager_updates(assets):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env_e, env_g = _per_env(assets, c), _per_env(assets, c)
    assert _same_tree(_tree(env_e), _tree(env_g))
    eager, graph = _agent(c, per=True, nstep=3), _agent(c, per=True, nstep=3)
    start, tree0 = _snapshot(graph), _tree(env_g)
    losses = graph.capture_update(env_g.replay, n, draws=False)
    torch.cuda.synchronize()
    assert _differing(_snapshot(graph), start) == [] and int(graph.draws) == 0 and graph.captures == 1 and _same_tree(_tree(env_g), tree0)
    assert 'per' in str(graph._graph_key(env_g.replay, n))
    gen = torch.Generator(device='cuda').manual_seed(32)
    drawn = []
    for u in range(3):
        eps = _eps(gen, n, A)
        want = eager.update(env_e.replay, n, eps=eps)
        got = graph.update_graph(eps=eps)
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert _same_bits(got, want) and bool(torch.isfinite(got).all()) and _differing(_snapshot(graph), _snapshot(eager)) == [], u
        assert sorted(graph.sample) == sorted(eager.sample) and all(torch.equal(graph.sample[k], eager.sample[k]) for k in eager.sample), u
        assert int(graph.draws) == int(eager.draws) == (u + 1) * n
        te, tg = _tree(env_e), _tree(env_g)
        assert _same_tree(te, tg) and np.array_equal(tg[1], pc.rebuild(tg[0])) and not np.array_equal(tg[0], tree0[0]), u
        drawn.append(graph.sample['indices'].clone())
    assert not torch.equal(drawn[0], drawn[1]) and tg[2]['beta'] == min(1.0, min(1.0, min(1.0, 0.5 + 0.125) + 0.125) + 0.125)
    # a ring that lost its priorities is refused, by the eager update and by the graph
    env_g.replay.set_priorities(None)
    for call in (lambda: graph.update(env_g.replay, n), lambda: graph.update_graph(eps=eps), lambda: graph.capture_update(env_g.replay, n)):
        with pytest.raises(ValueError):
            call()
    assert env_e.eng.device_errors() == 0 and env_g.eng.device_errors() == 0
    env_e.close()
    env_g.close()


def test_equal_priorities_are_the_unweighted_update(assets):
    """A fresh ring at exponent 0: every word is 2^16, every weight 1.0, and the parameters are those of update_batch of a per=False agent on
    the same rows."""
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _per_env(assets, c, dict(exponent=0.0), spread=False)
    rp = env.replay
    per, plain = _agent(c, per=True), _agent(c)
    gen = torch.Generator(device='cuda').manual_seed(33)
    for u in range(2):
        eps = _eps(gen, n, A)
        lp = per.update(rp, n, eps=eps)
        s = per.sample
        assert bool((s['weight'] == 1.0).all()) and bool((s['prio'] == pc.ONE).all()) and bool(s['ok'].all())
        at = rp.frames_at(s['indices'])
        frames, s_idx, ns_idx, a, r, d, ok = (at[k] for k in ('frames', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok'))
        lh = plain.update_batch(dict(frames=frames, s_idx=s_idx, ns_idx=ns_idx, a=a, r=r, d=d), eps=eps)
        assert _same_bits(lp, lh) and _differing(_snapshot(per), _snapshot(plain)) == [], u
        leaf, node, state = _tree(env)
        assert set(leaf.tolist()) <= {0, pc.ONE} and state['qmax'] == pc.ONE and np.array_equal(node, pc.rebuild(leaf))
    assert env.eng.device_errors() == 0
    env.close()


def test_per_false_ignores_a_rings_priorities(assets):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    with_p, without = _per_env(assets, c), _ring_env(assets, c)
    a, b = _agent(c, per=False), _agent(c)
    ka, kb = a._graph_key(with_p.replay, n), b._graph_key(without.replay, n)
    assert ka[1:] == kb[1:] and 'per' not in str(ka) and a.per is False and b.per is False
    tree0 = _tree(with_p)
    gen = torch.Generator(device='cuda').manual_seed(34)
    la = a.capture_update(with_p.replay, n, draws=False)
    for u in range(2):
        eps = _eps(gen, n, A)
        la, lb = a.update_graph(eps=eps), b.update(without.replay, n, eps=eps)
        torch.cuda.synchronize()
        assert _same_bits(la, lb) and _differing(_snapshot(a), _snapshot(b)) == [] and sorted(a.sample) == sorted(b.sample) and 'weight' not in a.sample
        assert all(torch.equal(a.sample[k], b.sample[k]) for k in b.sample)
    assert _same_tree(_tree(with_p), tree0)                          # (nothing is written back)
    from red_gym_amd import SACAgent
    with pytest.raises(ValueError):
        _agent(c, per=True).update(without.replay, n)
    assert SACAgent(per=1, **_kw(c)).per is True
    assert with_p.eng.device_errors() == 0 and without.eng.device_errors() == 0
    with_p.close()
    without.close()


def test_a_saved_ring_continues_to_the_same_tree(assets):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _per_env(assets, c)
    agent = _agent(c, per=True)
    gen = torch.Generator(device='cuda').manual_seed(35)
    for u in range(2):
        agent.update(env.replay, n, eps=_eps(gen, n, A))
    saved, sd, tree2 = env.replay.save(), agent.state_dict(), _tree(env)
    assert 'priority_leaf' in saved and 'priority_state' in saved and 'priority_node' not in saved
    fresh = _per_env(assets, c, spread=False)
    assert not _same_tree(_tree(fresh), tree2)
    fresh.replay.load(saved)
    assert _same_tree(_tree(fresh), tree2)                           # (the nodes were rebuilt)
    twin = _agent(c, per=True)
    twin.load_state_dict(sd)
    eps = _eps(gen, n, A)
    l0, l1 = agent.update(env.replay, n, eps=eps), twin.update(fresh.replay, n, eps=eps)
    assert _same_bits(l0, l1) and _differing(_snapshot(agent), _snapshot(twin)) == [] and torch.equal(agent.sample['indices'], twin.sample['indices'])
    assert _same_tree(_tree(env), _tree(fresh)) and not _same_tree(_tree(env), tree2)
    # a ring saved without priorities resets the tree: every valid transition at qmax
    plain = {k: v for k, v in saved.items() if not k.startswith('priority_')}
    fresh.replay.load(plain)
    leaf, node, state = _tree(fresh)
    valid = gk.to_host(fresh.replay.buf['valid']).reshape(-1)
    assert np.array_equal(leaf, np.where(valid != 0, state['qmax'], 0)) and np.array_equal(node, pc.rebuild(leaf))
    assert env.eng.device_errors() == 0 and fresh.eng.device_errors() == 0
    env.close()
    fresh.close()
