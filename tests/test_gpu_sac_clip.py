"""SACAgent(max_grad_norm=...) at tests/test_gpu_sac_agent.py's SMALL shape: None is the agent without the argument and 1e30 the
unclipped agent, bit for bit; a small norm `==` the same update composed by hand -- the agent's own forward and backward, then the
checker of tests/clip_cases.py on the .grad tensors it left -- ; replays are eager updates, the [3, 8] stats tensor included; a batch
with an infinite reward skips both critics' steps and the next clean update proceeds; grad_stats() returns views; the state dicts
stay torch.optim.Adam's."""
import numpy as np
import pytest

import clip_cases as cc
import gpu_checks as gk
import optim_cases as oc
import update_cases as uc
from test_gpu_sac_agent import SEED, SMALL, _differing, _kw, _ring_env, _snapshot

pytestmark = pytest.mark.gpu

SMALL_NORM = 0.05          # far below the norms of these updates (printed by the composed test): every step is clipped


def _agent(c, **kw):
    """A SACAgent on the tensors of a new fp32 mirror of the start every agent of test_gpu_sac_agent has."""
    import torch
    from red_gym_amd import SACAgent
    m = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=SEED, **_kw(c))
    return SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, **_kw(c), **kw)


def _batches(c, count):
    return [uc.lib_batch(uc.batch(1000 * SEED + u, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])) for u in range(count)]


def _update(agent, bl):
    return agent.update_batch(bl, eps=(bl['eps_next'], bl['eps_new']))


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('max_grad_norm', [None, 1e30])
def test_none_and_a_huge_norm_are_the_unclipped_agent(assets, max_grad_norm):
    """Two updates: every parameter, moment, state word and loss `==` the agent built without the argument; with None the graph key
    too, and nothing of the feature exists; with 1e30 the key differs, coef is 1.0f and nothing was clipped or skipped."""
    import torch
    c = SMALL
    plain, other = _agent(c), _agent(c, max_grad_norm=max_grad_norm)
    for bl in _batches(c, 2):
        a, b = _update(plain, bl), _update(other, bl)
        assert _same_bits(a, b)
    assert _differing(_snapshot(plain), _snapshot(other)) == []
    env = _ring_env(assets, c)
    if max_grad_norm is None:
        assert other._graph_key(env.replay, c['n']) == plain._graph_key(env.replay, c['n'])
        assert other.clip_states is None and other.max_grad_norm is None and all(o._partials is None for o in other.optimizers().values())
        with pytest.raises(ValueError, match='max_grad_norm'):
            other.grad_stats()
    else:
        assert other._graph_key(env.replay, c['n']) == plain._graph_key(env.replay, c['n']) + (('max_grad_norm', 1e30),)
        stats = other.grad_stats()
        assert stats['coef'].tolist() == [1.0] * 3 and stats['skip'].tolist() == [0] * 3
        assert stats['steps_clipped'].tolist() == [0] * 3 and stats['steps_skipped'].tolist() == [0] * 3
        assert bool((stats['norm'] > 0).all()) and bool(torch.isfinite(stats['norm']).all())
    env.close()


def _state_of(words):
    w = np.ascontiguousarray(words)
    return dict(t=int(w[0]), pow1=float(w.view(np.float64)[1]), pow2=float(w.view(np.float64)[2]), k2=w.view(np.float32)[6], a=w.view(np.float32)[7])


def _step_by_hand(opt, max_norm, clip):
    """What SacAdam.step() with max_grad_norm must do, from the .grad tensors as they are: the checker on host copies, written back
    into the (unclipped) optimizer's parameters, moments, targets and state -> the checker's clip state."""
    import torch
    ps = [gk.to_host(p) for p in opt.params]
    gs = [gk.to_host(p.grad) for p in opt.params]
    ms, vs = [gk.to_host(opt.moments(i)[0]) for i in range(len(ps))], [gk.to_host(opt.moments(i)[1]) for i in range(len(ps))]
    ts = None if opt.targets is None else [gk.to_host(t) for t in opt.targets]
    out = cc.run(ps, [gs], max_norm, ts, _state_of(gk.to_host(opt._state)), (ms, vs), clip, lr=opt.lr, betas=opt.betas, eps=opt.eps, tau=opt.tau)
    with torch.no_grad():
        for i, p in enumerate(opt.params):
            p.copy_(gk.to_device(out[0][i]))
            opt.moments(i)[0].copy_(gk.to_device(out[1][i]))
            opt.moments(i)[1].copy_(gk.to_device(out[2][i]))
            if ts is not None:
                opt.targets[i].copy_(gk.to_device(out[3][i]))
        opt._state.copy_(gk.to_device(oc.state_words(out[4])))
    return out[5]


def test_a_small_norm_equals_the_update_composed_by_hand():
    """Two updates.  `hand` is an unclipped agent whose three SacAdam.step are replaced by the checker on the host (the same forward
    and backward: SACAgent._update itself); the clipped agent's parameters, targets, moments, Adam state words, losses and the three
    clip states are `==`."""
    c = SMALL
    agent, hand = _agent(c, max_grad_norm=SMALL_NORM), _agent(c)
    clips = {name: None for name in hand.optimizers()}
    for name, opt in hand.optimizers().items():
        def step(opt=opt, name=name):
            clips[name] = _step_by_hand(opt, SMALL_NORM, clips[name])
        opt.step = step
    for u, bl in enumerate(_batches(c, 2)):
        got, want = _update(agent, bl), _update(hand, bl)
        assert _same_bits(got, want), u
        assert _differing(_snapshot(agent), _snapshot(hand)) == [], u
        words = gk.to_host(agent.clip_states)
        for k, name in enumerate(hand.optimizers()):
            assert np.array_equal(words[k], cc.clip_words(clips[name])), (u, name, words[k], cc.clip_words(clips[name]))
            print('update %d %s: norm %r coef %r' % (u, name, float(clips[name]['norm']), float(clips[name]['coef'])))
            assert clips[name]['coef'] < 1 and clips[name]['steps_clipped'] == u + 1 and clips[name]['skip'] == 0


def test_replays_equal_eager_updates_with_the_stats(assets):
    """Three update_graph(eps=...) replays against three eager update(eps=...) calls from one start on one ring: parameters, moments,
    state words, losses and the [3, 8] stats tensor are `==` after each; the capture moved nothing; max_grad_norm is in the key: changing
    it captures again."""
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    eager, graph = _agent(c, max_grad_norm=SMALL_NORM), _agent(c, max_grad_norm=SMALL_NORM)
    start = _snapshot(graph)
    losses = graph.capture_update(env.replay, n, draws=False)
    torch.cuda.synchronize()
    assert _differing(_snapshot(graph), start) == [] and not graph.clip_states.any() and graph.captures == 1
    gen = torch.Generator(device='cuda').manual_seed(11)
    for u in range(3):
        eps = tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))
        want = eager.update(env.replay, n, eps=eps)
        got = graph.update_graph(eps=eps)
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert _same_bits(got, want) and bool(torch.isfinite(got).all()), (u, got, want)
        assert _differing(_snapshot(graph), _snapshot(eager)) == [], u
        assert torch.equal(graph.clip_states, eager.clip_states), u
        assert graph.grad_stats()['steps_clipped'].tolist() == [u + 1] * 3
    graph.max_grad_norm = 2 * SMALL_NORM
    assert all(o.max_grad_norm == 2 * SMALL_NORM for o in graph.optimizers().values())
    graph.update_graph(eps=eps)
    assert graph.recaptured and graph.captures == 2
    assert env.eng.device_errors() == 0
    env.close()


def test_an_infinite_reward_skips_the_critics_steps():
    """One clean update, one whose batch holds an inf reward, one clean: the second leaves both critics and their moments and state
    words bitwise unchanged and counts one skipped step each, the targets still move, the actor (whose loss reads the unchanged
    critics) steps; the third proceeds from the unskipped step count."""
    import torch
    c = SMALL
    agent = _agent(c, max_grad_norm=cc.INF)
    b = _batches(c, 3)
    _update(agent, b[0])
    before = _snapshot(agent)
    poisoned = dict(b[1], r=b[1]['r'].clone())
    poisoned['r'][3] = float('inf')
    _update(agent, poisoned)
    after = _snapshot(agent)
    moved = _differing(before, after)
    assert not [m for m in moved if m.startswith(('critic1.', 'critic2.'))], moved
    assert all(any(m.startswith(name + '.') for m in moved) for name in ('actor', 'critic1_target', 'critic2_target')), moved
    stats = agent.grad_stats()
    assert stats['skip'].tolist() == [0, 1, 1] and stats['steps_skipped'].tolist() == [0, 1, 1] and stats['steps_clipped'].tolist() == [0, 0, 0]
    assert stats['coef'].tolist() == [1.0] * 3 and stats['norm'][1:].tolist() == [float('inf')] * 2 and bool(torch.isfinite(stats['norm'][0]))
    assert [o.device_state()[0] for o in agent.optimizers().values()] == [2, 1, 1]
    for name in ('critic1', 'critic2'):
        assert all(bool(torch.isfinite(p).all()) for p in agent.modules()[name].parameters())
    losses = _update(agent, b[2])
    assert bool(torch.isfinite(losses).all())
    assert [o.device_state()[0] for o in agent.optimizers().values()] == [3, 2, 2]
    stats = agent.grad_stats()
    assert stats['skip'].tolist() == [0, 0, 0] and stats['steps_skipped'].tolist() == [0, 1, 1]
    moved = _differing(after, _snapshot(agent))
    assert all(any(m.startswith(name + '.') for m in moved) for name in uc.NETS)
    assert all(bool(torch.isfinite(p).all()) for m in agent.modules().values() for p in m.parameters())


def test_grad_stats_are_views_and_the_state_dicts_are_adams():
    import torch
    c = SMALL
    agent = _agent(c, max_grad_norm=SMALL_NORM)
    s = agent.clip_states
    assert s.shape == (3, 8) and s.dtype == torch.int64
    stats = agent.grad_stats()
    assert sorted(stats) == ['coef', 'norm', 'skip', 'steps_clipped', 'steps_skipped', 'sumsq']
    assert stats['sumsq'].data_ptr() == s.data_ptr() and all(v.untyped_storage().data_ptr() == s.untyped_storage().data_ptr() for v in stats.values())
    assert (stats['norm'].dtype, stats['coef'].dtype, stats['skip'].dtype, stats['steps_skipped'].dtype) == (torch.float64, torch.float32, torch.int32, torch.int64)
    assert all(tuple(v.shape) == (3,) for v in stats.values())
    assert [o._clip.data_ptr() for o in agent.optimizers().values()] == [s[k].data_ptr() for k in range(3)]
    b = _batches(c, 2)
    _update(agent, b[0])
    assert stats['steps_clipped'].tolist() == [1, 1, 1] and bool((stats['norm'] > SMALL_NORM).all())      # the views see the update
    for k, opt in enumerate(agent.optimizers().values()):
        norm, coef, skip, clipped, skipped = opt.clip_stats()
        assert (norm, coef, skip, clipped, skipped) == (float(stats['norm'][k]), float(stats['coef'][k]), False, 1, 0)
    # configuration and diagnostics, not state
    full = agent.state_dict()
    assert sorted(full) == sorted(list(uc.NETS) + [n + '_optimizer' for n in uc.TRAINED] + ['draws'])
    for name, opt in agent.optimizers().items():
        sd = full[name + '_optimizer']
        assert set(sd) == {'state', 'param_groups'} and 'max_grad_norm' not in sd['param_groups'][0]
        adam = torch.optim.Adam(list(agent.modules()[name].parameters()), lr=1.0)
        adam.load_state_dict(sd)
        assert adam.param_groups[0]['lr'] == uc.LR and float(adam.state[opt.params[0]]['step']) == 1.0
    torch.manual_seed(99)
    from red_gym_amd import SACAgent
    other = SACAgent(gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, max_grad_norm=SMALL_NORM, **_kw(c))
    other.load_state_dict(full)
    assert not other.clip_states.any()
    la, lo = _update(agent, b[1]), _update(other, b[1])
    assert _same_bits(la, lo) and _differing(_snapshot(other), _snapshot(agent)) == []
    assert other.grad_stats()['steps_clipped'].tolist() == [1, 1, 1] and stats['steps_clipped'].tolist() == [2, 2, 2]
    for bad in (0.0, -1.0, float('nan'), 'x'):
        with pytest.raises(ValueError, match='max_grad_norm'):
            SACAgent(max_grad_norm=bad, **_kw(c))
