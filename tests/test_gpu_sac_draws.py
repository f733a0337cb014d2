"""SACAgent(draws='device'): the agent that draws Actor.sample's noise on the device (red_gym_amd/gauss.py) against a twin
draws='torch' agent that is handed NumPy's draws of the same (seed, stream, call, row) as eps (tests/gauss_cases.py) -- acting with
and without env numbers, a subset against the batch, evaluate=True, three eager updates, three replays of the captured update
against three eager ones, and a checkpoint that continues to the same bits.  Everything is `==` on raw bits.  The small shapes and
the helpers are those of tests/test_gpu_sac_agent.py."""
import numpy as np
import pytest

import gauss_cases as gc
import gpu_checks as gk
import test_gpu_sac_agent as sa
import update_cases as uc

pytestmark = pytest.mark.gpu

C = sa.SMALL
N, A = C['n'], C['action_dim']
SEED = 2025


def _device_agent(seed=SEED, networks=True):
    """A draws='device' agent; with `networks` on a new fp32 mirror of the start every _agent() of test_gpu_sac_agent has."""
    import torch
    from red_gym_amd import SACAgent
    m = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=sa.SEED, **sa._kw(C)) if networks else None
    return SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, draws='device', seed=seed, **sa._kw(C))


def _eps(stream, t, rows=N):
    return gk.to_device(gc.draws(SEED, stream, t, rows, A))


def _frames():
    b = uc.batch(1000 * sa.SEED, N, C['rows'], C['cols'], A, C['pool'])
    return uc.lib_batch(b), b


def _bits_equal(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int64 if a.element_size() == 8 else torch.int32),
                                                                      b.view(torch.int64 if b.element_size() == 8 else torch.int32))


def test_select_action_equals_the_twin_on_numpys_draws():
    import torch
    dev, (tor, _) = _device_agent(), sa._agent(C)
    bl, b = _frames()
    frames, idx = bl['frames'], bl['s_idx']
    m = int(frames.shape[0])
    assert dev.source is not None and tor.source is None and dev.source.calls() == [0, 0, 0, 0]
    # without an index the rows are 0 .. m-1
    got = dev.select_action(frames)
    assert got.dtype == torch.float64 and tuple(got.shape) == (m, A) and _bits_equal(got, tor.select_action(frames, eps=_eps(0, 0, m)))
    # with one, the env ids (a -1, the zero frame, is row 2^64 - 1)
    env_ids = idx.tolist()
    assert b['hole'] is not None and -1 in env_ids
    got = dev.select_action(frames, idx)
    assert _bits_equal(got, tor.select_action(frames, idx, eps=_eps(0, 1, env_ids)))
    assert dev.source.calls() == [2, 0, 0, 0]
    # evaluate draws nothing and advances nothing; an eps that is passed wins and advances nothing
    ev = dev.select_action(frames, idx, evaluate=True)
    assert _bits_equal(ev, tor.select_action(frames, idx, evaluate=True)) and not torch.equal(ev, got)
    eps = _eps(3, 9)
    assert _bits_equal(dev.select_action(frames, idx, eps=eps), tor.select_action(frames, idx, eps=eps))
    assert dev.source.calls() == [2, 0, 0, 0]
    # out= receives the action
    out = torch.zeros((N, A), dtype=torch.float64, device='cuda')
    assert dev.select_action(frames, idx, out=out) is out and _bits_equal(out, tor.select_action(frames, idx, eps=_eps(0, 2, env_ids)))
    assert dev.source.calls() == [3, 0, 0, 0]
    # PolicyHead.sample takes a source for eps: its stream 0, rows 0 .. m-1
    from red_gym_amd.gauss import GaussianSource
    src = GaussianSource(SEED)
    with torch.no_grad():
        h = dev.actor.features(frames)
        mine, theirs = dev.actor.head.sample(h, eps=src), dev.actor.head.sample(h, eps=_eps(0, 0, m))
    assert all(_bits_equal(x, y) for x, y in zip(mine, theirs)) and src.calls() == [1, 0, 0, 0]


def test_acting_on_a_subset_equals_the_subset_of_acting_on_all():
    import torch
    dev = _device_agent()
    bl, _ = _frames()
    frames = bl['frames']
    m = int(frames.shape[0])
    envs = torch.arange(m, dtype=torch.int64, device='cuda')
    dev.source.load_state_dict(dict(seed=SEED, calls=[4, 0, 0, 0]))
    whole = dev.select_action(frames, envs)
    for pick in ([0], [m - 1], [7, 3, 11], list(range(1, m, 2))):
        dev.source.load_state_dict(dict(seed=SEED, calls=[4, 0, 0, 0]))
        sub = dev.select_action(frames, envs[pick])
        assert _bits_equal(sub, whole[pick]), pick
    # another call is other noise for the same envs
    assert dev.source.calls() == [5, 0, 0, 0] and not torch.equal(dev.select_action(frames, envs), whole)


def _same_agents(a, b, u):
    import torch
    assert sa._differing(sa._snapshot(a), sa._snapshot(b)) == [], u
    assert all(torch.equal(a.sample[k], b.sample[k]) for k in b.sample) and int(a.draws) == int(b.draws) == (u + 1) * N, u


def test_three_eager_updates_equal_the_twin_on_numpys_draws(assets):
    import torch
    env = sa._ring_env(assets, C)
    dev, (tor, _) = _device_agent(), sa._agent(C)
    start = sa._snapshot(dev)
    assert sa._differing(sa._snapshot(tor), start) == []
    for u in range(3):
        want = tor.update(env.replay, N, eps=(_eps(1, u), _eps(2, u)))
        got = dev.update(env.replay, N)
        torch.cuda.synchronize()
        assert _bits_equal(got, want) and bool(torch.isfinite(got).all()), (u, got, want)
        _same_agents(dev, tor, u)
        assert dev.source.calls() == [0, u + 1, u + 1, 0]
    # draws that are passed win and advance nothing
    eps = (_eps(1, 50), _eps(2, 50))
    assert _bits_equal(dev.update(env.replay, N, eps=eps), tor.update(env.replay, N, eps=eps)) and dev.source.calls() == [0, 3, 3, 0]
    assert len(sa._differing(sa._snapshot(dev), start)) > 50 and env.eng.device_errors() == 0
    env.close()


def test_three_replays_of_the_captured_update_equal_three_eager_updates(assets):
    import torch
    env = sa._ring_env(assets, C)
    eager, graph = _device_agent(), _device_agent()
    start = sa._snapshot(graph)
    losses = graph.capture_update(env.replay, N)
    torch.cuda.synchronize()
    # the capture moved nothing, the source's counters included
    assert sa._differing(sa._snapshot(graph), start) == [] and int(graph.draws) == 0 and graph.source.calls() == [0, 0, 0, 0] and graph.captures == 1
    for u in range(3):
        want = eager.update(env.replay, N)
        got = graph.update_graph()
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert _bits_equal(got, want) and bool(torch.isfinite(got).all()), (u, got, want)
        _same_agents(graph, eager, u)
        assert torch.equal(graph.source.state, eager.source.state) and graph.source.calls() == [0, u + 1, u + 1, 0]
    # a loaded source is read by the same graph: its tensor is written in place
    for a in (eager, graph):
        a.source.load_state_dict(dict(seed=77, calls=[0, 2 ** 40, 2 ** 63, 0]))
    want, got = eager.update(env.replay, N), graph.update_graph()
    torch.cuda.synchronize()
    assert not graph.recaptured and graph.captures == 1 and _bits_equal(got, want)
    _same_agents(graph, eager, 3)
    assert graph.source.calls() == [0, 2 ** 40 + 1, 2 ** 63 + 1, 0] and env.eng.device_errors() == 0
    env.close()


def test_a_loaded_checkpoint_continues_to_the_same_bits(assets):
    """Two updates and two select_action calls, state_dict() into a fresh agent of another seed and initialisation: the next action
    and the third update are the uninterrupted agent's."""
    import torch
    env = sa._ring_env(assets, C)
    bl, _ = _frames()
    frames = bl['frames']
    first = _device_agent()
    for u in range(2):
        first.update(env.replay, N)
        first.select_action(frames)
    sd = first.state_dict()
    assert sd['source'] == dict(seed=SEED, calls=[2, 2, 2, 0]) and sd['draws'] == 2 * N
    torch.manual_seed(5)
    other = _device_agent(seed=9, networks=False)
    assert other.source.state_dict() == dict(seed=9, calls=[0, 0, 0, 0]) and sa._differing(sa._snapshot(other), sa._snapshot(first)) != []
    other.load_state_dict(sd)
    assert other.source.state_dict() == sd['source'] and torch.equal(other.source.state, first.source.state)
    assert _bits_equal(other.select_action(frames), first.select_action(frames))
    want, got = first.update(env.replay, N), other.update(env.replay, N)
    torch.cuda.synchronize()
    assert _bits_equal(got, want), (got, want)
    _same_agents(other, first, 2)
    assert other.source.calls() == first.source.calls() == [3, 3, 3, 0]
    # and it is NumPy's noise that continued: the twin on the checker's draws of call 2 gives the action the loaded agent gave next
    tor, _ = sa._agent(C)
    tor.load_state_dict({k: v for k, v in first.state_dict().items() if k != 'source'})
    assert _bits_equal(tor.select_action(frames, eps=_eps(0, 3, int(frames.shape[0]))), other.select_action(frames))
    env.close()


def test_the_torch_mode_is_what_it_was(assets):
    """draws='torch' (the default): no source, the state_dict's keys and _graph_key as they were before the device's draws existed."""
    from red_gym_amd import SACAgent
    env = sa._ring_env(assets, C, steps=2)
    agent, _ = sa._agent(C)
    assert agent.source is None
    assert sorted(agent.state_dict()) == sorted(list(uc.NETS) + [n + '_optimizer' for n in uc.TRAINED] + ['draws'])
    replay = env.replay
    opts = agent.optimizers().values()
    assert agent._graph_key(replay, N) == (id(replay), replay.generation, replay.steps, replay.eng.B, replay._seed(None), N,
                                           tuple((o.lr, o.betas, o.eps, o.tau) for o in opts))
    dev = _device_agent()
    key = dev._graph_key(replay, N)
    assert key[:-1] == agent._graph_key(replay, N) and key[-1] == ('source', dev.source.state.data_ptr())
    assert sorted(dev.state_dict()) == sorted(list(agent.state_dict()) + ['source'])
    with pytest.raises(ValueError):
        SACAgent(draws='numpy', **sa._kw(C))
    env.close()
