"""SACAgent(stack=k) and SACAgent.act_from: stack = 1 is the agent without the option (parameters, losses, graph key) and act_from is
select_action on the bitmap the step returned; stack = 3 is update_batch on a batch assembled by hand from frames_at(..., stack=3);
replays are eager updates; stack is part of the graph key; and an agent that shares five torch.nn networks with a 3-channel conv1 stays
within the project's 8 x framework-error bound of the fp64 mirror of tests/update_cases.py fed the unpacked stacks."""
import numpy as np
import pytest

import update_cases as uc
from test_gpu_sac_agent import FACTOR, FLOOR, SEED, SMALL, _agent_update, _differing, _force, _judge, _kw, _mirror_update, _ring_env, _snapshot

pytestmark = pytest.mark.gpu

K = 3


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _eps(gen, n, A):
    import torch
    return tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))


def _mirror(c, dtype, device, k, seed=None):
    """uc.MirrorAgent whose five conv1 take k input channels (the targets' loaded from the critics'), optimizers over the new tensors."""
    import torch
    m = uc.MirrorAgent(dtype=torch.float32, device='cpu', seed=seed, **_kw(c))
    if k > 1:
        for name in uc.NETS:
            m.net(name).conv1 = torch.nn.Conv2d(k, 16, kernel_size=8, stride=4)
        for name in ('critic1', 'critic2'):
            m.net(name + '_target').load_state_dict(m.net(name).state_dict())
    m.dtype, m.device = dtype, torch.device(device)
    for name in uc.NETS:
        m.net(name).to(device=m.device, dtype=dtype)
    m.optimizers = {name: torch.optim.Adam(m.net(name).parameters(), lr=uc.LR) for name in uc.TRAINED}
    return m


def _agent(c, stack=None, seed=SEED):
    """(a SACAgent on the tensors of a new fp32 mirror on the GPU, that mirror); stack=None: built without the option, on one-frame networks."""
    import torch
    from red_gym_amd import SACAgent
    m = _mirror(c, torch.float32, 'cuda', 1 if stack is None else stack, seed)
    kw = {} if stack is None else dict(stack=stack)
    return SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, **kw, **_kw(c)), m


def test_stack_1_is_the_agent_without_the_option(assets):
    """Three updates of SACAgent(stack=1) and of an agent built without the option: every parameter, moment, loss and index `==`, the same
    graph key, the same tensors in the sample; and what the constructor refuses."""
    import torch
    from red_gym_amd import SACAgent
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    (plain, _), (one, _) = _agent(c), _agent(c, 1)
    assert one.stack == 1 == plain.stack and _differing(_snapshot(one), _snapshot(plain)) == []
    assert one._graph_key(env.replay, n) == plain._graph_key(env.replay, n) and 'stack' not in str(plain._graph_key(env.replay, n))
    gen = torch.Generator(device='cuda').manual_seed(11)
    for u in range(3):
        eps = _eps(gen, n, A)
        lp, lo = plain.update(env.replay, n, eps=eps), one.update(env.replay, n, eps=eps)
        assert _same_bits(lp, lo) and _differing(_snapshot(one), _snapshot(plain)) == [], u
        assert sorted(one.sample) == sorted(plain.sample) == sorted(env.replay.sample_out(n)) and 's_stack' not in one.sample
        assert all(torch.equal(one.sample[k], plain.sample[k]) for k in plain.sample) and int(one.draws) == int(plain.draws) == (u + 1) * n
    assert 'stack' not in one.state_dict()
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError):
            SACAgent(stack=bad, **_kw(c))
    with pytest.raises(ValueError, match='in_channels'):                         # shared one-frame networks, stack = 3
        SACAgent(networks=_mirror(c, torch.float32, 'cuda', 1), stack=K, **_kw(c))
    with pytest.raises(ValueError, match='in_channels'):
        SACAgent(networks=_mirror(c, torch.float32, 'cuda', K), **_kw(c))
    own = SACAgent(stack=K, **_kw(c))
    assert all(tuple(net.trunk.conv1.weight.shape) == (16, K, 8, 8) for net in own.modules().values())
    assert env.eng.device_errors() == 0
    env.close()


def test_act_from_is_select_action_on_the_newest_frames(assets):
    """stack = 1: act_from(replay) `==` select_action(info['lidar_bitmap']) of the last step, evaluate and sampled, with torch's draws
    passed in and with the device's; stack = 3: `==` select_action on the ring's frame view with stack_latest's rows."""
    import torch
    from red_gym_amd import SACAgent
    c = SMALL
    A = c['action_dim']
    env = _ring_env(assets, c, steps=4)
    B = env.num_envs
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    _, _, _, info = env.step(acts)
    for stack in (1, K):
        agent, _ = _agent(c, stack)
        eps = torch.randn((B, A), device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
        rows, depth = env.replay.stack_latest(stack)
        assert bool((depth == min(stack, 5)).all())
        for kw in (dict(evaluate=True), dict(eps=eps)):
            got = agent.act_from(env.replay, **kw)
            if stack == 1:
                want = agent.select_action(info['lidar_bitmap'], **kw)
            else:
                want = agent.select_action(env.replay.frame_view(), rows, **kw)
            assert got.dtype == torch.float64 and tuple(got.shape) == (B, A) and torch.equal(got, want), (stack, sorted(kw))
        out = torch.zeros((B, A), dtype=torch.float64, device='cuda')
        assert agent.act_from(env.replay, eps=eps, out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)
    # the device's draws: row = the env number, as select_action on the whole batch numbers them
    a, b = (SACAgent(draws='device', seed=9, **_kw(c)) for _ in range(2))
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.act_from(env.replay), b.select_action(info['lidar_bitmap']))
    assert torch.equal(a.act_from(env.replay), b.select_action(info['lidar_bitmap'])) and env.eng.device_errors() == 0
    env.close()


def test_stack_3_is_update_batch_on_a_batch_assembled_by_hand(assets):
    """One update(stack = 3) `==` update_batch on frames_at(indices, stack=3)'s stacks, action, reward and done with the same eps; the
    stacks are not all full, and an agent that saw one frame per state could not have taken them (another graph key)."""
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    (three, _), (by_hand, _) = _agent(c, K), _agent(c, K)
    assert three.stack == K and _differing(_snapshot(three), _snapshot(by_hand)) == []
    eps = _eps(torch.Generator(device='cuda').manual_seed(12), n, A)
    l3 = three.update(env.replay, n, eps=eps)
    s = three.sample
    assert sorted(s) == sorted(env.replay.sample_out(n, stack=K))
    at = env.replay.frames_at(s['indices'], stack=K)
    frames, s_stack, ns_stack, a, r, d, ok, depth = (at[k] for k in ('frames', 's_stack', 'ns_stack', 'a', 'r', 'd', 'ok', 'depth'))
    assert torch.equal(at['s_idx'], s_stack[:, 0]) and torch.equal(at['ns_idx'], ns_stack[:, 0])
    assert bool(ok.all()) and tuple(s_stack.shape) == (n, K) and torch.equal(s_stack, s['s_stack']) and torch.equal(ns_stack, s['ns_stack'])
    assert torch.equal(depth, s['depth']) and bool((depth < K).any()) and bool((depth == K).any())
    assert torch.equal(s['s_idx'], s_stack[:, 0]) and torch.equal(s['ns_idx'], ns_stack[:, 0])
    lh = by_hand.update_batch(dict(frames=frames, s_idx=s_stack, ns_idx=ns_stack, a=a, r=r, d=d), eps=eps)
    assert _same_bits(l3, lh) and bool(torch.isfinite(l3).all()) and _differing(_snapshot(three), _snapshot(by_hand)) == []
    # the older frames matter: the same batch with every stack filled by its newest frame ends elsewhere
    (flat, _) = _agent(c, K)
    lf = flat.update_batch(dict(frames=frames, s_idx=s_stack[:, :1].repeat(1, K), ns_idx=ns_stack[:, :1].repeat(1, K), a=a, r=r, d=d), eps=eps)
    assert not _same_bits(lf, l3) and _differing(_snapshot(flat), _snapshot(three)) != []
    assert env.eng.device_errors() == 0
    env.close()


def test_stack_3_replays_equal_eager_updates_and_stack_is_in_the_graph_key(assets):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    (eager, _), (graph, _) = _agent(c, K), _agent(c, K)
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
        assert int(graph.draws) == int(eager.draws) == (u + 1) * n and 's_stack' in graph.sample
    # stack is part of the key, beside nstep; with the n-step walk the stacks follow the span's end
    (one, _) = _agent(c)
    key = graph._graph_key(env.replay, n)
    assert ('stack', K) in key and key != one._graph_key(env.replay, n) and ('stack', K) not in one._graph_key(env.replay, n)
    graph.nstep = 3
    assert graph._graph_key(env.replay, n) != key and ('stack', K) in graph._graph_key(env.replay, n)
    graph.update_graph(eps=eps)
    torch.cuda.synchronize()
    s = graph.sample
    assert graph.recaptured and graph.captures == 2 and 'span' in s and 's_stack' in s
    want_ns, _ = env.replay.stack_rows(s['ns_idx'], K)
    assert torch.equal(s['ns_stack'], want_ns) and env.eng.device_errors() == 0
    env.close()


def test_a_shared_three_channel_conv1_against_the_fp64_mirror():
    """One update_batch of an agent that shares five torch.nn networks with nn.Conv2d(3, 16, 8, 4): the losses and every parameter and
    target after it (conv1.weight among them: its step is driven by the stacked backward) are judged with e = ||x - x64|| / ||x64||
    against the fp64 mirror stepped from the same start on the unpacked stacks, e_lib <= 8 * max(e_torch32, 2^-23)."""
    import torch
    c = uc.CONFIGS['a']
    n, pool = c['n'], c['pool']
    agent, shared = _agent(c, K)
    m32, m64 = _mirror(c, torch.float32, 'cuda', K), _mirror(c, torch.float64, 'cpu', K)
    b = uc.batch(1000 * SEED + 7, n, c['rows'], c['cols'], c['action_dim'], pool)
    rng = np.random.default_rng([SEED, n, K])
    for key in ('s_idx', 'ns_idx'):                        # [n, K]: column 0 as drawn, older frames from the pool, the hole stays a hole
        older = rng.integers(0, pool, (n, K - 1)).astype(np.int64)
        older[b['hole']] = -1
        older[0, -1] = older[0, 0]                         # a repeat, as at an episode's start
        b[key] = np.concatenate([b[key][:, None], older], axis=1)
    bl = uc.lib_batch(b)
    assert tuple(bl['s_idx'].shape) == (n, K)

    def mirror_batch(dtype, device):
        mb = uc.mirror_batch(b, c['on'], dtype, device)
        mb['s'], mb['ns'] = mb['s'][:, 0], mb['ns'][:, 0]  # [n, 1, K, rows, cols] -> the K frames as channels
        assert tuple(mb['s'].shape) == (n, K, c['rows'], c['cols'])
        return mb

    _force(m32, agent, shared)
    _force(m64, agent, shared)
    t32 = _mirror_update(m32, mirror_batch(torch.float32, 'cuda'))
    t64 = _mirror_update(m64, mirror_batch(torch.float64, 'cpu'))
    before = _snapshot(agent)
    got = _agent_update(agent, bl)
    assert all(bool(torch.isfinite(got[k])) for k in got if k.startswith('loss.'))
    assert any('conv1.weight' in k for k in t64) and tuple(got['after.critic1.conv1.weight'].shape) == (16, K, 8, 8)
    missed = _judge('stack=%d n=%d' % (K, n), got, t32, t64)
    assert len(_differing(before, _snapshot(agent))) == len(before['params']) * 10 + 2 + 3 * 3      # every tensor and state word moved
    assert FACTOR == 8.0 and FLOOR == 2.0 ** -23 and not missed, '\n' + '\n'.join(missed)
