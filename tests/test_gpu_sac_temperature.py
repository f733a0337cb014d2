"""SACAgent(alpha='auto'): the temperature learnt on the device (red_gym_amd.temperature) inside the agent's update, at
test_gpu_sac_agent.py's SMALL shape.  The device-resident path is pinned, `==`, to the by-value path that file pins: the first update
against a twin agent with alpha = 0.2, three updates against a fixed-alpha agent whose alpha the host sets from a stand-alone
Temperature before each update, the captured update against the eager one, the state dicts, and the sign of a step."""
import numpy as np
import pytest

import update_cases as uc
from test_gpu_sac_agent import SEED, SMALL, _differing, _kw, _ring_env, _snapshot

pytestmark = pytest.mark.gpu


def _agent(c, alpha, seed=SEED, **kw):
    """A SACAgent on the tensors of a new fp32 mirror on the GPU: the same seed gives the same networks."""
    import torch
    from red_gym_amd import SACAgent
    m = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=seed, **_kw(c))
    return SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=alpha, actor_lr=uc.LR, critic_lr=uc.LR, **kw, **_kw(c))


def _batch(c, u):
    return uc.lib_batch(uc.batch(1000 * SEED + u, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool']))


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _words(t):
    return t.state_words().numpy()


def test_first_update_equals_the_fixed_alpha_twin():
    """The temperature before the first step is 0.2 exactly, so the first update moves every tensor as the twin's does."""
    c = SMALL
    auto, fixed = _agent(c, 'auto', init_alpha=0.2), _agent(c, 0.2)
    assert auto.temperature is not None and auto.alpha is auto.temperature.alpha and fixed.temperature is None and fixed.alpha == 0.2
    assert auto.temperature.target_entropy == -float(c['action_dim']) and float(auto.alpha.item()) == 0.2
    assert _differing(_snapshot(auto), _snapshot(fixed)) == []
    b = _batch(c, 0)
    la, lf = auto.update_batch(b, eps=(b['eps_next'], b['eps_new'])), fixed.update_batch(b, eps=(b['eps_next'], b['eps_new']))
    assert la.shape == lf.shape == (3,) and _same_bits(la, lf)
    assert _differing(_snapshot(auto), _snapshot(fixed)) == []
    sd = auto.temperature.state_dict()
    assert sd['step'] == 1 and sd['alpha'] != 0.2 and sd['alpha'] == float(auto.alpha.item())
    print('alpha after the first update: %r (log_alpha %r, loss %r, grad %r)' % (sd['alpha'], sd['log_alpha'], float(auto.temperature.loss.item()),
                                                                                  float(auto.temperature.grad.item())))


def _host_driven_update(agent, temp, b, losses):
    """SACAgent._update's pieces in its order on a fixed-alpha agent, the temperature stepped by the host behind the actor's loss."""
    import torch
    from red_gym_amd.qhead import td_target, twin_q
    from red_gym_amd.sac import _heads
    from red_gym_amd.sacloss import actor_loss, critic_loss
    frames, s_idx, ns_idx, a, r, d = (b[k] for k in ('frames', 's_idx', 'ns_idx', 'a', 'r', 'd'))
    actor, critics, targets = agent.actor, agent.critics, agent.targets
    agent.alpha = float(temp.alpha.item())
    with torch.no_grad():
        next_a, next_logp = actor.sample(frames, ns_idx, b['eps_next'])
        tv = td_target([t.trunk(frames, ns_idx) for t in targets], next_a, next_logp, r, d, *_heads(targets), agent.gamma, agent.alpha, dense=True)
    q, _ = twin_q([cr.trunk(frames, s_idx) for cr in critics], a, *_heads(critics), dense=True)
    grad_q = torch.empty_like(q)
    critic_loss(q[0], q[1], tv, loss=losses[1:3], grad=grad_q)
    for opt in agent.critic_opts:
        opt.zero_grad()
    torch.autograd.backward((q,), (grad_q,))
    for opt in agent.critic_opts:
        opt.step()
    new_a, logp = actor.sample(frames, s_idx, b['eps_new'])
    _, qn = twin_q([cr.trunk(frames, s_idx) for cr in critics], new_a, *_heads(critics), dense=True)
    _, g_logp, g_qn = actor_loss(logp, qn, agent.alpha, loss=losses[0:1])
    temp.step(logp.detach())
    agent.actor_opt.zero_grad()
    torch.autograd.backward((logp, qn), (g_logp, g_qn))
    agent.actor_opt.step()
    return losses


def test_three_updates_equal_a_host_driven_run():
    import torch
    from red_gym_amd.temperature import Temperature
    c = SMALL
    auto, host = _agent(c, 'auto', alpha_lr=1e-2), _agent(c, 0.2)
    temp = Temperature(init_alpha=0.2, target_entropy=-float(c['action_dim']), lr=1e-2)
    alphas = []
    for u in range(uc.UPDATES):
        b = _batch(c, u)
        got = auto.update_batch(b, eps=(b['eps_next'], b['eps_new']))
        want = _host_driven_update(host, temp, b, torch.empty(3, device='cuda'))
        assert _same_bits(got, want), (u, got, want)
        assert _differing(_snapshot(auto), _snapshot(host)) == [], u
        assert np.array_equal(_words(auto.temperature), _words(temp)), u
        alphas.append(float(temp.alpha.item()))
    print('alpha after each update:', alphas)
    assert len(set(alphas)) == 3 and host.alpha != 0.2          # the second and third updates ran on a temperature that had moved


def test_graph_replays_equal_eager_updates(assets):
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    eager, graph = _agent(c, 'auto', alpha_lr=1e-2), _agent(c, 'auto', alpha_lr=1e-2)
    start, start_t = _snapshot(graph), _words(graph.temperature)
    losses = graph.capture_update(env.replay, n, draws=False)
    torch.cuda.synchronize()
    assert _differing(_snapshot(graph), start) == [] and np.array_equal(_words(graph.temperature), start_t) and graph.captures == 1
    gen = torch.Generator(device='cuda').manual_seed(11)
    for u in range(3):
        eps = tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))
        want = eager.update(env.replay, n, eps=eps)
        got = graph.update_graph(eps=eps)
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert _same_bits(got, want) and bool(torch.isfinite(got).all()), (u, got, want)
        assert _differing(_snapshot(graph), _snapshot(eager)) == [], u
        assert np.array_equal(_words(graph.temperature), _words(eager.temperature)), u
    assert int(_words(graph.temperature)[0]) == 3 and float(graph.alpha.item()) != 0.2
    before = _words(graph.temperature).copy()
    graph.temperature.lr = 1e-3                                  # alpha_lr is a scalar of the captured launch
    eps = tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))
    eager.temperature.lr = 1e-3
    want = eager.update(env.replay, n, eps=eps)
    got = graph.update_graph(eps=eps)
    torch.cuda.synchronize()
    assert graph.recaptured and graph.captures == 2 and _same_bits(got, want)
    after = _words(graph.temperature)
    assert int(after[0]) == int(before[0]) + 1 and np.array_equal(after, _words(eager.temperature))      # the state was kept and stepped once
    assert env.eng.device_errors() == 0
    env.close()


def test_state_dicts_and_the_graph_key(assets):
    import torch
    c = SMALL
    agent = _agent(c, 'auto', alpha_lr=1e-2, init_alpha=0.3, target_entropy=-4.0)
    b0, b1 = _batch(c, 0), _batch(c, 1)
    agent.update_batch(b0, eps=(b0['eps_next'], b0['eps_new']))
    sd = agent.state_dict()
    assert sorted(sd) == sorted(list(uc.NETS) + [n + '_optimizer' for n in uc.TRAINED] + ['draws', 'temperature'])
    assert sorted(sd['temperature']) == sorted(['log_alpha', 'alpha', 'm', 'v', 'step', 'lr', 'betas', 'eps', 'target_entropy'])
    assert sd['temperature']['step'] == 1 and sd['temperature']['target_entropy'] == -4.0 and sd['temperature']['lr'] == 1e-2
    other = _agent(c, 'auto', seed=SEED + 1)
    assert _differing(_snapshot(other), _snapshot(agent)) != []
    other.load_state_dict(sd)
    assert (other.temperature.lr, other.temperature.target_entropy) == (1e-2, -4.0)
    la, lo = (x.update_batch(b1, eps=(b1['eps_next'], b1['eps_new'])) for x in (agent, other))
    assert _same_bits(la, lo) and _differing(_snapshot(other), _snapshot(agent)) == []
    assert np.array_equal(_words(other.temperature), _words(agent.temperature)) and int(_words(agent.temperature)[0]) == 2
    # with a number nothing changes: no key, the same graph key
    fixed = _agent(c, 0.2)
    assert 'temperature' not in fixed.state_dict() and sorted(fixed.state_dict()) == sorted(k for k in sd if k != 'temperature')
    env = _ring_env(assets, c, steps=2)
    kf, ka = fixed._graph_key(env.replay, c['n']), agent._graph_key(env.replay, c['n'])
    assert len(kf) == 7 and ka[:7] == kf and ka[7:] == ((1e-2, (0.9, 0.999), 1e-8, -4.0),)
    env.close()
    from red_gym_amd import SACAgent
    with pytest.raises(ValueError):
        SACAgent(alpha='learnt', **_kw(c))


def test_the_direction_of_a_step():
    """loss = -(log_alpha * mean(logp + H)): where the mean is positive (less entropy than the target) the gradient -mean is negative
    and alpha rises; where it is negative alpha falls."""
    import torch
    from red_gym_amd.temperature import Temperature
    for shift, sign in ((30.0, 1), (-30.0, -1)):
        t = Temperature(init_alpha=0.2, target_entropy=-16.0)
        logp = torch.full((64,), 16.0 + shift, dtype=torch.float64, device='cuda')
        assert float((logp + t.target_entropy).mean()) * sign > 0
        t.step(logp)
        assert (float(t.alpha.item()) - 0.2) * sign > 0 and float(t.grad.item()) == -shift, (shift, float(t.alpha.item()))
