"""red_gym_amd.sac.SACAgent: the library's own agent against tests/update_cases.py -- LibAgent (the composition of
examples/sac_update.py that test_gpu_update.py pins on the fp64 mirror) bit for bit at a power-of-two batch, the fp64 mirror itself under
test_gpu_update.py's tolerance rule at n = 24, the captured update against the eager one, acting, the state dicts and the examples.

At n = 16 the agent's loss kernels hand autograd the gradients the framework's own expressions give, bit for bit (2 / n, 1 / n and
alpha / n are exact scalings), and everything behind them is the same kernels on the same tensors: `==` is required of every parameter,
target, moment and state word.  The loss VALUES are summed in another order than the framework's, so they (and, at n = 24, the
parameters) are judged with e = ||x - x64|| / ||x64|| against the fp64 mirror stepped from the same parameters and moments: e_lib <=
8 * max(e_torch32, 2^-23), e_torch32 the fp32 mirror's own error on the same start (test_gpu_update.py says where the 8 comes from)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import update_cases as uc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(rows=68, cols=76, hidden=96, action_dim=16, n=16, on=1.0, pool=20)
SEED = 6
FACTOR, FLOOR = 8.0, 2.0 ** -23


def _kw(c):
    return dict(rows=c['rows'], cols=c['cols'], hidden=c['hidden'], action_dim=c['action_dim'], on=c['on'])


def _agent(c, seed=SEED):
    """(a SACAgent on the tensors of a new fp32 mirror on the GPU, that mirror)."""
    import torch
    from red_gym_amd import SACAgent
    m = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=seed, **_kw(c))
    agent = SACAgent(networks=m, gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, **_kw(c))
    for name, mod in agent.modules().items():
        shared = {uc.lib_key(k): p for k, p in mod.named_parameters()}
        assert list(shared) == uc.keys_of(name) and all(shared[k] is m.net(name).get_parameter(k) for k in shared)
    return agent, m


def _snapshot(agent):
    return uc.LibAgent.snapshot(agent)                    # (SACAgent has LibAgent's modules() and optimizers())


def _differing(a, b):
    """The names of what differs between two snapshots (raw bits)."""
    import torch
    bad = ['%s.%s' % (n, k) for n in a['params'] for k in a['params'][n] if not torch.equal(a['params'][n][k].view(torch.int32), b['params'][n][k].view(torch.int32))]
    for n in a['opt']:
        bad += ['%s.%s' % (n, w) for w, x, y in zip(('exp_avg', 'exp_avg_sq', 'state'), a['opt'][n], b['opt'][n])
                if not torch.equal(x.view(torch.int32), y.view(torch.int32))]
    return bad


def _force(mirror, agent, source):
    """A mirror started where the agent stands: `source`'s parameters and the agent's Adam moments and step counts."""
    mirror.load_from(source)
    for name, opt in agent.optimizers().items():
        mirror.optimizers[name].load_state_dict(opt.state_dict())


def _judge(tag, got, t32, t64):
    missed = []
    for k in sorted(t64):
        e32, el = uc.rel_err(t32[k], t64[k]), uc.rel_err(got[k], t64[k])
        line = '%s %-34s e_torch32 %.3e e_lib %.3e ratio %.3f' % (tag, k, e32, el, el / max(e32, FLOOR))
        print(line)
        if not el <= FACTOR * max(e32, FLOOR):
            missed.append(line + '  ABOVE %g' % FACTOR)
    return missed


def _mirror_update(mirror, b):
    """composed_update -> {the three losses and every parameter and target after it}."""
    cp, ap = mirror.composed_update(b, b['eps_next'], b['eps_new'])
    out = {'loss.actor': ap['a_loss'], 'loss.critic1': cp['c_loss'][0], 'loss.critic2': cp['c_loss'][1]}
    for name in uc.NETS:
        out.update({'after.%s.%s' % (name, k): mirror.net(name).get_parameter(k).detach() for k in uc.keys_of(name)})
    return out


def _agent_update(agent, bl):
    losses = agent.update_batch(bl, eps=(bl['eps_next'], bl['eps_new']))
    out = {'loss.actor': losses[0], 'loss.critic1': losses[1], 'loss.critic2': losses[2]}
    for name, mod in agent.modules().items():
        out.update({'after.%s.%s' % (name, uc.lib_key(k)): p.detach() for k, p in mod.named_parameters()})
    return out


def _three_updates(c, judge_keys, lib=None):
    """Three teacher-forced update_batch calls; each is judged on `judge_keys(key)` against the fp64 mirror stepped from the same
    parameters and moments, and, with `lib`, compared bit for bit with LibAgent's two phases."""
    import torch
    agent, shared = _agent(c)
    m32 = uc.MirrorAgent(dtype=torch.float32, device='cuda', **_kw(c))
    m64 = uc.MirrorAgent(dtype=torch.float64, device='cpu', **_kw(c))
    missed = []
    for u in range(uc.UPDATES):
        b = uc.batch(1000 * SEED + u, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])
        bl = uc.lib_batch(b)
        _force(m32, agent, shared)
        _force(m64, agent, shared)
        t32 = _mirror_update(m32, uc.mirror_batch(b, c['on'], torch.float32, 'cuda'))
        t64 = _mirror_update(m64, uc.mirror_batch(b, c['on'], torch.float64, 'cpu'))
        before = _snapshot(agent)
        got = _agent_update(agent, bl)
        assert got['loss.actor'].dtype == torch.float32 and all(bool(torch.isfinite(got[k])) for k in got if k.startswith('loss.'))
        keys = [k for k in t64 if judge_keys(k)]
        missed += _judge('n=%d u%d' % (c['n'], u), got, t32, {k: t64[k] for k in keys})
        after = _snapshot(agent)
        assert len(_differing(before, after)) == len(before['params']) * 10 + 2 + 3 * 3      # every tensor and state word moved
        if lib is not None:
            lib_agent, _ = lib
            cp = lib_agent.critic_phase(bl, bl['eps_next'])
            ap = lib_agent.actor_phase(bl, bl['eps_new'])
            assert _differing(lib_agent.snapshot(), after) == [], u
            # the framework's own losses on the same q, tv, log_prob: the critics' are n squares, n - 1 additions and a division in
            # fp32 on positive terms, (n + 2) * 2^-24 to first order; the actor's is formed in fp64 (log_prob is), one rounding from ours
            for mine, theirs in ((got['loss.actor'], ap['a_loss']), (got['loss.critic1'], cp['c_loss'][0]), (got['loss.critic2'], cp['c_loss'][1])):
                assert abs(float(mine) - float(theirs)) <= (c['n'] + 2) * 2.0 ** -24 * abs(float(theirs)), (u, float(mine), float(theirs))
    return missed


def test_three_updates_equal_libagent_at_a_power_of_two():
    import torch
    c = SMALL
    assert c['n'] & (c['n'] - 1) == 0
    lib_mirror = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=SEED, **_kw(c))
    lib = uc.LibAgent.from_mirror(lib_mirror, c['cols'])
    missed = _three_updates(c, lambda k: k.startswith('loss.'), lib=(lib, lib_mirror))
    assert not missed, '\n' + '\n'.join(missed)


def test_three_updates_against_the_fp64_mirror_at_n_24():
    c = uc.CONFIGS['a']
    assert c['n'] == 24
    missed = _three_updates(c, lambda k: True)
    assert not missed, '\n' + '\n'.join(missed)


def _ring_env(assets, c, B=8, T=6, steps=10):
    import torch
    from red_gym_amd import F110VecEnv, workload
    env = F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, autoreset=True)
    env.shape_rewards(rows=c['rows'], cols=c['cols'])
    env.record_replay(steps=T, action_dim=c['action_dim'])
    env.reset(workload.spawn_poses(B, 1))
    gen = torch.Generator(device=env.device).manual_seed(3)
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    for k in range(steps):
        env.replay_action.copy_(torch.rand((B, c['action_dim']), device=env.device, generator=gen) * 2.0 - 1.0)
        acts[:, 0, 0] = 0.1 * (k % 3 - 1)
        acts[:, 0, 1] = 2.0
        env.step(acts)
    return env


def test_graph_replays_equal_eager_updates(assets):
    """Two agents from one start on one ring: three update_graph(eps=...) replays against three eager update(eps=...) calls.
    Parameters, targets, moments, state words, losses, the drawn indices and the draw counter are `==` after each; the capture moved
    nothing; the second replay drew other transitions than the first."""
    import torch
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c)
    eager, _ = _agent(c)
    graph, _ = _agent(c)
    start = _snapshot(graph)
    assert _differing(_snapshot(eager), start) == []
    losses = graph.capture_update(env.replay, n, draws=False)
    torch.cuda.synchronize()
    assert _differing(_snapshot(graph), start) == [] and int(graph.draws) == 0 and not losses.any() and graph.captures == 1
    gen = torch.Generator(device='cuda').manual_seed(11)
    drawn = []
    for u in range(3):
        eps = tuple(torch.randn((n, A), device='cuda', generator=gen) for _ in range(2))
        want = eager.update(env.replay, n, eps=eps)
        got = graph.update_graph(eps=eps)
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(torch.isfinite(got).all()), (u, got, want)
        assert _differing(_snapshot(graph), _snapshot(eager)) == [], u
        assert torch.equal(graph.sample['indices'], eager.sample['indices']) and all(torch.equal(graph.sample[k], eager.sample[k]) for k in eager.sample)
        assert int(graph.draws) == int(eager.draws) == (u + 1) * n
        assert bool(graph.sample['ok'].all())
        drawn.append(graph.sample['indices'].clone())
    assert not torch.equal(drawn[0], drawn[1])
    assert len(_differing(_snapshot(graph), start)) > 50
    assert env.eng.device_errors() == 0
    env.close()


def test_recapture_check_and_the_variant_that_draws(assets):
    """update(check=True) on a ring with fewer valid transitions than the batch returns zeros and changes nothing; a re-installed
    ring, and a changed lr, make update_graph capture again (the flag, not a fault); the variant that records torch.randn replays."""
    import torch
    c = SMALL
    n = c['n']
    env = _ring_env(assets, c, steps=1)                       # two frames per env: 8 valid transitions at most, fewer than 16
    agent, _ = _agent(c)
    start = _snapshot(agent)
    assert 0 < len(env.replay) < n
    out = agent.update(env.replay, n, check=True)
    assert out.shape == (3,) and not out.any() and _differing(_snapshot(agent), start) == [] and int(agent.draws) == 0
    env.close()
    env = _ring_env(assets, c)
    agent.capture_update(env.replay, n)
    agent.update_graph()
    assert not agent.recaptured and agent.captures == 1 and int(agent.draws) == n
    first = agent.update_graph().clone()
    assert agent.captures == 1 and bool(torch.isfinite(first).all()) and int(agent.draws) == 2 * n
    env.record_replay(steps=6, action_dim=c['action_dim'])      # a new ring: the old one's tensors are freed
    losses = agent.update_graph()
    assert agent.recaptured and agent.captures == 2
    torch.cuda.synchronize()
    assert not agent.sample['ok'].any() and bool(torch.isfinite(losses).all())       # (an empty ring: zero transitions, as documented)
    agent.update_graph()
    assert not agent.recaptured and agent.captures == 2
    agent.actor_opt.lr = 1e-4
    agent.update_graph()
    assert agent.recaptured and agent.captures == 3
    agent.update_graph(eps=tuple(torch.zeros((n, c['action_dim']), device='cuda') for _ in range(2)))
    assert not agent.recaptured and agent.captures == 4           # the other variant, captured on first use
    torch.cuda.synchronize()
    assert int(agent.draws) == 6 * n and env.eng.device_errors() == 0
    env.close()


def test_select_action():
    """The sampled action `==` LibActor.sample on the same draws, evaluate=True `==` tanh(mean); a row alone `==` that row in the
    batch; out= receives the action; uint8 bitmaps give what their bits give."""
    import torch
    from red_gym_amd import replay
    c = SMALL
    agent, m = _agent(c)
    lib_actor = uc.LibActor(m.actor, c['on'], c['cols'])
    b = uc.batch(1000 * SEED, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])
    bl = uc.lib_batch(b)
    eps = bl['eps_new']
    with torch.no_grad():
        want, _ = lib_actor.sample(bl['frames'], bl['s_idx'], eps)
        mean, _ = agent.actor.head(agent.actor.features(bl['frames'], bl['s_idx']))
    got = agent.select_action(bl['frames'], bl['s_idx'], eps=eps)
    assert got.dtype == torch.float64 and got.shape == (c['n'], c['action_dim']) and got.grad_fn is None and torch.equal(got, want)
    ev = agent.select_action(bl['frames'], bl['s_idx'], evaluate=True)
    assert torch.equal(ev, torch.tanh(mean.double())) and not torch.equal(ev, got)
    for i in (0, b['hole'], c['n'] - 1):
        assert torch.equal(agent.select_action(bl['frames'], bl['s_idx'][i:i + 1], eps=eps[i:i + 1])[0], got[i]), i
        assert torch.equal(agent.select_action(bl['frames'], bl['s_idx'][i:i + 1], evaluate=True)[0], ev[i]), i
    out = torch.zeros_like(got)
    assert agent.select_action(bl['frames'], bl['s_idx'], eps=eps, out=out) is out and torch.equal(out, got)
    imgs = torch.as_tensor(b['imgs'], device='cuda')
    assert torch.equal(replay.pack_bitmaps(imgs), bl['frames'])
    rows = bl['s_idx'].clamp(min=0)
    assert torch.equal(agent.select_action(imgs, rows, evaluate=True), agent.select_action(bl['frames'], rows, evaluate=True))
    a1, a2 = agent.select_action(bl['frames'], bl['s_idx']), agent.select_action(bl['frames'], bl['s_idx'])
    assert not torch.equal(a1, a2) and float(a1.abs().max()) <= 1.0                  # without eps: fresh torch.randn draws


def test_state_dicts():
    """actor_state_dict() has exactly the reference's keys and loads into a MirrorActor with strict=True; a state_dict round trip into
    a fresh agent (another initialisation, its own networks), then one update, is `==` the original's."""
    import torch
    from red_gym_amd import SACAgent
    c = SMALL
    agent, _ = _agent(c)
    batches = [uc.lib_batch(uc.batch(1000 * SEED + u, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])) for u in range(2)]
    agent.update_batch(batches[0], eps=(batches[0]['eps_next'], batches[0]['eps_new']))
    agent.draws.fill_(77)
    sd = {k: v.clone() for k, v in agent.actor_state_dict().items()}          # (the dict holds the live tensors, as a module's does)
    assert list(sd) == uc.ACTOR_KEYS
    fresh_actor = uc.MirrorActor(uc.feature_width(c['rows'], c['cols']), c['hidden'], c['action_dim'])
    fresh_actor.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    full = agent.state_dict()
    assert sorted(full) == sorted(list(uc.NETS) + [n + '_optimizer' for n in uc.TRAINED] + ['draws']) and full['draws'] == 77
    assert all(list(full[n]) == uc.keys_of(n) for n in uc.NETS)
    torch.manual_seed(99)
    other = SACAgent(gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, **_kw(c))
    assert _differing(_snapshot(other), _snapshot(agent)) != []
    other.load_state_dict(full)
    # every tensor is back; of the optimizers' device state the step count and the two powers are (k2 and a are outputs of the next
    # step's advance, which a load leaves at zero)
    assert all(name.endswith('.state') for name in _differing(_snapshot(other), _snapshot(agent))) and int(other.draws) == 77
    assert all(o.device_state()[:3] == p.device_state()[:3] and p.device_state()[0] == 1
               for o, p in zip(other.optimizers().values(), agent.optimizers().values()))
    eps = (batches[1]['eps_next'], batches[1]['eps_new'])
    la, lo = agent.update_batch(batches[1], eps=eps), other.update_batch(batches[1], eps=eps)
    assert torch.equal(la.view(torch.int32), lo.view(torch.int32)) and _differing(_snapshot(other), _snapshot(agent)) == []
    other.load_actor_state_dict(sd)
    assert torch.equal(other.actor.fc1.weight, sd['fc1.weight']) and not torch.equal(other.actor.fc1.weight, agent.actor.fc1.weight)
    with pytest.raises(ValueError):
        other.load_actor_state_dict({k: v for k, v in sd.items() if k != 'fc1.bias'})
    with pytest.raises(ValueError):
        SACAgent(device='cpu', **_kw(c))


@pytest.mark.parametrize('example,args,marks', [('sac_update.py', ['64', '12', '16'], ['update 1:', 'update 3:', 'feature columns filled: True, action columns filled: True']),
                                                ('sac_train.py', [], ['losses', 'captures 1'])])
def test_the_examples_run(example, args, marks):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', example)] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    for mark in marks:
        assert mark in proc.stdout, (mark, proc.stdout[-2000:])
    assert 'nan' not in proc.stdout.lower()
