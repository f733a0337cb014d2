"""Generates tests/golden/g21_critic.npz from the reference's own SACAgent.update (src/SAL.py:521-580) on the CPU: one call per group
of 16 transitions, with a stub buffer whose sample() returns prepared arrays.  Hooks record what the critics' tails see and make, not
a restatement of them: the input and output of every fc1 (the two target critics in the no_grad block, the two critics on (s, a)),
what each critic returns, what actor.sample returns, the (cq, tv) pairs that reach F.mse_loss, the two critic losses, and through an
optimizer step pre-hook the gradients of fc2.weight, fc2.bias, fc1.bias and fc1.weight[:, F:] as they stand before each critic's step.
From the captured fc1 inputs the fixture keeps the feature part pre = f @ W[:, :F].T (fp64, rounded once to fp32), the absolute-value
dot products sum |w||x| + |b| per (row, unit) (rounded UP to fp16: they only enter bounds), the small parameters, and per group
fc1_rel_err = max |z_ref - z_64| / sum |w||x|: the reference's own fc1 output against its fp64 recomputation.  Data only.

Groups (qhead_cases.GROUPS): images fed as 0 / 1 with critic2_target.fc2.bias shifted so that each side of the min wins half of the
rows; images as 0 / 255 (what update() feeds, :536) with such a shift; and 0 / 255 with the default initialisation.
Run through make_golden.py.
"""
import numpy as np
import torch

import reference
import qhead_cases as qc
from reference import StubBuffer

# per group: the value of a set pixel, whether critic2_target.fc2.bias is shifted to balance the min
MODS = ((1.0, True), (255.0, True), (255.0, False))
CRITICS = ('critic1_target', 'critic2_target', 'critic1', 'critic2')
F, A, H = 32 * 28 * 28, 16, 512


def round_up_fp16(x):
    h = x.astype(np.float16)
    h = np.where(h.astype(np.float64) < x, np.nextafter(h, np.float16(np.inf)), h)
    assert (h.astype(np.float64) >= x).all() and np.isfinite(h).all()
    return h


def run_update(sal, agent, arrays):
    """One agent.update on `arrays` with every hook in place -> dict of what they saw."""
    seen = {'fc1': {k: [] for k in CRITICS}, 'ret': {k: [] for k in CRITICS}, 'sample': [], 'mse': [], 'grads': {}}
    handles = []
    for name in CRITICS:
        net = getattr(agent, name)
        handles.append(net.fc1.register_forward_hook(lambda m, i, o, name=name: seen['fc1'][name].append((i[0].detach().clone(), o.detach().clone()))))
        handles.append(net.register_forward_hook(lambda m, i, o, name=name: seen['ret'][name].append(o.detach().clone())))
    for name in ('critic1', 'critic2'):
        net = getattr(agent, name)

        def pre_step(opt, args, kwargs, net=net, name=name):
            seen['grads'][name] = dict(w2=net.fc2.weight.grad.clone(), b2=net.fc2.bias.grad.clone(), b1=net.fc1.bias.grad.clone(),
                                       w_act=net.fc1.weight.grad[:, F:].clone())
        handles.append(getattr(agent, name + '_optimizer').register_step_pre_hook(pre_step))
    sample = agent.actor.sample

    def recording_sample(x):
        out = sample(x)
        seen['sample'].append(tuple(t.detach().clone() for t in out))
        return out
    agent.actor.sample = recording_sample
    mse = sal.F.mse_loss

    def recording_mse(a, b, *args, **kw):
        seen['mse'].append((a.detach().clone(), b.detach().clone()))
        return mse(a, b, *args, **kw)
    sal.F.mse_loss = recording_mse
    try:
        seen['losses'] = agent.update(StubBuffer(arrays), batch_size=len(arrays[0]))
    finally:
        sal.F.mse_loss = mse
        del agent.actor.sample
        for h in handles:
            h.remove()
    return seen


def g21_critic():
    sal = reference.load_sal()
    torch.manual_seed(21)
    torch.set_num_threads(1)
    agent = sal.SACAgent(torch.device('cpu'), action_dim=A)
    nets = CRITICS + ('actor',)
    base = {k: {n: v.clone() for n, v in getattr(agent, k).state_dict().items()} for k in nets}
    rng = np.random.default_rng(21)
    R = qc.GROUP_ROWS
    out = {k: [] for k in ('pre', 'mag', 'action', 'ret', 'next_logp', 'reward', 'done', 'cq', 'tv', 'losses', 'b2', 'fc1_rel_err', 'shift',
                           'grad_w2', 'grad_b2', 'grad_b1', 'grad_w_act')}
    active, near = [], []
    for gi, (on, balance) in enumerate(MODS):
        blocks = [rng.random((R, 32, 32)) < rng.uniform(0.2, 0.8, (R, 1, 1)) for _ in range(2)]
        s, ns = ((np.kron(b, np.ones((8, 8))) * on).astype(np.float32) for b in blocks)
        a = np.tanh(rng.normal(size=(R, A))).astype(np.float32)
        r = rng.normal(size=R)
        d = rng.random(R) < 0.5
        arrays = (s, a, r, ns, d)
        shift = np.float32(0.0)
        for attempt in range(2 if balance else 1):                      # a dry run measures tq1 - tq2, the recorded run has the shift
            for k in nets:
                getattr(agent, k).load_state_dict(base[k])
            with torch.no_grad():
                agent.critic2_target.fc2.bias.add_(float(shift))
            torch.manual_seed(2100 + gi)
            seen = run_update(sal, agent, arrays)
            if balance and attempt == 0:
                shift = np.float32(np.median((seen['ret']['critic1_target'][0] - seen['ret']['critic2_target'][0]).numpy()))
        assert len(seen['sample']) == 2 and len(seen['mse']) == 2 and all(len(seen['fc1'][k]) == (1 if 'target' in k else 2) for k in CRITICS)
        next_a, next_logp = seen['sample'][0]
        pres, mags, acts, rets, b2s, rel = [], [], [], [], [], 0.0
        for name in CRITICS:
            x, z_ref = seen['fc1'][name][0]                               # the first call: (ns, next_a) for the targets, (s, a) for the critics
            W, b = base[name]['fc1.weight'].double(), base[name]['fc1.bias'].double()
            x64 = x.double()
            assert torch.equal(x[:, F:], next_a if 'target' in name else torch.from_numpy(a))
            pres.append((x64[:, :F] @ W[:, :F].T).numpy().astype(np.float32))
            mag = (x64.abs() @ W.abs().T + b.abs()).numpy()
            z64 = (x64 @ W.T + b).numpy()
            rel = max(rel, float((np.abs(z_ref.numpy().astype(np.float64) - z64) / mag).max()))
            mags.append(round_up_fp16(mag))
            acts.append(x[:, F:].numpy())
            rets.append(seen['ret'][name][0].numpy()[:, 0])
            b2s.append(base[name]['fc2.bias'].numpy()[0] + (shift if name == 'critic2_target' else np.float32(0.0)))
            dz = qc.dz_bound(mags[-1].astype(np.float64), rel, A)
            active.append(z64 > 0)
            near.append((np.abs(z64), dz))
        out['pre'].append(np.stack(pres))
        out['mag'].append(np.stack(mags))
        out['action'].append(np.stack(acts))
        out['ret'].append(np.stack(rets))
        out['b2'].append(np.array(b2s, np.float32))
        out['fc1_rel_err'].append(rel)
        out['shift'].append(shift)
        out['next_logp'].append(next_logp.numpy()[:, 0])
        out['reward'].append(r)
        out['done'].append(d.astype(np.uint8))
        (cq1, tv1), (cq2, tv2) = seen['mse']
        assert torch.equal(tv1, tv2) and torch.equal(cq1, seen['ret']['critic1'][0]) and torch.equal(cq2, seen['ret']['critic2'][0])
        out['cq'].append(np.stack([cq1.numpy()[:, 0], cq2.numpy()[:, 0]]))
        out['tv'].append(tv1.numpy()[:, 0])
        out['losses'].append(np.array(seen['losses'][1:], np.float64))  # (a_loss, c1_loss, c2_loss): the two critic losses, .item() of fp32
        for key in ('w2', 'b2', 'b1', 'w_act'):
            out['grad_' + key].append(np.stack([seen['grads'][n][key].numpy().reshape((H, A) if key == 'w_act' else -1) for n in ('critic1', 'critic2')]))
    fix = {k: np.stack(v) for k, v in out.items()}
    fix['fc1_rel_err'] = fix['fc1_rel_err'].astype(np.float64)
    for name, key in (('w_act', 'fc1.weight'), ('b1', 'fc1.bias'), ('w2', 'fc2.weight')):
        pair = [base[n][key].numpy() for n in ('critic1', 'critic2')]
        fix[name] = np.stack([p[:, F:] if name == 'w_act' else p.reshape(-1) for p in pair])
        assert all(torch.equal(base[n][key], base[n + '_target'][key]) for n in ('critic1', 'critic2'))
    fix['keys'] = np.array(list(base['critic1'].keys()))
    fix['on'] = np.array([m[0] for m in MODS], np.float32)
    # the conditions of the fixture
    tq = fix['ret'][:, :2]                                               # [G, 2, R]: the target critics
    side = {'tq1 < tq2': float((tq[:, 0] < tq[:, 1]).mean()), 'tq2 < tq1': float((tq[:, 1] < tq[:, 0]).mean())}
    done_share = float(fix['done'].mean())
    active_share = float(np.mean([m.mean() for m in active]))
    near_share = float(np.mean([(z <= dz).mean() for z, dz in near]))
    print(side, 'd = 1: %.3f' % done_share, 'active: %.3f' % active_share, 'within dz of zero: %.5f' % near_share, 'fc1_rel_err', fix['fc1_rel_err'],
          'shift', fix['shift'])
    assert min(side.values()) >= 0.25, side
    assert 0.25 <= done_share <= 0.75, done_share
    assert 0.20 <= active_share <= 0.80 and all(0.20 <= m.mean() <= 0.80 for m in active), active_share
    assert near_share <= 0.01, near_share
    assert all(v.dtype in (np.float32, np.float64, np.float16, np.uint8) for k, v in fix.items() if k != 'keys')
    assert reference.save('g21_critic.npz', **fix) <= 1000000
