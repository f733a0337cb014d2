"""Generates tests/golden/g24_update.npz from the reference's own SACAgent.update (src/SAL.py:521-580) on the CPU with one thread: one
call on a stub buffer of 8 transitions under a fixed seed.  Nothing of the update is restated here; wrappers record what it computes:
the standard-normal draw of both rsample calls as the distribution draws it (torch.distributions.normal._standard_normal), what
actor.sample returns, the (cq, tv) pairs that reach F.mse_loss, the second torch.min (qn), the three losses, through an optimizer step
pre-hook every parameter's .grad as it stands at its optimizer's step, and every tensor of the five networks after the update.

The fixture holds the batch (images as bits), both draws, those quantities, and per parameter tensor the fp64 sum and sum of squares
of its initial value (the check that a rebuild from the seed worked), its gradient's L2 norm, and 256 entries (all of a smaller tensor)
of the gradient and of the parameter after the update at positions drawn from a seed stored in the file.  Data only.
Run through make_golden.py.
"""
import numpy as np
import torch

import reference
import update_cases as uc
from reference import StubBuffer

SEED, DRAW_SEED, POSITION_SEED, ROWS, A, ENTRIES = 24, 2400, 240, 8, 16, 256


def positions(numel, key):
    """The sampled flat positions of a tensor: all of a small one, else ENTRIES drawn from (POSITION_SEED, key)."""
    if numel <= ENTRIES:
        return np.arange(numel, dtype=np.int64)
    return np.sort(np.random.default_rng([POSITION_SEED, key]).choice(numel, ENTRIES, replace=False)).astype(np.int64)


def run_update(sal, agent, arrays):
    seen = {'eps': [], 'sample': [], 'mse': [], 'min': [], 'grads': {}}
    handles = []
    for name in uc.TRAINED:
        net = getattr(agent, name)

        def pre_step(opt, args, kwargs, net=net, name=name):
            seen['grads'][name] = {k: p.grad.clone() for k, p in net.named_parameters()}
        handles.append(getattr(agent, name + '_optimizer').register_step_pre_hook(pre_step))
    normal = torch.distributions.normal
    draw, sample, mse, tmin = normal._standard_normal, agent.actor.sample, sal.F.mse_loss, torch.min

    def recording_draw(*args, **kw):
        eps = draw(*args, **kw)
        seen['eps'].append(eps.detach().clone())
        return eps

    def recording_sample(x):
        out = sample(x)
        seen['sample'].append(tuple(t.detach().clone() for t in out))
        return out

    def recording_mse(a, b, *args, **kw):
        seen['mse'].append((a.detach().clone(), b.detach().clone()))
        return mse(a, b, *args, **kw)

    def recording_min(*args, **kw):
        out = tmin(*args, **kw)
        if len(args) == 2 and torch.is_tensor(args[1]):
            seen['min'].append(out.detach().clone())
        return out

    normal._standard_normal, agent.actor.sample, sal.F.mse_loss, torch.min = recording_draw, recording_sample, recording_mse, recording_min
    try:
        seen['losses'] = agent.update(StubBuffer(arrays), batch_size=len(arrays[0]))
    finally:
        normal._standard_normal, sal.F.mse_loss, torch.min = draw, mse, tmin
        del agent.actor.sample
        for h in handles:
            h.remove()
    return seen


def g24_update():
    sal = reference.load_sal()
    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    agent = sal.SACAgent(torch.device('cpu'), action_dim=A)
    init = {n: {k: v.clone() for k, v in getattr(agent, n).state_dict().items()} for n in uc.NETS}
    assert all(list(init[n]) == uc.keys_of(n) for n in uc.NETS)
    rng = np.random.default_rng(SEED)
    blocks = [rng.random((ROWS, 32, 32)) < rng.uniform(0.2, 0.8, (ROWS, 1, 1)) for _ in range(2)]
    s, ns = ((np.kron(b, np.ones((8, 8))) * 255.0).astype(np.float32) for b in blocks)
    a = np.tanh(rng.normal(size=(ROWS, A))).astype(np.float32)
    r = rng.normal(size=ROWS)
    d = rng.random(ROWS) < 0.5
    assert 0 < d.sum() < ROWS
    torch.manual_seed(DRAW_SEED)
    seen = run_update(sal, agent, (s, a, r, ns, d))
    assert len(seen['eps']) == 2 and len(seen['sample']) == 2 and len(seen['mse']) == 2 and len(seen['min']) == 2, {k: len(v) for k, v in seen.items() if k != 'losses'}
    (cq1, tv1), (cq2, tv2) = seen['mse']
    assert torch.equal(tv1, tv2)
    fix = dict(seed=np.int64(SEED), position_seed=np.int64(POSITION_SEED), entries=np.int64(ENTRIES),
               s_bits=np.packbits(s == 255.0, axis=2), ns_bits=np.packbits(ns == 255.0, axis=2), a=a, r=r, d=d.astype(np.uint8),
               eps_next=seen['eps'][0].numpy(), eps_new=seen['eps'][1].numpy(),
               losses=np.array(seen['losses'], np.float64),                        # (a_loss, c1_loss, c2_loss): .item() of fp32
               tv=tv1.numpy()[:, 0], cq1=cq1.numpy()[:, 0], cq2=cq2.numpy()[:, 0], next_logp=seen['sample'][0][1].numpy()[:, 0],
               logp=seen['sample'][1][1].numpy()[:, 0], qn=seen['min'][1].numpy()[:, 0])
    assert fix['eps_next'].shape == fix['eps_new'].shape == (ROWS, A) and fix['eps_next'].dtype == np.float32
    for ni, n in enumerate(uc.NETS):
        after = getattr(agent, n).state_dict()
        for ki, k in enumerate(uc.keys_of(n)):
            p0 = init[n][k].double()
            at = positions(p0.numel(), 100 * ni + ki)
            fix['%s/%s/init' % (n, k)] = np.array([p0.sum().item(), (p0 * p0).sum().item()], np.float64)
            fix['%s/%s/after' % (n, k)] = after[k].numpy().reshape(-1)[at]
            if n in uc.TRAINED:
                g = seen['grads'][n][k]
                fix['%s/%s/grad_norm' % (n, k)] = np.float64(g.double().norm().item())
                fix['%s/%s/grad' % (n, k)] = g.numpy().reshape(-1)[at]
                assert fix['%s/%s/grad_norm' % (n, k)] > 0
    assert all(v.dtype in (np.float32, np.float64, np.uint8, np.int64) for v in fix.values())
    print('losses', fix['losses'], 'tv', fix['tv'], 'done', fix['d'])
    assert reference.save('g24_update.npz', **fix) <= 1000000
