"""The mirror of tests/update_cases.py is the reference's update, without a device: MirrorAgent at SAL's shape in fp32 on the CPU with
one thread, rebuilt from the seed, reproduces every quantity the reference's own SACAgent.update left in g24_update.npz (tests/golden/
make_golden.py g24) with `==` -- the same torch operations in the same order; the phases compose to the whole update bit for bit;
and the ring's "no transition" row (index -1) is a zero image that adds nothing to conv1.weight's gradient.

Measured where the fixture was generated (profiles/r19_update.txt): every forward quantity, the three losses, all 32 gradients' 256
entries and all 52 tensors' entries after the update differ from the recording by exactly 0."""
import numpy as np
import pytest
import torch

import update_cases as uc


@pytest.fixture(scope='module')
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(threads)


@pytest.fixture(scope='module')
def pinned(golden, one_thread):
    """(the fixture, the initial sums of the rebuilt mirror, what its whole_update returns, the mirror after it)."""
    g = golden('g24_update.npz')
    m = uc.MirrorAgent(on=255.0, dtype=torch.float32, device='cpu', seed=int(g['seed']), **uc.SAL)
    init = {}
    for n in uc.NETS:
        for k, v in m.net(n).state_dict().items():
            p = v.double()
            init[n, k] = (p.sum().item(), (p * p).sum().item(), p.abs().sum().item())
    b = uc.mirror_batch(uc.golden_batch(g), 255.0, torch.float32, 'cpu')
    return g, init, m.whole_update(b, b['eps_next'], b['eps_new']), m


def test_the_rebuild_from_the_seed_is_the_reference_s_initialisation(pinned):
    """Every tensor's fp64 sum and sum of squares equal the recording's up to the order of an fp64 sum (2^-40 of the sum of
    magnitudes; another draw moves them by far more), the state dicts have the reference's keys, and the targets start as the
    critics."""
    g, init, _, m = pinned
    assert [list(m.net(n).state_dict()) for n in uc.NETS] == [uc.ACTOR_KEYS] + [uc.CRITIC_KEYS] * 4
    assert m.net('actor').fc1.weight.shape == (512, 25088) and m.net('critic1').fc1.weight.shape == (512, 25104)
    for (n, k), (s, ss, mag) in init.items():
        want = g['%s/%s/init' % (n, k)]
        assert abs(s - want[0]) <= 2.0 ** -40 * mag and abs(ss - want[1]) <= 2.0 ** -40 * want[1], (n, k, s, ss, want)
    for n in ('critic1', 'critic2'):
        assert all(init[n, k] == init[n + '_target', k] for k in uc.CRITIC_KEYS)
    assert init['critic1', 'fc1.weight'] != init['critic2', 'fc1.weight']


def test_whole_update_reproduces_the_reference(pinned):
    """`==` on tv, cq1, cq2, next_logp, logp, qn, the three losses, the 256 recorded entries of every gradient as it stood at its
    optimizer's step and of every tensor of the five networks after the update; the gradients' norms to 1e-12 (an fp64 sum)."""
    g, _, out, m = pinned
    diffs = {}

    def same(name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
        diffs[name] = uc.rel_err(got, want)
        return np.array_equal(got, want)

    bad = [name for name, got in (('tv', out['tv']), ('cq1', out['cq'][0]), ('cq2', out['cq'][1]), ('next_logp', out['next_logp']), ('logp', out['logp']),
                                  ('qn', out['qn'])) if not same(name, got.numpy(), g[name])]
    losses = np.array([out['a_loss'].item(), out['c_loss'][0].item(), out['c_loss'][1].item()], np.float64)
    bad += [] if same('losses', losses, g['losses']) else ['losses']
    count = 0
    for n in uc.NETS:
        after = m.net(n).state_dict()
        for k in uc.keys_of(n):
            at = uc.golden_positions(g, n, k, after[k].numel())
            bad += [] if same('%s/%s/after' % (n, k), after[k].numpy().reshape(-1)[at], g['%s/%s/after' % (n, k)]) else ['%s/%s/after' % (n, k)]
            count += 1
            if n in uc.TRAINED:
                grad = out['grads'][n][k]
                bad += [] if same('%s/%s/grad' % (n, k), grad.numpy().reshape(-1)[at], g['%s/%s/grad' % (n, k)]) else ['%s/%s/grad' % (n, k)]
                norm, want = grad.double().norm().item(), float(g['%s/%s/grad_norm' % (n, k)])
                assert want > 0 and abs(norm - want) <= 1e-12 * want, (n, k, norm, want)
                count += 1
    print('worst normwise difference from the recording: %.3g over %d quantities' % (max(diffs.values()), len(diffs)))
    assert count == 52 + 32 and not bad, {name: diffs[name] for name in bad}
    # the update moved every trained tensor and every target, and a target by less than its critic
    for n in uc.TRAINED:
        assert all(float(np.abs(g['%s/%s/grad' % (n, k)]).max()) > 0 for k in uc.keys_of(n))


def test_the_phases_compose_to_the_whole_update(one_thread):
    """critic_phase + Adam + actor_phase + Adam + Polyak equals whole_update bit for bit over three updates at config (a)'s shape:
    every forward quantity, every gradient in front of its step (the critics' from their own loss, the actor's) and all five
    networks after each update."""
    c = uc.CONFIGS['a']
    kw = dict(rows=c['rows'], cols=c['cols'], hidden=c['hidden'], action_dim=c['action_dim'], on=c['on'])
    whole, parts = uc.MirrorAgent(seed=5, **kw), uc.MirrorAgent(seed=5, **kw)
    for u in range(uc.UPDATES):
        b = uc.mirror_batch(uc.batch(50 + u, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool']), c['on'], torch.float32, 'cpu')
        w = uc.flatten(whole.whole_update(b, b['eps_next'], b['eps_new']))
        cp, ap = parts.composed_update(b, b['eps_next'], b['eps_new'])
        got = uc.flatten(cp)
        got.update({k: v for k, v in uc.flatten(ap).items() if not k.startswith('grads.critic')})
        assert sorted(got) == sorted(w)
        assert [k for k in w if not torch.equal(w[k], got[k])] == []
        for n in uc.NETS:
            a, p = whole.net(n).state_dict(), parts.net(n).state_dict()
            assert all(torch.equal(a[k], p[k]) for k in a), (u, n)
        # what the actor's loss leaves in the critics is there, and non-zero
        assert all(float(ap['grads'][n][k].abs().max()) > 0 for n in ('critic1', 'critic2') for k in uc.CRITIC_KEYS)
        for n in ('critic1', 'critic2'):
            for k in uc.CRITIC_KEYS:
                assert torch.equal(whole.net(n).get_parameter(k).grad, cp['grads'][n][k] + ap['grads'][n][k])
    assert not torch.equal(whole.net('critic1_target').fc1.weight, whole.net('critic1').fc1.weight)


def test_the_hole_is_a_zero_image_without_a_gradient_for_conv1_weight():
    """batch()'s row with s_idx = ns_idx = -1 reaches the mirror as a zero image with zero action, reward and done; in fp64 the
    gradient of conv1.weight is, up to the division by n, that of the batch without the row, while conv1.bias does get its share;
    frames repeat and one row's next state is another's state."""
    c = uc.CONFIGS['a']
    b = uc.batch(3, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])
    n, hole = c['n'], b['hole']
    assert b['s_idx'][hole] == b['ns_idx'][hole] == -1 and (b['s_idx'] >= 0).sum() == n - 1 and b['ns_idx'][1] == b['s_idx'][0]
    assert len(set(b['s_idx'].tolist())) < n and b['packed'].shape == (c['pool'], c['rows'], 2) and set(np.unique(b['imgs']).tolist()) == {0, 255}
    assert b['a'].dtype == np.float32 and b['r'].dtype == np.float64 and b['d'].dtype == np.uint8 and b['eps_next'].dtype == np.float32
    assert not b['a'][hole].any() and b['r'][hole] == 0 and b['d'][hole] == 0 and np.abs(b['a']).max() < 1
    kw = dict(rows=c['rows'], cols=c['cols'], hidden=c['hidden'], action_dim=c['action_dim'], on=c['on'])
    m = uc.MirrorAgent(dtype=torch.float64, seed=3, **kw)
    full = uc.mirror_batch(b, c['on'], torch.float64, 'cpu')
    assert not full['s'][hole].any() and not full['ns'][hole].any() and full['s'][0].any() and full['s'].shape == (n, 1, c['rows'], c['cols'])
    assert set(np.unique(full['s'].numpy()).tolist()) == {0.0, c['on']}
    less = uc.mirror_batch(uc.without_row(b, hole), c['on'], torch.float64, 'cpu')
    assert less['s'].shape[0] == n - 1 and torch.equal(less['s'][hole], full['s'][hole + 1])
    for phase, eps in (('critic_phase', 'eps_next'), ('actor_phase', 'eps_new')):
        gf, gl = getattr(m, phase)(full, full[eps])['grads'], getattr(m, phase)(less, less[eps])['grads']
        for net in gf:
            assert uc.rel_err(gf[net]['conv1.weight'] * n, gl[net]['conv1.weight'] * (n - 1)) <= 1e-12, (phase, net)
            if phase == 'critic_phase' or net == 'actor':           # (a critic that loses the min in every row gets no gradient at all)
                assert uc.rel_err(gf[net]['conv1.bias'] * n, gl[net]['conv1.bias'] * (n - 1)) > 1e-6, (phase, net)
