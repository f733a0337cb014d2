"""The critic loss under importance weights (f110_sac_critic_loss_weighted, csrc/f110_sacloss.h): with w = 1 everywhere the bits of
f110_sac_critic_loss; with random weights the loss, both gradients and td_out `==` the checker of tests/priority_cases.py bit for bit."""
import numpy as np
import pytest

import gpu_checks as gk
import priority_cases as pc
import sacloss_cases as sl

pytestmark = pytest.mark.gpu

NS = (1, 64, 255, 256, 257, 4096)


def _run(c, w, td=True):
    import torch
    from red_gym_amd import sacloss
    q1, q2, tv = (gk.to_device(c[k]) for k in ('q1', 'q2', 'tv'))
    out = torch.full((len(c['tv']),), -3.0, dtype=torch.float32, device='cuda') if td else None
    loss, g1, g2 = sacloss.critic_loss(q1, q2, tv, weight=gk.to_device(w), td=out)
    return loss, g1, g2, out


@pytest.mark.parametrize('n', NS)
def test_ones_give_the_unweighted_bits(n):
    from red_gym_amd import sacloss
    c = sl.case(n, seed=3)
    plain = sacloss.critic_loss(*(gk.to_device(c[k]) for k in ('q1', 'q2', 'tv')))
    loss, g1, g2, _ = _run(c, np.ones(n, np.float32), td=False)
    assert gk.same(loss, gk.to_host(plain[0])) and gk.same(g1, gk.to_host(plain[1])) and gk.same(g2, gk.to_host(plain[2]))
    want = sl.critic(c['q1'], c['q2'], c['tv'])
    assert gk.same(loss, want[0]) and gk.same(g1, want[1]) and gk.same(g2, want[2])


@pytest.mark.parametrize('n', NS)
def test_random_weights_equal_the_checker(n):
    c = sl.case(n, seed=4)
    rng = np.random.default_rng([n, 4])
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    w[rng.integers(0, n)] = 1.0
    if n > 2:
        w[rng.integers(0, n)] = 0.0
    loss, g1, g2, td = _run(c, w)
    want = pc.weighted_critic(c['q1'], c['q2'], c['tv'], w)
    bad = [gk.differing(got, wanted) for got, wanted in zip((loss, g1, g2, td), want)]
    print('n %d: differing loss %d, grad_q1 %d, grad_q2 %d, td %d' % ((n,) + tuple(bad)))
    assert bad == [0, 0, 0, 0]
    if n >= 64:
        plain = sl.critic(c['q1'], c['q2'], c['tv'])
        assert not gk.same(loss, plain[0]) and not gk.same(g1, plain[1])                 # (the weights show)
    assert (gk.to_host(td) >= 0).all()


def test_refusals():
    import torch
    from red_gym_amd import sacloss
    c = sl.case(8)
    q1, q2, tv = (gk.to_device(c[k]) for k in ('q1', 'q2', 'tv'))
    w = torch.ones(8, device='cuda')
    for kw in (dict(td=torch.empty(8, device='cuda')), dict(weight=w[:7]), dict(weight=w.double()), dict(weight=w.cpu()), dict(weight=w, td=torch.empty(7, device='cuda')),
               dict(weight=w, td=torch.empty(8, dtype=torch.float64, device='cuda'))):
        with pytest.raises(ValueError):
            sacloss.critic_loss(q1, q2, tv, **kw)
