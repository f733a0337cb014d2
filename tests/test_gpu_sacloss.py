"""The two SAC losses on the GPU (csrc/f110_sacloss.h) against the NumPy checker of tests/sacloss_cases.py, compared as raw bits:
through the raw ABI on guarded buffers at every n of sl.GPU_N with log_prob in fp64 and in fp32, the order of the sum where it shows,
the Python wrappers and autograd at a power of two, and a captured replay."""
import ctypes as C

import numpy as np
import pytest

import gpu_checks as gk
import sacloss_cases as sl

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ALPHA = 0.2


def _exact(got, want):
    """The same dtype and the same bits (gk.same alone would cast the checker's array to the buffer's dtype)."""
    return got.dtype == want.dtype and gk.same(got, want)


def _critic_raw(q1, q2, tv, grads=(True, True)):
    import torch
    from red_gym_amd import _lib
    n = tv.shape[0]
    ins = [gk.Guarded(n, fill=SENTINEL, values=x) for x in (q1, q2, tv)]
    loss, g1, g2 = (gk.Guarded(m, fill=SENTINEL) for m in (2, n, n))
    _lib.check(_lib.load().f110_sac_critic_loss(ins[0].ptr, ins[1].ptr, ins[2].ptr, n, loss.ptr, g1.ptr if grads[0] else None,
                                                g2.ptr if grads[1] else None, _lib.stream(torch.device('cuda', torch.cuda.current_device()))))
    torch.cuda.synchronize()
    for t, x in zip(ins, (q1, q2, tv)):
        assert _exact(t.read(), x), 'an input was written'
    return loss.read(), g1.read(), g2.read()


def _actor_raw(logp, qn, alpha):
    import torch
    from red_gym_amd import _lib
    n = qn.shape[0]
    f64 = logp.dtype == np.float64
    dt = torch.float64 if f64 else torch.float32
    lp, q = gk.Guarded(n, dtype=dt, fill=SENTINEL, values=logp), gk.Guarded(n, fill=SENTINEL, values=qn)
    loss, glp, gqn = gk.Guarded(1, fill=SENTINEL), gk.Guarded(n, dtype=dt, fill=SENTINEL), gk.Guarded(n, fill=SENTINEL)
    _lib.check(_lib.load().f110_sac_actor_loss(lp.ptr, int(f64), q.ptr, alpha, n, loss.ptr, glp.ptr, gqn.ptr,
                                               _lib.stream(torch.device('cuda', torch.cuda.current_device()))))
    torch.cuda.synchronize()
    assert _exact(lp.read(), logp) and _exact(q.read(), qn), 'an input was written'
    return loss.read(), glp.read(), gqn.read()


@pytest.mark.parametrize('n', sl.GPU_N)
def test_raw_abi_equals_the_checker(n):
    """Both losses and all four gradients `==` the checker, log_prob in fp64 and in fp32, inputs and outputs between guards; a NULL
    gradient is left out and the rest is unchanged."""
    c = sl.case(n)
    want = sl.critic(c['q1'], c['q2'], c['tv'])
    got = _critic_raw(c['q1'], c['q2'], c['tv'])
    print('n = %d: critic losses %r (checker %r)' % (n, got[0].tolist(), want[0].tolist()))
    assert all(_exact(g, w) for g, w in zip(got, want))
    only = _critic_raw(c['q1'], c['q2'], c['tv'], grads=(False, True))
    assert _exact(only[0], want[0]) and (only[1] == SENTINEL).all() and _exact(only[2], want[2])
    for dt in (np.float64, np.float32):
        c = sl.case(n, logp_dtype=dt)
        want = sl.actor(c['logp'], c['qn'], ALPHA)
        got = _actor_raw(c['logp'], c['qn'], ALPHA)
        print('n = %d: actor loss %r (checker %r), log_prob %s' % (n, got[0].tolist(), want[0].tolist(), np.dtype(dt).name))
        assert all(_exact(g, w) for g, w in zip(got, want)), (n, dt)


def test_the_order_of_the_sum():
    """The same rows permuted: swapping whole chains that the tree adds to one another (i -> i ^ m) leaves the loss as it is; moving
    a row to another chain changes it where the checker says so, here visibly in fp32."""
    n = 4096
    c = sl.case(n)
    base = _critic_raw(c['q1'], c['q2'], c['tv'])[0]
    assert _exact(base, sl.critic(c['q1'], c['q2'], c['tv'])[0])
    for m in (1, 128):
        p = sl.butterfly(n, m)
        assert _exact(_critic_raw(c['q1'][p], c['q2'][p], c['tv'][p])[0], base), m
    for n in (257, 4097):
        losses = []
        for apart in (False, True):
            k = sl.cancelling(n, apart)
            got, want = _actor_raw(k['logp'], k['qn'], 1.0)[0], sl.actor(k['logp'], k['qn'], 1.0)[0]
            assert _exact(got, want), (n, apart, got, want)
            losses.append(got[0])
        assert losses[0] == np.float32(-(n - 2) / n) and losses[1] != losses[0], (n, losses)


def test_wrappers_and_autograd_at_a_power_of_two():
    """critic_loss / actor_loss on [n] and [n, 1] tensors, into a slice of one [3] loss tensor: `==` the checker, and at n = 64 the
    gradients `==` what autograd gives on the GPU for F.mse_loss and (alpha * logp - qn).mean().  Bad arguments raise ValueError."""
    import torch
    import torch.nn.functional as F
    from red_gym_amd.sacloss import actor_loss, critic_loss
    n = 64
    c = sl.case(n)
    dev = gk.to_device
    losses = torch.zeros(3, device='cuda')
    q = torch.stack([dev(c['q1']), dev(c['q2'])])
    grad = torch.empty_like(q)
    out, g1, g2 = critic_loss(q[0], q[1], dev(c['tv'])[:, None], loss=losses[1:3], grad=grad)
    _, glp, gqn = actor_loss(dev(c['logp']), dev(c['qn']), ALPHA, loss=losses[0:1])
    wc, wa = sl.critic(c['q1'], c['q2'], c['tv']), sl.actor(c['logp'], c['qn'], ALPHA)
    assert out.data_ptr() == losses[1:3].data_ptr() and g1.data_ptr() == grad[0].data_ptr()
    assert _exact(losses.cpu().numpy(), np.concatenate([wa[0], wc[0]]))
    assert _exact(grad.cpu().numpy(), np.stack([wc[1], wc[2]])) and _exact(glp.cpu().numpy(), wa[1]) and _exact(gqn.cpu().numpy(), wa[2])
    x1, x2 = dev(c['q1']).requires_grad_(), dev(c['q2']).requires_grad_()
    (F.mse_loss(x1, dev(c['tv'])) + F.mse_loss(x2, dev(c['tv']))).backward()
    assert torch.equal(x1.grad, g1) and torch.equal(x2.grad, g2)
    lp, qn = dev(c['logp']).requires_grad_(), dev(c['qn']).requires_grad_()
    (ALPHA * lp - qn).mean().backward()
    assert torch.equal(lp.grad, glp) and torch.equal(qn.grad, gqn) and glp.dtype == torch.float64
    for bad in (lambda: critic_loss(q[0], q[1][:5], dev(c['tv'])), lambda: critic_loss(q[0].double(), q[1], dev(c['tv'])),
                lambda: critic_loss(q[0].cpu(), q[1].cpu(), dev(c['tv']).cpu()), lambda: actor_loss(dev(c['logp']), dev(c['qn']), float('nan')),
                lambda: actor_loss(dev(c['logp']), dev(c['qn']), ALPHA, loss=losses), lambda: critic_loss(q[0][:0], q[1][:0], dev(c['tv'])[:0])):
        with pytest.raises(ValueError):
            bad()


def test_graph_replay_equals_eager():
    """Both kernels captured in one torch.cuda.graph, the inputs refilled in place between two replays: every output `==` eager."""
    import torch
    from red_gym_amd.sacloss import actor_loss, critic_loss
    n = 257
    fills = [sl.case(n, seed=s) for s in (0, 5)]
    dev = gk.to_device

    def run(t, losses):
        _, g1, g2 = critic_loss(t['q1'], t['q2'], t['tv'], loss=losses[1:3])
        _, glp, gqn = actor_loss(t['logp'], t['qn'], ALPHA, loss=losses[0:1])
        return losses, g1, g2, glp, gqn

    eager = [[x.clone() for x in run({k: dev(v) for k, v in c.items()}, torch.zeros(3, device='cuda'))] for c in fills]
    assert not torch.equal(eager[0][0], eager[1][0])
    static = {k: torch.zeros_like(dev(v)) for k, v in fills[0].items()}
    losses = torch.zeros(3, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        outs = run(static, losses)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not losses.any()                                                      # a capture runs nothing
    for c, want in zip(fills, eager):
        for k, v in c.items():
            static[k].copy_(dev(v))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, want))
