"""The two losses of the reference's SACAgent.update on the GPU (csrc/f110_sacloss.h): F.mse_loss of each critic against the TD target
(src/SAL.py:553-554) and (alpha * log_prob - min_q).mean() (:568), each with its gradients in ONE launch, in place of a dozen
element-wise and reduction launches of the framework.  The value of a loss is a sum in fp64 in the fixed order of include/f110_hip.h
(256 chains and a tree, whatever the launch's shape), divided by n once and rounded to fp32 once; no atomics, so an update that ends in
these kernels repeats bit for bit and a captured one replays.  Neither function is an autograd function: each returns the gradient
tensors, which the caller hands on with torch.autograd.backward((q,), (grad_q,)) and torch.autograd.backward((log_prob, min_q),
(grad_log_prob, grad_min_q)), and nothing here calls .item().  There is no CPU path and no torch fallback: the kernels of libf110_hip.so
do the work."""
import torch

from . import _lib
from .temperature import alpha_argument

MAX_ROWS = 2 ** 24


def _rows(who, name, t, n=None, dtypes=(torch.float32,)):
    """A detached contiguous [n] view of a [n] or [n, 1] tensor on a GPU."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype not in dtypes:
        raise ValueError('%s: %s must be a %s tensor on a GPU' % (who, name, ' or '.join(str(d) for d in dtypes)))
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] != 1) or (n is not None and t.shape[0] != n):
        raise ValueError('%s: %s must be [n] or [n, 1]%s, not %s' % (who, name, '' if n is None else ' with n = %d' % n, tuple(t.shape)))
    if not 1 <= t.shape[0] <= MAX_ROWS:
        raise ValueError('%s: n = %d rows (1..2^24)' % (who, t.shape[0]))
    return t.detach().reshape(-1).contiguous()


def _loss(who, loss, k, dev):
    if loss is None:
        return torch.empty((k,), dtype=torch.float32, device=dev)
    if not torch.is_tensor(loss) or loss.dtype != torch.float32 or tuple(loss.shape) != (k,) or loss.device != dev or not loss.is_contiguous():
        raise ValueError('%s: loss must be a contiguous fp32 [%d] tensor on %s' % (who, k, dev))
    return loss


def critic_loss(q1, q2, tv, loss=None, grad=None, weight=None, td=None):
    """f110_sac_critic_loss: (loss [2] fp32, grad_q1 [n], grad_q2 [n] fp32) for q1, q2, tv [n] (or [n, 1]) fp32 on one GPU: loss[c] =
    mean((q_c - tv) ** 2) summed in the contract's order, grad_q_c = (q_c - tv) * float(2 / n), which for n a power of two is autograd's
    gradient of F.mse_loss(q_c, tv) bit for bit.  loss: a [2] fp32 tensor to write into (a slice of the agent's [3]); grad: a [2, n] fp32
    tensor whose rows receive the two gradients (twin_q returns q as such a tensor: one backward call takes it whole).  One launch on the
    current stream, no synchronisation.
    weight: [n] fp32 importance weights (ReplayBuffer.sample_priority_dev's) -- f110_sac_critic_loss_weighted, a kernel of its own: loss[c]
    = mean(weight * (q_c - tv) ** 2) in the same order and grad_q_c = ((q_c - tv) * float(2 / n)) * weight; td: an [n] fp32 tensor that
    then receives max(|q1 - tv|, |q2 - tv|), what PriorityTree.update takes (td needs a weight; ones give the unweighted bits)."""
    who = 'critic_loss'
    q1 = _rows(who, 'q1', q1)
    n, dev = int(q1.shape[0]), q1.device
    q2, tv = _rows(who, 'q2', q2, n), _rows(who, 'tv', tv, n)
    if q2.device != dev or tv.device != dev:
        raise ValueError('%s: q1, q2 and tv must be on one device' % who)
    loss = _loss(who, loss, 2, dev)
    if grad is None:
        grad = torch.empty((2, n), dtype=torch.float32, device=dev)
    elif not torch.is_tensor(grad) or grad.dtype != torch.float32 or tuple(grad.shape) != (2, n) or grad.device != dev or not grad.is_contiguous():
        raise ValueError('%s: grad must be a contiguous fp32 [2, %d] tensor on %s' % (who, n, dev))
    if weight is None and td is not None:
        raise ValueError('%s: td is written by the weighted kernel only (give weight)' % who)
    if weight is not None:
        weight = _rows(who, 'weight', weight, n)
        if weight.device != dev:
            raise ValueError('%s: weight must be on %s' % (who, dev))
        if td is not None and (not torch.is_tensor(td) or td.dtype != torch.float32 or tuple(td.shape) != (n,) or td.device != dev or not td.is_contiguous()):
            raise ValueError('%s: td must be a contiguous fp32 [%d] tensor on %s' % (who, n, dev))
        with torch.cuda.device(dev):
            _lib.check(_lib.load().f110_sac_critic_loss_weighted(q1.data_ptr(), q2.data_ptr(), tv.data_ptr(), weight.data_ptr(), n, loss.data_ptr(),
                                                                 grad[0].data_ptr(), grad[1].data_ptr(), _lib.ptr(td), _lib.stream(dev)))
        return loss, grad[0], grad[1]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f110_sac_critic_loss(q1.data_ptr(), q2.data_ptr(), tv.data_ptr(), n, loss.data_ptr(), grad[0].data_ptr(),
                                                    grad[1].data_ptr(), _lib.stream(dev)))
    return loss, grad[0], grad[1]


def actor_loss(logp, qn, alpha, loss=None):
    """f110_sac_actor_loss: (loss [1] fp32, grad_logp [n] of logp's dtype, grad_qn [n] fp32) for logp [n] (or [n, 1]) fp64 or fp32, as
    the policy head returns it, and qn [n] fp32 (twin_q's qmin): loss = mean(alpha * logp - qn) summed in the contract's order,
    grad_logp = alpha / n and grad_qn = -1 / n, which for n a power of two are autograd's gradients of that expression bit for bit.
    alpha: a finite number, or a [1] fp64 tensor on logp's device (Temperature.alpha): the kernel then reads it there
    (f110_sac_actor_loss_alpha_dev) and divides alpha / n on the device, with the same bits.
    loss: a [1] fp32 tensor to write into.  One launch on the current stream, no synchronisation."""
    who = 'actor_loss'
    logp = _rows(who, 'logp', logp, dtypes=(torch.float64, torch.float32))
    n, dev = int(logp.shape[0]), logp.device
    qn = _rows(who, 'qn', qn, n)
    if qn.device != dev:
        raise ValueError('%s: logp and qn must be on one device' % who)
    alpha, alpha_dev = alpha_argument(who, alpha, dev)
    loss = _loss(who, loss, 1, dev)
    g_logp = torch.empty((n,), dtype=logp.dtype, device=dev)
    g_qn = torch.empty((n,), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        if alpha_dev is None:
            _lib.check(lib.f110_sac_actor_loss(logp.data_ptr(), int(logp.dtype == torch.float64), qn.data_ptr(), alpha, n, loss.data_ptr(),
                                               g_logp.data_ptr(), g_qn.data_ptr(), _lib.stream(dev)))
        else:
            _lib.check(lib.f110_sac_actor_loss_alpha_dev(logp.data_ptr(), int(logp.dtype == torch.float64), qn.data_ptr(), alpha_dev.data_ptr(), n,
                                                         loss.data_ptr(), g_logp.data_ptr(), g_qn.data_ptr(), _lib.stream(dev)))
    return loss, g_logp, g_qn
