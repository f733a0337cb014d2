"""The head of the reference's policy on the GPU (csrc/f110_policyhead.h): the end of Actor.forward and Actor.sample (src/SAL.py:
410-421) -- fc_mean and fc_log_std on the features of fc1, clamp(-20, 2), exp, rsample, tanh and the squashed-Gaussian log_prob
summed over the action -- as one forward kernel and a deterministic backward, in place of two GEMMs and a dozen element-wise
launches on [B, 16] tensors.  The action comes out in fp64, the dtype F110VecEnv.path_actions and the replay ring take.  There is no
CPU path and no torch fallback: the kernels of libf110_hip.so do the work."""
import ctypes as C

import torch

from . import _lib
from .gauss import GaussianSource

MAX_IN_FEATURES, MAX_ACTION_DIM = 4096, 32
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0


def make_config(in_features, action_dim, out_fp64=True):
    """An f110_policyhead_config; out-of-range integers are clamped into int32 so that validate() can name them."""
    c = _lib.PolicyheadConfig()
    c.in_features, c.action_dim, c.out_fp64 = _lib.clamp(in_features), _lib.clamp(action_dim), 1 if out_fp64 else 0
    return c


def validate(in_features, action_dim, out_fp64=True):
    """f110_policyhead_validate (host only, no device): ValueError for in_features outside 1..4096 and action_dim outside 1..32."""
    c = make_config(in_features, action_dim, out_fp64)
    _lib.check(_lib.load().f110_policyhead_validate(C.byref(c)))
    return c


def workspace_bytes(in_features, action_dim, n):
    """f110_policyhead_workspace: bytes of the backward pass's workspace for n rows (0 for what validate refuses or n < 1)."""
    c = make_config(in_features, action_dim)
    return int(_lib.load().f110_policyhead_workspace(C.byref(c), int(n)))


_ptr = _lib.ptr


class _SampleActions(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w_mean, b_mean, w_log_std, b_log_std, eps, cfg, out):
        lib = _lib.load()
        dev = h.device
        n, a = int(h.shape[0]), cfg.action_dim
        dt = torch.float64 if cfg.out_fp64 else torch.float32
        tensors = [None if t is None else t.detach().contiguous() for t in (h, w_mean, b_mean, w_log_std, b_log_std, eps)]
        pre = torch.empty((n, 2 * a), dtype=torch.float32, device=dev)
        action = out if out is not None else torch.empty((n, a), dtype=dt, device=dev)
        log_prob = None if eps is None else torch.empty((n,), dtype=dt, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.f110_policyhead_forward(C.byref(cfg), tensors[0].data_ptr(), n, *[_ptr(t) for t in tensors[1:]], pre.data_ptr(),
                                                   action.data_ptr(), _ptr(log_prob), _lib.stream(dev)))
        ctx.cfg, ctx.n, ctx.has_bias = cfg, n, (b_mean is not None, b_log_std is not None)
        ctx.save_for_backward(tensors[0], tensors[1], tensors[3], tensors[5], pre)
        ctx.set_materialize_grads(False)
        if out is not None:
            ctx.mark_dirty(out)
        if log_prob is None:
            return action, pre
        return action, log_prob, pre

    @staticmethod
    def backward(ctx, grad_action, *rest):
        lib = _lib.load()
        h, w_mean, w_log_std, eps, pre = ctx.saved_tensors
        cfg, n = ctx.cfg, ctx.n
        dev = h.device
        dt = torch.float64 if cfg.out_fp64 else torch.float32
        grad_log_prob = rest[0] if eps is not None else None
        grad_pre = rest[-1]
        if n == 0 or (grad_action is None and grad_log_prob is None and grad_pre is None):
            zeros = lambda t, on: torch.zeros_like(t) if on else None  # noqa: E731
            need = ctx.needs_input_grad
            return (zeros(h, need[0]), zeros(w_mean, need[1]), zeros(w_mean[:, 0], need[2] and ctx.has_bias[0]), zeros(w_log_std, need[3]),
                    zeros(w_log_std[:, 0], need[4] and ctx.has_bias[1]), None, None, None)
        ga = torch.zeros((n, cfg.action_dim), dtype=dt, device=dev) if grad_action is None else grad_action.to(dt).contiguous()
        glp = None if grad_log_prob is None else grad_log_prob.to(dt).contiguous()
        gp = None if grad_pre is None else grad_pre.to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        new = lambda like, on: torch.empty_like(like) if on else None  # noqa: E731
        gh, gwm, gwl = new(h, need[0]), new(w_mean, need[1]), new(w_log_std, need[3])
        gbm = torch.empty((cfg.action_dim,), dtype=torch.float32, device=dev) if need[2] and ctx.has_bias[0] else None
        gbl = torch.empty((cfg.action_dim,), dtype=torch.float32, device=dev) if need[4] and ctx.has_bias[1] else None
        nbytes = lib.f110_policyhead_workspace(C.byref(cfg), n)
        assert nbytes >= 4 * n * 2 * cfg.action_dim
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.f110_policyhead_backward(C.byref(cfg), h.data_ptr(), n, w_mean.data_ptr(), w_log_std.data_ptr(), pre.data_ptr(), _ptr(eps),
                                                    ga.data_ptr(), _ptr(glp), _ptr(gp), _ptr(gh), _ptr(gwm), _ptr(gbm), _ptr(gwl), _ptr(gbl), ws.data_ptr(),
                                                    _lib.stream(dev)))
        return gh, gwm, gbm, gwl, gbl, None, None, None


def sample_actions(h, w_mean, b_mean, w_log_std, b_log_std, eps=None, dtype=torch.float64, out=None):
    """Actor.sample's tail on features h: (action, log_prob, mean, log_std).
    h [n, K] fp32; w_mean, w_log_std [A, K] fp32 and b_mean, b_log_std [A] fp32 or None (nn.Linear's weight and bias), all on h's GPU;
    K in 1..4096, A in 1..32.  eps: [n, A] fp32 standard normal draws (rsample's), or None for the reference's evaluate=True: action
    = tanh(mean) and log_prob is None.  dtype: torch.float64 (what path_actions and the replay ring take) or torch.float32, of action
    and log_prob.  out: a [n, A] tensor of `dtype` on h's GPU that receives the action in place (a static buffer a captured step
    graph reads); it is then the returned action, and nothing the call returns carries a gradient.
    action = tanh(mean + exp(log_std) * eps) [n, A]; log_prob [n] = the squashed-Gaussian log density summed over the action; mean
    [n, A] fp32 and log_std [n, A] fp32 clamped to [-20, 2] are a view and one clamp of the kernel's pre-activations.  All four are
    differentiable in h and the four parameters (a gradient that arrives at mean or log_std joins the backward kernel's g_pre); eps
    is data.  One kernel on the caller's current
    stream, without synchronising; the numerics are the contract of include/f110_hip.h (fp32 fmaf chains in k order, the tail in
    fp64).  ValueError for what f110_policyhead_validate refuses and for a dtype, shape or device mismatch."""
    who = 'sample_actions'
    if not all(torch.is_tensor(t) for t in (h, w_mean, w_log_std)):
        raise ValueError('%s: h, w_mean and w_log_std must be tensors' % who)
    if not h.is_cuda or w_mean.device != h.device or w_log_std.device != h.device:
        raise ValueError('%s: h, w_mean and w_log_std must be on the same GPU' % who)
    if h.dtype != torch.float32 or h.dim() != 2:
        raise ValueError('%s: h must be fp32 [n, K], not %s %s' % (who, h.dtype, tuple(h.shape)))
    k = int(h.shape[1])
    if w_mean.dtype != torch.float32 or w_mean.dim() != 2 or w_mean.shape[1] != k:
        raise ValueError('%s: w_mean must be fp32 [A, %d], not %s %s' % (who, k, w_mean.dtype, tuple(w_mean.shape)))
    a = int(w_mean.shape[0])
    if w_log_std.dtype != torch.float32 or tuple(w_log_std.shape) != (a, k):
        raise ValueError('%s: w_log_std must be fp32 [%d, %d], not %s %s' % (who, a, k, w_log_std.dtype, tuple(w_log_std.shape)))
    for name, b in (('b_mean', b_mean), ('b_log_std', b_log_std)):
        if b is not None and (not torch.is_tensor(b) or b.dtype != torch.float32 or tuple(b.shape) != (a,) or b.device != h.device):
            raise ValueError('%s: %s must be fp32 [%d] on h\'s device' % (who, name, a))
    n = int(h.shape[0])
    if eps is not None and (not torch.is_tensor(eps) or eps.dtype != torch.float32 or tuple(eps.shape) != (n, a) or eps.device != h.device):
        raise ValueError('%s: eps must be fp32 [%d, %d] on h\'s device' % (who, n, a))
    if dtype not in (torch.float64, torch.float32):
        raise ValueError('%s: dtype must be torch.float64 or torch.float32, not %s' % (who, dtype))
    if out is not None and (not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != (n, a) or out.device != h.device
                            or not out.is_contiguous() or out.requires_grad):
        raise ValueError('%s: out must be a contiguous %s [%d, %d] tensor on h\'s device that does not require grad' % (who, dtype, n, a))
    cfg = validate(k, a, dtype == torch.float64)
    if out is not None:
        with torch.no_grad():           # (a static buffer is for acting: what is written into it carries no gradient)
            res = _SampleActions.apply(h, w_mean, b_mean, w_log_std, b_log_std, eps, cfg, out)
    else:
        res = _SampleActions.apply(h, w_mean, b_mean, w_log_std, b_log_std, eps, cfg, None)
    action, log_prob, pre = (res[0], None, res[1]) if eps is None else res
    return action, log_prob, pre[:, :a], pre[:, a:].clamp(LOG_STD_MIN, LOG_STD_MAX)


def _plain_linear(who, lin):
    if not isinstance(lin, torch.nn.Linear):
        raise ValueError('%s: not an nn.Linear' % who)
    return lin


class PolicyHead(torch.nn.Module):
    """fc_mean and fc_log_std of the reference's Actor (src/SAL.py:402-403) with Actor.sample's tail, computed by sample_actions.
    Submodules fc_mean and fc_log_std are nn.Linear(in_features, action_dim), so a state dict has the reference's keys
    fc_mean.weight, fc_mean.bias, fc_log_std.weight, fc_log_std.bias.
    forward(h) and every result of sample() carry gradients to h and the four parameters; only out= (a static buffer for acting)
    and act() cut the graph."""

    def __init__(self, in_features=512, action_dim=16, device=None):
        super().__init__()
        validate(in_features, action_dim)
        self.fc_mean = torch.nn.Linear(int(in_features), int(action_dim), device=device)
        self.fc_log_std = torch.nn.Linear(int(in_features), int(action_dim), device=device)

    @classmethod
    def from_linears(cls, fc_mean, fc_log_std):
        """A head that shares the parameters of an Actor's two layers (the same tensors: training one trains the other).
        ValueError unless both are nn.Linear of one shape that f110_policyhead_validate accepts."""
        who = 'PolicyHead.from_linears'
        _plain_linear(who, fc_mean)
        _plain_linear(who, fc_log_std)
        if (fc_mean.in_features, fc_mean.out_features) != (fc_log_std.in_features, fc_log_std.out_features):
            raise ValueError('%s: fc_mean is %d -> %d but fc_log_std %d -> %d' % (who, fc_mean.in_features, fc_mean.out_features,
                                                                                 fc_log_std.in_features, fc_log_std.out_features))
        validate(fc_mean.in_features, fc_mean.out_features)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.fc_mean, m.fc_log_std = fc_mean, fc_log_std
        return m

    def _params(self):
        return self.fc_mean.weight, self.fc_mean.bias, self.fc_log_std.weight, self.fc_log_std.bias

    def sample(self, h, eps=None, generator=None, dtype=torch.float64, out=None):
        """Actor.sample(evaluate=False) on features h [n, in_features]: (action, log_prob, mean, log_std) of sample_actions.  eps:
        the [n, action_dim] fp32 draws; None draws them with torch.randn on h's device (from `generator` when given), so the
        random numbers stay torch's; a gauss.GaussianSource draws them on the device from its stream 0, rows 0 .. n-1, and advances it."""
        if isinstance(eps, GaussianSource):
            eps = eps.normal(h.shape[0], self.fc_mean.out_features)
        if eps is None:
            if not torch.is_tensor(h) or h.dim() != 2:
                raise ValueError('PolicyHead.sample: h must be [n, in_features]')
            eps = torch.randn((h.shape[0], self.fc_mean.out_features), dtype=torch.float32, device=h.device, generator=generator)
        return sample_actions(h, *self._params(), eps=eps, dtype=dtype, out=out)

    def forward(self, h):
        """(mean, log_std) of Actor.forward, log_std clamped to [-20, 2], from the kernel's pre-activations; differentiable."""
        _, _, mean, log_std = sample_actions(h, *self._params(), eps=None, dtype=torch.float32)
        return mean, log_std

    def act(self, h, evaluate=False, out=None, generator=None):
        """The fp64 action for acting (select_action, src/SAL.py:510-519) under no_grad: tanh(mean) with evaluate, else a sample.
        out: as sample_actions'."""
        with torch.no_grad():
            if evaluate:
                return sample_actions(h, *self._params(), eps=None, dtype=torch.float64, out=out)[0]
            return self.sample(h, generator=generator, dtype=torch.float64, out=out)[0]
