"""The tail of the reference's critics on the GPU (csrc/f110_qhead.h): what Critic.forward does behind conv3 (src/SAL.py:440-442) and
what SACAgent.update makes of two critics (:546-549) -- the action columns of fc1, bias, ReLU, fc2, the min over the twin critics and
the TD target -- as one forward kernel and a deterministic backward, for one or two critics at once.  fc1(cat([f, a])) = f @ W[:, :F].T
+ a @ W[:, F:].T + b: the first term is one GEMM of the framework on the strided view W[:, :F]; the kernel takes the view W[:, F:] with
its row stride, so neither the concatenated input nor a copy of the weight ever exists (dense=True: that GEMM and its two backward
GEMMs are the dense layer's kernels on the same view, red_gym_amd.dense, instead of the framework's).  The action, next_log_prob, reward and done
arrive as the policy head and the replay ring produce them (fp64 or fp32, fp64, uint8).  There is no CPU path and no torch
fallback: the kernels of libf110_hip.so do the work."""
import ctypes as C

import torch

from . import _lib
from . import dense as _dense
from .temperature import alpha_argument

MAX_HIDDEN, MAX_ACTION_DIM, MAX_CRITICS = 4096, 32, 2


def make_config(hidden, action_dim, critics=2, ld=None, action_fp64=True):
    """An f110_qhead_config; out-of-range integers are clamped into int32 so that validate() can name them.  ld: the row stride of
    the action columns in elements (None: action_dim, a dense [H, A] array)."""
    c = _lib.QheadConfig()
    c.hidden, c.action_dim, c.critics = _lib.clamp(hidden), _lib.clamp(action_dim), _lib.clamp(critics)
    c.ld, c.action_fp64 = _lib.clamp(action_dim if ld is None else ld), 1 if action_fp64 else 0
    return c


def validate(hidden, action_dim, critics=2, ld=None, action_fp64=True):
    """f110_qhead_validate (host only, no device): ValueError for hidden outside 1..4096, action_dim outside 1..32, critics outside
    1..2 and ld below action_dim."""
    c = make_config(hidden, action_dim, critics, ld, action_fp64)
    _lib.check(_lib.load().f110_qhead_validate(C.byref(c)))
    return c


def workspace_bytes(hidden, action_dim, critics, n):
    """f110_qhead_workspace: bytes of the backward pass's workspace for n rows (0 for what validate refuses or n outside 1..2^24)."""
    c = make_config(hidden, action_dim, critics)
    return int(_lib.load().f110_qhead_workspace(C.byref(c), int(n)))


_ptr = _lib.ptr


def _critics_struct(pres, w1s, b1s, w2s, b2s, F):
    """f110_qhead_critics over the views W[:, F:] of the fc1 weights (the address of column F; the stride is the config's ld)."""
    p = _lib.QheadCritics()
    for c in range(len(pres)):
        p.pre[c], p.w_act[c], p.b1[c] = pres[c].data_ptr(), w1s[c].data_ptr() + 4 * F, _ptr(b1s[c])
        p.w2[c], p.b2[c] = w2s[c].data_ptr(), _ptr(b2s[c])
    return p


def _launch_forward(cfg, pres, w1s, b1s, w2s, b2s, F, action, target_inputs=None):
    """One f110_qhead_forward on the caller's current stream -> (q [C, n], qmin [n], target [n] or None)."""
    lib = _lib.load()
    dev, n, nc = action.device, int(action.shape[0]), len(pres)
    q = torch.empty((nc, n), dtype=torch.float32, device=dev)
    qmin = torch.empty((n,), dtype=torch.float32, device=dev)
    target = None if target_inputs is None else torch.empty((n,), dtype=torch.float32, device=dev)
    reward, done, nlp, gamma, alpha = target_inputs if target_inputs is not None else (None, None, None, 0.0, 0.0)
    p = _critics_struct(pres, w1s, b1s, w2s, b2s, F)
    with torch.cuda.device(dev):
        if torch.is_tensor(gamma):                      # the [n] fp64 device tensor td_target has checked: a discount per row
            by_dev = torch.is_tensor(alpha)
            _lib.check(lib.f110_qhead_forward_rows(C.byref(cfg), C.byref(p), action.data_ptr(), n, _ptr(reward), _ptr(done), _ptr(nlp), gamma.data_ptr(),
                                                   0.0 if by_dev else float(alpha), alpha.data_ptr() if by_dev else None, q.data_ptr(), qmin.data_ptr(),
                                                   _ptr(target), _lib.stream(dev)))
        elif torch.is_tensor(alpha):                    # the [1] fp64 device tensor td_target has checked
            _lib.check(lib.f110_qhead_forward_alpha_dev(C.byref(cfg), C.byref(p), action.data_ptr(), n, _ptr(reward), _ptr(done), _ptr(nlp),
                                                        float(gamma), alpha.data_ptr(), q.data_ptr(), qmin.data_ptr(), _ptr(target), _lib.stream(dev)))
        else:
            _lib.check(lib.f110_qhead_forward(C.byref(cfg), C.byref(p), action.data_ptr(), n, _ptr(reward), _ptr(done), _ptr(nlp), float(gamma),
                                              float(alpha), q.data_ptr(), qmin.data_ptr(), _ptr(target), _lib.stream(dev)))
    return q, qmin, target


def _feature_pre(feats, w1s, F, A, segment):
    """pre[c] = feats[c] @ w1s[c][:, :F].T by f110_dense_forward on the view's address with ld = F + A -> (the config, the list)."""
    H = int(w1s[0].shape[0])
    cfg = _dense.validate(F, H, F + A, segment)
    return cfg, [_dense.forward_into(cfg, f, w.data_ptr(), None, torch.empty((int(f.shape[0]), H), dtype=torch.float32, device=f.device))
                 for f, w in zip(feats, w1s)]


class _TwinQ(torch.autograd.Function):
    """(q [C, n], qmin [n]) of C critics.  Arguments: action, (C, the segment of the dense layer or None for the framework's GEMM), then
    per critic feat, fc1.weight, fc1.bias, fc2.weight, fc2.bias."""

    @staticmethod
    def forward(ctx, action, spec, *flat):
        nc, segment = spec
        feats, w1s, b1s, w2s, b2s = (list(flat[k::5]) for k in range(5))
        F, A = int(feats[0].shape[1]), int(action.shape[1])
        cfg = validate(int(w1s[0].shape[0]), A, nc, F + A, action.dtype == torch.float64)
        act = action.detach().contiguous()
        w1s = [w.detach() for w in w1s]
        feats = [f.detach() for f in feats]
        ctx.dense = None
        if segment is not None:
            # the feature part of fc1 under the dense layer's contract, on the same view
            feats = [f.contiguous() for f in feats]
            ctx.dense, pres = _feature_pre(feats, w1s, F, A, segment)
        else:
            # the feature part of fc1: the framework's GEMM on the strided view W[:, :F] (no copy of the weight)
            pres = [torch.mm(f, w[:, :F].t()) for f, w in zip(feats, w1s)]
        b1d, w2d, b2d = ([None if t is None else t.detach().contiguous() for t in ts] for ts in (b1s, w2s, b2s))
        q, qmin, _ = _launch_forward(cfg, pres, w1s, b1d, w2d, b2d, F, act)
        ctx.cfg, ctx.nc, ctx.F = cfg, nc, F
        ctx.has_b1, ctx.has_b2 = [b is not None for b in b1s], [b is not None for b in b2s]
        saved = [act, q] + feats + w1s + pres + w2d + [b for b in b1d if b is not None]
        ctx.save_for_backward(*saved)
        ctx.set_materialize_grads(False)
        return q, qmin

    @staticmethod
    def backward(ctx, grad_q, grad_qmin):
        lib = _lib.load()
        cfg, nc, F = ctx.cfg, ctx.nc, ctx.F
        s = ctx.saved_tensors
        act, q = s[0], s[1]
        feats, w1s, pres, w2s = (list(s[2 + k * nc:2 + (k + 1) * nc]) for k in range(4))
        rest = list(s[2 + 4 * nc:])
        b1s = [rest.pop(0) if has else None for has in ctx.has_b1]
        dev, n, H, A = act.device, int(act.shape[0]), cfg.hidden, cfg.action_dim
        need = ctx.needs_input_grad
        need_c = [need[2 + 5 * c:7 + 5 * c] for c in range(nc)]          # feat, fc1.weight, fc1.bias, fc2.weight, fc2.bias
        out = [None, None] + [None] * (5 * nc)
        if n == 0 or (grad_q is None and grad_qmin is None):
            if need[0]:
                out[0] = torch.zeros_like(act)
            for c in range(nc):
                like = (feats[c], w1s[c], w1s[c][:, 0], w2s[c], w2s[c].reshape(-1)[:1])
                on = (True, True, ctx.has_b1[c], True, ctx.has_b2[c])
                for k in range(5):
                    if need_c[c][k] and on[k]:
                        out[2 + 5 * c + k] = torch.zeros_like(like[k])
            return tuple(out)
        gq = None if grad_q is None else grad_q.to(torch.float32).contiguous()
        gm = None if grad_qmin is None else grad_qmin.to(torch.float32).contiguous()
        g = _lib.QheadGrads()
        gpre, gw1, gb1, gw2, gb2 = [], [], [], [], []
        for c in range(nc):
            nf, nw, nb1, nw2, nb2 = need_c[c]
            gpre.append(torch.empty((n, H), dtype=torch.float32, device=dev) if nf or nw else None)
            # ONE gradient of fc1.weight's full shape: the kernel writes the action columns with the row stride F + A, the framework's
            # GEMM the feature columns (below)
            gw1.append(torch.empty_like(w1s[c]) if nw else None)
            gb1.append(torch.empty((H,), dtype=torch.float32, device=dev) if nb1 and ctx.has_b1[c] else None)
            gw2.append(torch.empty_like(w2s[c]) if nw2 else None)
            gb2.append(torch.empty((1,), dtype=torch.float32, device=dev) if nb2 and ctx.has_b2[c] else None)
            g.grad_pre[c], g.grad_w_act[c] = _ptr(gpre[c]), None if gw1[c] is None else gw1[c].data_ptr() + 4 * F
            g.grad_b1[c], g.grad_w2[c], g.grad_b2[c] = _ptr(gb1[c]), _ptr(gw2[c]), _ptr(gb2[c])
        ga = torch.empty_like(act) if need[0] else None
        ws = None
        if any(t is not None for t in gw1 + gb1 + gw2 + gb2):
            nbytes = lib.f110_qhead_workspace(C.byref(cfg), n)
            assert nbytes > 0
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        p = _critics_struct(pres, w1s, b1s, w2s, [None] * nc, F)
        with torch.cuda.device(dev):
            _lib.check(lib.f110_qhead_backward(C.byref(cfg), C.byref(p), act.data_ptr(), n, q.data_ptr(), _ptr(gq), _ptr(gm), C.byref(g), _ptr(ga),
                                               _ptr(ws), _lib.stream(dev)))
        out[0] = ga
        for c in range(nc):
            nf, nw, _, _, _ = need_c[c]
            if ctx.dense is not None and (nf or nw):
                # grad_feat, and the feature columns of the one gradient written with its row stride
                out[2 + 5 * c] = torch.empty_like(feats[c]) if nf else None
                _dense.backward_into(ctx.dense, feats[c], None, gpre[c], w1s[c].data_ptr(), out[2 + 5 * c], _ptr(gw1[c]), None)
            elif nf or nw:
                if nf:
                    out[2 + 5 * c] = torch.mm(gpre[c], w1s[c][:, :F])
                if nw:
                    torch.mm(gpre[c].t(), feats[c], out=gw1[c][:, :F])      # into the view: the feature columns of the one gradient
            out[3 + 5 * c], out[4 + 5 * c], out[5 + 5 * c], out[6 + 5 * c] = gw1[c], gb1[c], gw2[c], gb2[c]
        return tuple(out)


def _linears(who, fc1s, fc2s, feats, action):
    """The checks twin_q and td_target share -> (C, F, A)."""
    if not isinstance(feats, (list, tuple)) or not isinstance(fc1s, (list, tuple)) or not isinstance(fc2s, (list, tuple)):
        raise ValueError('%s: feats, fc1s and fc2s must be lists, one entry per critic' % who)
    nc = len(feats)
    if not 1 <= nc <= MAX_CRITICS or len(fc1s) != nc or len(fc2s) != nc:
        raise ValueError('%s: %d feature tensors, %d fc1 and %d fc2 layers (1..%d critics, one of each per critic)' % (who, nc, len(fc1s), len(fc2s), MAX_CRITICS))
    if not torch.is_tensor(action) or not action.is_cuda or action.dim() != 2 or action.dtype not in (torch.float64, torch.float32):
        raise ValueError('%s: action must be a fp64 or fp32 [n, A] tensor on a GPU' % who)
    n, A = int(action.shape[0]), int(action.shape[1])
    dev = action.device
    F = H = None
    for c in range(nc):
        f, l1, l2 = feats[c], fc1s[c], fc2s[c]
        if not isinstance(l1, torch.nn.Linear) or not isinstance(l2, torch.nn.Linear):
            raise ValueError('%s: fc1s and fc2s must hold nn.Linear layers' % who)
        if not torch.is_tensor(f) or f.dtype != torch.float32 or f.dim() != 2 or int(f.shape[0]) != n or f.device != dev:
            raise ValueError('%s: feats[%d] must be fp32 [%d, F] on the action\'s device' % (who, c, n))
        if F is None:
            F, H = int(f.shape[1]), l1.out_features
        if int(f.shape[1]) != F or l1.in_features != F + A or l1.out_features != H or (l2.in_features, l2.out_features) != (H, 1):
            raise ValueError('%s: critic %d: features %d wide, fc1 %d -> %d, fc2 %d -> %d; expected fc1 %d -> %d and fc2 %d -> 1'
                             % (who, c, int(f.shape[1]), l1.in_features, l1.out_features, l2.in_features, l2.out_features, F + A, H, H))
        for t in (l1.weight, l1.bias, l2.weight, l2.bias):
            if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()):
                raise ValueError('%s: the parameters of critic %d must be contiguous fp32 tensors on the action\'s device' % (who, c))
    validate(H, A, nc, F + A, action.dtype == torch.float64)
    return nc, F, A


def _flat(feats, fc1s, fc2s):
    flat = []
    for f, l1, l2 in zip(feats, fc1s, fc2s):
        flat += [f, l1.weight, l1.bias, l2.weight, l2.bias]
    return flat


def _segment(dense, segment):
    """The _TwinQ spec's second entry: None for the framework's GEMM, else the dense layer's segment."""
    return None if not dense else int(_dense.DEFAULT_SEGMENT if segment is None else segment)


def twin_q(feats, action, fc1s, fc2s, dense=False, segment=None):
    """(q [C, n] fp32, qmin [n] fp32) of C = 1 or 2 critics: q[c] = fc2s[c](relu(fc1s[c](cat([feats[c], action], 1))))[:, 0] and
    qmin = min(q[0], q[1]) (C = 1: q[0]), differentiable in the features, the action and every parameter.
    feats: a list of C fp32 [n, F] tensors, each critic's own flattened conv3 output; action [n, A] fp64 (what the policy head and
    path_actions produce; rounded to fp32 once, in the kernel) or fp32 (what the ring stores); fc1s: C nn.Linear(F + A, H), fc2s: C
    nn.Linear(H, 1); H in 1..4096, A in 1..32.
    Forward: C GEMMs of the framework on the views fc1.weight[:, :F] and one kernel on the views fc1.weight[:, F:].  Backward: one
    [H, F + A] gradient per fc1.weight is allocated; the framework's GEMM writes its feature columns through torch.mm(out=view) and
    the kernel its action columns with the row stride, so no zero-filled full-size temporaries are built and added.  The numerics are
    the contract of include/f110_hip.h; at a tie of the two critics each gets half of qmin's gradient, as torch.minimum gives.
    dense=True (opt-in; the default launches what it always did): the three GEMMs on the feature columns are the dense layer's
    (red_gym_amd.dense, csrc/f110_dense.h) on the same views -- f110_dense_forward on the address of fc1.weight with ld = F + A, no
    bias and no ReLU, for `pre`; f110_dense_backward for grad_feat and, with the row stride, for the feature columns of the one
    gradient -- so every number of the critics is under the contract of include/f110_hip.h and a row's q does not depend on the
    batch around it.  segment: the dense layer's k's per chain (None: dense.DEFAULT_SEGMENT).
    ValueError for what f110_qhead_validate (and, with dense, f110_dense_validate) refuses and for a dtype, shape, device or
    contiguity mismatch."""
    nc, F, A = _linears('twin_q', fc1s, fc2s, feats, action)
    seg = _segment(dense, segment)
    if seg is not None:
        _dense.validate(F, fc1s[0].out_features, F + A, seg)
    return _TwinQ.apply(action, (nc, seg), *_flat(feats, fc1s, fc2s))


def td_target(feats, next_action, next_log_prob, reward, done, fc1s, fc2s, gamma, alpha, dense=False, segment=None):
    """tv [n] fp32 of SACAgent.update (src/SAL.py:546-549) under no_grad: tv = reward + (1 - done) * gamma * (min(q1, q2) - alpha *
    next_log_prob), the last two lines in fp64 and rounded once.  feats, fc1s, fc2s as twin_q's, of the TARGET critics on the next
    state; next_action [n, A] and next_log_prob [n] or [n, 1] of one dtype (fp64 or fp32: the policy head's outputs); reward [n] fp64
    and done [n] uint8 or bool as the ring's sample() returns them.  alpha: a finite number, or a [1] fp64 tensor on the action's
    device (Temperature.alpha), which the kernel then reads there (f110_qhead_forward_alpha_dev).  gamma: a finite number, or an [n]
    fp64 tensor on the action's device that holds a discount per row (ReplayBuffer.sample_frames_dev's with nstep > 1, beside a reward
    that is the n-step return): row b's target then takes gamma[b] in gamma's place (f110_qhead_forward_rows, with either kind of
    alpha); ValueError for another dtype, shape or device.  C GEMMs plus one launch; dense, segment: as twin_q's."""
    who = 'td_target'
    nc, F, A = _linears(who, fc1s, fc2s, feats, next_action)
    n, dev = int(next_action.shape[0]), next_action.device
    if not torch.is_tensor(next_log_prob) or next_log_prob.dtype != next_action.dtype or next_log_prob.numel() != n or next_log_prob.device != dev:
        raise ValueError('%s: next_log_prob must be %s [%d] on the action\'s device' % (who, next_action.dtype, n))
    if not torch.is_tensor(reward) or reward.dtype != torch.float64 or reward.numel() != n or reward.device != dev:
        raise ValueError('%s: reward must be fp64 [%d] on the action\'s device' % (who, n))
    if not torch.is_tensor(done) or done.dtype not in (torch.uint8, torch.bool) or done.numel() != n or done.device != dev:
        raise ValueError('%s: done must be uint8 or bool [%d] on the action\'s device' % (who, n))
    import math
    if torch.is_tensor(alpha):
        alpha = alpha_argument(who, alpha, dev)[1]
    if torch.is_tensor(gamma):
        if gamma.dtype != torch.float64 or tuple(gamma.shape) != (n,) or gamma.device != dev:
            raise ValueError('%s: a gamma per row must be a fp64 [%d] tensor on the action\'s device' % (who, n))
        gamma = gamma.detach().contiguous()
    if not ((torch.is_tensor(gamma) or math.isfinite(gamma)) and (torch.is_tensor(alpha) or math.isfinite(alpha))):
        raise ValueError('%s: gamma and alpha must be finite' % who)
    with torch.no_grad():
        cfg = validate(fc1s[0].out_features, A, nc, F + A, next_action.dtype == torch.float64)
        w1s = [l.weight.detach() for l in fc1s]
        seg = _segment(dense, segment)
        if seg is not None:
            _, pres = _feature_pre([f.detach().contiguous() for f in feats], w1s, F, A, seg)
        else:
            pres = [torch.mm(f.detach(), w[:, :F].t()) for f, w in zip(feats, w1s)]
        d = done.detach().reshape(n).contiguous()
        d = d.view(torch.uint8) if d.dtype == torch.bool else d
        inputs = (reward.detach().reshape(n).contiguous(), d, next_log_prob.detach().reshape(n).contiguous(), gamma, alpha)
        _, _, tv = _launch_forward(cfg, pres, w1s, [l.bias for l in fc1s], [l.weight.detach() for l in fc2s], [l.bias for l in fc2s], F,
                                   next_action.detach().contiguous(), inputs)
    return tv


class QHead(torch.nn.Module):
    """fc1 and fc2 of the reference's Critic (src/SAL.py:432-433) computed by twin_q.  Submodules fc1 = nn.Linear(F + A, H) and fc2 =
    nn.Linear(H, 1), so a state dict has the reference's keys fc1.weight, fc1.bias, fc2.weight, fc2.bias.  dense, segment: as twin_q's."""

    def __init__(self, in_features, action_dim=16, hidden=512, device=None, dense=False, segment=None):
        super().__init__()
        validate(hidden, action_dim, 1)
        self.dense, self.segment = bool(dense), segment
        if int(in_features) < 1:
            raise ValueError('QHead: in_features %d' % int(in_features))
        self.fc1 = torch.nn.Linear(int(in_features) + int(action_dim), int(hidden), device=device)
        self.fc2 = torch.nn.Linear(int(hidden), 1, device=device)

    @classmethod
    def from_linears(cls, fc1, fc2, dense=False, segment=None):
        """A head that shares the parameters of a Critic's two layers (the same tensors: training one trains the other).  ValueError
        unless both are nn.Linear, fc2 is fc1.out_features -> 1 and f110_qhead_validate accepts the hidden width."""
        who = 'QHead.from_linears'
        if not isinstance(fc1, torch.nn.Linear) or not isinstance(fc2, torch.nn.Linear):
            raise ValueError('%s: not an nn.Linear' % who)
        if (fc2.in_features, fc2.out_features) != (fc1.out_features, 1):
            raise ValueError('%s: fc1 is %d -> %d but fc2 %d -> %d' % (who, fc1.in_features, fc1.out_features, fc2.in_features, fc2.out_features))
        validate(fc1.out_features, 1, 1)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.fc1, m.fc2 = fc1, fc2
        m.dense, m.segment = bool(dense), segment
        return m

    def forward(self, feat, action):
        """q [n, 1] fp32 of Critic.forward behind conv3: feat [n, F] fp32 (the flattened features), action [n, A] fp64 or fp32 with F +
        A = fc1.in_features; differentiable."""
        q, _ = twin_q([feat], action, [self.fc1], [self.fc2], dense=self.dense, segment=self.segment)
        return q[0].unsqueeze(1)
