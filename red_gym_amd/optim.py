"""The parameter update of the reference's SACAgent.update on the GPU (csrc/f110_adam.h): what three torch.optim.Adam.step() calls
(src/SAL.py:556-572) and the Polyak loop over the target critics (:575-578) do, as one pass over the parameters per network.  p, g, m
and v are read once and p, m and v written once; with targets the target is moved from the new p in the same pass.  The step counter
and the running powers of the betas live on the device, so step() passes no host value that changes from step to step and a
captured step replays.  The arithmetic is the contract of include/f110_hip.h, bit for bit what tests/optim_cases.py restates in
NumPy.  There is no CPU path and no torch fallback: the kernels of libf110_hip.so do the work."""
import ctypes as C
import math

import torch

from . import _lib

CHUNK, MAX_TENSORS = _lib.F110_ADAM_CHUNK, _lib.F110_ADAM_MAX_TENSORS


def _tensor_list(who, what, tensors):
    if isinstance(tensors, torch.nn.Module):
        tensors = tensors.parameters()
    if torch.is_tensor(tensors):
        raise ValueError('%s: %s must be a list of tensors or a module, not one tensor' % (who, what))
    tensors = list(tensors)
    for i, t in enumerate(tensors):
        if not torch.is_tensor(t):
            raise ValueError('%s: %s[%d] is not a tensor' % (who, what, i))
    return tensors


def _check(who, what, tensors, dev=None):
    """fp32, contiguous, on one GPU -> that device (None for an empty list)."""
    for i, t in enumerate(tensors):
        if t.dtype != torch.float32:
            raise ValueError('%s: %s[%d] is %s, not float32' % (who, what, i, t.dtype))
        if not t.is_cuda:
            raise ValueError('%s: %s[%d] is on the CPU; there is no CPU path' % (who, what, i))
        if not t.is_contiguous():
            raise ValueError('%s: %s[%d] is not contiguous' % (who, what, i))
        if t.numel() > 2 ** 31:
            raise ValueError('%s: %s[%d] has %d elements (at most 2^31)' % (who, what, i, t.numel()))
        if dev is None:
            dev = t.device
        if t.device != dev:
            raise ValueError('%s: %s[%d] is on %s, the others on %s (mixed devices)' % (who, what, i, t.device, dev))
    return dev


def _check_no_alias(who, named):
    """ValueError when two of the (name, tensor) pairs share memory."""
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel(), name) for name, t in named if t.numel() > 0)
    for (_, e0, n0), (s1, _, n1) in zip(spans, spans[1:]):
        if s1 < e0:
            raise ValueError('%s: %s and %s share memory (aliased tensors)' % (who, n0, n1))


def _check_targets(who, params, targets):
    if len(targets) != len(params):
        raise ValueError('%s: %d targets for %d parameters' % (who, len(targets), len(params)))
    for i, (p, t) in enumerate(zip(params, targets)):
        if tuple(t.shape) != tuple(p.shape):
            raise ValueError('%s: targets[%d] has shape %s, the parameter %s' % (who, i, tuple(t.shape), tuple(p.shape)))


def _launches(entries):
    """The (p, g, m, v, target, n) rows in groups of at most MAX_TENSORS, as f110_adam_tensor arrays."""
    for first in range(0, len(entries), MAX_TENSORS):
        rows = entries[first:first + MAX_TENSORS]
        table = (_lib.AdamTensor * len(rows))()
        for e, (p, g, m, v, t, n) in zip(table, rows):
            e.p, e.g, e.m, e.v, e.target, e.n = p, g, m, v, t, n
        yield table, len(rows)


def soft_update(targets, sources, tau):
    """tp = tp + tau (p - tp) for every pair, the reference's soft update (src/SAL.py:575-578) as one launch per 64 tensors: u = p -
    tp; tp' = fmaf(float(tau), u, tp).  For users who keep another optimizer, and what SacAdam.step() does for a parameter without a
    gradient.  targets and sources: parallel lists of tensors or modules; the sources are not written.  ValueError for a length or shape
    mismatch, for non-fp32, non-contiguous, CPU, mixed-device or aliased tensors and for tau outside [0, 1]."""
    who = 'soft_update'
    sources, targets = _tensor_list(who, 'sources', sources), _tensor_list(who, 'targets', targets)
    _check_targets(who, sources, targets)
    dev = _check(who, 'targets', targets, _check(who, 'sources', sources))
    _check_no_alias(who, [('sources[%d]' % i, t) for i, t in enumerate(sources)] + [('targets[%d]' % i, t) for i, t in enumerate(targets)])
    if not isinstance(tau, (int, float)) or not math.isfinite(tau) or not 0.0 <= tau <= 1.0:
        raise ValueError('%s: tau %r (0 <= tau <= 1)' % (who, tau))
    if dev is None:
        return
    _soft_update(dev, [(p.data_ptr(), None, None, None, t.data_ptr(), p.numel()) for p, t in zip(sources, targets)], tau)


def _soft_update(dev, entries, tau):
    lib = _lib.load()
    with torch.cuda.device(dev):
        for table, n in _launches(entries):
            _lib.check(lib.f110_soft_update(table, n, float(tau), _lib.stream(dev)))


class SacAdam:
    """Adam with torch.optim.Adam's defaults and the reference's (weight_decay 0, no amsgrad, no maximize) over `params`, and with
    `targets` the soft update of one target tensor per parameter in the same pass (tp' = tp + tau (p' - tp) from the parameter just
    written).  params: a list of fp32 contiguous tensors on one GPU, or a module; targets: a parallel list, or a module whose
    parameters() are parallel, of the same shapes.  exp_avg and exp_avg_sq are one flat zero-initialised allocation each.
    The step counter is ONE per optimizer (torch keeps one per parameter): a parameter that gets its first gradient at step 5 is
    corrected for step 5, where torch would correct it for step 1.  With every gradient present, as in SAL, the two agree.  The counter
    t (int64, from 0) and the running products beta1 ** t and beta2 ** t (fp64) live on the device and are advanced by a one-wave
    launch in front of each step, so a step captured in a torch.cuda.graph replays; `lr` is a host scalar of each launch, settable
    between eager steps and frozen in a captured one.
    ValueError for non-fp32, non-contiguous, CPU, mixed-device or aliased tensors, a targets list of another length or other shapes,
    and for what f110_adam_validate refuses (betas outside [0, 1), eps <= 0, tau outside [0, 1]).
    max_grad_norm: None -- every launch as above, nothing of what follows exists.  A positive float or float('inf'): each step first
    forms the global L2 norm of all the .grad tensors on the device (f110_adam_gradnorm, f110_adam_clip: fp64, a fixed order; the
    contract "Gradient clipping" of include/f110_hip.h), then steps with g * coef, coef = min(1, max_grad_norm / (norm + 1e-6)) as
    torch.nn.utils.clip_grad_norm_ forms it, and SKIPS the step when the norm is inf or NaN: parameters, moments and the step counter
    keep their bits, the targets still move.  float('inf') is the guard alone.  Two launches more per 64 tensors.  Unlike torch's
    function this does NOT write the scaled gradient back to .grad.  max_grad_norm is a host scalar of the launch like lr: settable
    between eager steps, frozen under capture.  clip_state: an int64 [8] device tensor that then holds the f110_adam_clip_state
    (None: the optimizer allocates one); clip_stats() reads it.  max_grad_norm and the counters are configuration and diagnostics,
    not state: state_dict() and load_state_dict() do not know them."""

    def __init__(self, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, targets=None, tau=0.005, max_grad_norm=None, clip_state=None):
        who = 'SacAdam'
        self.params = _tensor_list(who, 'params', params)
        dev = _check(who, 'params', self.params)
        named = [('params[%d]' % i, t) for i, t in enumerate(self.params)]
        self.targets = None
        if targets is not None:
            self.targets = _tensor_list(who, 'targets', targets)
            _check_targets(who, self.params, self.targets)
            _check(who, 'targets', self.targets, dev)
            named += [('targets[%d]' % i, t) for i, t in enumerate(self.targets)]
        _check_no_alias(who, named)
        if not self.params:
            raise ValueError('%s: an empty parameter list' % who)
        self.device = dev
        self.lr, self.betas, self.eps, self.tau = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(tau)
        self._config(True)                                             # (validates)
        if not math.isfinite(self.lr):
            raise ValueError('%s: lr is not finite' % who)
        # every tensor's moments start 16-byte aligned in the flat allocations
        self._offsets, total = [], 0
        for p in self.params:
            self._offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.exp_avg = torch.zeros((max(total, 4),), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros((max(total, 4),), dtype=torch.float32, device=dev)
        assert _lib.load().f110_adam_state_bytes() == _lib.F110_ADAM_STATE_BYTES
        self._state = torch.zeros((_lib.F110_ADAM_STATE_BYTES // 8,), dtype=torch.int64, device=dev)   # f110_adam_state
        self._set_state(0)
        self._max_grad_norm, self._partials, self._clip = None, None, None
        if max_grad_norm is None:
            if clip_state is not None:
                raise ValueError('%s: clip_state without max_grad_norm' % who)
            return
        self._max_grad_norm = self._checked_norm(max_grad_norm)
        assert _lib.load().f110_adam_clip_state_bytes() == _lib.F110_ADAM_CLIP_STATE_BYTES == C.sizeof(_lib.AdamClipState)
        words = _lib.F110_ADAM_CLIP_STATE_BYTES // 8
        if clip_state is None:
            clip_state = torch.zeros((words,), dtype=torch.int64, device=dev)
        elif (not torch.is_tensor(clip_state) or clip_state.dtype != torch.int64 or tuple(clip_state.shape) != (words,)
              or clip_state.device != dev or not clip_state.is_contiguous()):
            raise ValueError('%s: clip_state must be a contiguous int64 [%d] tensor on %s' % (who, words, dev))
        self._clip = clip_state                                        # f110_adam_clip_state
        self._partials = torch.zeros((max(1, sum((p.numel() + CHUNK - 1) // CHUNK for p in self.params)),), dtype=torch.float64, device=dev)

    # ---- gradient clipping
    @staticmethod
    def _checked_norm(value):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value) or not value > 0:
            raise ValueError('SacAdam: max_grad_norm %r: a positive number or float(\'inf\')' % (value,))
        return float(value)

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if self._clip is None or value is None:
            raise ValueError('SacAdam: max_grad_norm is switched on or off at construction only (it owns device buffers); its value may change')
        self._max_grad_norm = self._checked_norm(value)

    def clip_stats(self):
        """(norm, coef, skip, steps_clipped, steps_skipped) of the last step as the device holds them (synchronises): the twin of
        device_state().  norm is inf on a skipped step.  ValueError without max_grad_norm."""
        if self._clip is None:
            raise ValueError('SacAdam.clip_stats: the optimizer was built without max_grad_norm')
        host = _lib.AdamClipState.from_buffer_copy(self._clip.cpu().numpy().tobytes())
        return float(host.norm), float(host.coef), bool(host.skip), int(host.steps_clipped), int(host.steps_skipped)

    # ---- the device state
    def _set_state(self, t):
        """t steps taken; the powers are beta ** t, computed once on the host."""
        host = torch.zeros((4,), dtype=torch.int64)
        host[0] = int(t)
        host.view(torch.float64)[1] = self.betas[0] ** int(t)
        host.view(torch.float64)[2] = self.betas[1] ** int(t)
        self._state.copy_(host)

    def device_state(self):
        """(t, beta1 ** t, beta2 ** t, k2, a) as the device holds them (synchronises)."""
        host = self._state.cpu()
        f64, f32 = host.view(torch.float64), host.view(torch.float32)
        return int(host[0]), float(f64[1]), float(f64[2]), float(f32[6]), float(f32[7])

    def moments(self, i):
        """(exp_avg, exp_avg_sq) of parameter i: views into the flat allocations, of the parameter's shape."""
        p, o = self.params[i], self._offsets[i]
        return self.exp_avg[o:o + p.numel()].view(p.shape), self.exp_avg_sq[o:o + p.numel()].view(p.shape)

    def _config(self, advance):
        c = _lib.AdamConfig()
        c.beta1, c.beta2, c.eps, c.tau = self.betas[0], self.betas[1], self.eps, self.tau
        c.with_target, c.advance = 0 if self.targets is None else 1, 1 if advance else 0
        _lib.check(_lib.load().f110_adam_validate(C.byref(c)))
        return c

    # ---- the step
    @torch.no_grad()
    def step(self):
        """One Adam step of every parameter that has a .grad, from the .grad tensors as they are now (autograd may have put them
        anywhere), and the soft update of every target.  A parameter whose .grad is None is left untouched, with its moments; its
        target is still moved.  Launches on the current stream: one state advance, one update kernel per 64 tensors; with
        max_grad_norm in front of them one norm kernel per 64 tensors and the one-workgroup clip kernel.  When no parameter has a
        .grad nothing of the step is launched and the clip state is left alone."""
        who = 'SacAdam.step'
        lib, dev = _lib.load(), self.device
        m0, v0 = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        with_grad, without = [], []
        for i, p in enumerate(self.params):
            t = None if self.targets is None else self.targets[i].data_ptr()
            g = p.grad
            if g is None:
                if t is not None:
                    without.append((p.data_ptr(), None, None, None, t, p.numel()))
                continue
            if g.dtype != torch.float32 or g.device != dev or not g.is_contiguous() or g.shape != p.shape or g.layout != torch.strided:
                raise ValueError('%s: the gradient of params[%d] must be a contiguous fp32 tensor of its shape on %s' % (who, i, dev))
            o = 4 * self._offsets[i]
            with_grad.append((p.data_ptr(), g.data_ptr(), m0 + o, v0 + o, t, p.numel()))
        with torch.cuda.device(dev):
            stream = _lib.stream(dev)
            first = True
            if self._clip is not None and with_grad:
                partials, base = self._partials.data_ptr(), 0
                for table, n in _launches(with_grad):                  # chunks numbered over the whole step, across calls
                    _lib.check(lib.f110_adam_gradnorm(table, n, base, partials, self._partials.numel(), stream))
                    base += sum((e.n + CHUNK - 1) // CHUNK for e in table)
                _lib.check(lib.f110_adam_clip(partials, base, self._max_grad_norm, self._clip.data_ptr(), stream))
            for table, n in _launches(with_grad):
                cfg = self._config(first)                              # the first launch of the step advances the state
                if self._clip is None:
                    _lib.check(lib.f110_adam_step(C.byref(cfg), table, n, self._state.data_ptr(), self.lr, stream))
                else:
                    _lib.check(lib.f110_adam_step_clipped(C.byref(cfg), table, n, self._state.data_ptr(), self._clip.data_ptr(), self.lr, stream))
                first = False
        if without:
            _soft_update(dev, without, self.tau)

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad: drops every .grad (the next backward allocates fresh ones), or zeroes them in place."""
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.requires_grad_(False)
                p.grad.zero_()

    # ---- checkpoints in torch.optim.Adam's format
    def _param_group(self):
        """torch.optim.Adam's own param group for these hyperparameters (whatever keys this torch version keeps), over n parameters."""
        group = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=self.betas, eps=self.eps).state_dict()['param_groups'][0]
        group['params'] = list(range(len(self.params)))
        return group

    def state_dict(self):
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} as torch.optim.Adam.state_dict() gives it, so that
        torch.optim.Adam(params).load_state_dict() continues this run.  Before the first step the state is empty, as torch's is; after
        it every parameter has an entry with the optimizer's one step count (copies; synchronises)."""
        t = self.device_state()[0]
        state = {}
        if t > 0:
            for i in range(len(self.params)):
                m, v = self.moments(i)
                state[i] = {'step': torch.tensor(float(t)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        return {'state': state, 'param_groups': [self._param_group()]}

    def load_state_dict(self, state_dict):
        """Continues from a torch.optim.Adam (or SacAdam) state_dict: lr, betas and eps of its one param group, exp_avg and exp_avg_sq
        per parameter (zeros for a parameter without an entry), and the step count, which must be the same for every entry: ValueError
        otherwise, and for weight_decay, amsgrad or maximize set, more than one group, or other shapes.  The powers of the betas are
        beta ** step, computed once on the host."""
        who = 'SacAdam.load_state_dict'
        groups = state_dict['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.params):
            raise ValueError('%s: expected one param group of %d parameters' % (who, len(self.params)))
        g = groups[0]
        if g.get('weight_decay', 0) != 0 or g.get('amsgrad', False) or g.get('maximize', False):
            raise ValueError('%s: weight_decay, amsgrad and maximize are not supported' % who)
        index = {pid: i for i, pid in enumerate(g['params'])}
        steps, entries = set(), {}
        for pid, s in state_dict['state'].items():
            if pid not in index:
                raise ValueError('%s: state of parameter %r, which the param group does not list' % (who, pid))
            i = index[pid]
            step = float(s['step'].item() if torch.is_tensor(s['step']) else s['step'])
            if step != int(step) or step < 0:
                raise ValueError('%s: step %r of parameter %d' % (who, step, i))
            steps.add(int(step))
            for key in ('exp_avg', 'exp_avg_sq'):
                if tuple(s[key].shape) != tuple(self.params[i].shape):
                    raise ValueError('%s: %s of parameter %d has shape %s, the parameter %s' % (who, key, i, tuple(s[key].shape), tuple(self.params[i].shape)))
            entries[i] = s
        if len(steps) > 1:
            raise ValueError('%s: the parameters have different step counts %s; this optimizer keeps one' % (who, sorted(steps)))
        lr, betas, eps = float(g['lr']), (float(g['betas'][0]), float(g['betas'][1])), float(g['eps'])
        old = self.lr, self.betas, self.eps
        self.lr, self.betas, self.eps = lr, betas, eps
        try:
            self._config(True)
            if not math.isfinite(lr):
                raise ValueError('%s: lr is not finite' % who)
        except ValueError:
            self.lr, self.betas, self.eps = old
            raise
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for i, s in entries.items():
            m, v = self.moments(i)
            m.copy_(s['exp_avg'])
            v.copy_(s['exp_avg_sq'])
        self._set_state(steps.pop() if steps else 0)
