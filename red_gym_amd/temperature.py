"""SAC's entropy temperature learnt on the GPU (csrc/f110_temperature.h): log_alpha moves by Adam towards a target entropy, loss =
-(log_alpha * mean(log_prob + target_entropy)), and alpha = exp(log_alpha) stays in device memory, where qhead.td_target and
sacloss.actor_loss read it when they are handed the [1] tensor `alpha`.  One step is ONE launch of one workgroup -- the sum in the
losses' fixed order, the loss and its gradient, the state's advance, Adam on the one element and the exp -- so a step captured in a
torch.cuda.graph replays, and an update that contains it replays with the temperature of its own step.  The arithmetic is the contract
of include/f110_hip.h, bit for bit what tests/temperature_cases.py restates in NumPy (alpha itself within one device exp of it).  There
is no CPU path and no torch fallback: the kernel of libf110_hip.so does the work."""
import ctypes as C
import math

import torch

from . import _lib

MAX_ROWS = 2 ** 24
_S = _lib.TemperatureState
STATE_BYTES = C.sizeof(_S)


def alpha_argument(who, alpha, dev):
    """What td_target and actor_loss accept for alpha -> (the finite Python number, None) or (None, the [1] fp64 tensor on `dev`
    that the *_alpha_dev entry points read: Temperature.alpha).  ValueError for anything else, before any library call."""
    if torch.is_tensor(alpha):
        if alpha.dtype != torch.float64 or tuple(alpha.shape) != (1,) or alpha.device != dev:
            raise ValueError('%s: a tensor alpha must be fp64 [1] on %s, not %s %s on %s' % (who, dev, alpha.dtype, tuple(alpha.shape), alpha.device))
        return None, alpha.detach()
    if not isinstance(alpha, (int, float)) or not math.isfinite(alpha):
        raise ValueError('%s: alpha %r must be a finite number or a [1] fp64 tensor' % (who, alpha))
    return float(alpha), None


def fresh_state_bytes(init_alpha, betas=(0.9, 0.999), step=0, log_alpha=None, m=0.0, v=0.0):
    """The 64 bytes of an f110_temperature_state as the host writes it: adam = {step, beta1 ** step, beta2 ** step, 0, 0}, alpha =
    init_alpha exactly, log_alpha = float(log(init_alpha)) unless given, the moments, grad = loss = 0."""
    s = _S()
    s.adam.t, s.adam.pow1, s.adam.pow2 = int(step), float(betas[0]) ** int(step), float(betas[1]) ** int(step)
    s.alpha = float(init_alpha)
    s.log_alpha = math.log(float(init_alpha)) if log_alpha is None else float(log_alpha)     # (the c_float field rounds once)
    s.m, s.v = float(m), float(v)
    return bytes(s)


class Temperature:
    """Temperature(init_alpha, target_entropy, lr, betas, eps): the temperature of one SAC agent and its optimizer.  target_entropy
    is SAC's usual -action_dim (SAL: 16 action values).  The 64-byte f110_temperature_state is one device tensor; alpha [1] fp64 and
    log_alpha, loss, grad [1] fp32 are views into it, so reading them synchronises only when the caller calls .item().  Before the
    first step alpha is init_alpha, bit for bit.  `lr` is a host scalar of each launch, settable between eager steps and frozen in a
    captured one.
    ValueError for init_alpha not finite or <= 0, for a CPU device and for what f110_temperature_validate refuses (betas outside
    [0, 1), eps <= 0, target_entropy or lr not finite)."""

    def __init__(self, init_alpha=0.2, target_entropy=-16.0, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, device='cuda'):
        who = 'Temperature'
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('%s: device %s: there is no CPU path' % (who, self.device))
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if not isinstance(init_alpha, (int, float)) or not math.isfinite(init_alpha) or not init_alpha > 0.0:
            raise ValueError('%s: init_alpha %r must be finite and > 0' % (who, init_alpha))
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.target_entropy = float(target_entropy)
        self._config()                                                  # (validates)
        if not math.isfinite(self.lr):
            raise ValueError('%s: lr is not finite' % who)
        assert _lib.load().f110_temperature_state_bytes() == STATE_BYTES
        self._state = torch.zeros((STATE_BYTES // 8,), dtype=torch.int64, device=self.device)
        f64, f32 = self._state.view(torch.float64), self._state.view(torch.float32)
        at = lambda field, size: getattr(_S, field).offset // size     # noqa: E731
        self.alpha = f64[at('alpha', 8):at('alpha', 8) + 1]
        self.log_alpha, self.loss, self.grad = (f32[at(k, 4):at(k, 4) + 1] for k in ('log_alpha', 'loss', 'grad'))
        self._m, self._v = (f32[at(k, 4):at(k, 4) + 1] for k in ('m', 'v'))
        self._write(fresh_state_bytes(init_alpha, self.betas))

    def _config(self):
        c = _lib.TemperatureConfig()
        c.beta1, c.beta2, c.eps, c.target_entropy = self.betas[0], self.betas[1], self.eps, self.target_entropy
        _lib.check(_lib.load().f110_temperature_validate(C.byref(c)))
        return c

    def _write(self, raw):
        """The whole state from 64 host bytes, in place (a captured step keeps reading this tensor)."""
        self._state.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int64))

    def state_words(self):
        """The state as the device holds it, eight int64 words on the host (synchronises)."""
        return self._state.cpu()

    @torch.no_grad()
    def step(self, logp):
        """One step on log_prob [n] or [n, 1], fp64 or fp32, 1 <= n <= 2^24, as the policy head returns it (it is detached here):
        one launch on the current stream, no synchronisation; afterwards .alpha is the next temperature and .loss / .grad are this
        step's.  Returns .loss."""
        who = 'Temperature.step'
        if not torch.is_tensor(logp) or logp.device != self.device or logp.dtype not in (torch.float64, torch.float32):
            raise ValueError('%s: logp must be a fp64 or fp32 tensor on %s' % (who, self.device))
        if logp.dim() not in (1, 2) or (logp.dim() == 2 and logp.shape[1] != 1) or not 1 <= logp.shape[0] <= MAX_ROWS:
            raise ValueError('%s: logp must be [n] or [n, 1] with n in 1..2^24, not %s' % (who, tuple(logp.shape)))
        if not math.isfinite(self.lr):
            raise ValueError('%s: lr is not finite' % who)
        x = logp.detach().reshape(-1).contiguous()
        cfg = self._config()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().f110_temperature_step(C.byref(cfg), x.data_ptr(), int(x.dtype == torch.float64), int(x.shape[0]),
                                                         self._state.data_ptr(), self.lr, _lib.stream(self.device)))
        return self.loss

    # ---- checkpoints
    def state_dict(self):
        """log_alpha, alpha, the moments m and v, the step count and the hyperparameters, as Python numbers (synchronises)."""
        s = _S.from_buffer_copy(self.state_words().numpy().tobytes())
        return dict(log_alpha=s.log_alpha, alpha=s.alpha, m=s.m, v=s.v, step=int(s.adam.t), lr=self.lr, betas=self.betas, eps=self.eps,
                    target_entropy=self.target_entropy)

    def load_state_dict(self, sd):
        """Continues from state_dict()'s result, written in place; the powers of the betas are beta ** step, computed once on the
        host, as SacAdam.load_state_dict does.  ValueError for a negative step and for hyperparameters that validate refuses."""
        who = 'Temperature.load_state_dict'
        step = int(sd['step'])
        if step < 0 or step != sd['step']:
            raise ValueError('%s: step %r' % (who, sd['step']))
        old = self.lr, self.betas, self.eps, self.target_entropy
        self.lr, self.betas, self.eps = float(sd['lr']), (float(sd['betas'][0]), float(sd['betas'][1])), float(sd['eps'])
        self.target_entropy = float(sd['target_entropy'])
        try:
            self._config()
            if not math.isfinite(self.lr):
                raise ValueError('%s: lr is not finite' % who)
        except ValueError:
            self.lr, self.betas, self.eps, self.target_entropy = old
            raise
        self._write(fresh_state_bytes(sd['alpha'], self.betas, step, sd['log_alpha'], sd['m'], sd['v']))
