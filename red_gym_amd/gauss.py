"""The policy's Gaussian draws made on the GPU (csrc/f110_gauss.h): the eps of PolicyHead.sample, in place of torch.randn.  Element
(row r, column j) of call t of stream s under `seed` is
    float32(numpy.random.Generator(numpy.random.Philox(key=[seed, s], counter=[0, j, r, t])).standard_normal())
-- NumPy's bits, the contract of include/f110_hip.h -- so a row's draws do not depend on the batch around it or on what was drawn
before, and the whole of the generator is a seed and four call counters in one 64-byte device tensor that a checkpoint holds.  A fill
reads its t on the device and a one-lane kernel behind it advances the counter, so a fill captured in a torch.cuda.graph replays with
a fresh t.  There is no CPU path and no torch fallback: the kernel of libf110_hip.so does the work."""
import ctypes as C

import torch

from . import _lib

STREAMS = _lib.F110_GAUSS_STREAMS
MAX_COLUMNS = _lib.F110_GAUSS_MAX_COLUMNS
_S = _lib.GaussState
STATE_BYTES = C.sizeof(_S)
_CALLS = _S.calls.offset // 8
_MASK = 2 ** 64 - 1


def _signed(v):
    """A 64-bit pattern as the int64 that holds it."""
    v = int(v) & _MASK
    return v - 2 ** 64 if v >= 2 ** 63 else v


def fresh_state_words(seed, calls=(0, 0, 0, 0)):
    """The eight int64 words of an f110_gauss_state as the host writes it: seed, calls[4], zeros."""
    if len(calls) != STREAMS:
        raise ValueError('GaussianSource: calls must hold %d counters' % STREAMS)
    s = _S()
    s.seed = int(seed) & _MASK
    for k, c in enumerate(calls):
        s.calls[k] = int(c) & _MASK
    return [_signed(w) for w in (C.c_uint64 * (STATE_BYTES // 8)).from_buffer_copy(bytes(s))]


class GaussianSource:
    """GaussianSource(seed, device): the draws of one agent.  `state` is the int64 [8] device tensor (seed, one call counter per
    stream, padding); streams 0 .. 3 count their calls separately.  seed: any integer, taken modulo 2^64.
    ValueError for a CPU device, and from normal / normal_at for what f110_gauss_fill refuses (n < 1, A outside 1 .. 32, a stream
    outside 0 .. 3, n * A above 2^31) and for an out or rows of another dtype, shape or device."""

    def __init__(self, seed=0, device='cuda'):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('GaussianSource: device %s: there is no CPU path' % (self.device,))
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        assert _lib.load().f110_gauss_state_bytes() == STATE_BYTES
        self.seed = int(seed) & _MASK
        self.state = torch.tensor(fresh_state_words(self.seed), dtype=torch.int64, device=self.device)
        # one element now: the runtime loads a code object at its first launch, and a source's first fill may stand inside a capture
        self.normal_at(0, 0, 1, 1)

    def _arguments(self, who, n, A, rows, out):
        n, A = int(n), int(A)
        if rows is not None:
            if not torch.is_tensor(rows) or rows.dtype != torch.int64 or tuple(rows.shape) != (n,) or rows.device != self.device:
                raise ValueError('%s: rows must be int64 [%d] on %s' % (who, n, self.device))
            rows = rows.contiguous()
        if out is None:
            if n < 1 or not 1 <= A <= MAX_COLUMNS or n * A > 2 ** 31:
                raise ValueError('%s: n=%d rows of A=%d columns (n >= 1, A in 1..%d, n * A <= 2^31)' % (who, n, A, MAX_COLUMNS))
            out = torch.empty((n, A), dtype=torch.float32, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (n, A) or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError('%s: out must be a contiguous fp32 [%d, %d] tensor on %s' % (who, n, A, self.device))
        return n, _lib.clamp(A), rows, out

    @torch.no_grad()
    def normal(self, n, A, stream=0, rows=None, out=None, advance=True):
        """The [n, A] fp32 draws of call t = calls()[stream], read on the device; rows: the int64 [n] row ids (None: 0 .. n-1); out:
        the tensor that receives them (a static buffer of a captured graph).  advance: the counter of `stream` then stands at t + 1.
        One or two launches on the current stream, no synchronisation."""
        n, A, rows, out = self._arguments('GaussianSource.normal', n, A, rows, out)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().f110_gauss_fill(self.state.data_ptr(), _lib.clamp(stream), n, A, _lib.ptr(rows), out.data_ptr(),
                                                   1 if advance else 0, _lib.stream(self.device)))
        return out

    @torch.no_grad()
    def normal_at(self, stream, t, n, A, rows=None, out=None):
        """The draws of call `t` of `stream` under this source's seed, whatever the counters say; nothing advances."""
        n, A, rows, out = self._arguments('GaussianSource.normal_at', n, A, rows, out)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().f110_gauss_fill_at(self.seed, _lib.clamp(stream), int(t) & _MASK, n, A, _lib.ptr(rows), out.data_ptr(),
                                                      _lib.stream(self.device)))
        return out

    def calls(self):
        """The four call counters as Python integers (one synchronisation)."""
        return [int(w) & _MASK for w in self.state[_CALLS:_CALLS + STREAMS].tolist()]

    # ---- checkpoints
    def state_dict(self):
        return dict(seed=self.seed, calls=self.calls())

    def load_state_dict(self, sd):
        """Continues from state_dict()'s result, written in place: a captured fill keeps reading this tensor."""
        words = fresh_state_words(sd['seed'], list(sd['calls']))
        self.seed = int(sd['seed']) & _MASK
        self.state.copy_(torch.tensor(words, dtype=torch.int64))
