"""Host side of prioritized replay (csrc/f110_priority.h, the contract is include/f110_hip.h's): an exact integer sum tree over the
replay ring's transitions, on the device.  A priority is a uint32 word (fixed point, 16 fraction bits), a node the uint64 sum of its up
to 64 children, so every sum is exact and the tree is the same in every run.  PriorityTree is what F110VecEnv.record_replay(...,
priorities=...) hangs on the ring as env.replay.priorities; the stateless functions below run the tree alone at any leaf count.  There is
no CPU path: the kernels of libf110_hip.so do the work."""
import ctypes as C

import torch

from . import _lib

DEFAULTS = dict(exponent=0.6, eps=1e-6, beta=0.4, beta_end=1.0, beta_updates=100000)
SHIFT = _lib.F110_PRIORITY_SHIFT
STATE_BYTES = _lib.F110_PRIORITY_STATE_BYTES
ONE = 1 << SHIFT                       # the word of priority 1.0: what qmax starts at


def node_words(leaves):
    """f110_priority_node_words: uint64 words of node[] for `leaves` leaves (0 while leaves <= 64); ValueError outside the limits."""
    w = int(_lib.load().f110_priority_node_words(int(leaves)))
    if w < 0:
        raise ValueError('priority: %d leaves (1..2^31)' % int(leaves))
    return w


def fresh_state_bytes(beta=DEFAULTS['beta'], beta_step=0.0, beta_end=DEFAULTS['beta_end'], qmax=ONE):
    """The 64 bytes of an f110_priority_state."""
    s = _lib.PriorityState()
    s.qmax, s.beta, s.beta_step, s.beta_end = int(qmax), float(beta), float(beta_step), float(beta_end)
    return bytes(s)


def _u32(t, name, dev=None):
    """A tensor that holds uint32 words: int32 bits (torch's uint32 has few kernels), contiguous, on a GPU."""
    if not torch.is_tensor(t) or t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or (dev is not None and t.device != dev):
        raise ValueError('priority: %s must be a contiguous int32 tensor (the bits of uint32 words) on %s' % (name, dev or 'a GPU'))
    return t


def _nodes(leaf, node):
    want = node_words(leaf.numel())
    if not torch.is_tensor(node) or node.dtype != torch.int64 or node.device != leaf.device or not node.is_contiguous() or node.numel() < want:
        raise ValueError('priority: node must be a contiguous int64 tensor of at least %d words on %s' % (want, leaf.device))
    return node


def new_nodes(leaf):
    """A zeroed node array for the leaves `leaf` (at least one word, so that it always has an address)."""
    return torch.zeros((max(node_words(leaf.numel()), 1),), dtype=torch.int64, device=leaf.device)


def rebuild(leaf, node):
    """f110_ptree_rebuild: every level of `node` from `leaf` ([L] int32 = the bits of the uint32 words)."""
    leaf = _u32(leaf, 'leaf')
    node = _nodes(leaf, node)
    with torch.cuda.device(leaf.device):
        _lib.check(_lib.load().f110_ptree_rebuild(leaf.data_ptr(), node.data_ptr(), leaf.numel(), _lib.stream(leaf.device)))
    return node


def set_words(leaf, node, idx, q):
    """f110_ptree_set: leaf[idx] = q (the maximum where several rows name one leaf; rows outside 0 .. L - 1 are skipped) and every
    ancestor fixed.  idx [n] int64, q [n] int32 bits."""
    leaf = _u32(leaf, 'leaf')
    node = _nodes(leaf, node)
    q = _u32(q, 'q', leaf.device)
    if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.device != leaf.device or not idx.is_contiguous() or idx.shape != q.shape:
        raise ValueError('priority: idx must be a contiguous int64 tensor of q\'s shape on %s' % (leaf.device,))
    with torch.cuda.device(leaf.device):
        _lib.check(_lib.load().f110_ptree_set(leaf.data_ptr(), node.data_ptr(), leaf.numel(), idx.data_ptr(), q.data_ptr(), idx.numel(),
                                              _lib.stream(leaf.device)))


def pick(leaf, node, seed, first_draw, n):
    """f110_ptree_pick: (idx [n] int64, q [n] int32 bits) of draws first_draw .. first_draw + n - 1 of the stream `seed`."""
    leaf = _u32(leaf, 'leaf')
    node = _nodes(leaf, node)
    idx = torch.empty((int(n),), dtype=torch.int64, device=leaf.device)
    q = torch.empty((int(n),), dtype=torch.int32, device=leaf.device)
    with torch.cuda.device(leaf.device):
        _lib.check(_lib.load().f110_ptree_pick(leaf.data_ptr(), node.data_ptr(), leaf.numel(), int(seed) & (2 ** 64 - 1),
                                               int(first_draw) & (2 ** 64 - 1), int(n), idx.data_ptr(), q.data_ptr(), _lib.stream(leaf.device)))
    return idx, q


def make_options(priorities):
    """record_replay's `priorities` as a full dict of DEFAULTS' keys; TypeError for an unknown key, ValueError for a bad schedule."""
    import math
    opt = dict(DEFAULTS)
    if isinstance(priorities, dict):
        unknown = set(priorities) - set(DEFAULTS)
        if unknown:
            raise TypeError('unknown priority option(s): %s' % ', '.join(sorted(unknown)))
        opt.update(priorities)
    elif priorities is not True:
        raise TypeError('priorities must be None, True or a dict of %s' % ', '.join(sorted(DEFAULTS)))
    for k in ('exponent', 'eps', 'beta', 'beta_end'):
        if isinstance(opt[k], bool) or not isinstance(opt[k], (int, float)) or not math.isfinite(opt[k]):
            raise ValueError('priority: %s %r is no finite number' % (k, opt[k]))
    if opt['beta'] < 0.0 or opt['beta_end'] < opt['beta']:
        raise ValueError('priority: 0 <= beta <= beta_end, not %r and %r' % (opt['beta'], opt['beta_end']))
    if isinstance(opt['beta_updates'], bool) or not isinstance(opt['beta_updates'], int) or opt['beta_updates'] < 1:
        raise ValueError('priority: beta_updates %r (an int >= 1)' % (opt['beta_updates'],))
    return opt


class PriorityTree(object):
    """The priorities of one ReplayBuffer (f110_priority_install / _bind / _reset / _update / _set).  leaf [T * B] int32 (the bits of the
    uint32 words; the position is the transition index), node int64 (the bits of the uint64 sums, level 1 first) and state [8] int64 (the
    64 bytes of f110_priority_state) live on the env's device.  While it is installed every push gives the pushed row the word qmax
    (0 where the transition is invalid), ReplayBuffer.sample_priority_dev draws in proportion to the words and update() writes the
    words of new TD errors back."""

    def __init__(self, replay, priorities=True):
        self.replay, self.opt = replay, make_options(priorities)
        eng = replay.eng
        cfg = _lib.PriorityConfig()
        cfg.exponent, cfg.eps = float(self.opt['exponent']), float(self.opt['eps'])
        _lib.check(eng.lib.f110_priority_install(eng._h, C.byref(cfg)))
        try:
            L = replay.cfg.steps * eng.B
            with torch.cuda.device(eng.device):
                self.leaf = torch.zeros((L,), dtype=torch.int32, device=eng.device)
                self.node = new_nodes(self.leaf)
                self.state = torch.zeros((STATE_BYTES // 8,), dtype=torch.int64, device=eng.device)
            self._write_state(self.opt['beta'], ONE)
            b = _lib.PriorityBuffers()
            b.leaf, b.node, b.state = self.leaf.data_ptr(), self.node.data_ptr(), self.state.data_ptr()
            torch.cuda.synchronize(eng.device)
            _lib.check(eng.lib.f110_priority_bind(eng._h, C.byref(b)))
        except Exception:
            eng.lib.f110_priority_install(eng._h, None)
            raise
        self.reset()

    beta_step = property(lambda self: (self.opt['beta_end'] - self.opt['beta']) / self.opt['beta_updates'])

    def _write_state(self, beta, qmax):
        raw = fresh_state_bytes(beta, self.beta_step, self.opt['beta_end'], qmax)
        self.state.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int64))

    def remove(self):
        eng = self.replay.eng
        _lib.check(eng.lib.f110_priority_install(eng._h, None))
        torch.cuda.synchronize(eng.device)     # an enqueued push may still write the tree

    def reset(self):
        """f110_priority_reset: every valid transition gets the word qmax, every other one 0, and the nodes are rebuilt (after the feature
        is switched on over a filled ring, and after a load() that carried no priorities)."""
        eng = self.replay.eng
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_priority_reset(eng._h, eng._stream()))

    def rebuild(self):
        """The nodes from the leaves as they stand (after the leaves were loaded)."""
        rebuild(self.leaf, self.node)

    def set_beta(self, beta):
        """beta as the next sample reads it (it goes on by beta_step per sample, up to beta_end).  One synchronisation."""
        beta = float(beta)
        if not 0.0 <= beta <= self.opt['beta_end']:
            raise ValueError('priority: beta %r (0..beta_end = %r)' % (beta, self.opt['beta_end']))
        self._write_state(beta, self.qmax)

    @property
    def beta(self):
        """beta on the device (one synchronisation)."""
        return float(self.state[1:2].view(torch.float64).item())

    @property
    def qmax(self):
        """qmax on the device (one synchronisation)."""
        return int(self.state[0].item()) & 0xFFFFFFFF

    def update(self, indices, ok, td, q_out=None):
        """f110_priority_update: the words of the TD errors td [n] fp32 written to the transitions indices [n] int64 on the rows with ok
        [n] uint8 whose transition is valid; the maximum where several rows name one transition; qmax raised to the largest.  q_out: an
        [n] int32 tensor that receives the words applied (0 on a skipped row).  Two launches on the current stream, no synchronisation."""
        eng = self.replay.eng
        dev = torch.device(eng.device)
        for name, t, dt in (('indices', indices, torch.int64), ('ok', ok, torch.uint8), ('td', td, torch.float32)):
            if not torch.is_tensor(t) or t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() != indices.numel():
                raise ValueError('priority: %s must be a contiguous %s tensor of n elements on %s' % (name, dt, dev))
        if q_out is not None:
            _u32(q_out, 'q_out', dev)
        with torch.cuda.device(dev):
            _lib.check(eng.lib.f110_priority_update(eng._h, indices.data_ptr(), ok.data_ptr(), td.data_ptr(), indices.numel(), _lib.ptr(q_out),
                                                    eng._stream()))
        return q_out

    def set(self, indices, q):
        """f110_priority_set: update() with the words given (q [n] int32 bits) on every row whose transition is valid."""
        eng = self.replay.eng
        dev = torch.device(eng.device)
        _u32(q, 'q', dev)
        if not torch.is_tensor(indices) or indices.dtype != torch.int64 or indices.device != dev or not indices.is_contiguous() or indices.numel() != q.numel():
            raise ValueError('priority: indices must be a contiguous int64 tensor of q\'s size on %s' % (dev,))
        with torch.cuda.device(dev):
            _lib.check(eng.lib.f110_priority_set(eng._h, indices.data_ptr(), q.data_ptr(), q.numel(), eng._stream()))

    def save(self):
        return {'priority_leaf': self.leaf.clone(), 'priority_state': self.state.clone()}

    def load(self, d):
        """The leaves and the state of save(); the nodes are rebuilt.  A dict without them (or of another shape) resets the tree."""
        if all(k in d and tuple(d[k].shape) == tuple(t.shape) for k, t in (('priority_leaf', self.leaf), ('priority_state', self.state))):
            self.leaf.copy_(d['priority_leaf'])
            self.state.copy_(d['priority_state'])
            self.rebuild()
        else:
            self.reset()
