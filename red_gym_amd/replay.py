"""Host side of the replay buffer (csrc/f110_replay.h): the ReplayBuffer of the reference's RL consumer (src/SAL.py:447-463)
and the `replay_buffer.push(obs, action, reward, next_obs, done)` of its training loop (:996-1001), kept on the device behind
the reward shaper.  A FILL image has two values, so a frame is stored as bits (8 KiB instead of 64 for 256 x 256), and once:
next_obs of step t is obs of step t + 1.  DEFAULTS are SAL's numbers (capacity 1 000 000 transitions, the raw action's 16
values).  There is no CPU path: frames are packed, drawn and unpacked by libf110_hip.so's replay kernels."""
import ctypes as C

import torch

from . import _lib
from .consumer import Consumer

DEFAULTS = dict(capacity=1000000, steps=None, action_dim=16)
TRIES = _lib.F110_REPLAY_TRIES
MAX_NSTEP = _lib.F110_REPLAY_MAX_NSTEP
MAX_STACK = _lib.F110_REPLAY_MAX_STACK


def make_config(num_envs=1, **cfg):
    """An f110_replay_config from keyword options; the missing ones take DEFAULTS.  `capacity` counts transitions as the
    reference's does: steps = capacity // num_envs step slots, unless `steps` says so itself."""
    unknown = set(cfg) - set(DEFAULTS)
    if unknown:
        raise TypeError('unknown replay option(s): %s' % ', '.join(sorted(unknown)))
    c = _lib.ReplayConfig()
    steps = cfg.get('steps')
    if steps is None:
        capacity = cfg.get('capacity')
        steps = int(DEFAULTS['capacity'] if capacity is None else capacity) // max(int(num_envs), 1)
    c.steps = max(min(int(steps), 2 ** 31 - 1), -1)
    c.action_dim = max(min(int(cfg.get('action_dim', DEFAULTS['action_dim'])), 2 ** 31 - 1), -1)
    return c


def validate(num_envs=1, shaping=None, **cfg):
    """f110_replay_validate (host only, no device): ValueError for what an install would refuse.  `shaping`: the options of the
    shaper the buffer records (a dict for red_gym_amd.shaping.make_config), None = shaping is off."""
    from .shaping import make_config as shaping_config
    sc = None if shaping is None else C.byref(shaping_config(**shaping))
    _lib.check(_lib.load().f110_replay_validate(C.byref(make_config(num_envs, **cfg)), sc, int(num_envs)))


def words(cols):
    return (int(cols) + 63) // 64


def pack_bitmaps(bitmaps):
    """f110_replay_pack: [n, rows, cols] uint8 device tensor -> [n, rows, ceil(cols / 64)] int64 (the bits of uint64 words: bit
    k of word w = (pixel[64 w + k] == 255), tail bits 0)."""
    lib = _lib.load()
    n, rows, cols = bitmaps.shape
    dev = bitmaps.device
    src = bitmaps.to(torch.uint8).contiguous()
    out = torch.empty((n, rows, words(cols)), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.f110_replay_pack(src.data_ptr(), n, rows, cols, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()   # the contiguous copy above may be a temporary
    return out


def unpack_bitmaps(packed, cols):
    """f110_replay_unpack: [n, rows, ceil(cols / 64)] int64 device tensor -> [n, rows, cols] uint8 of 0 / 255."""
    lib = _lib.load()
    n, rows, w = packed.shape
    if w != words(cols):
        raise ValueError('%d words per row do not hold %d pixels' % (w, cols))
    dev = packed.device
    src = packed.to(torch.int64).contiguous()
    out = torch.empty((n, rows, int(cols)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.f110_replay_unpack(src.data_ptr(), n, rows, int(cols), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()
    return out


def sample_fields(n, action_dim, nstep=1, priorities=False, stack=1):
    """THE FIELD TABLE of a batch of n transitions: name -> (shape, dtype).  frames_at, sample_frames, sample_frames_dev and
    sample_priority_dev return a dict of these fields plus 'frames' (ReplayBuffer.frame_view()); sample_out allocates them, and the
    device entries' `out` takes them.  A pure function: no ring, no device.
      indices [n] int64         the transitions (step slot * B + env; -1: none was found)
      s_idx, ns_idx [n] int64   rows of 'frames' that hold the frame before and the frame after (-1 for both: a zero transition)
      a [n, action_dim] fp32, r [n] fp64, d [n] uint8, ok [n] uint8    as sample_at returns them
    with nstep > 1, and always from the priority draw (r is then the n-step return, ns_idx and d those of the span's end):
      discount [n] fp64, span [n] int32      as nstep_at returns them
    from the priority draw only:
      prio [n] int32            the bits of the drawn uint32 priority words
      weight [n] fp32           the importance weights (N P(i))^-beta over the batch's maximum, 0 where ok is 0
    with stack > 1 (s_idx and ns_idx stay [n]: they are column 0 of the stacks):
      s_stack, ns_stack [n, stack] int64     stack_rows of s_idx and of ns_idx
      depth [2, n] int32        of s_idx, of ns_idx
      pair [2, n], stacks [2, n, stack] int64    storage: s_idx / ns_idx and s_stack / ns_stack are their halves, so that one
                                launch of the walk serves both"""
    shapes = {'indices': ((n,), torch.int64), 's_idx': ((n,), torch.int64), 'ns_idx': ((n,), torch.int64),
              'a': ((n, action_dim), torch.float32), 'r': ((n,), torch.float64), 'd': ((n,), torch.uint8), 'ok': ((n,), torch.uint8)}
    if nstep > 1 or priorities:
        shapes.update({'discount': ((n,), torch.float64), 'span': ((n,), torch.int32)})
    if priorities:
        shapes.update({'prio': ((n,), torch.int32), 'weight': ((n,), torch.float32)})
    if stack > 1:
        shapes.update({'pair': ((2, n), torch.int64), 'stacks': ((2, n, stack), torch.int64), 's_stack': ((n, stack), torch.int64),
                       'ns_stack': ((n, stack), torch.int64), 'depth': ((2, n), torch.int32)})
    return shapes


class ReplayBuffer(Consumer):
    """The replay buffer of one Engine (f110_replay_install / _bind / _update / _draw / _gather / _locate / _sample / _nstep / _sample_nstep / _stack).  The ring lives in `buf`:
    frames [T + 1, B, rows, words] int64 (bit-packed), actions [T, B, action_dim] fp32, rewards [T, B] fp64, dones and valid
    [T, B] uint8, count and chain_start [1] int64, t_seen [B] fp64, last_valid [B] uint8 and action_in [B, action_dim] fp32 (what
    the next push stores: F110VecEnv.replay_action).  A transition is named by index = step slot * B + env.  The ring is no part
    of state_dict(): save() / load() hand it over explicitly.  `priorities` is the ring's PriorityTree (red_gym_amd.priority) while
    record_replay(..., priorities=...) is on, else None: sample_priority_dev draws from it, save() and load() carry its leaves and state."""
    NAME = 'replay'
    INFO = {'replay_count': 'count', 'replay_valid': 'last_valid'}
    STATE = {}
    RING = ('frames', 'actions', 'rewards', 'dones', 'valid', 'count', 'chain_start', 't_seen')
    cfg, rows, cols, _draws = None, 0, 0, 0
    priorities = None               # the PriorityTree while record_replay(priorities=...) is on (red_gym_amd.priority)
    generation = 0                  # installs made: a graph captured on the ring of an earlier one holds freed addresses (SACAgent)

    steps = property(lambda self: self.cfg.steps)
    action_dim = property(lambda self: self.cfg.action_dim)

    def install(self, **cfg):
        """`cfg`: options of DEFAULTS.  An install allocates a new, empty ring for the image size of the shaper as it is
        installed now.  TypeError for an unknown option, ValueError for what the library refuses (the shaper is off)."""
        eng = self.eng
        c = make_config(eng.B, **cfg)
        _lib.check(eng.lib.f110_replay_install(eng._h, C.byref(c)))
        rows, cols = eng.shaper.cfg.rows, eng.shaper.cfg.cols
        T, B, ad = c.steps, eng.B, c.action_dim
        self.buf, self.info = None, {}          # (the old ring goes before the new one is allocated)
        self.priorities = None                  # (the library drops the priorities with the ring they were built over)
        try:
            with torch.cuda.device(eng.device):
                z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
                buf = {'frames': z((T + 1, B, rows, words(cols)), torch.int64), 'actions': z((T, B, ad), torch.float32),
                       'rewards': z((T, B), torch.float64), 'dones': z((T, B), torch.uint8), 'valid': z((T, B), torch.uint8),
                       'count': z((1,), torch.int64), 'chain_start': z((1,), torch.int64), 't_seen': z((B,), torch.float64),
                       'last_valid': z((B,), torch.uint8), 'action_in': z((B, ad), torch.float32)}
                buf['t_seen'].fill_(-1.0)
                self._bind(buf, _lib.ReplayBuffers)
        except Exception:
            eng.lib.f110_replay_install(eng._h, None)
            self.on = False
            raise
        self.cfg, self.rows, self.cols, self.on, self._draws = c, rows, cols, True, 0
        self.generation += 1

    def remove(self):
        """No launch, no info key remains and the ring is freed."""
        if self.on:
            _lib.check(self.eng.lib.f110_replay_install(self.eng._h, None))
            torch.cuda.synchronize(self.eng.device)   # an enqueued push may still write the ring
        self.cfg, self.on, self.buf, self.info, self.priorities = None, False, None, {}, None

    def set_priorities(self, priorities):
        """Switches prioritized replay on over the ring as it stands (True or a dict of red_gym_amd.priority.DEFAULTS' keys: every valid
        transition enters with the word of priority 1.0), or off (None or False: no launch remains)."""
        self._require_on()
        if self.priorities is not None:
            self.priorities.remove()
            self.priorities = None
        if priorities is not None and priorities is not False:
            from .priority import PriorityTree
            self.priorities = PriorityTree(self, priorities)

    def restart(self):
        """Breaks the chain of frames: the next push stores a frame and an invalid transition; what is stored stays."""
        self.buf['chain_start'].copy_(self.buf['count'])
        self.buf['t_seen'].fill_(-1.0)

    def on_load_state_dict(self, sd):
        self.restart()

    def save(self):
        """The ring and its counter as a dict of new tensors (gigabytes at the reference's capacity)."""
        d = {k: self.buf[k].clone() for k in self.RING}
        if self.priorities is not None:
            d.update(self.priorities.save())    # (the leaves and the state; the nodes are rebuilt on load)
        return d

    def load(self, d):
        """Restores what save() returned into a ring of the same shape; ValueError otherwise.  The chain of frames is restored
        with it: if the envs are not in the state they had at save(), call restart() (load_state_dict does)."""
        for k in self.RING:
            if k not in d or tuple(d[k].shape) != tuple(self.buf[k].shape):
                raise ValueError('replay: the saved ring does not fit (%s)' % k)
        for k in self.RING:
            self.buf[k].copy_(d[k])
        if self.priorities is not None:
            self.priorities.load(d)             # (a dict that carries no priorities resets the tree over the restored ring)

    def __len__(self):
        """Valid transitions held (one small reduction and one synchronisation: not for the step path)."""
        return int(self.buf['valid'].sum().item()) if self.on else 0

    def _require_on(self, priorities=False):
        if priorities and (not self.on or self.priorities is None):
            raise ValueError('replay: priorities are off (record_replay(..., priorities=True))')
        if not self.on:
            raise ValueError('replay: the buffer is off (record_replay())')

    def _indices(self, x):
        """Indices or frame rows as the kernels read them: [n] int64, contiguous, on the env's device."""
        return torch.as_tensor(x).to(device=self.eng.device, dtype=torch.int64).contiguous().reshape(-1)

    def _seed(self, seed):
        if seed is None:
            seed = self.eng.seed
            if seed is None:
                seed = 0
        return int(seed) & (2 ** 64 - 1)

    def draw(self, n, seed=None):
        """f110_replay_draw: (indices [n] int64, ok [n] uint8) of n draws, no synchronisation.  The draw counter moves on by n."""
        eng = self.eng
        idx = torch.empty((int(n),), dtype=torch.int64, device=eng.device)
        ok = torch.empty((int(n),), dtype=torch.uint8, device=eng.device)
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_replay_draw(eng._h, self._seed(seed), self._draws & (2 ** 64 - 1), int(n), idx.data_ptr(), ok.data_ptr(),
                                                eng._stream()))
        self._draws += int(n)
        return idx, ok

    def sample_at(self, indices, dtype=torch.uint8, scale=1.0):
        """f110_replay_gather for the transitions `indices` [n] (step slot * B + env; -1 or an invalid one: zeros and ok = 0).
        Returns (s, a, r, ns, d, ok): s and ns uint8 [n, rows, cols], or with dtype=torch.float32 fp32 [n, 1, rows, cols] =
        pixel * scale; a [n, action_dim] fp32, r [n] fp64, d [n] and ok [n] uint8.  Device tensors, no synchronisation."""
        self._require_on()
        if dtype not in (torch.uint8, torch.float32):
            raise ValueError('replay: dtype must be torch.uint8 or torch.float32')
        eng = self.eng
        idx = self._indices(indices)
        n = idx.shape[0]
        f32 = dtype == torch.float32
        shape = (n, 1, self.rows, self.cols) if f32 else (n, self.rows, self.cols)
        s, ns = torch.empty(shape, dtype=dtype, device=eng.device), torch.empty(shape, dtype=dtype, device=eng.device)
        a = torch.empty((n, self.cfg.action_dim), dtype=torch.float32, device=eng.device)
        r = torch.empty((n,), dtype=torch.float64, device=eng.device)
        d, ok = torch.empty((n,), dtype=torch.uint8, device=eng.device), torch.empty((n,), dtype=torch.uint8, device=eng.device)
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_replay_gather(eng._h, idx.data_ptr(), n, s.data_ptr(), ns.data_ptr(), int(f32), float(scale),
                                                  a.data_ptr(), r.data_ptr(), d.data_ptr(), ok.data_ptr(), eng._stream()))
        self._keep = idx   # (kept until the next call: the stream may not have read it yet)
        return s, a, r, ns, d, ok

    def sample(self, batch_size, seed=None, dtype=torch.uint8, scale=1.0):
        """batch_size transitions drawn uniformly over the valid ones, as sample_at returns them.  `seed` defaults to the
        env's; the host keeps the draw counter, so two calls never reuse draws.  A draw that found no valid transition in TRIES
        attempts (an empty buffer is one case) has ok = 0 and zeros."""
        self._require_on()
        idx, _ = self.draw(batch_size, seed)
        return self.sample_at(idx, dtype, scale)

    def _nstep(self, nstep, gamma):
        """(nstep, gamma) as the n-step entries take them; ValueError for nstep outside 1 .. MAX_NSTEP, a gamma that is no finite
        number, and a missing gamma where nstep > 1 (with nstep = 1 no product is formed and gamma only fills `discount`)."""
        import math
        if isinstance(nstep, bool) or not isinstance(nstep, int) or not 1 <= nstep <= MAX_NSTEP:
            raise ValueError('replay: nstep %r (an int in 1..%d)' % (nstep, MAX_NSTEP))
        if gamma is None and nstep > 1:
            raise ValueError('replay: nstep = %d needs a gamma' % nstep)
        if gamma is None:
            gamma = 1.0
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma):
            raise ValueError('replay: gamma %r is no finite number' % (gamma,))
        return nstep, float(gamma)

    def nstep_at(self, indices, nstep, gamma):
        """f110_replay_nstep: the truncated n-step return of the transitions `indices` [n], walked through the ring on the device
        (include/f110_hip.h has the contract).  Returns (ns_idx, ret, d, discount, span): ns_idx [n] int64 the row of frames_at's
        frame tensor that holds the frame after the span's last step, ret [n] fp64 = r_0 + gamma r_1 + ... over the span, d [n] uint8
        the done of its last step, discount [n] fp64 = gamma^span by running products (what the bootstrap is multiplied with) and
        span [n] int32, at most nstep: a span ends behind a terminal step, in front of an invalid transition and at the newest push.
        -1, 0, 0, gamma, 0 where frames_at gives a zero transition.  Device tensors, no synchronisation."""
        self._require_on()
        nstep, gamma = self._nstep(nstep, gamma)
        eng = self.eng
        idx = self._indices(indices)
        n = idx.shape[0]
        ns_idx = torch.empty((n,), dtype=torch.int64, device=eng.device)
        ret, discount = torch.empty((n,), dtype=torch.float64, device=eng.device), torch.empty((n,), dtype=torch.float64, device=eng.device)
        d, span = torch.empty((n,), dtype=torch.uint8, device=eng.device), torch.empty((n,), dtype=torch.int32, device=eng.device)
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_replay_nstep(eng._h, idx.data_ptr(), n, nstep, gamma, ns_idx.data_ptr(), ret.data_ptr(), d.data_ptr(),
                                                 discount.data_ptr(), span.data_ptr(), eng._stream()))
        self._keep_nstep = idx   # (kept until the next call: the stream may not have read it yet)
        return ns_idx, ret, d, discount, span

    @staticmethod
    def _stack(stack):
        """`stack` as the walk takes it; ValueError unless it is an int in 1 .. MAX_STACK."""
        if isinstance(stack, bool) or not isinstance(stack, int) or not 1 <= stack <= MAX_STACK:
            raise ValueError('replay: stack %r (an int in 1..%d)' % (stack, MAX_STACK))
        return stack

    def _walk_back(self, rows, n, stack, stack_rows, depth):
        eng = self.eng
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_replay_stack(eng._h, _lib.ptr(rows), n, stack, stack_rows.data_ptr(), depth.data_ptr(), eng._stream()))

    def stack_rows(self, rows, stack):
        """f110_replay_stack: the last `stack` frames of the env behind each of the frame rows `rows` [n] (rows of frames_at's frame
        tensor: an s_idx or ns_idx), walked backwards through the ring on the device (include/f110_hip.h "Frame stacks").  Returns
        (stack_rows [n, stack] int64, depth [n] int32): column 0 is `rows`, column j the row of the frame j pushes earlier while the
        pushes between them belong to one episode and are still stored, else the oldest row reached, repeated; depth counts the
        distinct frames, 1 .. stack.  -1 in every column and depth 0 for a row outside the tensor (-1) or one no push has written.
        A stack at learning time can be shorter than the one the policy acted on, for the stack - 1 oldest pushes of the ring only
        (their predecessors are overwritten); depth shows it.  Device tensors, no synchronisation; stack in 1 .. MAX_STACK."""
        self._require_on()
        stack = self._stack(stack)
        eng = self.eng
        r = self._indices(rows)
        n = r.shape[0]
        out = torch.empty((n, stack), dtype=torch.int64, device=eng.device)
        depth = torch.empty((n,), dtype=torch.int32, device=eng.device)
        if n:
            self._walk_back(r, n, stack, out, depth)
        self._keep_stack = r   # (kept until the next call: the stream may not have read it yet)
        return out, depth

    def stack_latest(self, stack, out=None):
        """f110_replay_stack's latest mode: stack_rows of every env's newest frame (the bitmap its last step returned), [B, stack]
        int64 and depth [B] int32 -- the stack a policy acts on.  Nothing crosses from the host that changes from call to call, so
        a captured call follows the ring.  An empty ring gives -1 and depth 0.  out: (stack_rows, depth) tensors to write into."""
        self._require_on()
        stack = self._stack(stack)
        eng, B = self.eng, self.eng.B
        if out is None:
            out = (torch.empty((B, stack), dtype=torch.int64, device=eng.device), torch.empty((B,), dtype=torch.int32, device=eng.device))
        rows, depth = out
        for t, shape, dt in ((rows, (B, stack), torch.int64), (depth, (B,), torch.int32)):
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != torch.device(eng.device) or not t.is_contiguous():
                raise ValueError('replay: out must be contiguous (%s [%d, %d], int32 [%d]) tensors on %s' % (torch.int64, B, stack, B, eng.device))
        self._walk_back(None, B, stack, rows, depth)
        return rows, depth

    def frame_view(self):
        """The ring's frame tensor viewed as [(T + 1) * B, rows, words] int64: what the rows of frames_at, stack_rows and
        stack_latest point into (a view, no copy: it changes with the next push)."""
        return self.buf['frames'].view((self.cfg.steps + 1) * self.eng.B, self.rows, words(self.cols))

    def _stacked(self, b, stack):
        """The one launch of the walk over b['pair'] (s_idx above ns_idx) into b['stacks'] and b['depth']."""
        n = int(b['pair'].shape[1])
        if n:
            self._walk_back(b['pair'], 2 * n, stack, b['stacks'], b['depth'])

    def frames_at(self, indices, nstep=1, gamma=None, stack=1):
        """The transitions `indices` [n] without unpacking an image, for consumers that read bits (red_gym_amd.bitconv).
        Returns the batch as a dict: the fields of sample_fields(n, action_dim, nstep, stack=stack) -- the table is there -- and
        'frames', the ring's frame tensor as frame_view() gives it (a view, no copy: it changes with the next push).  s_idx and
        ns_idx are f110_replay_locate's, and a, r, d, ok exactly what sample_at(indices) returns.  Device tensors, no synchronisation.
        nstep > 1 (gamma is then required): r, ns_idx, d, discount and span are what nstep_at(indices, nstep, gamma) gives.
        stack > 1: s_stack, ns_stack and depth are stack_rows of s_idx and of ns_idx (with nstep > 1 ns_idx is the span's end)."""
        self._require_on()
        nstep, gamma = self._nstep(nstep, gamma)
        stack = self._stack(stack)
        eng = self.eng
        idx = self._indices(indices)
        n = idx.shape[0]
        s_idx = torch.empty((n,), dtype=torch.int64, device=eng.device)
        ns_idx = torch.empty((n,), dtype=torch.int64, device=eng.device)
        with torch.cuda.device(eng.device):
            _lib.check(eng.lib.f110_replay_locate(eng._h, idx.data_ptr(), n, s_idx.data_ptr(), ns_idx.data_ptr(), eng._stream()))
        self._keep = idx   # (kept until the next call: the stream may not have read it yet)
        T, B = self.cfg.steps, eng.B
        found = s_idx >= 0
        at = torch.where(found, idx, torch.zeros_like(idx))
        a = torch.where(found[:, None], self.buf['actions'].view(T * B, -1)[at], torch.zeros((), dtype=torch.float32, device=eng.device))
        r = torch.where(found, self.buf['rewards'].view(-1)[at], torch.zeros((), dtype=torch.float64, device=eng.device))
        d = torch.where(found, self.buf['dones'].view(-1)[at], torch.zeros((), dtype=torch.uint8, device=eng.device))
        b = dict(frames=self.frame_view(), indices=idx, s_idx=s_idx, ns_idx=ns_idx, a=a, r=r, d=d, ok=found.to(torch.uint8))
        if nstep > 1:
            b['ns_idx'], b['r'], b['d'], b['discount'], b['span'] = self.nstep_at(idx, nstep, gamma)
        if stack > 1:
            b['pair'] = self._keep_pair = torch.stack((b['s_idx'], b['ns_idx']))
            b['stacks'] = torch.empty((2, n, stack), dtype=torch.int64, device=eng.device)
            b['depth'] = torch.empty((2, n), dtype=torch.int32, device=eng.device)
            b['s_stack'], b['ns_stack'] = b['stacks'][0], b['stacks'][1]
            self._stacked(b, stack)
        return b

    def sample_frames(self, batch_size, seed=None):
        """batch_size transitions drawn as sample() draws them (the same draw counter), returned as frames_at returns them."""
        self._require_on()
        idx, _ = self.draw(batch_size, seed)
        return self.frames_at(idx)

    def _sample_dev(self, batch_size, counter, seed, out, nstep, gamma, stack, priorities):
        """What sample_frames_dev and sample_priority_dev share: the inputs checked, `out` picked or checked, the one library call of the
        combination (f110_priority_sample with priorities, else f110_replay_sample_nstep with nstep > 1, else f110_replay_sample)
        and, with stack > 1, the one launch of the walk over out['pair'] behind it.  Returns a NEW dict -- out's own tensors and
        'frames' -- and leaves `out` as it was: a caller keeps `out` across re-installs of the ring, and a frame view stored there
        would pin the old ring's memory."""
        self._require_on(priorities)
        nstep, gamma = self._nstep(nstep, gamma)
        stack = self._stack(stack)
        eng, n = self.eng, int(batch_size)
        if not torch.is_tensor(counter) or counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != torch.device(eng.device):
            raise ValueError('replay: counter must be a [1] int64 tensor on %s' % (eng.device,))
        o = self.sample_out(n, nstep, priorities, stack) if out is None else out
        self._check_out(o, n, nstep, priorities, stack)
        draw = (eng._h, self._seed(seed), counter.data_ptr(), n)
        ptr = lambda *keys: tuple(o[k].data_ptr() for k in keys)  # noqa: E731
        batch = ptr('indices', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok')
        with torch.cuda.device(eng.device):
            if priorities:
                _lib.check(eng.lib.f110_priority_sample(*draw, nstep, gamma, *batch, *ptr('discount', 'span', 'prio', 'weight'), eng._stream()))
            elif nstep > 1:
                _lib.check(eng.lib.f110_replay_sample_nstep(*draw, nstep, gamma, *batch, *ptr('discount', 'span'), eng._stream()))
            else:
                _lib.check(eng.lib.f110_replay_sample(*draw, *batch, eng._stream()))
        if stack > 1:
            self._stacked(o, stack)
        return dict(o, frames=self.frame_view())

    def sample_frames_dev(self, batch_size, counter, seed=None, out=None, nstep=1, gamma=None, stack=1):
        """f110_replay_sample: batch_size transitions drawn from a draw counter that lives on the device, in one kernel.  counter: a
        [1] int64 tensor on the env's device (the bits of the library's uint64; start it at 0) that the caller owns; the call draws
        draw numbers counter .. counter + batch_size - 1 of the stream `seed` (default: the env's) exactly as draw() would with
        that counter, and a one-lane kernel behind it adds batch_size.  Nothing crosses from the host that changes from call to
        call, so a captured call replays with fresh draws.  The host counter of draw(), sample() and sample_frames() does not move.
        Returns the batch as a dict (sample_fields has the table): everything but 'indices' is what frames_at(indices, nstep, gamma,
        stack) returns.  out: a dict of the static tensors to write into (sample_out(n, nstep, stack=stack) allocates one); the
        returned dict is a new one that holds the same tensors and 'frames', `out` itself is not changed.  Device tensors, no
        synchronisation.
        nstep > 1 (gamma is then required): f110_replay_sample_nstep, the same draws with the n-step walk in the same kernel.
        stack > 1: the sample kernels are untouched and one launch of the walk (stack_rows) runs behind them."""
        return self._sample_dev(batch_size, counter, seed, out, nstep, gamma, stack, False)

    def sample_priority_dev(self, batch_size, counter, seed=None, out=None, nstep=1, gamma=None, stack=1):
        """f110_priority_sample: sample_frames_dev with draws in proportion to the transitions' priority words (record_replay(...,
        priorities=...)), from the caller's device counter, in two launches.  The batch holds 'discount' and 'span' whatever nstep
        is, and 'prio' and 'weight' (sample_fields(..., priorities=True)): the weights are exactly 1.0 on the rows of the smallest
        word, for the beta the tree held before this call moved it on.  out: sample_out(n, nstep, priorities=True, stack=stack).
        Device tensors, no synchronisation; a captured call replays with fresh draws."""
        return self._sample_dev(batch_size, counter, seed, out, nstep, gamma, stack, True)

    def _check_out(self, o, n, nstep, priorities, stack):
        dev = torch.device(self.eng.device)
        for k, (shape, dt) in self._sample_shapes(n, nstep, priorities, stack).items():
            t = o.get(k)
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError('replay: out[%r] must be a contiguous %s tensor of shape %s on %s' % (k, dt, shape, dev))
        if stack > 1 and (o['s_idx'].data_ptr() != o['pair'].data_ptr() or o['ns_idx'].data_ptr() != o['pair'][1].data_ptr()
                          or o['s_stack'].data_ptr() != o['stacks'].data_ptr() or o['ns_stack'].data_ptr() != o['stacks'][1].data_ptr()):
            raise ValueError("replay: out['s_idx'] / out['ns_idx'] and out['s_stack'] / out['ns_stack'] must be the halves of out['pair'] and "
                             "out['stacks'] (sample_out(..., stack=k))")

    def _sample_shapes(self, n, nstep=1, priorities=False, stack=1):
        return sample_fields(n, self.cfg.action_dim, nstep, priorities, stack)

    def sample_out(self, batch_size, nstep=1, priorities=False, stack=1):
        """The tensors sample_frames_dev writes, newly allocated: what its `out` takes (sample_fields(batch_size, action_dim, nstep,
        priorities, stack); priorities=True: what sample_priority_dev writes).  With stack > 1 's_idx' / 'ns_idx' are the halves of
        'pair' and the two stacks the halves of 'stacks'."""
        stack = self._stack(stack)
        shapes = self._sample_shapes(int(batch_size), int(nstep), bool(priorities), stack)
        o = {k: torch.empty(shape, dtype=dt, device=self.eng.device) for k, (shape, dt) in shapes.items() if stack == 1 or k not in ('s_idx', 'ns_idx', 's_stack', 'ns_stack')}
        if stack > 1:
            o['s_idx'], o['ns_idx'], o['s_stack'], o['ns_stack'] = o['pair'][0], o['pair'][1], o['stacks'][0], o['stacks'][1]
        return o

    def bytes_held(self):
        return sum(self.buf[k].numel() * self.buf[k].element_size() for k in ('frames', 'actions', 'rewards', 'dones', 'valid'))

    def bytes_raw(self):
        """What the same transitions cost as the reference stores them: two raw uint8 images, the action, reward and done."""
        T, B = self.cfg.steps, self.eng.B
        return T * B * (2 * self.rows * self.cols + 4 * self.cfg.action_dim + 8 + 1)
