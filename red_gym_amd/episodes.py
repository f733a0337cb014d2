"""Host side of the episode tracker (csrc/f110_episodes.h): the episode of the reference's training loop (src/SAL.py:986-1015:
`ep_reward = 0; for st in range(max_steps): ...; ep_reward += reward; if done: break`) for every env on the device -- the running
return and length, a step limit per env (max_steps = 2000 there) that ends an episode the env itself never ends, and a log of the
finished episodes.  There is no CPU path: the rules run in libf110_hip.so's episodes kernels."""
import ctypes as C

import torch

from . import _lib
from .consumer import Consumer

DONE, LIMIT, RESET = _lib.F110_EPISODE_DONE, _lib.F110_EPISODE_LIMIT, _lib.F110_EPISODE_RESET
REASONS = {DONE: 'done', LIMIT: 'limit', RESET: 'reset'}
DEFAULTS = dict(limit=2000, log=4096)
STATE_DTYPES = {'ep_return': torch.float64, 'ep_length': torch.int32, 'ep_open': torch.uint8, 't_seen': torch.float64,
                'truncated': torch.uint8, 'limit': torch.int32}
LOG_DTYPES = {'log_env': torch.int32, 'log_length': torch.int32, 'log_return': torch.float64, 'log_reason': torch.uint8,
              'log_time': torch.float64, 'log_laps': torch.int32}


def make_config(limit=DEFAULTS['limit'], log=DEFAULTS['log']):
    """An f110_episodes_config; sizes beyond int32 reach the library's validate clamped, which names them."""
    c = _lib.EpisodesConfig()
    c.limit, c.log = _lib.clamp(limit), _lib.clamp(log)
    return c


def validate(limit=DEFAULTS['limit'], log=DEFAULTS['log']):
    """f110_episodes_validate (host only, no device): ValueError for a negative limit and for a log outside 1..2^24."""
    _lib.check(_lib.load().f110_episodes_validate(C.byref(make_config(limit, log))))


def blocks(n):
    """Entries of the scratch array block_counts for n envs."""
    return max((int(n) + _lib.F110_EPISODES_BLOCK - 1) // _lib.F110_EPISODES_BLOCK, 1)


def new_buffers(n, log, device):
    """The tracker's arrays for n envs and a log of `log` records, as a fresh run starts: every episode open, nothing seen."""
    buf = {k: torch.zeros((n,), dtype=dt, device=device) for k, dt in STATE_DTYPES.items()}
    buf.update({k: torch.zeros((log,), dtype=dt, device=device) for k, dt in LOG_DTYPES.items()})
    buf['count'] = torch.zeros((1,), dtype=torch.int64, device=device)
    buf['block_counts'] = torch.zeros((blocks(n),), dtype=torch.int32, device=device)
    buf['ep_open'].fill_(1)
    buf['t_seen'].fill_(-1.0)
    return buf


def pointers(buf, limit=True):
    """The f110_episodes_buffers of the tensors `buf` (limit=False: no limit array, the config's limit for every env)."""
    ptrs = _lib.EpisodesBuffers()
    for name in _lib.EPISODES_FIELDS:
        setattr(ptrs, name, None if name == 'limit' and not limit else buf[name].data_ptr())
    return ptrs


def apply(buf, current_time, done, timestep, reward=None, laps=None, pending_reset=None, limit=None, log=None):
    """f110_episodes_apply: one update of the arrays `buf` (new_buffers) for what a step left -- current_time [n] fp64, done [n]
    uint8 or bool, reward [n] fp64 (None: the constant timestep), laps [n] int32 (None: 0 is logged), pending_reset [n] uint8 (None:
    autoreset off).  limit: one int for every env (None: buf['limit'] per env).  Contiguous device tensors; no synchronisation."""
    n = current_time.shape[0]
    c = make_config(0 if limit is None else limit, buf['log_env'].shape[0] if log is None else log)
    ptrs = pointers(buf, limit is None)
    dev = current_time.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f110_episodes_apply(C.byref(c), n, float(timestep), _lib.ptr(reward), _lib.ptr(done), _lib.ptr(current_time),
                                                   _lib.ptr(laps), 1, _lib.ptr(pending_reset), C.byref(ptrs), _lib.stream(dev)))


class EpisodeTracker(Consumer):
    """The episode tracker of one Engine (f110_episodes_install / _bind / _update).  Its arrays live in `buf`: ep_return [B] fp64,
    ep_length [B] int32, ep_open, truncated [B] uint8, t_seen [B] fp64, limit [B] int32 (the step limit of every env; 0: none), the
    log of L records log_env, log_length, log_laps int32, log_return, log_time fp64, log_reason uint8, and count [1] int64, the
    episodes closed so far: record k of the run lives in slot k % L.  The log is small: unlike the replay ring it is part of
    state_dict()."""
    NAME = 'episodes'
    INFO = {'episode_return': 'ep_return', 'episode_length': 'ep_length', 'truncated': 'truncated', 'episodes_finished': 'count'}
    STATE = {'episode_return': 'ep_return', 'episode_length': 'ep_length', 'episode_open': 'ep_open', 'episode_t_seen': 't_seen',
             'episode_truncated': 'truncated', 'episode_limit': 'limit', 'episode_log_env': 'log_env',
             'episode_log_length': 'log_length', 'episode_log_return': 'log_return', 'episode_log_reason': 'log_reason',
             'episode_log_time': 'log_time', 'episode_log_laps': 'log_laps', 'episodes_finished': 'count'}
    DONE, LIMIT, RESET = DONE, LIMIT, RESET
    cfg = None

    log_size = property(lambda self: self.cfg.log)

    def install(self, max_steps=DEFAULTS['limit'], log=DEFAULTS['log']):
        """`max_steps`: the step limit, one int for every env or an int tensor / array [B] (0: no limit, statistics only); `log`: the
        records the log holds.  An install starts the tracker anew: every env opens a fresh episode, the log is empty.  ValueError
        for a negative limit, a log outside 1..2^24 or a limit array of another shape."""
        eng = self.eng
        per_env = None
        if torch.is_tensor(max_steps) or hasattr(max_steps, '__len__'):
            per_env = torch.as_tensor(max_steps).to(device=eng.device)
            if tuple(per_env.shape) != (eng.B,) or per_env.dtype.is_floating_point or per_env.dtype == torch.bool:
                raise ValueError('max_steps must be one int or an int tensor of shape (%d,)' % eng.B)
            if int(per_env.min()) < 0 or int(per_env.max()) > 2 ** 31 - 1:
                raise ValueError('max_steps: a step limit is negative or beyond int32 (0: no limit)')
        c = make_config(0 if per_env is not None else max_steps, log)
        _lib.check(eng.lib.f110_episodes_install(eng._h, C.byref(c)))
        try:
            with torch.cuda.device(eng.device):
                buf = new_buffers(eng.B, c.log, eng.device)
                if per_env is not None:
                    buf['limit'].copy_(per_env)
                else:
                    buf['limit'].fill_(c.limit)
                self._bind(buf, _lib.EpisodesBuffers)
        except Exception:
            eng.lib.f110_episodes_install(eng._h, None)
            self.on = False
            raise
        self.cfg, self.on = c, True

    def remove(self):
        """No launch, no info key, no state_dict key remains and the arrays are freed."""
        if self.on:
            _lib.check(self.eng.lib.f110_episodes_install(self.eng._h, None))
            torch.cuda.synchronize(self.eng.device)   # an enqueued update may still write the arrays
        self.cfg, self.on, self.buf, self.info = None, False, None, {}

    def restart(self):
        """Every env opens a fresh episode and nothing is logged for the one that ran; the log and the limits stay."""
        b = self.buf
        b['ep_return'].zero_()
        b['ep_length'].zero_()
        b['truncated'].zero_()
        b['ep_open'].fill_(1)
        b['t_seen'].fill_(-1.0)

    def finished(self, last=None):
        """The log's records in the order their episodes closed, oldest first, as a dict of device tensors env, length, laps (int32),
        ret, time (fp64) and reason (uint8: DONE, LIMIT or RESET); `last`: at most that many, the newest.  Records already overwritten
        are gone.  Reading `count` is the only synchronisation."""
        if not self.on:
            raise ValueError('episodes: the tracker is off (track_episodes())')
        count, L = int(self.buf['count'].item()), self.cfg.log
        n = min(count, L) if last is None else min(count, L, max(int(last), 0))
        at = torch.arange(count - n, count, dtype=torch.int64, device=self.eng.device) % L
        b = self.buf
        return {'env': b['log_env'][at], 'length': b['log_length'][at], 'ret': b['log_return'][at], 'reason': b['log_reason'][at],
                'time': b['log_time'][at], 'laps': b['log_laps'][at]}

    def summary(self, last=100):
        """On the host: count (episodes closed in the whole run), and over the newest `last` records still in the log their number
        n, mean_return, mean_length and the share of each reason (done, limit, reset)."""
        rec = self.finished(last)
        n = int(rec['env'].shape[0])
        out = {'count': int(self.buf['count'].item()), 'n': n, 'mean_return': float('nan'), 'mean_length': float('nan')}
        reason = rec['reason'].cpu()
        for code, name in REASONS.items():
            out[name] = float((reason == code).sum().item()) / n if n else 0.0
        if n:
            out['mean_return'] = float(rec['ret'].mean().item())
            out['mean_length'] = float(rec['length'].to(torch.float64).mean().item())
        return out
