"""A pure-Python mirror of the episode tracker's rules (include/f110_hip.h, "Episodes"; csrc/f110_episodes.h), what the CPU and
the GPU tests of the tracker share: EpisodeChecker is fed what step() returned -- reward, done and clock per env -- and holds the
accumulators, the flags, the log and the counter; reference_loop is the reference's training loop (src/SAL.py:986-1015) written
down literally for one env."""
import numpy as np

DONE, LIMIT, RESET = 1, 2, 3
STATE = ('ep_return', 'ep_length', 'ep_open', 't_seen', 'truncated')
LOG = ('log_env', 'log_length', 'log_return', 'log_reason', 'log_time', 'log_laps')
DTYPES = {'ep_return': np.float64, 'ep_length': np.int32, 'ep_open': np.uint8, 't_seen': np.float64, 'truncated': np.uint8,
          'limit': np.int32, 'log_env': np.int32, 'log_length': np.int32, 'log_return': np.float64, 'log_reason': np.uint8,
          'log_time': np.float64, 'log_laps': np.int32}


class EpisodeChecker(object):
    """B envs, the clock's `timestep`, `limit` (one int or [B]; 0: none), a log of L records, and whether the engine runs with
    autoreset (then a LIMIT raises pending_reset).  order: the order in which the envs that close in one update take their slots
    (None: ascending env, the contract; a permutation of range(B) to show that another order is told apart)."""

    def __init__(self, B, timestep, limit, L, autoreset, order=None):
        self.B, self.timestep, self.L, self.autoreset = int(B), float(timestep), int(L), bool(autoreset)
        self.limit = np.broadcast_to(np.asarray(limit, np.int32), (B,)).copy()
        self.ep_return = np.zeros(B, np.float64)
        self.ep_length = np.zeros(B, np.int32)
        self.ep_open = np.ones(B, np.uint8)
        self.t_seen = np.full(B, -1.0)
        self.truncated = np.zeros(B, np.uint8)
        self.log_env = np.zeros(L, np.int32)
        self.log_length = np.zeros(L, np.int32)
        self.log_return = np.zeros(L, np.float64)
        self.log_reason = np.zeros(L, np.uint8)
        self.log_time = np.zeros(L, np.float64)
        self.log_laps = np.zeros(L, np.int32)
        self.count = 0
        self.records = []               # every record of the run, in closing order: (env, length, return, reason, time, laps)
        self.order = list(range(B)) if order is None else list(order)

    def restart(self):
        self.ep_return[:] = 0.0
        self.ep_length[:] = 0
        self.ep_open[:] = 1
        self.t_seen[:] = -1.0
        self.truncated[:] = 0

    def update(self, reward, done, clock, laps=None, pending_reset=None):
        """One update behind a step.  reward: [B] or None (the constant timestep); pending_reset: the [B] uint8 array of the
        engine's flags, raised in place at a LIMIT while autoreset is on (None: not kept).  Returns the envs closed, in slot order."""
        closing = {}
        for e in range(self.B):
            now = float(clock[e])
            if now == self.t_seen[e]:
                continue                                   # rule 2: not stepped
            if now == self.timestep:                       # rule 1: the env's reset
                if self.ep_open[e] and self.ep_length[e] > 0:
                    closing[e] = (RESET, int(self.ep_length[e]), float(self.ep_return[e]))
                self.ep_return[e], self.ep_length[e], self.ep_open[e], self.truncated[e] = 0.0, 0, 1, 0
            elif self.ep_open[e]:                          # rule 3: a step of an open episode
                r = self.timestep if reward is None else float(reward[e])
                self.ep_return[e] = self.ep_return[e] + r
                self.ep_length[e] += 1
                reason = 0
                if done[e]:
                    reason = DONE
                elif self.limit[e] > 0 and self.ep_length[e] >= self.limit[e]:
                    reason = LIMIT
                    self.truncated[e] = 1
                    if self.autoreset and pending_reset is not None:
                        pending_reset[e] = 1
                if reason:
                    self.ep_open[e] = 0
                    closing[e] = (reason, int(self.ep_length[e]), float(self.ep_return[e]))
            self.t_seen[e] = now                           # (rule 4: a step of a closed episode changes nothing else)
        envs = [e for e in self.order if e in closing]
        total = len(envs)
        for g, e in enumerate(envs):
            reason, length, ret = closing[e]
            rec = (e, length, ret, reason, float(clock[e]), 0 if laps is None else int(laps[e]))
            self.records.append(rec)
            if g >= total - self.L:                        # of more than L only the last L are written
                s = (self.count + g) % self.L
                (self.log_env[s], self.log_length[s], self.log_return[s], self.log_reason[s], self.log_time[s],
                 self.log_laps[s]) = rec
        self.count += total
        return envs

    def arrays(self):
        out = {k: getattr(self, k) for k in STATE + LOG}
        out['limit'] = self.limit
        out['count'] = np.array([self.count], np.int64)
        return out

    def finished(self, last=None):
        """The records still in the log, oldest first: what EpisodeTracker.finished returns."""
        n = min(self.count, self.L) if last is None else min(self.count, self.L, last)
        at = np.arange(self.count - n, self.count) % self.L
        return {'env': self.log_env[at], 'length': self.log_length[at], 'ret': self.log_return[at], 'reason': self.log_reason[at],
                'time': self.log_time[at], 'laps': self.log_laps[at]}


def reference_loop(rewards, dones, max_steps):
    """src/SAL.py:986-1015 for one env whose step k would return (rewards[k], dones[k]): episodes until the script runs out.
    Returns [(ep_reward, steps, reason)]; the last, unfinished episode is not reported (the reference prints at the break)."""
    out, k = [], 0
    while k < len(rewards):
        ep_reward = 0                                      # obs = env.reset(); ep_reward = 0
        steps, ended = 0, None
        for st in range(max_steps):
            if k >= len(rewards):
                break
            reward, done = rewards[k], dones[k]
            k += 1
            ep_reward += reward
            steps = st + 1
            if done:
                ended = DONE
                break
        else:
            ended = LIMIT
        if ended is None:
            break
        out.append((ep_reward, steps, ended))
    return out
