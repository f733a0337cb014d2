"""The composed checker of the env with all five consumers on -- what F110VecEnv._after_step enqueues behind every step: the
progress tracker's update, the reward shaper's (its kernel, then the FILL render into the one shared image), the path follower's,
the replay ring's push, the episode tracker's.  LoopChecker owns one instance of each consumer's own checker (progress_cases,
shaping_cases, path_cases, replay_cases, episodes_cases) and writes no arithmetic of its own: it only says who reads whose output,
and in which order.  Like the device it keeps the values the consumers hand each other in buffers -- the image, the shaper's total,
the action the next push stores -- so that another order reads another value.  The keywords order, render_first and late restate
mistakes of the composition (tests/test_trainer_cpu.py shows that each one is told apart); the GPU tests use the defaults."""
import numpy as np

import episodes_cases as ec
import path_cases as pc
import progress_cases as gc
import replay_cases as rc
import shaping_cases as sc

ORDER = ('progress', 'shaping', 'follow', 'replay', 'episodes')       # F110VecEnv.consumers
STEP_INFO = ('checkpoint_done', 'collision_idx', 'current_time', 'toggles')
IMAGE_KEYS = ('lidar_bitmap', 'lidar_bitmap_bits')                     # bytes, bits


def fill_render(rows, cols):
    """scans [B, beams] -> the FILL images [B, rows, cols] the shaper draws (src/SAL.py:76-77), by the CPU oracle."""
    from oracle import bitmap as ob

    def render(scans):
        return ob.lidar_to_bitmap(np.asarray(scans, np.float64), output_image_dims=(rows, cols), bg_color='black', draw_mode='FILL')
    return render


class LoopChecker(object):
    """B envs of A cars; shaper, follower and ring follow car `agent`.  raceline: [M, >= 2]; rows, cols: the shaper's image; steps,
    action_dim: the ring; limits (one int or [B]) and log: the episode tracker; shaping / follow: the other options of the two
    configs; bits: the image's key and form in `info` (the words of replay_cases.pack); render: scans [B, ...] -> images [B, rows,
    cols] (None: fill_render).
    order: the consumers in the order they run; render_first: the shaper's image is drawn before its kernel reads it; late: the
    name of one consumer that is shown the clock (the tracker: the reset flags) of the step before."""

    def __init__(self, B, A, agent, timestep, raceline, rows, cols, steps, action_dim=16, limits=0, log=4096, autoreset=True,
                 shaping=None, follow=None, bits=False, render=None, order=ORDER, render_first=False, late=None):
        assert sorted(order) == sorted(ORDER) and late in (None,) + ORDER and 0 <= agent < A
        self.B, self.A, self.agent, self.timestep, self.bits = B, A, agent, float(timestep), bool(bits)
        self.order, self.render_first, self.late = tuple(order), bool(render_first), late
        self.render = fill_render(rows, cols) if render is None else render
        self.frenet = gc.FrenetChecker(raceline)
        self.progress = gc.ProgressChecker([self.frenet], np.zeros(B * A, dtype=int))
        self.shaper = sc.ShapingChecker(B, timestep, sc.config(rows=rows, cols=cols, agent=agent, **(shaping or {})))
        self.follower = pc.FollowChecker(B, timestep, agent=agent, **(follow or {}))
        self.mirror = rc.Mirror(steps, B, rows, cols, action_dim, timestep)
        self.episodes = ec.EpisodeChecker(B, timestep, limits, log, autoreset)
        # what the consumers hand each other
        self.image = np.zeros((B, rows, cols), np.uint8)              # the shaper's bitmap: read by its kernel, then drawn anew
        self.total = np.zeros(B)                                      # the shaper's total: the ring's r, the tracker's reward
        self.action_in = np.zeros((B, action_dim), np.float32)        # replay_action: what the next push stores
        self.pending_reset = np.zeros(B, np.uint8)                    # the engine's flags as the last update left them
        self.accel, self.replanned = np.zeros((B, 2)), np.zeros(B, np.uint8)
        self.pose, self.vx = np.zeros((B, 3)), np.zeros(B)            # car `agent` as the last step left it: what act() reads
        self.valid = np.zeros(B, np.uint8)
        self.out = {}
        self.clock_seen, self.flags_seen = np.zeros(B), np.zeros(B * A, dtype=bool)

    # ------------------------------------------------------------------ in front of the step
    def act(self, raw, poses=None, vx=None):
        """FollowChecker.act at the poses and velocities given (None: car `agent`'s as the last after_step saw them); the raw
        action becomes what the next push stores, as path_actions hands it to the ring."""
        raw = np.asarray(raw, np.float64)
        actions, self.accel, self.replanned = self.follower.act(raw, self.pose if poses is None else poses, self.vx if vx is None else vx)
        if raw.shape[1] == self.action_in.shape[1]:
            self.action_in = raw.astype(np.float32)
        return actions, self.accel, self.replanned

    # ------------------------------------------------------------------ behind the step
    def after_step(self, state, clock, done, laps, pending, scans, mask=None):
        """What the step itself left: state [B, A, 7], current_time [B], done [B], the ego's lap counts [B], pending_reset [B] as
        read BEFORE the step (the envs the step respawned), mask [B] of a masked reset (None: a step; all ones for a reset of
        every env) and the scans [B, A, ...].  Runs the five updates in `order` and returns (info, reward): the expected value of
        every key the consumers add to `info`, and the reward step() returns.  pending_reset holds the flags expected afterwards."""
        state, clock = np.asarray(state, np.float64), np.asarray(clock, np.float64)
        flags = np.asarray(pending).astype(bool) | (np.zeros(self.B, bool) if mask is None else np.asarray(mask).astype(bool))
        s = dict(state=state, clock=clock, done=np.asarray(done).astype(bool), laps=np.asarray(laps), scans=np.asarray(scans),
                 flags=np.repeat(flags, self.A))
        self.pose, self.vx = state[:, self.agent][:, [0, 1, 4]].copy(), state[:, self.agent, 3].copy()
        self.pending_reset = s['done'].astype(np.uint8) if self.episodes.autoreset else np.zeros(self.B, np.uint8)
        for name in self.order:
            late = name == self.late
            getattr(self, '_' + name)(s, self.clock_seen if late else clock, self.flags_seen if late else s['flags'])
        self.clock_seen, self.flags_seen = clock.copy(), s['flags'].copy()
        info = {}
        for name in ORDER:
            info.update(self.out[name])
        return info, self.total.copy()

    def _progress(self, s, clock, flags):
        o = self.progress.update(s['state'].reshape(-1, 7)[:, [0, 1, 4]], flags)
        shape = (self.B, self.A)
        self.out['progress'] = {'frenet_s': o['s'].reshape(shape), 'frenet_d': o['d'].reshape(shape),
                                'heading_error': o['heading_error'].reshape(shape), 'progress': o['progress'].reshape(shape),
                                'progress_delta': o['delta'].reshape(shape), 'lap_length': np.full(self.B, self.frenet.L)}

    def _shaping(self, s, clock, flags):
        if self.render_first:
            self.image = self.render(s['scans'][:, self.agent])
        o = self.shaper.update(self.image, s['state'][:, self.agent, :2], clock)      # the image of the PREVIOUS scan
        self.total = o['total']
        self.image = self.render(s['scans'][:, self.agent])
        self.out['shaping'] = {'reward_collision': o['collision_term'], 'reward_progress': o['progress_term'],
                               'reward_centering': o['centering_term'], 'bitmap_collided': o['collided'],
                               IMAGE_KEYS[self.bits]: rc.pack(self.image) if self.bits else self.image.copy()}

    def _follow(self, s, clock, flags):
        self.follower.update(s['state'][:, self.agent, :2], clock)
        self.out['follow'] = {'path_points': self.follower.paths.copy(), 'path_index': self.follower.index.copy(),
                              'path_replanned': self.replanned.copy(), 'mpc_accel': self.accel.copy()}

    def _replay(self, s, clock, flags):
        self.valid = self.mirror.push(self.image, self.action_in, self.total, s['done'], clock)
        self.out['replay'] = {'replay_count': np.array([self.mirror.count], np.int64), 'replay_valid': self.valid.copy()}

    def _episodes(self, s, clock, flags):
        e = self.episodes
        e.update(self.total, s['done'], clock, s['laps'], self.pending_reset)
        self.out['episodes'] = {'episode_return': e.ep_return.copy(), 'episode_length': e.ep_length.copy(),
                                'truncated': e.truncated.copy(), 'episodes_finished': np.array([e.count], np.int64)}

    # ------------------------------------------------------------------ the ring as read back
    def newest_slot(self):
        """(step slot, frame slot) of the push just made (csrc/f110_replay.h: push c writes step slot c % T, frame slot c % (T + 1))."""
        c = self.mirror.count - 1
        return c % self.mirror.T, c % (self.mirror.T + 1)
