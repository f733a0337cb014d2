"""F110VecEnv: B independent F1TENTH envs stepped in lock-step on one MI355X.

Same constructor keywords, observation keys and step order as the reference's
F110Env (gym/f110_gym/envs/f110_env.py:100-157, :261-347), with a leading batch
dimension and torch tensors instead of Python lists.  Nothing is computed here:
reset/step enqueue the HIP kernels of libf110_hip.so on the current stream.
"""
import os

import numpy as np
import torch

from .base_classes import Integrator
from .engine import DEFAULT_PARAMS, Engine
from .maps import BUILTIN_MAPS, DEFAULT_MAP, builtin_map_yaml


def resolve_map_path(map_name):
    """f110_env.py:106-118: 'berlin' / 'skirk' / 'levine' are packaged maps, any other name (an explicit 'vegas'
    included) means '<map>.yaml' relative to the working directory, and only an ABSENT `map` keyword (None
    here) selects the packaged vegas."""
    if map_name is None:
        return builtin_map_yaml(DEFAULT_MAP)
    if map_name in BUILTIN_MAPS:
        return builtin_map_yaml(map_name)
    return map_name + '.yaml'


class F110VecEnv(object):
    def __init__(self, num_envs, map=None, map_ext='.png', params=None, num_agents=2, timestep=0.01,
                 ego_idx=0, integrator=Integrator.RK4, fov=2 * np.pi, seed=12345, device=0, autoreset=True,
                 num_beams=1080, noise_std=0.01, noise_steps=0, keep_f64_scans=False, count_lookups=False,
                 noise_source='device', side_distances='shared', **_ignored):
        """The reference's constructor keywords (f110_env.py:100-157) plus the batch: `params` and `seed` may each be ONE
        value for every env, or a sequence of num_envs values -- env e is then what `F110Env(params=params[e],
        seed=seed[e])` would be (equal values share a slot on the device; more than 64 distinct seeds switch the device noise to
        one generator per env, `noise_source='per_env'`).  The scan angles and beam cosines depend on fov / num_beams alone and are
        built once.  `side_distances` chooses the car outline of each env's iTTC wall test (a function of `width`, `lf`, `lr`):
        'shared' (default) builds ONE table from env 0's params -- what reference envs created in one process share through
        RaceCar's class-level statics (base_classes.py:116-156); 'per_env' gives every env the table of its own params -- what
        num_envs independently constructed envs (one process each) would have, e.g. when vehicle geometry is randomised per
        env.  With a single `params` dict the two are the same."""
        self.num_envs, self.num_agents = int(num_envs), int(num_agents)
        self.map_name, self.map_ext = map, map_ext
        self.map_path = resolve_map_path(map)
        self.params = dict(DEFAULT_PARAMS if params is None else (params if isinstance(params, dict) else params[0]))
        self.timestep, self.ego_idx, self.seed = timestep, ego_idx, seed
        self.eng = Engine(num_envs=num_envs, num_agents=num_agents, params=self.params if params is None or isinstance(params, dict) else params,
                          seed=seed, fov=fov,
                          timestep=timestep, integrator=integrator, ego_idx=ego_idx, num_beams=num_beams,
                          device=device, autoreset=autoreset, noise_std=noise_std, noise_steps=noise_steps,
                          keep_f64_scans=keep_f64_scans, count_lookups=count_lookups, noise_source=noise_source,
                          side_distances=side_distances)
        self.eng.set_map(self.map_path, self.map_ext)
        self.device = self.eng.device
        t = self.eng.t
        st = t['state']
        # observation views (no copies): obs keys of base_classes.py:587-603 + f110_env.py:277-278
        self._obs = {
            'ego_idx': ego_idx,
            'scans': t['scans'],
            'poses_x': st[..., 0], 'poses_y': st[..., 1], 'poses_theta': st[..., 4],
            'linear_vels_x': st[..., 3],
            'linear_vels_y': torch.zeros((self.num_envs, self.num_agents), dtype=torch.float64, device=self.device),
            'ang_vels_z': st[..., 5],
            'collisions': t['collisions'],
            'lap_times': t['lap_times'], 'lap_counts': t['lap_counts'],
        }
        if t['scans_f64'] is not None:
            self._obs['scans_f64'] = t['scans_f64']
        self._reward = torch.full((self.num_envs,), float(timestep), dtype=torch.float64, device=self.device)
        self._g_actions, self._graphs, self._lg = None, [], None   # capture_step / build_step_graph
        # track_progress, shape_rewards, follow_paths, record_replay, track_episodes: the ones that are `on` run, in this order
        self.consumers = (self.eng.tracker, self.eng.shaper, self.eng.follower, self.eng.replay, self.eng.episodes)

    def _result(self):
        t = self.eng.t
        done = t['done']  # bool tensor written by env_kernel (no per-step torch kernels here)
        info = {'checkpoint_done': t['checkpoint_done'], 'collision_idx': t['collision_idx'],
                'current_time': t['current_time'], 'toggles': t['toggles']}
        reward = None
        for c in self.consumers:
            if c.on:
                info.update(c.info)
                if reward is None:
                    reward = c.reward
        return self._obs, self._reward if reward is None else reward, done, info

    def _after_step(self):
        """What follows every step on the same stream: the progress tracker's update, the reward shaper's, the path follower's,
        the replay buffer's push, the episode tracker's."""
        for c in self.consumers:
            if c.on:
                c.update()

    def _as_dev(self, a, last):
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
        a = a.to(device=self.device, dtype=torch.float64)
        if a.dim() == 2 and self.num_envs == 1:
            a = a.unsqueeze(0)
        if tuple(a.shape) != (self.num_envs, self.num_agents, last):
            raise ValueError('expected shape (%d, %d, %d), got %s' % (self.num_envs, self.num_agents, last, tuple(a.shape)))
        return a.contiguous()

    def reset(self, poses, mask=None):
        """poses [B,A,3] (x, y, yaw).  Returns (obs, reward, done, info) like the
        reference's reset (which performs one zero-action step, f110_env.py:335-347).
        mask [B]: reset only those envs (others keep running untouched)."""
        try:
            poses = self._as_dev(poses, 3)
        except ValueError:
            raise ValueError('Number of poses for reset does not match number of agents.')
        self.eng.reset(poses, mask)
        self._after_step()
        return self._result()

    def step(self, actions):
        """actions [B,A,2] = (steer, speed) per car (f110_env.py:261-302)."""
        self.eng.step(self._as_dev(actions, 2))
        self._after_step()
        return self._result()

    # ------------------------------------------------------------------ progress along the raceline
    def track_progress(self, racelines, assign=None):
        """Switches the progress tracker on: `racelines` one [M, >= 2] array (columns 0, 1 = x, y; a planner's [M,3]
        waypoints fit) or a list of K of them with `assign` [num_envs] = the raceline of every env (the form
        raceline_slots takes, e.g. the slots of randomize_tracks with the tracks' centre lines).  From then on reset, step,
        step_graph and step_lib_graph leave the tracker updated for the step they ran, and `info` also holds frenet_s
        (metres along the raceline), frenet_d (lateral offset, left positive), heading_error, progress (metres driven
        since the car's reset), progress_delta (this step's share; combine it into a reward as you like) -- views [B, A],
        no copies -- and lap_length [B].  A reset (masked, whole batch or autoreset) restarts the car's progress at 0 in the
        step that performs it.  None switches tracking off: no launch, no info key, no state_dict key remains."""
        if racelines is None:
            self.eng.tracker.remove()
            return
        if isinstance(racelines, (list, tuple)):
            if assign is None and len(racelines) > 1:
                raise ValueError('a list of racelines needs assign [num_envs]')
            if assign is not None:
                assign = self._raceline_of_env(assign, len(racelines))
        elif assign is not None:
            raise ValueError('assign goes with a list of racelines')
        self.eng.tracker.install(racelines, assign)

    def _raceline_of_env(self, assign, K):
        assign = np.asarray(assign)
        if assign.shape != (self.num_envs,) or assign.min() < 0 or assign.max() >= K:
            raise ValueError('assign must hold one raceline index (0..%d) per env' % (K - 1))
        return assign

    # ------------------------------------------------------------------ reward shaping
    def shape_rewards(self, enable=True, **cfg):
        """Switches the reward shaper on: the reward of the reference's RL consumer (src/SAL.py:219-250, SACF110Env.
        _calculate_rewards) for every env, computed on the GPU from the FILL bitmap of the env's previous scan and its new
        pose.  `cfg`: options of red_gym_amd.shaping.DEFAULTS (rows, cols, agent, neighborhood, clip_max, scale, origin_x,
        origin_y, max_lane_halfwidth, w_collision, w_progress, w_centering; SAL's numbers where absent).  From then on
        reset, step, step_graph and step_lib_graph run the shaper's kernel and then draw the new scan of car `agent` with
        lidar_to_bitmap(scan, output_image_dims=(rows, cols), bg_color='black', draw_mode='FILL') (SAL.py:76-77) into the
        same buffer; the second return value is the total reward [B] instead of the constant time step, and `info` also
        holds reward_collision, reward_progress, reward_centering [B] fp64, bitmap_collided [B] uint8 and lidar_bitmap
        [B, rows, cols] uint8 (the image of the scan just returned: the next step's reward reads it) -- views, no copies.
        A reset (masked, whole batch or autoreset) pays 0 in the step that performs it and restarts from the reset pose.
        shape_rewards(False) switches it off: no launch, no info key, no state_dict key remains and the reward is the
        constant again.  Switched on in the middle of a run, the first update pays no progress and reads the image of the
        scans as they stand.
        image='bits' (default 'bytes') keeps the bitmap as one bit per pixel from the renderer on: reset, step, step_graph and
        step_lib_graph then run the bits forms of the render, the shaper and the replay push, with the same rewards and the same
        ring, and `info` and state_dict() hold lidar_bitmap_bits [B, rows, ceil(cols / 64)] int64 instead of lidar_bitmap -- the
        bits of uint64 words, bit k of word w of a row = (pixel[64 w + k] == 255), bits beyond cols 0: the replay ring's frame
        format, which bitconv.BitConvStem(..., cols=cols) and conv_bits read as they are, and which
        replay.unpack_bitmaps(info['lidar_bitmap_bits'], cols) turns back into the byte image.  load_state_dict takes a
        checkpoint of either form in either mode.  Installing the shaper again in the other form at the same image size
        restarts the shaper and keeps the replay buffer.  The replay buffer records the shaper's image and reward: switching the shaper off, or installing it
        again with another image size, while record_replay() is on removes the replay buffer too (its ring is freed)."""
        if enable:
            self.eng.shaper.install(**cfg)
        else:
            self.eng.shaper.remove()
        rp, sh = self.eng.replay, self.eng.shaper
        if rp.on and (not sh.on or (sh.cfg.rows, sh.cfg.cols) != (rp.rows, rp.cols)):
            rp.remove()

    # ------------------------------------------------------------------ path actions
    def follow_paths(self, enable=True, **cfg):
        """Switches the path follower on: the action side of the reference's RL consumer (src/SAL.py, SACF110Env.step) for
        every env on the GPU.  `cfg`: options of red_gym_amd.pathfollow.DEFAULTS (agent, car_length, vector_length,
        max_diff_deg, dist_threshold, replan_at, desired_velocity, timestep, horizon, q, r, p, max_steer; SAL's numbers where
        absent).  From then on path_actions(raw_actions) turns the policy's [B, 16] numbers into (steer, speed) of car
        `agent`, and reset, step, step_graph and step_lib_graph run the follower's update behind the step: the waypoint index
        follows the new pose (_update_path_index), and an env that was reset (masked, whole batch or autoreset) loses its
        path and decodes a new one at its next path_actions.  `info` also holds path_points [B, 8, 2] fp64, path_index [B]
        int32 (< 0: no path), path_replanned [B] uint8 (the last path_actions decoded a new path) and mpc_accel [B, 2] fp64
        -- views, no copies.  The reference's pending_action (never set) is left out, and where it would raise IndexError
        (its path has 8 points, it replans at index 16) a new path is decoded: replan_at, default 8.
        follow_paths(False) switches it off: no launch, no info key, no state_dict key remains."""
        if enable:
            self.eng.follower.install(**cfg)
        else:
            self.eng.follower.remove()

    def path_actions(self, raw_actions, out=None):
        """The follower's actions [B, A, 2] for the policy's raw_actions [B, 16] (device tensor) at the current poses and
        velocities: one kernel on the current stream, no synchronisation.  With `out` ([B, A, 2] or its [B * A, 2] view)
        only car `agent`'s pairs are written and the others stay as they are; without it a new tensor is returned whose
        other entries are 0.  Usable as the policy of capture_step -- `lambda env, out: env.path_actions(raw, out=out)` with
        `raw` a tensor that is refilled in place -- and in front of step_lib_graph, writing into the static action buffer.
        ValueError while the follower is off."""
        if not self.eng.follower.on:
            raise ValueError('path_actions: the path follower is off (follow_paths())')
        if out is None:
            out = torch.zeros((self.num_envs, self.num_agents, 2), dtype=torch.float64, device=self.device)
        if not torch.is_tensor(raw_actions):
            raw_actions = torch.as_tensor(np.ascontiguousarray(raw_actions, dtype=np.float64))
        if raw_actions.dtype != torch.float64 or raw_actions.device != self.device or not raw_actions.is_contiguous():
            raw_actions = raw_actions.to(device=self.device, dtype=torch.float64).contiguous()
        self.eng.follower.act(raw_actions, out)
        rp = self.eng.replay
        if rp.on and rp.action_dim == raw_actions.shape[1]:
            rp.buf['action_in'].copy_(raw_actions)   # what the next push stores (one capturable copy)
        return out.view(self.num_envs, self.num_agents, 2)

    # ------------------------------------------------------------------ replay buffer
    def record_replay(self, capacity=None, steps=None, action_dim=16, priorities=None):
        """Switches the replay buffer on: the ReplayBuffer of the reference's RL consumer (src/SAL.py:447-463) and the push of
        its training loop (:996-1001) on the GPU.  `capacity` counts transitions as the reference's does: the ring has steps =
        capacity // num_envs step slots for all envs (or give `steps` itself; at least 2).  From then on reset, step, step_graph
        and step_lib_graph push behind the shaper: the transition of env e at step t is (F[t-1, e], a[t, e], r[t, e], F[t, e],
        done[t, e]) with F the shaper's lidar_bitmap as the step left it (stored bit-packed and once: 1/16 of the raw bytes; behind
        shape_rewards(image='bits') the shaper's bits are copied as they are), a =
        replay_action as it stands at the push, r the shaper's total reward.  A transition is invalid and never sampled when
        the step was the env's reset (masked, whole batch or autoreset: terminal frame and spawn frame are no transition),
        when the env was not stepped by the call, or when there is no previous frame (the first push after this call or after
        load_state_dict).  The terminal step itself is valid.  With track_episodes() on, the transition of the step that hit the
        limit is valid and carries d = 0 -- what the reference pushes at st == max_steps - 1 -- and the respawn step behind it is
        invalid, like every reset.  Eviction is FIFO by step, like the reference's deque.  `info`
        also holds replay_count [1] int64 (pushes made) and replay_valid [B] uint8 (the push just made) -- views.  The ring is
        not part of state_dict().  env.replay.sample(batch_size) returns (s, a, r, ns, d, ok) on the device.
        record_replay(None) or record_replay(False) switches it off and frees the ring: no launch, no allocation, no info key
        remains.  ValueError while shape_rewards() is off; switching the shaper off, or installing it again with another image
        size, removes the buffer too.
        priorities: None (the default: uniform draws, nothing more is launched), True or a dict of exponent=0.6, eps=1e-6, beta=0.4,
        beta_end=1.0, beta_updates=100000 -- prioritized replay (red_gym_amd.priority): an exact integer sum tree over the ring on the
        device, exposed as env.replay.priorities.  Every push then gives its transitions the largest priority seen so far,
        env.replay.sample_priority_dev draws in proportion to (|td| + eps)^exponent and returns importance weights for beta, which goes
        from `beta` to `beta_end` in `beta_updates` samples, and env.replay.priorities.update writes new TD errors back."""
        if not capacity and steps is None:
            self.eng.replay.remove()
            return
        if not self.eng.shaper.on:
            raise ValueError('record_replay: the reward shaper is off (shape_rewards())')
        if priorities is not None and priorities is not False:
            from .priority import make_options
            make_options(priorities)            # (refused before the ring is replaced)
        self.eng.replay.install(capacity=None if capacity is True else capacity, steps=steps, action_dim=action_dim)
        self.eng.replay.set_priorities(priorities)

    @property
    def replay(self):
        """The Engine's ReplayBuffer (sample, sample_at, len(), save, load)."""
        return self.eng.replay

    @property
    def replay_action(self):
        """[B, action_dim] fp32: what the next push stores as the action.  path_actions(raw) fills it while the buffer is on
        (when action_dim is raw's width); users of another policy write into it themselves."""
        if not self.eng.replay.on:
            raise ValueError('replay_action: the replay buffer is off (record_replay())')
        return self.eng.replay.buf['action_in']

    # ------------------------------------------------------------------ episodes
    def track_episodes(self, max_steps=2000, log=4096):
        """Switches the episode tracker on: the episode of the reference's training loop (src/SAL.py:986-1015) for every env on the
        GPU.  `max_steps` (the reference's 2000): the step limit, one int or an int tensor [B] -- staggered limits keep envs
        spawned together from ending together; 0: no limit, statistics only.  `log`: the records the log of finished episodes
        holds (1..2^24).  From then on reset, step, step_graph and step_lib_graph run the tracker behind every other consumer: an
        episode's return is the sum of the rewards step() returned (the shaper's total while shape_rewards() is on, else the
        constant time step), added in step order; the reset step pays nothing and counts no step.  An episode closes when the env
        reports done (DONE), when its length reaches the limit (LIMIT), or when a reset of the user's cuts it (RESET).  At a LIMIT
        `truncated` is raised -- `done` is never written -- and, with autoreset=True, the env's pending_reset, so that the next step
        respawns it at its spawn pose exactly as after a done; with autoreset=False the env keeps stepping, its accumulators
        frozen, until the user resets it.  `info` also holds episode_return [B] fp64, episode_length [B] int32, truncated [B] uint8
        and episodes_finished [1] int64 -- views, no copies; env.episodes.finished() returns the log, env.episodes.summary() its
        means.  Switched on in the middle of a run, or restored from a checkpoint without its keys, every env opens a fresh episode
        and nothing is logged for the one that ran.  track_episodes(None) or track_episodes(False) switches it off: no launch, no
        info key, no state_dict key remains."""
        if max_steps is None or max_steps is False:
            self.eng.episodes.remove()
            return
        self.eng.episodes.install(max_steps=max_steps, log=log)

    @property
    def episodes(self):
        """The Engine's EpisodeTracker (finished, summary, DONE / LIMIT / RESET)."""
        return self.eng.episodes

    # ------------------------------------------------------------------ checkpoint / resume
    _STATE_KEYS = ('state', 'steer_buf', 'steer_cnt', 'noise_step', 'spawn', 'start_rot', 'near_start', 'toggles',
                   'current_time', 'pending_reset', 'collisions', 'collision_idx', 'in_collision', 'lap_counts',
                   'lap_times', 'done', 'checkpoint_done', 'scans')

    def state_dict(self):
        """Everything a step depends on lives in the caller-owned tensors bound to the handle
        (f110_buffers): a copy of them is a complete checkpoint of all B envs."""
        sd = {k: self.eng.t[k].clone() for k in self._STATE_KEYS if self.eng.t[k] is not None}
        for c in self.consumers:
            if c.on:
                sd.update(c.state())
        return sd

    def load_state_dict(self, sd):
        """While tracking is on the checkpoint's progress, s_prev and seen are restored with it; one taken without them
        starts every car's progress anew.  Likewise the shaper's prev_xy, t_seen and bitmap while shaping is on; without
        them the shaper restarts: the next update pays no progress and reads the image of the restored scans.  The replay
        buffer's ring is no part of a checkpoint: what it holds stays, and the next push stores a frame and an invalid transition."""
        theirs = {k for c in self.consumers for k in c.state_keys()}
        self.eng.load_state({k: v for k, v in sd.items() if k not in theirs})
        for c in self.consumers:
            if c.on:
                c.on_load_state_dict(sd)

    # ------------------------------------------------------------------ hipGraph replay
    def capture_step(self, policy=None, copies=1):
        """Captures one step (optionally preceded by a device-side policy that fills the
        action buffer, e.g. `lambda env, out: env.eng.pure_pursuit(wp, tlad, vgain, out=out)`)
        into a HIP graph.  f110_step neither allocates nor synchronises, so the three or four
        kernel launches replay from one graph launch; `step_graph()` then costs one host call.
        Returns the static action buffer [B,A,2] to write into when no policy is given (it stays the
        same tensor across re-captures)."""
        self._static_actions()
        self._g_policy = policy
        self.eng.ready_noise()
        # `copies` > 1 captures that many identical graphs, replayed in turn (an experiment: two alternating execs
        # replay no faster than one, profiles/r02_graph_vs_eager.txt)
        if self._graphs:
            # a replay of the graphs being dropped may still be in flight (f110_set_scan_stages bumps the epoch without
            # synchronising): a graph exec must outlive its last launch
            torch.cuda.current_stream(self.device).synchronize()
        self._graphs, self._g_next = [], 0
        for _ in range(max(1, int(copies))):
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            g = torch.cuda.CUDAGraph()
            with self.eng.capturing(), torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
                if policy is not None:
                    policy(self, self._g_actions.view(-1, 2))
                self.eng.step(self._g_actions)
                self._after_step()
            torch.cuda.current_stream(self.device).wait_stream(side)
            self._graphs.append(g)
        self._g_copies = len(self._graphs)
        # a capture freezes the kernel choice and the by-value arguments (noise table address and length, map
        # template flags, env -> map table): it is valid for this launch epoch only
        self._g_epoch = self.eng.launch_epoch()
        return self._g_actions

    def _static_actions(self):
        """The action buffer the replayed steps read: allocated once, shared by both kinds of graph."""
        if self._g_actions is None:
            self._g_actions = torch.zeros((self.num_envs, self.num_agents, 2), dtype=torch.float64, device=self.device)

    def step_graph(self, actions=None):
        """Replays the captured step.  With `actions` they are copied into the static buffer first; cheaper is to
        write into the buffer capture_step returned (or to capture a policy).  If the handle's launch epoch moved
        since the capture (the noise table grew, a map with other template flags was installed, tracks were
        randomised) the step is re-captured first, so a replay never reads a freed table."""
        if actions is not None:
            self._g_actions.copy_(self._as_dev(actions, 2))
        self.eng.ready_noise()
        if self.eng.launch_epoch() != self._g_epoch:
            self.capture_step(self._g_policy, self._g_copies)
        self._graphs[self._g_next].replay()
        self._g_next = (self._g_next + 1) % len(self._graphs)
        self.eng.count_step()
        return self._result()

    # ------------------------------------------------------------------ hipGraph built by the library
    def build_step_graph(self, how='nodes'):
        """The step as a HIP graph built by the library itself (f110_graph_create: 'nodes' = explicit kernel nodes,
        'capture' = a capture on a private non-blocking stream) instead of a torch capture.  Returns the static action
        buffer [B,A,2]; `step_lib_graph()` replays."""
        self._static_actions()
        self._drop_graph()
        self.eng.ready_noise()
        self._lg = self.eng.create_graph(self._g_actions, how)
        self._lg_how, self._lg_epoch = how, self.eng.launch_epoch()
        return self._g_actions

    def _drop_graph(self):
        if self._lg is not None:
            self.eng.destroy_graph(self._lg)
            self._lg = None

    def lib_graph_info(self, dot_path=None):
        return self.eng.graph_info(self._lg, dot_path)

    def step_lib_graph(self, actions=None):
        if actions is not None:
            self._g_actions.copy_(self._as_dev(actions, 2))
        self.eng.ready_noise()
        if self.eng.launch_epoch() != self._lg_epoch:
            self.build_step_graph(self._lg_how)
        self.eng.launch_graph(self._lg)
        self._after_step()               # behind the graph launch, on the same stream
        return self._result()

    def pure_pursuit(self, waypoints, lookahead, vgain, wheelbase=0.17145 + 0.15875, prepare=True):
        """Batched pure-pursuit actions for the current poses (examples/waypoint_follow.py planner
        on the GPU); waypoints [M,3] = (x, y, speed).  A device tensor that is planned on repeatedly is prepared once
        (Engine.pure_pursuit) and then costs one lane per car.  A NumPy array (or a tensor on another device) is copied
        to the device on every call and never prepared: its in-place edits could not be detected."""
        if not torch.is_tensor(waypoints) or waypoints.device != self.device:
            waypoints = torch.as_tensor(np.ascontiguousarray(waypoints, dtype=np.float64), device=self.device)
            prepare = False
        return self.eng.pure_pursuit(waypoints, lookahead, vgain, wheelbase, prepare=prepare)

    def raceline_slots(self, waypoint_sets, assign):
        """Packs K racelines [M_k,3] = (x, y, speed) and the raceline of every env (int array [num_envs], e.g. the map
        slots of randomize_tracks) for pure_pursuit_tracks: the planner's counterpart of f110_assign_maps.  Returns
        (TrackSet, int32 device tensor [num_envs * num_agents])."""
        from .engine import TrackSet
        assign = self._raceline_of_env(assign, len(waypoint_sets))
        ts = TrackSet(waypoint_sets, self.device)
        of_car = torch.as_tensor(np.repeat(assign.astype(np.int32), self.num_agents), device=self.device)
        return ts, of_car

    def pure_pursuit_tracks(self, tracks, track_of_car, lookahead, vgain, wheelbase=0.17145 + 0.15875):
        """Pure-pursuit actions [B,A,2] when every env has its own raceline (raceline_slots): ONE planner launch for
        all tracks, racelines of any length, capturable in a hipGraph together with the step."""
        return self.eng.pure_pursuit_tracks(tracks, track_of_car, lookahead, vgain, wheelbase)

    def pure_pursuit_blocks(self, waypoint_sets, assign, lookahead, vgain, wheelbase=0.17145 + 0.15875):
        """Pure-pursuit actions when blocks of envs drive on different tracks (randomize_tracks): waypoint_sets[k]
        is the raceline [M_k,3] = (x, y, speed) of slot k, assign the int array [num_envs] of slots.  One planner
        launch for all of them (the packed racelines are cached while the same objects are passed)."""
        # (the packed form is rebuilt unless the very same raceline objects -- held here, so that their ids cannot be
        # handed to new ones -- and the same assignment are passed; a raceline edited IN PLACE is not noticed -- build a
        # new TrackSet with raceline_slots for that)
        lines, assign_bytes = list(waypoint_sets), np.asarray(assign).tobytes()
        src = getattr(self, '_pp_tracks_src', None)
        if src is None or src[1] != assign_bytes or len(src[0]) != len(lines) or any(a is not b for a, b in zip(src[0], lines)):
            self._pp_tracks = self.raceline_slots(lines, assign)
            self._pp_tracks_src = (lines, assign_bytes)
        ts, of_car = self._pp_tracks
        return self.eng.pure_pursuit_tracks(ts, of_car, lookahead, vgain, wheelbase)

    def update_params(self, params, index=-1):
        """base_classes.py:507-527: index < 0 updates every agent, otherwise agent `index` of
        every env; IndexError beyond the agent list."""
        self.eng.update_params(params, index)
        if index < 0:
            self.params = dict(params)

    def update_map(self, map_path, map_ext):
        self.eng.set_map(map_path, map_ext)

    def update_map_occupancy(self, free, resolution, orig_x, orig_y, orig_theta=0.0):
        """Installs a map given as an occupancy mask (NumPy array or CUDA uint8 tensor, nonzero = free, row 0 at the
        bottom); with a device tensor nothing but two scalars leaves the GPU."""
        self.eng.set_map_occupancy(free, resolution, orig_x, orig_y, orig_theta)

    def randomize_track(self, seed):
        """Domain randomisation: draws a random closed track (red_gym_amd.trackgen, the reference's
        unittest/random_trackgen.py) on the GPU, installs it as the map of every env of this shard and returns the
        Track (centre-line waypoints [N,3] = x, y, heading in world metres; waypoint 0 is the world origin)."""
        from . import trackgen
        t = trackgen.generate(seed, device=self.device)
        self.eng.set_map_occupancy(t.free, t.resolution, t.orig_x, t.orig_y, 0.0)
        return t

    def randomize_tracks(self, seeds):
        """One random track per seed, installed in map slots 0..K-1, with the envs split into K equal blocks (env e
        drives on track e*K // num_envs) -- what K separate reference envs with their own `map` would be.  Returns
        the Tracks and the int array [num_envs] of slots."""
        from . import trackgen
        seeds = list(seeds)
        tracks = []
        for k, seed in enumerate(seeds):
            t = trackgen.generate(seed, device=self.device)
            self.eng.set_map_occupancy(t.free, t.resolution, t.orig_x, t.orig_y, 0.0, slot=k)
            tracks.append(t)
        assign = (np.arange(self.num_envs) * len(seeds)) // self.num_envs
        self.eng.assign_maps(assign)
        return tracks, assign

    @property
    def state(self):
        return self.eng.t['state']

    def close(self):
        self._drop_graph()
        self.eng.close()
