"""The reference's SACAgent (src/SAL.py:468-580) on the GPU: its five networks on the library's modules (featconv.Trunk from the
ring's bits, dense.Dense, policyhead.PolicyHead, qhead.QHead with dense=True), three optim.SacAdam and one update that samples on the
device (ReplayBuffer.sample_frames_dev with the agent's own draw counter), takes both losses from csrc/f110_sacloss.h and never calls
.item().  Every kernel in it adds in a fixed order, so an update repeats bit for bit and the whole of it -- sample, forward, losses,
backward, the three optimizer steps with the soft update of the targets -- is captured once in a torch.cuda.graph and replayed:
K replays equal K eager updates.
The order is that of examples/sac_update.py: the critics' losses are handed to ONE backward pass (their parameters are disjoint, so
each critic gets the gradient the reference's two passes give it), and a target critic moves in the step of its critic, in front of the
actor's loss where the reference moves it behind: that loss reads the critics, never the targets.  As in the reference the actor's
backward leaves gradients in the critics, which the critics' next zero_grad drops.
There is no CPU path and no torch fallback: the kernels of libf110_hip.so do the work."""
import torch

from .dense import Dense
from .featconv import Trunk
from .gauss import GaussianSource
from .optim import SacAdam
from .policyhead import PolicyHead, sample_actions
from .qhead import QHead, td_target, twin_q
from .replay import MAX_NSTEP, MAX_STACK
from .sacloss import actor_loss, critic_loss
from .temperature import Temperature

NETS = ('actor', 'critic1', 'critic2', 'critic1_target', 'critic2_target')      # the reference's order of construction (:486-495)
OPTIMIZERS = ('actor', 'critic1', 'critic2')


def feature_width(rows, cols):
    """Values behind conv1(8, 4), conv2(4, 2), conv3(3, 1) without padding, 32 channels."""
    for k, s in ((8, 4), (4, 2), (3, 1)):
        rows, cols = (rows - k) // s + 1, (cols - k) // s + 1
    if rows < 1 or cols < 1:
        raise ValueError('SACAgent: an image of this size leaves no output behind conv3')
    return 32 * rows * cols


def _key(name):
    """A module's parameter name -> the reference's key."""
    return name.replace('trunk.', '').replace('head.', '')


class Actor(torch.nn.Module):
    """The reference's Actor (src/SAL.py:390-421): trunk, fc1 + ReLU, fc_mean / fc_log_std and the sampling tail."""

    def __init__(self, trunk, fc1, head):
        super().__init__()
        self.trunk, self.fc1, self.head = trunk, fc1, head

    @classmethod
    def new(cls, width, hidden, action_dim, on, cols, device, stack=1):
        return cls(Trunk(on=on, cols=cols, device=device, stack=stack), Dense(width, hidden, relu=True, device=device),
                   PolicyHead(hidden, action_dim, device=device))

    @classmethod
    def sharing(cls, m, on, cols, stack=1):
        """On the tensors of a torch.nn network with the reference's attributes conv1 .. conv3, fc1, fc_mean, fc_log_std."""
        return cls(Trunk.from_convs(m.conv1, m.conv2, m.conv3, on=on, cols=cols, stack=stack), Dense.from_linear(m.fc1, relu=True),
                   PolicyHead.from_linears(m.fc_mean, m.fc_log_std))

    def features(self, frames, index=None):
        return self.fc1(self.trunk(frames, index))

    def sample(self, frames, index=None, eps=None):
        action, log_prob, _, _ = self.head.sample(self.features(frames, index), eps=eps)
        return action, log_prob


class Critic(torch.nn.Module):
    """The reference's Critic (src/SAL.py:424-442): trunk, and fc1 + ReLU + fc2 on cat([features, action]) by qhead.twin_q."""

    def __init__(self, trunk, head):
        super().__init__()
        self.trunk, self.head = trunk, head

    @classmethod
    def new(cls, width, hidden, action_dim, on, cols, device, stack=1):
        return cls(Trunk(on=on, cols=cols, device=device, stack=stack), QHead(width, action_dim, hidden, device=device, dense=True))

    @classmethod
    def sharing(cls, m, on, cols, stack=1):
        return cls(Trunk.from_convs(m.conv1, m.conv2, m.conv3, on=on, cols=cols, stack=stack), QHead.from_linears(m.fc1, m.fc2, dense=True))


def _heads(nets):
    return [c.head.fc1 for c in nets], [c.head.fc2 for c in nets]


class SACAgent:
    """SACAgent(action_dim, gamma, tau, alpha, actor_lr, critic_lr) with the reference's defaults, for images of rows x cols pixels
    and fc1 layers `hidden` wide; on: what a set pixel is worth (255.0: update() feeds the raw 0 / 255 images, :536; select_action
    here sees the same scale, where the reference divides by 255 for acting only).  networks: a dict (or an object with these
    attributes) of five torch.nn networks 'actor', 'critic1', 'critic2', 'critic1_target', 'critic2_target' with the reference's layers
    (conv1 .. conv3, fc1, fc_mean / fc_log_std or fc2) whose tensors the agent then shares: training the agent trains them.  Without it
    the agent builds its own, in the reference's order, the targets loaded from the critics.
    alpha: the reference's fixed temperature (0.2), or 'auto': the temperature is learnt (red_gym_amd.temperature.Temperature, from
    init_alpha towards target_entropy, None: -action_dim, with Adam at alpha_lr) and lives on the device -- `temperature` is that object
    and `alpha` its [1] fp64 tensor, which the target and the actor's loss of update k read before the temperature's step of update k
    makes the next one; the step is captured with the rest.  With a number nothing of this exists (temperature is None).
    draws: where the Gaussian draws of Actor.sample come from when no eps is passed.  'torch': torch.randn, as before.  'device':
    red_gym_amd.gauss.GaussianSource(seed) -- `source` is that object -- whose stream 0 serves select_action (row = the env: `index`
    where one is given, so an env's noise is the same alone and in the batch), stream 1 an update's next_action and stream 2 its
    new_action (row = the batch row); each call that draws advances its stream's counter on the device, the fills and their advances
    are captured with the update, and state_dict() holds the seed and the counters, so a loaded agent continues to the same bits.  An
    eps that is passed wins and advances nothing, and so does evaluate=True.  With 'torch' nothing of this exists (source is None).
    nstep: 1 is the reference's one-step target.  k > 1 (up to replay.MAX_NSTEP): the updates that draw from a ring -- update,
    capture_update, update_graph -- draw with the n-step walk (ReplayBuffer.sample_frames_dev(nstep=k, gamma=gamma)) and the target is
    tv = R + (1 - d) * gamma^m * (min Q'(s_m, a') - alpha * logp'), R = r_0 + gamma r_1 + ... + gamma^(m - 1) r_(m - 1) over a span of m
    <= k stored steps that ends behind a terminal step, in front of a reset and at the newest push; the discount arrives per row.  This
    is the UNCORRECTED n-step return: no importance weights for the off-policy steps inside the span and no entropy bonus on the
    intermediate steps -- the entropy term enters through the bootstrap only, as in the common implementations.  nstep is
    configuration, not state: state_dict() does not hold it.  With nstep = 1 nothing changes: the same launches, graph key and bits.
    per: True -- prioritized replay (Schaul et al.) on a ring with record_replay(..., priorities=...): update, capture_update and
    update_graph draw with ReplayBuffer.sample_priority_dev (which composes with nstep), the critics' loss takes the batch's importance
    weights (sacloss.critic_loss(weight=...)) and the priorities of the drawn transitions are written back right behind it from max(|q1
    - tv|, |q2 - tv|) (PriorityTree.update), all captured with the rest; the actor's loss stays unweighted.  ValueError from those three
    on a ring without priorities.  False, the default, changes nothing: the same launches, graph key and bits, on any ring.
    stack: 1 is the reference's one frame.  k > 1 (up to replay.MAX_STACK): every network's conv1 has k input channels, the last k
    frames of the env (ReplayBuffer.stack_rows: repeated at an episode's start, never across a reset); update, capture_update and
    update_graph draw with stack=k and read the batch's 's_stack' / 'ns_stack', update_batch takes those (or 's_idx' / 'ns_idx' as
    [n, k]), and act_from acts on the ring's newest stacks.
    Shared networks must have a conv1 of k input channels (ValueError otherwise).  stack is configuration, not state.  With stack = 1
    nothing changes: the same launches, graph key and bits.
    max_grad_norm: None, or a positive number or float('inf') that every one of the three SacAdam takes as its max_grad_norm: each
    optimizer clips the global L2 norm of ITS network's gradients on the device, as torch.nn.utils.clip_grad_norm_(net.parameters(),
    max_grad_norm) per network would, and skips its step when that norm is inf or NaN (parameters, moments and step counter keep
    their bits; a critic's target still moves).  float('inf') is the guard alone.  .grad is not rewritten.  The three clip states are
    the rows (actor, critic1, critic2) of ONE [3, 8] int64 tensor `clip_states`; grad_stats() returns views of it, nothing
    synchronises, and a replayed graph leaves fresh values there.  The Temperature's one-parameter step is NOT clipped or guarded.
    max_grad_norm is configuration, not state: state_dict() does not hold it, nor the counters.  It may be changed (not switched on
    or off) after construction; a captured update is then captured again.  With None nothing changes: the same launches, graph key
    and bits.
    Attributes: actor, critics [2], targets [2]; actor_opt, critic_opts [2] (SacAdam; a critic's also moves its target); draws, the [1]
    int64 draw counter on the device; sample, the tensors of the batch the last update drew (sample['indices'] names the transitions)."""

    def __init__(self, action_dim=16, gamma=0.99, tau=0.005, alpha=0.2, actor_lr=3e-4, critic_lr=3e-4, rows=256, cols=256, hidden=512,
                 on=255.0, device='cuda', networks=None, target_entropy=None, alpha_lr=3e-4, init_alpha=0.2, draws='torch', seed=0, nstep=1,
                 per=False, stack=1, max_grad_norm=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('SACAgent: device %s: there is no CPU path' % (self.device,))
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.action_dim, self.gamma, self.tau = int(action_dim), float(gamma), float(tau)
        if isinstance(nstep, bool) or not isinstance(nstep, int) or not 1 <= nstep <= MAX_NSTEP:
            raise ValueError('SACAgent: nstep %r: an int in 1..%d' % (nstep, MAX_NSTEP))
        self.nstep = nstep
        self.per = bool(per)
        if isinstance(stack, bool) or not isinstance(stack, int) or not 1 <= stack <= MAX_STACK:
            raise ValueError('SACAgent: stack %r: an int in 1..%d' % (stack, MAX_STACK))
        self.stack = stack
        self.temperature = None
        if isinstance(alpha, str):
            if alpha != 'auto':
                raise ValueError('SACAgent: alpha %r: a number, or \'auto\' for a learnt temperature' % (alpha,))
            self.temperature = Temperature(init_alpha=init_alpha, target_entropy=-float(self.action_dim) if target_entropy is None else target_entropy,
                                           lr=alpha_lr, device=self.device)
            self.alpha = self.temperature.alpha
        else:
            self.alpha = float(alpha)
        if draws not in ('torch', 'device'):
            raise ValueError('SACAgent: draws %r: \'torch\' or \'device\'' % (draws,))
        self.source = GaussianSource(seed, self.device) if draws == 'device' else None
        self.rows, self.cols, self.hidden, self.on = int(rows), int(cols), int(hidden), float(on)
        self.width = feature_width(self.rows, self.cols)
        if networks is None:
            make = lambda cls: cls.new(self.width, self.hidden, self.action_dim, self.on, self.cols, self.device, self.stack)  # noqa: E731
            self.actor = make(Actor)
            self.critics = [make(Critic), make(Critic)]
            self.targets = [make(Critic), make(Critic)]
            for t, c in zip(self.targets, self.critics):
                t.load_state_dict(c.state_dict())
        else:
            get = networks.__getitem__ if isinstance(networks, dict) else lambda name: getattr(networks, name)  # noqa: E731
            self.actor = Actor.sharing(get('actor'), self.on, self.cols, self.stack)
            self.critics = [Critic.sharing(get(n), self.on, self.cols, self.stack) for n in ('critic1', 'critic2')]
            self.targets = [Critic.sharing(get(n), self.on, self.cols, self.stack) for n in ('critic1_target', 'critic2_target')]
        fc1 = self.actor.fc1.weight
        if tuple(fc1.shape) != (self.hidden, self.width) or self.actor.head.fc_mean.out_features != self.action_dim:
            raise ValueError('SACAgent: the actor\'s fc1 is %s and its action has %d values; rows, cols, hidden and action_dim say %s and %d'
                             % (tuple(fc1.shape), self.actor.head.fc_mean.out_features, (self.hidden, self.width), self.action_dim))
        for p in self.modules()['actor'].parameters():
            if p.device != self.device:
                raise ValueError('SACAgent: the networks are on %s, not on %s' % (p.device, self.device))
        self.clip_states = None
        clip = [{}, {}, {}]
        if max_grad_norm is not None:
            self.clip_states = torch.zeros((len(OPTIMIZERS), 8), dtype=torch.int64, device=self.device)       # f110_adam_clip_state each
            clip = [dict(max_grad_norm=max_grad_norm, clip_state=row) for row in self.clip_states]
        self.actor_opt = SacAdam(self.actor, lr=actor_lr, **clip[0])
        self.critic_opts = [SacAdam(c, lr=critic_lr, targets=t, tau=self.tau, **kw) for c, t, kw in zip(self.critics, self.targets, clip[1:])]
        self.draws = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.sample = None
        # the captured update
        self._g_losses = torch.zeros((3,), dtype=torch.float32, device=self.device)
        self._g_key, self._g_replay, self._g_sample, self._g_eps, self._graphs = None, None, None, None, {}
        self.captures, self.recaptured = 0, False

    # ---- the parts
    def modules(self):
        return dict(actor=self.actor, critic1=self.critics[0], critic2=self.critics[1], critic1_target=self.targets[0], critic2_target=self.targets[1])

    def optimizers(self):
        return dict(actor=self.actor_opt, critic1=self.critic_opts[0], critic2=self.critic_opts[1])

    def zero_grad(self, set_to_none=True):
        for opt in self.optimizers().values():
            opt.zero_grad(set_to_none)

    @property
    def max_grad_norm(self):
        return self.actor_opt.max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        for opt in self.optimizers().values():
            opt.max_grad_norm = value

    def grad_stats(self):
        """The last update's clipping per network (rows: actor, critic1, critic2) as views of `clip_states`, on the device, without a
        synchronisation: 'sumsq' and 'norm' [3] fp64 (inf on a skipped step), 'coef' [3] fp32, 'skip' [3] int32, 'steps_clipped' and
        'steps_skipped' [3] int64.  ValueError without max_grad_norm."""
        if self.clip_states is None:
            raise ValueError('SACAgent: the agent was built without max_grad_norm')
        s = self.clip_states
        f64, f32, i32 = s.view(torch.float64), s.view(torch.float32), s.view(torch.int32)
        return dict(sumsq=f64[:, 0], norm=f64[:, 1], coef=f32[:, 4], skip=i32[:, 5], steps_clipped=s[:, 3], steps_skipped=s[:, 4])

    # ---- acting
    def select_action(self, frames, index=None, evaluate=False, out=None, eps=None):
        """select_action (src/SAL.py:499-519) for a batch of envs under no_grad -> the fp64 [n, action_dim] action that
        F110VecEnv.path_actions and replay_action take: tanh(mean) with evaluate, else a sample.  frames: the env's uint8 bitmaps [n,
        rows, cols] or their bits [m, rows, words] int64 (info['lidar_bitmap'] either way); index: rows of `frames` to act on (None:
        all).  eps: the [n, action_dim] fp32 draws (None: torch.randn, or stream 0 of `source` with the envs' numbers as rows); out: a
        [n, action_dim] fp64 tensor that receives the action, a static buffer that path_actions or a captured step reads.  A row's action does not depend on the batch around it."""
        with torch.no_grad():
            return self._act(self.actor.features(frames, index), index, evaluate, out, eps)

    def _act(self, h, rows, evaluate, out, eps):
        """The actor's tail on the features h, under the caller's no_grad: tanh(mean) with evaluate, else a sample whose draws, where
        none are passed, are the device's for the rows `rows` (None: row i is env i)."""
        head = self.actor.head
        if evaluate:
            return sample_actions(h, head.fc_mean.weight, head.fc_mean.bias, head.fc_log_std.weight, head.fc_log_std.bias, eps=None,
                                  dtype=torch.float64, out=out)[0]
        if eps is None and self.source is not None:
            eps = self.source.normal(h.shape[0], self.action_dim, stream=0, rows=rows)
        return head.sample(h, eps=eps, dtype=torch.float64, out=out)[0]

    def act_from(self, replay, evaluate=False, out=None, eps=None):
        """select_action on what the ring `replay` (F110VecEnv.replay) holds as every env's newest frames: ReplayBuffer.stack_latest(stack)
        over the ring's own frame tensor, nothing is copied or unpacked.  Row i is env i (so are the rows of the device's draws).  With
        stack = 1 this is select_action(info['lidar_bitmap']) of the step that made the last push, bit for bit.  An env whose ring is
        empty acts on frames of zeros.  evaluate, out, eps: as select_action."""
        self._check_replay(replay)
        rows, _ = replay.stack_latest(self.stack)
        with torch.no_grad():
            return self._act(self.actor.features(replay.frame_view(), rows[:, 0] if self.stack == 1 else rows), None, evaluate, out, eps)

    # ---- learning
    def _eps(self, eps, n):
        if eps is None:
            return None, None
        if not isinstance(eps, (tuple, list)) or len(eps) != 2:
            raise ValueError('SACAgent: eps must be (eps_next, eps_new)')
        for e in eps:
            if not torch.is_tensor(e) or e.dtype != torch.float32 or tuple(e.shape) != (n, self.action_dim) or e.device != self.device:
                raise ValueError('SACAgent: eps_next and eps_new must be fp32 [%d, %d] on %s' % (n, self.action_dim, self.device))
        return eps[0], eps[1]

    def _update(self, batch, eps_next, eps_new, losses, writeback=None):
        """:544-580 on one batch, a dict under the names of replay.sample_fields; the three losses go to `losses` [3] (actor, critic1,
        critic2), which is returned.  The frame rows are 's_stack' / 'ns_stack' where the batch has them, else 's_idx' / 'ns_idx'.
        'discount': [n] fp64, the target's discount per row ('r' is then the n-step return); without it gamma.  'weight': [n] fp32
        importance weights of the critics' loss; writeback: the PriorityTree that then takes the new TD errors of the rows 'indices'
        with 'ok'."""
        actor, critics, targets = self.actor, self.critics, self.targets
        frames, a, discount, weight = batch['frames'], batch['a'], batch.get('discount'), batch.get('weight')
        s_idx, ns_idx = batch.get('s_stack', batch['s_idx']), batch.get('ns_stack', batch['ns_idx'])
        n = int(s_idx.shape[0])
        if eps_next is None and self.source is not None:
            eps_next = self.source.normal(n, self.action_dim, stream=1)
            eps_new = self.source.normal(n, self.action_dim, stream=2)
        with torch.no_grad():                                                    # :544-549
            next_a, next_logp = actor.sample(frames, ns_idx, eps_next)
            tv = td_target([t.trunk(frames, ns_idx) for t in targets], next_a, next_logp, batch['r'], batch['d'], *_heads(targets),
                           self.gamma if discount is None else discount, self.alpha, dense=True)
        q, _ = twin_q([c.trunk(frames, s_idx) for c in critics], a, *_heads(critics), dense=True)     # :551-552, a as the ring stores it (fp32)
        grad_q = torch.empty_like(q)
        if weight is None:
            critic_loss(q[0], q[1], tv, loss=losses[1:3], grad=grad_q)           # :553-554
        else:
            td = torch.empty((n,), dtype=torch.float32, device=self.device)
            critic_loss(q[0], q[1], tv, loss=losses[1:3], grad=grad_q, weight=weight, td=td)
            if writeback is not None:
                writeback.update(batch['indices'], batch['ok'], td)
        for opt in self.critic_opts:
            opt.zero_grad()
        torch.autograd.backward((q,), (grad_q,))
        for opt in self.critic_opts:
            opt.step()                                                           # :556-562 and, in the same pass, :575-578
        new_a, logp = actor.sample(frames, s_idx, eps_new)                       # :564-568
        _, qn = twin_q([c.trunk(frames, s_idx) for c in critics], new_a, *_heads(critics), dense=True)
        _, g_logp, g_qn = actor_loss(logp, qn, self.alpha, loss=losses[0:1])
        if self.temperature is not None:
            self.temperature.step(logp)                                          # alpha of the NEXT update; this one's is read above
        self.actor_opt.zero_grad()
        torch.autograd.backward((logp, qn), (g_logp, g_qn))
        self.actor_opt.step()                                                    # :570-572
        return losses

    def update_batch(self, batch, eps=None, replay=None):
        """One update on a batch that is given, not drawn: a dict with 'frames' [m, rows, words] int64, 's_idx' and 'ns_idx' [n] int64
        rows of it (-1: a zero frame), 'a' [n, action_dim] fp32, 'r' [n] fp64 and 'd' [n] uint8, as ReplayBuffer.sample_frames returns
        them; with stack = k > 1 the frame rows are 's_stack' and 'ns_stack' [n, k] (ReplayBuffer.frames_at(..., stack=k)), or 's_idx'
        and 'ns_idx' themselves given as [n, k].  An optional 'discount' [n] fp64 is the target's discount per row in gamma's place ('r' is then the n-step return and
        'ns_idx', 'd' those of the span's end, as ReplayBuffer.frames_at with nstep > 1 returns them); without it gamma, whatever the agent's nstep.
        An optional 'weight' [n] fp32 weighs the critics' loss row by row (ReplayBuffer.sample_priority_dev's importance weights); with
        'indices' [n] int64 and 'ok' [n] uint8 beside it and `replay` (a ring with priorities) the rows' new priorities are written back
        as update() does with per=True; without them nothing is written back.
        eps = (eps_next, eps_new), fp32 [n, action_dim], replace the two torch.randn draws.  Returns the new [3] fp32 loss tensor
        (actor, critic1, critic2) on the device; no synchronisation."""
        n = int(batch['s_idx'].shape[0])
        eps_next, eps_new = self._eps(eps, n)
        losses = torch.empty((3,), dtype=torch.float32, device=self.device)
        writeback = None
        if batch.get('weight') is not None and replay is not None and 'indices' in batch and 'ok' in batch:
            if replay.priorities is None:
                raise ValueError('SACAgent: the ring has no priorities (record_replay(..., priorities=True))')
            writeback = replay.priorities
        # (a 'discount' the caller supplies is used as it is, whatever the agent's nstep: only _draw drops one)
        return self._update(batch, eps_next, eps_new, losses, writeback)

    def _check_replay(self, replay):
        if not replay.on:
            raise ValueError('SACAgent: the replay buffer is off (record_replay())')
        if (replay.rows, replay.cols, replay.action_dim) != (self.rows, self.cols, self.action_dim) or replay.eng.device != self.device:
            raise ValueError('SACAgent: the ring holds %d x %d images and %d action values on %s; the agent takes %d x %d and %d on %s'
                             % (replay.rows, replay.cols, replay.action_dim, replay.eng.device, self.rows, self.cols, self.action_dim, self.device))
        if self.per and replay.priorities is None:
            raise ValueError('SACAgent: per=True, but the ring has no priorities (record_replay(..., priorities=True))')

    def update(self, replay, batch_size=64, eps=None, check=False):
        """SACAgent.update (src/SAL.py:521-580) from the ring `replay` (F110VecEnv.replay): batch_size transitions drawn on the
        device with the agent's own draw counter, then update_batch.  Returns the [3] loss tensor; nothing synchronises.
        check=True is the reference's `len(replay_buffer) < batch_size` test (:532): one synchronisation, and with fewer valid
        transitions in the ring it returns zeros and touches nothing, the draw counter included.  Without it a draw that finds no valid
        transition (ok = 0: an empty ring, or 64 misses in a sparse one) is a zero transition -- zero frames, action, reward and done --
        and is learnt from like any other; the caller keeps the ring filled (update_after in examples/sac_train.py)."""
        self._check_replay(replay)
        n = int(batch_size)
        eps_next, eps_new = self._eps(eps, n)
        if check and len(replay) < n:
            return torch.zeros((3,), dtype=torch.float32, device=self.device)
        self.sample = replay.sample_out(n, self.nstep, self.per, self.stack)
        batch, writeback = self._draw(replay, n, self.sample)
        return self._update(batch, eps_next, eps_new, torch.empty((3,), dtype=torch.float32, device=self.device), writeback)

    def _draw(self, replay, n, out):
        """The batch of an update drawn into `out` with the agent's draw counter -> (batch, writeback): the batch as the ring returns
        it (a new dict: `out` gains nothing), writeback the ring's PriorityTree with per=True, else None."""
        draw = replay.sample_priority_dev if self.per else replay.sample_frames_dev
        batch = draw(n, self.draws, out=out, nstep=self.nstep, gamma=self.gamma, stack=self.stack)
        if self.nstep == 1:
            # the target takes gamma BY VALUE, as it always has with nstep = 1 (the same launches, graph key and bits): the
            # 'discount' column the priority draw wrote, gamma's bits in every row, is not handed on
            batch.pop('discount', None)
        return batch, replay.priorities if self.per else None

    # ---- the captured update
    def _graph_key(self, replay, n):
        opts = self.optimizers().values()
        key = (id(replay), replay.generation, replay.steps, replay.eng.B, replay._seed(None), n,
               tuple((o.lr, o.betas, o.eps, o.tau) for o in opts))
        t = self.temperature
        key = key if t is None else key + ((t.lr, t.betas, t.eps, t.target_entropy),)
        key = key if self.nstep == 1 else key + (('nstep', self.nstep, self.gamma),)
        key = key if self.stack == 1 else key + (('stack', self.stack),)
        key = key if self.clip_states is None else key + (('max_grad_norm', self.max_grad_norm),)
        if self.per:                                # (a ring that lost its priorities: another key, and the capture refuses it)
            p = replay.priorities
            key = key + (('per', self.gamma) + ((None,) if p is None else (p.leaf.data_ptr(), p.state.data_ptr())),)
        return key if self.source is None else key + (('source', self.source.state.data_ptr()),)

    def capture_update(self, replay, batch_size=64, draws=True):
        """Captures the whole of update(replay, batch_size) -- the sample and the advance of the draw counter, both forward and
        backward passes, the losses, the three optimizer steps -- in one torch.cuda.graph on a side stream.  A capture executes
        nothing: no parameter, moment or counter moves.  The batch, the two draws and the losses live in static tensors (the losses:
        the tensor update_graph returns, the same across re-captures); .grad is dropped inside the capture, so the gradients live in the
        graph's pool.  draws=True records the two draws inside the graph (torch.randn of the framework's graph-safe generator, or the
        two fills of `source` and the advances of their counters); draws=False
        captures the variant that reads the static draws update_graph(eps=...) fills.  update_graph captures what it needs by itself;
        calling this first only moves the cost."""
        self._check_replay(replay)
        n, dev = int(batch_size), self.device
        key = self._graph_key(replay, n)
        if key != self._g_key:
            self._graphs = {}
            self._g_key, self._g_replay = key, replay
            self._g_sample = replay.sample_out(n, self.nstep, self.per, self.stack)
            self._g_eps = [torch.zeros((n, self.action_dim), dtype=torch.float32, device=dev) for _ in range(2)]
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
            self.zero_grad(set_to_none=True)
            batch, writeback = self._draw(replay, n, self._g_sample)
            eps_next, eps_new = (None, None) if draws else self._g_eps
            self._update(batch, eps_next, eps_new, self._g_losses, writeback)
        cur.wait_stream(side)
        self._graphs[bool(draws)] = g
        self.captures += 1
        return self._g_losses

    def update_graph(self, eps=None):
        """Replays the update captured for the ring and batch size of the last capture_update: one host call.  eps = (eps_next,
        eps_new) are copied into the static draws first; without them the graph draws by itself.  Returns the static [3] loss tensor
        (read it before the next replay).  The update is captured again first -- `recaptured` says so, `captures` counts -- when the
        ring was installed anew (its old tensors are freed), or an optimizer's (or the temperature's) lr, betas, eps, tau or target
        entropy, the env's seed, or nstep (and, with nstep > 1, gamma, which the walk takes by value) has changed:
        a captured launch keeps the addresses and scalars it was captured with."""
        if self._g_key is None:
            raise ValueError('SACAgent: no update is captured (capture_update(replay, batch_size))')
        replay, n = self._g_replay, self._g_key[5]
        draws = eps is None
        if not draws:
            eps_next, eps_new = self._eps(eps, n)
        self.recaptured = not replay.on or self._graph_key(replay, n) != self._g_key
        if self.recaptured or draws not in self._graphs:
            self.capture_update(replay, n, draws)
        if not draws:
            self._g_eps[0].copy_(eps_next)
            self._g_eps[1].copy_(eps_new)
        self.sample = self._g_sample
        self._graphs[draws].replay()
        return self._g_losses

    # ---- state
    def actor_state_dict(self):
        """The actor under the reference's keys (conv1.weight .. fc_log_std.bias): what main() saves as sac_actor.pth."""
        return {_key(k): p.detach() for k, p in self.actor.named_parameters()}

    def load_actor_state_dict(self, sd):
        self._load_net('actor', sd)

    def _load_net(self, name, sd):
        net = self.modules()[name]
        own = {_key(k): p.detach() for k, p in net.named_parameters()}
        if sorted(own) != sorted(sd):
            raise ValueError('SACAgent: the state of %s has the keys %s, expected %s' % (name, sorted(sd), sorted(own)))
        with torch.no_grad():
            for k, v in own.items():
                if tuple(v.shape) != tuple(sd[k].shape):
                    raise ValueError('SACAgent: %s of %s has shape %s, expected %s' % (k, name, tuple(sd[k].shape), tuple(v.shape)))
            for k, v in own.items():
                v.copy_(sd[k])                                                  # in place: a captured update keeps reading these tensors

    def state_dict(self):
        """The five networks under the reference's keys, the three optimizers in torch.optim.Adam's format (SacAdam.state_dict) and
        the draw counter, under 'temperature' the learnt temperature's state where there is one and under 'source' the seed and the
        call counters of the device's draws where it makes them (copies; synchronises)."""
        sd = {name: {_key(k): p.detach().clone() for k, p in net.named_parameters()} for name, net in self.modules().items()}
        for name, opt in self.optimizers().items():
            sd[name + '_optimizer'] = opt.state_dict()
        sd['draws'] = int(self.draws.item())
        if self.temperature is not None:
            sd['temperature'] = self.temperature.state_dict()
        if self.source is not None:
            sd['source'] = self.source.state_dict()
        return sd

    def load_state_dict(self, sd):
        """Continues from state_dict()'s result, written in place into the agent's own tensors."""
        for name in NETS:
            self._load_net(name, sd[name])
        for name, opt in self.optimizers().items():
            opt.load_state_dict(sd[name + '_optimizer'])
        self.draws.fill_(int(sd['draws']))
        if self.temperature is not None:
            self.temperature.load_state_dict(sd['temperature'])
        if self.source is not None:
            self.source.load_state_dict(sd['source'])
