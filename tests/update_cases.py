"""One whole SACAgent.update (src/SAL.py:521-580) twice over: MirrorAgent, the reference's networks and its update restated in plain
torch.nn for any image size and dtype (pinned on the reference's own update by tests/golden/g24_update.npz, test_update_cpu.py), and
LibAgent, the same five networks on the same tensors computed by the library's modules in the order of examples/sac_update.py.  The
mirror runs as fp32 on the GPU (the reference's arithmetic on this stack), as fp32 on the CPU and as fp64 on the CPU (the truth); its
phases are pure functions of the parameters, the batch and the draws, so that the library can be compared phase by phase from its own
parameters (teacher forcing) and the framework's own fp32 error measured on the same inputs."""
import numpy as np
import torch
import torch.nn.functional as F

import replay_cases as rc

GAMMA, TAU, ALPHA, LR = 0.99, 0.005, 0.2, 3e-4                  # SACAgent's defaults (:478-480)
NETS = ('actor', 'critic1', 'critic2', 'critic1_target', 'critic2_target')        # the reference's order of construction (:486-495)
TRAINED = NETS[:3]
CONV_KEYS = ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias']
ACTOR_KEYS = CONV_KEYS + ['fc1.weight', 'fc1.bias', 'fc_mean.weight', 'fc_mean.bias', 'fc_log_std.weight', 'fc_log_std.bias']
CRITIC_KEYS = CONV_KEYS + ['fc1.weight', 'fc1.bias', 'fc2.weight', 'fc2.bias']
SAL = dict(rows=256, cols=256, hidden=512, action_dim=16)

# config: rows, cols, hidden, action_dim, n, on, pool (tests/test_gpu_update.py says what each reaches)
CONFIGS = {
    'a': dict(rows=68, cols=76, hidden=96, action_dim=16, n=24, on=1.0, pool=30),
    'b': dict(rows=68, cols=76, hidden=96, action_dim=15, n=24, on=1.0, pool=30),
    'c': dict(rows=68, cols=76, hidden=96, action_dim=16, n=24, on=255.0, pool=30),
    'd': dict(rows=44, cols=44, hidden=64, action_dim=16, n=3, on=1.0, pool=4),
}
UPDATES = 3


def keys_of(net):
    return ACTOR_KEYS if net == 'actor' else CRITIC_KEYS


def feature_shape(rows, cols):
    """(OH, OW) behind conv1(8, 4), conv2(4, 2), conv3(3, 1) without padding."""
    for k, s in ((8, 4), (4, 2), (3, 1)):
        rows, cols = (rows - k) // s + 1, (cols - k) // s + 1
    return rows, cols


def feature_width(rows, cols):
    oh, ow = feature_shape(rows, cols)
    return 32 * oh * ow


# ------------------------------------------------------------------------------------------------ the mirror
class _Trunk(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(1, 16, kernel_size=8, stride=4)
        self.conv2 = torch.nn.Conv2d(16, 32, kernel_size=4, stride=2)
        self.conv3 = torch.nn.Conv2d(32, 32, kernel_size=3, stride=1)

    def features(self, x):
        x = F.relu(self.conv1(x))
        x = F.relu(self.conv2(x))
        x = F.relu(self.conv3(x))
        return x.view(x.size(0), -1)


class MirrorActor(_Trunk):
    def __init__(self, width, hidden, action_dim):
        super().__init__()
        self.fc1 = torch.nn.Linear(width, hidden)
        self.fc_mean = torch.nn.Linear(hidden, action_dim)
        self.fc_log_std = torch.nn.Linear(hidden, action_dim)

    def forward(self, x):
        x = F.relu(self.fc1(self.features(x)))
        return self.fc_mean(x), torch.clamp(self.fc_log_std(x), -20, 2)

    def sample(self, x, eps):
        """Actor.sample with rsample's draw passed in: Normal.rsample is loc + eps * scale."""
        mean, log_std = self.forward(x)
        std = log_std.exp()
        dist = torch.distributions.Normal(mean, std)
        x_t = mean + eps * std
        y_t = torch.tanh(x_t)
        log_prob = (dist.log_prob(x_t) - torch.log(1 - y_t.pow(2) + 1e-6)).sum(1, keepdim=True)
        return y_t, log_prob


class MirrorCritic(_Trunk):
    def __init__(self, width, hidden, action_dim):
        super().__init__()
        self.fc1 = torch.nn.Linear(width + action_dim, hidden)
        self.fc2 = torch.nn.Linear(hidden, 1)

    def forward(self, x, action):
        x = torch.cat([self.features(x), action], dim=1)
        return self.fc2(F.relu(self.fc1(x)))


class MirrorAgent:
    """The five networks, built in fp32 on the CPU in the reference's order (so torch.manual_seed(seed) in front reproduces its
    initialisation at SAL's shape), the targets loaded from the critics, then moved to `device` and `dtype`.  on: what a set pixel is
    worth.  A batch is mirror_batch()'s dict."""

    def __init__(self, rows, cols, hidden, action_dim, on=1.0, dtype=torch.float32, device='cpu', seed=None):
        if seed is not None:
            torch.manual_seed(seed)
        width = feature_width(rows, cols)
        self.rows, self.cols, self.hidden, self.action_dim, self.width = rows, cols, hidden, action_dim, width
        self.on, self.dtype, self.device = float(on), dtype, torch.device(device)
        self.actor = MirrorActor(width, hidden, action_dim)
        self.critic1 = MirrorCritic(width, hidden, action_dim)
        self.critic2 = MirrorCritic(width, hidden, action_dim)
        self.critic1_target = MirrorCritic(width, hidden, action_dim)
        self.critic2_target = MirrorCritic(width, hidden, action_dim)
        self.critic1_target.load_state_dict(self.critic1.state_dict())
        self.critic2_target.load_state_dict(self.critic2.state_dict())
        for name in NETS:
            getattr(self, name).to(device=self.device, dtype=dtype)
        self.optimizers = {name: torch.optim.Adam(getattr(self, name).parameters(), lr=LR) for name in TRAINED}

    def net(self, name):
        return getattr(self, name)

    def load_from(self, other):
        """Every tensor of the five networks from another mirror, converted to this one's dtype and device."""
        with torch.no_grad():
            for name in NETS:
                mine, theirs = self.net(name).state_dict(), other.net(name).state_dict()
                assert list(mine) == list(theirs)
                for k in mine:
                    mine[k].copy_(theirs[k].to(device=self.device, dtype=self.dtype))

    # ---- the phases: pure functions, torch.autograd.grad, no .grad written
    def _target_value(self, b, eps_next):
        with torch.no_grad():
            next_a, next_logp = self.actor.sample(b['ns'], eps_next)
            tq1 = self.critic1_target(b['ns'], next_a)
            tq2 = self.critic2_target(b['ns'], next_a)
            tq = torch.min(tq1, tq2) - ALPHA * next_logp
            tv = b['r'] + (1 - b['d']) * GAMMA * tq
        return next_a, next_logp, tv

    def critic_phase(self, b, eps_next):
        """:544-554 -> next_a, next_logp, tv, cq [2], c_loss [2] and grads[critic][key] of each critic's own loss."""
        next_a, next_logp, tv = self._target_value(b, eps_next)
        cq = [self.critic1(b['s'], b['a']), self.critic2(b['s'], b['a'])]
        losses = [F.mse_loss(cq[0], tv), F.mse_loss(cq[1], tv)]
        grads = {}
        for name, loss in zip(('critic1', 'critic2'), losses):
            net = self.net(name)
            grads[name] = dict(zip(CRITIC_KEYS, torch.autograd.grad(loss, [net.get_parameter(k) for k in CRITIC_KEYS])))
        return dict(next_a=next_a, next_logp=next_logp[:, 0], tv=tv[:, 0], cq=[q.detach()[:, 0] for q in cq], c_loss=[v.detach() for v in losses],
                    grads=grads)

    def actor_phase(self, b, eps_new):
        """:564-568 -> new_a, logp, qn, a_loss, grads['actor'][key], and grads['critic1' / 'critic2'][key]: what the actor's loss
        leaves in the critics."""
        new_a, logp = self.actor.sample(b['s'], eps_new)
        q1n = self.critic1(b['s'], new_a)
        q2n = self.critic2(b['s'], new_a)
        qn = torch.min(q1n, q2n)
        a_loss = (ALPHA * logp - qn).mean()
        leaves = [(name, k, self.net(name).get_parameter(k)) for name in TRAINED for k in keys_of(name)]
        got = torch.autograd.grad(a_loss, [p for _, _, p in leaves])
        grads = {name: {} for name in TRAINED}
        for (name, k, _), g in zip(leaves, got):
            grads[name][k] = g
        return dict(new_a=new_a.detach(), logp=logp.detach()[:, 0], qn=qn.detach()[:, 0], a_loss=a_loss.detach(), grads=grads)

    # ---- the parameter update
    def adam_step(self, name, grads):
        """optimizer.zero_grad(); .grad = grads[key]; optimizer.step() of one network."""
        net = self.net(name)
        for k in keys_of(name):
            net.get_parameter(k).grad = grads[k].clone()
        self.optimizers[name].step()

    def polyak(self):
        for name in ('critic1', 'critic2'):                                                # :575-578
            for tp, p in zip(self.net(name + '_target').parameters(), self.net(name).parameters()):
                tp.data.copy_(TAU * p.data + (1 - TAU) * tp.data)

    def composed_update(self, b, eps_next, eps_new):
        """critic_phase + Adam + actor_phase + Adam + Polyak -> (the two phases' results)."""
        cp = self.critic_phase(b, eps_next)
        for name in ('critic1', 'critic2'):
            self.adam_step(name, cp['grads'][name])
        ap = self.actor_phase(b, eps_new)
        for name in ('critic1', 'critic2'):          # the actor's backward adds to what the critics' own left (no zero_grad between)
            for k in CRITIC_KEYS:
                self.net(name).get_parameter(k).grad.add_(ap['grads'][name][k])
        self.adam_step('actor', ap['grads']['actor'])
        self.polyak()
        return cp, ap

    def whole_update(self, b, eps_next, eps_new):
        """The reference's sequence (:544-580) with .backward() and its three optimizers -> every recorded quantity, with .grad
        cloned in front of each step()."""
        opt = self.optimizers
        next_a, next_logp, tv = self._target_value(b, eps_next)
        cq1 = self.critic1(b['s'], b['a'])
        cq2 = self.critic2(b['s'], b['a'])
        c1_loss = F.mse_loss(cq1, tv)
        c2_loss = F.mse_loss(cq2, tv)
        grads = {}

        def snap(name):
            grads[name] = {k: self.net(name).get_parameter(k).grad.clone() for k in keys_of(name)}

        opt['critic1'].zero_grad()
        c1_loss.backward()
        snap('critic1')
        opt['critic1'].step()
        opt['critic2'].zero_grad()
        c2_loss.backward()
        snap('critic2')
        opt['critic2'].step()
        new_a, logp = self.actor.sample(b['s'], eps_new)
        q1n = self.critic1(b['s'], new_a)
        q2n = self.critic2(b['s'], new_a)
        qn = torch.min(q1n, q2n)
        a_loss = (ALPHA * logp - qn).mean()
        opt['actor'].zero_grad()
        a_loss.backward()
        snap('actor')
        opt['actor'].step()
        self.polyak()
        return dict(next_a=next_a, next_logp=next_logp[:, 0], tv=tv[:, 0], cq=[cq1.detach()[:, 0], cq2.detach()[:, 0]],
                    c_loss=[c1_loss.detach(), c2_loss.detach()], new_a=new_a.detach(), logp=logp.detach()[:, 0], qn=qn.detach()[:, 0],
                    a_loss=a_loss.detach(), grads=grads)


# ------------------------------------------------------------------------------------------------ the batch
def batch(seed, n, rows, cols, A, pool):
    """A replay sample as the ring hands it out, NumPy only: `pool` Bernoulli images (a density of 0.2..0.8 each, 0 / 255) and their
    packed frames, s_idx and ns_idx [n] into the pool (pool < 2 n: frames repeat, and row 1's next state is row 0's state), one row
    (`hole`) with s_idx = ns_idx = -1 and zero action, reward and done; action = tanh(normal) fp32, reward fp64, done uint8 with both
    values, and the two draws eps_next, eps_new fp32."""
    assert pool < 2 * n and n >= 3
    rng = np.random.default_rng([seed, n, rows, cols, A, pool])
    imgs = ((rng.random((pool, rows, cols)) < rng.uniform(0.2, 0.8, (pool, 1, 1))) * 255).astype(np.uint8)
    s_idx, ns_idx = rng.integers(0, pool, n).astype(np.int64), rng.integers(0, pool, n).astype(np.int64)
    ns_idx[1] = s_idx[0]
    a = np.tanh(rng.normal(size=(n, A))).astype(np.float32)
    r = rng.normal(size=n)
    d = (rng.random(n) < 0.5).astype(np.uint8)
    hole = n // 2
    d[0], d[n - 1] = 1, 0
    s_idx[hole] = ns_idx[hole] = -1
    a[hole], r[hole], d[hole] = 0.0, 0.0, 0
    eps_next, eps_new = (rng.normal(size=(n, A)).astype(np.float32) for _ in range(2))
    assert set(d.tolist()) == {0, 1} and len(set(s_idx.tolist()) | set(ns_idx.tolist())) < 2 * n
    return dict(imgs=imgs, packed=rc.pack(imgs), s_idx=s_idx, ns_idx=ns_idx, a=a, r=r, d=d, eps_next=eps_next, eps_new=eps_new, hole=hole,
                rows=rows, cols=cols)


def golden_batch(g):
    """g24_update.npz's batch in batch()'s form: a pool of the 8 states followed by the 8 next states, and the draws as recorded."""
    imgs = np.concatenate([np.unpackbits(g[k], axis=2) for k in ('s_bits', 'ns_bits')]).astype(np.uint8) * 255
    n = int(g['a'].shape[0])
    assert imgs.shape == (2 * n, SAL['rows'], SAL['cols'])
    return dict(imgs=imgs, packed=rc.pack(imgs), s_idx=np.arange(n, dtype=np.int64), ns_idx=np.arange(n, 2 * n, dtype=np.int64), a=g['a'], r=g['r'],
                d=g['d'], eps_next=g['eps_next'], eps_new=g['eps_new'], hole=None, rows=SAL['rows'], cols=SAL['cols'])


def golden_positions(g, net, key, numel):
    """The flat positions of the entries the fixture keeps of a tensor (the draw of g24's generator, tests/golden/make_golden.py g24)."""
    entries = int(g['entries'])
    if numel <= entries:
        return np.arange(numel, dtype=np.int64)
    at = np.random.default_rng([int(g['position_seed']), 100 * NETS.index(net) + keys_of(net).index(key)]).choice(numel, entries, replace=False)
    return np.sort(at).astype(np.int64)


def without_row(b, i):
    """The batch without row i (the pool stays)."""
    out = dict(b)
    for k in ('s_idx', 'ns_idx', 'a', 'r', 'd', 'eps_next', 'eps_new'):
        out[k] = np.delete(b[k], i, axis=0)
    out['hole'] = None
    return out


def mirror_batch(b, on, dtype, device):
    """What update() makes of the sample (:536-542) for a mirror: s, ns [n, 1, rows, cols] = the image's 0 / 1 times `on` (a zero
    image for index -1), a [n, A], r and d [n, 1], and the two draws, all of `dtype` (reward and done rounded as FloatTensor would at
    fp32)."""
    unit = np.concatenate([(b['imgs'] == 255), np.zeros((1,) + b['imgs'].shape[1:], bool)])      # entry -1: the zero image
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(device=device, dtype=dtype)  # noqa: E731
    return dict(s=t(unit[b['s_idx']][:, None]) * on, ns=t(unit[b['ns_idx']][:, None]) * on, a=t(b['a']), r=t(b['r'])[:, None],
                d=t(b['d'])[:, None], eps_next=t(b['eps_next']), eps_new=t(b['eps_new']))


def lib_batch(b, device='cuda'):
    """What ReplayRing.sample_frames returns, on the GPU: packed frames int64, s_idx, ns_idx int64, action fp32, reward fp64, done
    uint8, and the draws fp32."""
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=device)  # noqa: E731
    return dict(frames=t(b['packed'].view(np.int64)), s_idx=t(b['s_idx']), ns_idx=t(b['ns_idx']), a=t(b['a']), r=t(b['r']), d=t(b['d']),
                eps_next=t(b['eps_next']), eps_new=t(b['eps_new']))


# ------------------------------------------------------------------------------------------------ the library agent
def lib_key(name):
    """A library module's parameter name -> the reference's key."""
    return name.replace('trunk.', '').replace('head.', '')


class LibActor(torch.nn.Module):
    def __init__(self, m, on, cols):
        super().__init__()
        from red_gym_amd.dense import Dense
        from red_gym_amd.featconv import Trunk
        from red_gym_amd.policyhead import PolicyHead
        self.trunk = Trunk.from_convs(m.conv1, m.conv2, m.conv3, on=on, cols=cols)
        self.fc1 = Dense.from_linear(m.fc1, relu=True)
        self.head = PolicyHead.from_linears(m.fc_mean, m.fc_log_std)

    def sample(self, frames, index, eps):
        action, log_prob, _, _ = self.head.sample(self.fc1(self.trunk(frames, index)), eps=eps)
        return action, log_prob


class LibCritic(torch.nn.Module):
    def __init__(self, m, on, cols):
        super().__init__()
        from red_gym_amd.featconv import Trunk
        from red_gym_amd.qhead import QHead
        self.trunk = Trunk.from_convs(m.conv1, m.conv2, m.conv3, on=on, cols=cols)
        self.head = QHead.from_linears(m.fc1, m.fc2, dense=True)


def _heads(nets):
    return [c.head.fc1 for c in nets], [c.head.fc2 for c in nets]


class LibAgent:
    """examples/sac_update.py's Actor, Critic, optimizers and update() on the tensors of an fp32 mirror on the GPU."""

    def __init__(self, actor, critics, targets):
        from red_gym_amd.optim import SacAdam
        self.actor, self.critics, self.targets = actor, critics, targets
        self.actor_opt = SacAdam(actor, lr=LR)
        self.critic_opts = [SacAdam(c, lr=LR, targets=t, tau=TAU) for c, t in zip(critics, targets)]

    @classmethod
    def from_mirror(cls, mirror, cols):
        assert mirror.dtype == torch.float32 and mirror.device.type == 'cuda'
        on = mirror.on
        return cls(LibActor(mirror.actor, on, cols), [LibCritic(mirror.critic1, on, cols), LibCritic(mirror.critic2, on, cols)],
                   [LibCritic(mirror.critic1_target, on, cols), LibCritic(mirror.critic2_target, on, cols)])

    def modules(self):
        return dict(actor=self.actor, critic1=self.critics[0], critic2=self.critics[1], critic1_target=self.targets[0], critic2_target=self.targets[1])

    def optimizers(self):
        return dict(actor=self.actor_opt, critic1=self.critic_opts[0], critic2=self.critic_opts[1])

    def grads(self, name):
        """.grad of one network as it stands, cloned, under the reference's keys (None where there is none)."""
        return {lib_key(k): None if p.grad is None else p.grad.detach().clone() for k, p in self.modules()[name].named_parameters()}

    def critic_phase(self, b, eps_next, hook=None, zero_grad=True):
        """update()'s lines up to the critics' step; hook(name, optimizer) runs in front of each step()."""
        with torch.no_grad():
            next_a, next_logp = self.actor.sample(b['frames'], b['ns_idx'], eps_next)
            from red_gym_amd.qhead import td_target, twin_q
            tv = td_target([t.trunk(b['frames'], b['ns_idx']) for t in self.targets], next_a, next_logp, b['r'], b['d'], *_heads(self.targets), GAMMA,
                           ALPHA, dense=True)
        q, _ = twin_q([c.trunk(b['frames'], b['s_idx']) for c in self.critics], b['a'], *_heads(self.critics), dense=True)
        c_losses = [F.mse_loss(q[0], tv), F.mse_loss(q[1], tv)]
        if zero_grad:
            for opt in self.critic_opts:
                opt.zero_grad()
        (c_losses[0] + c_losses[1]).backward()
        for name, opt in zip(('critic1', 'critic2'), self.critic_opts):
            if hook is not None:
                hook(name, opt)
            opt.step()
        return dict(next_a=next_a, next_logp=next_logp, tv=tv, cq=[q[0].detach(), q[1].detach()], c_loss=[v.detach() for v in c_losses])

    def actor_phase(self, b, eps_new, hook=None):
        from red_gym_amd.qhead import twin_q
        new_a, logp = self.actor.sample(b['frames'], b['s_idx'], eps_new)
        _, qn = twin_q([c.trunk(b['frames'], b['s_idx']) for c in self.critics], new_a, *_heads(self.critics), dense=True)
        a_loss = (ALPHA * logp - qn).mean()
        self.actor_opt.zero_grad()
        a_loss.backward()
        if hook is not None:
            hook('actor', self.actor_opt)
        self.actor_opt.step()
        return dict(new_a=new_a.detach(), logp=logp.detach(), qn=qn.detach(), a_loss=a_loss.detach())

    # ---- everything a step may change, for the exact checks
    def snapshot(self):
        """Clones of every parameter and target, every optimizer's moments and its device state."""
        snap = {'params': {n: {lib_key(k): p.detach().clone() for k, p in m.named_parameters()} for n, m in self.modules().items()}}
        snap['opt'] = {n: (o.exp_avg.clone(), o.exp_avg_sq.clone(), o._state.clone()) for n, o in self.optimizers().items()}
        return snap

    def restore(self, snap):
        with torch.no_grad():
            for n, m in self.modules().items():
                for k, p in m.named_parameters():
                    p.copy_(snap['params'][n][lib_key(k)])
                    p.grad = None
            for n, o in self.optimizers().items():
                m, v, s = snap['opt'][n]
                o.exp_avg.copy_(m)
                o.exp_avg_sq.copy_(v)
                o._state.copy_(s)


# ------------------------------------------------------------------------------------------------ measuring
def rel_err(x, x64):
    """||x - x64||_2 / ||x64||_2 in fp64 on the host (0 for two zero arrays, inf for a non-zero x against zeros)."""
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64).reshape(-1)
    ref = np.asarray(x64.detach().cpu().numpy() if torch.is_tensor(x64) else x64, np.float64).reshape(-1)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    num, den = float(np.linalg.norm(x - ref)), float(np.linalg.norm(ref))
    if den == 0.0:
        return 0.0 if num == 0.0 else float('inf')
    return num / den


def flatten(phase, prefix=''):
    """A phase's result as {name: tensor}: cq.0, c_loss.1, grads.critic1.fc1.weight ..."""
    out = {}
    for k, v in phase.items():
        if isinstance(v, dict):
            out.update(flatten(v, prefix + k + '.'))
        elif isinstance(v, (list, tuple)):
            out.update({'%s%s.%d' % (prefix, k, i): t for i, t in enumerate(v)})
        else:
            out[prefix + k] = v
    return out
