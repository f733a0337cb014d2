"""One complete SACAgent.update (src/SAL.py:521-580) from the replay ring on the GPU, in the reference's order, the parameter update
included (SacAdam: Adam and the soft update of the target critics in one pass per network):
    python examples/sac_update.py [envs] [steps] [batch]
    sample_frames -> Trunk (conv1 from the ring's bits, conv2, conv3: featconv) -> Dense (fc1 + ReLU) -> PolicyHead   (the actor)
                                                                                 -> twin_q / td_target, dense=True (the critics' fc1, fc2, min, target)
    -> the two critic losses, the actor loss; SacAdam.step() per network, which also moves the target critics (:575-578).
Every fc1 is the dense layer's kernels (red_gym_amd.dense): segments of 784 k's, each a fixed chain, added in a fixed order.
The critics never see cat([features, action]) (:440): the feature part of fc1 is that layer on the view fc1.weight[:, :F], and one
kernel does the action part, bias, ReLU, fc2, the min over the twin critics and the TD target, reading the policy head's fp64 action
and log_prob and the ring's fp64 reward and uint8 done as they are.  A random policy fills the ring first.  The two critic losses
are summed for one backward pass (their parameters are disjoint, so each critic gets the gradient the reference's two passes give
it), which runs the shared backward kernels once.  A target critic moves in the pass that updates its critic, before the actor's loss
where the reference moves it after: the actor's loss reads the critics, never the targets, so the update computes the same."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from red_gym_amd import F110VecEnv, workload
from red_gym_amd.dense import Dense
from red_gym_amd.featconv import Trunk
from red_gym_amd.optim import SacAdam
from red_gym_amd.policyhead import PolicyHead
from red_gym_amd.qhead import QHead, td_target, twin_q

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
BATCH = int(sys.argv[3]) if len(sys.argv) > 3 else 64
GAMMA, TAU, ALPHA, LR, AD = 0.99, 0.005, 0.2, 3e-4, 16                         # SACAgent's defaults (:478-480)
ON = 255.0                                                                     # a set pixel: update() feeds the raw 0 / 255 images (:536)
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.shape_rewards()
env.follow_paths()
env.record_replay(capacity=16 * B, action_dim=AD)
dev, cols = env.device, env.eng.shaper.cfg.cols
torch.manual_seed(0)


class Actor(torch.nn.Module):
    def __init__(self, width):
        super().__init__()
        self.trunk, self.fc1, self.head = Trunk(on=ON, cols=cols), Dense(width, 512, relu=True), PolicyHead(512, AD)

    def sample(self, frames, index):
        action, log_prob, _, _ = self.head.sample(self.fc1(self.trunk(frames, index)))
        return action, log_prob


class Critic(torch.nn.Module):
    def __init__(self, width):
        super().__init__()
        self.trunk, self.head = Trunk(on=ON, cols=cols), QHead(width, AD, 512, dense=True)


gen = torch.Generator(device=dev).manual_seed(0)
env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=dev))
for k in range(STEPS):
    raw = torch.rand((B, AD), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
    env.step(env.path_actions(raw))
frames, s_idx, ns_idx, a, r, d, ok = env.replay.sample_frames(BATCH)
with torch.no_grad():
    width = Trunk(on=ON, cols=cols).to(dev)(frames, s_idx).shape[1]
actor = Actor(width).to(dev)
critics = [Critic(width).to(dev) for _ in range(2)]
targets = [Critic(width).to(dev) for _ in range(2)]
for t, c in zip(targets, critics):
    t.load_state_dict(c.state_dict())
actor_opt = SacAdam(actor, lr=LR)
critic_opts = [SacAdam(c, lr=LR, targets=t, tau=TAU) for c, t in zip(critics, targets)]


def heads(nets):
    return [c.head.fc1 for c in nets], [c.head.fc2 for c in nets]


def update():
    frames, s_idx, ns_idx, a, r, d, ok = env.replay.sample_frames(BATCH)
    with torch.no_grad():                                                    # :544-549
        next_a, next_logp = actor.sample(frames, ns_idx)
        tv = td_target([t.trunk(frames, ns_idx) for t in targets], next_a, next_logp, r, d, *heads(targets), GAMMA, ALPHA, dense=True)
    q, _ = twin_q([c.trunk(frames, s_idx) for c in critics], a, *heads(critics), dense=True)     # :551-552, a as the ring stores it (fp32)
    c_losses = [F.mse_loss(q[0], tv), F.mse_loss(q[1], tv)]
    for opt in critic_opts:
        opt.zero_grad()
    (c_losses[0] + c_losses[1]).backward()
    for opt in critic_opts:
        opt.step()                                                           # :556-562 and, in the same pass, :575-578
    new_a, logp = actor.sample(frames, s_idx)                                 # :564-568
    _, qn = twin_q([c.trunk(frames, s_idx) for c in critics], new_a, *heads(critics), dense=True)
    a_loss = (ALPHA * logp - qn).mean()
    actor_opt.zero_grad()
    a_loss.backward()
    actor_opt.step()
    return a_loss.item(), c_losses[0].item(), c_losses[1].item()


print('ring: %d of %d transitions valid; batch %d, features %d wide, fc1.weight of a critic %s' % (
    len(env.replay), env.replay.steps * B, BATCH, width, tuple(critics[0].head.fc1.weight.shape)))
for k in range(3):
    print('update %d: actor loss %.6f, critic losses %.6f %.6f' % ((k + 1,) + update()))
g = critics[0].head.fc1.weight.grad
print('critic fc1.weight.grad %s: feature columns filled: %s, action columns filled: %s' % (
    tuple(g.shape), bool((g[:, :width] != 0).any()), bool((g[:, width:] != 0).any())))
if __name__ == '__main__':                                                   # (tools/time_featconv.py runs this file for its update() and closes the env itself)
    env.close()
