"""One complete SACAgent.update (src/SAL.py:521-580) from the replay ring on the GPU, in the reference's order, the parameter update
included, by red_gym_amd.SACAgent:
    python examples/sac_update.py [envs] [steps] [batch]
    sample_frames_dev -> Trunk (conv1 from the ring's bits, conv2, conv3: featconv) -> Dense (fc1 + ReLU) -> PolicyHead   (the actor)
                                                                                     -> twin_q / td_target, dense=True (the critics' fc1, fc2, min, target)
    -> critic_loss, actor_loss (csrc/f110_sacloss.h: each loss and its gradients in one launch); SacAdam.step() per network, which also
    moves the target critics (:575-578).
The batch is drawn on the device from the agent's own draw counter, and the three losses stay in one device tensor: the update never
waits for the host, which is what lets examples/sac_train.py replay it from a graph.  A random policy fills the ring first.  The two
critic losses go to one backward pass (their parameters are disjoint, so each critic gets the gradient the reference's two passes give
it).  A target critic moves in the pass that updates its critic, before the actor's loss where the reference moves it after: the
actor's loss reads the critics, never the targets, so the update computes the same."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import F110VecEnv, SACAgent, workload

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
BATCH = int(sys.argv[3]) if len(sys.argv) > 3 else 64
AD = 16
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.shape_rewards()
env.follow_paths()
env.record_replay(capacity=16 * B, action_dim=AD)
dev, cfg = env.device, env.eng.shaper.cfg
torch.manual_seed(0)
agent = SACAgent(action_dim=AD, rows=cfg.rows, cols=cfg.cols, device=dev)          # SACAgent's defaults (:478-480); on = 255: the raw images (:536)
actor, critics, targets = agent.actor, agent.critics, agent.targets

gen = torch.Generator(device=dev).manual_seed(0)
env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=dev))
for k in range(STEPS):
    raw = torch.rand((B, AD), dtype=torch.float64, device=dev, generator=gen) * 2.0 - 1.0
    env.step(env.path_actions(raw))


def update():
    """One eager update -> (actor loss, critic loss 1, critic loss 2) as floats (the one synchronisation is this read)."""
    return tuple(agent.update(env.replay, BATCH).tolist())


print('ring: %d of %d transitions valid; batch %d, features %d wide, fc1.weight of a critic %s' % (
    len(env.replay), env.replay.steps * B, BATCH, agent.width, tuple(critics[0].head.fc1.weight.shape)))
for k in range(3):
    print('update %d: actor loss %.6f, critic losses %.6f %.6f' % ((k + 1,) + update()))
g = critics[0].head.fc1.weight.grad
print('critic fc1.weight.grad %s: feature columns filled: %s, action columns filled: %s' % (
    tuple(g.shape), bool((g[:, :agent.width] != 0).any()), bool((g[:, agent.width:] != 0).any())))
if __name__ == '__main__':                                                   # (tools/time_featconv.py runs this file for its update() and closes the env itself)
    env.close()
