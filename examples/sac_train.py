"""The training loop of the reference's RL consumer (main(), src/SAL.py:975-1019) for many envs at once, everything on the GPU:
    python examples/sac_train.py [envs] [steps] [batch] [update_after] [update_every] [max_steps] [nstep] [auto] [device] [per] [stack3] [clip10]
    select_action (the policy on the shaper's bitmap) -> path_actions (SAL's action decode and MPC step, which also hands the raw
    action to the ring) -> step (scan, shaper, the ring's push) -> after update_after steps, every update_every steps, one SACAgent
    update replayed from a graph: the batch is drawn on the device, the losses stay there.  The episodes are kept on the GPU too
    (track_episodes: max_steps ends an episode the env never ends, as the reference's `for st in range(max_steps)` does): the
    `Episode ... Reward=...` lines main() prints come from the log of finished episodes, read where the losses are printed.
The defaults are small, so that it finishes in seconds; the reference's are batch 64, update_after 1000, update_every 50, max_steps
2000.  The loss
tensor is read (one synchronisation) only where it is printed.  With a trailing `auto` the temperature is learnt on the device
(SACAgent(alpha='auto'): its step is part of the replayed graph) and alpha is printed beside the losses.  With a trailing `device`
the policy's Gaussian draws are made on the device (SACAgent(draws='device'): NumPy's Philox normals per env and call, the fills part of
the replayed graph, the counters part of state_dict()) and the number of calls per stream is printed at the end.  At the end the actor is saved under the reference's keys, as main()
saves sac_actor.pth.  With nstep > 1 (a seventh number) the targets are built on truncated n-step returns walked through the ring on
the device (SACAgent(nstep=k)), and the mean span of the last sampled batch is printed beside the losses: below k where episodes end,
resets intervene or the newest push cuts a walk short.  With a trailing `per` the ring keeps priorities (record_replay(priorities=True): an
exact integer sum tree on the device) and the agent draws in proportion to them, weighs the critics' loss and writes the new TD errors
back, all inside the replayed graph (SACAgent(per=True)); the mean importance weight of the last batch and beta are printed beside the
losses.  With a trailing `stack3` (any count up to 8) the networks see the last three frames of an env (SACAgent(stack=3): conv1 has three
input channels, read as three rows of the ring's frame tensor, no frame is stored twice): the policy acts on the ring's newest stacks
(act_from) and the mean depth of the last batch's stacks is printed beside the losses -- below 3 at the start of an episode, where the
first frame fills the stack.  With a trailing `clip10` (any positive number, or `clipinf` for the non-finite guard alone) every
optimizer clips the global norm of its network's gradients at 10 on the device and skips a step whose norm is not finite
(SACAgent(max_grad_norm=10)): the three norms (actor, critic 1, critic 2) and the skipped-step counters are printed beside the losses."""
import os
import sys
import tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import F110VecEnv, SACAgent, workload
from red_gym_amd.episodes import REASONS

arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
B, STEPS, BATCH, UPDATE_AFTER, UPDATE_EVERY, MAX_STEPS = arg(1, 64), arg(2, 48), arg(3, 64), arg(4, 16), arg(5, 4), arg(6, 12)
AD = 16
NSTEP = int(sys.argv[7]) if len(sys.argv) > 7 and sys.argv[7].isdigit() else 1
AUTO, DEVICE, PER = 'auto' in sys.argv[7:], 'device' in sys.argv[7:], 'per' in sys.argv[7:]
STACK = ([int(a[5:]) for a in sys.argv[7:] if a.startswith('stack') and a[5:].isdigit()] + [0])[0]      # 0: not asked for
CLIP = ([float(a[4:]) for a in sys.argv[7:] if a.startswith('clip') and a[4:]] + [None])[0]               # None: not asked for
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.shape_rewards()
env.follow_paths()
env.record_replay(capacity=16 * B, action_dim=AD, priorities=True if PER else None)
env.track_episodes(MAX_STEPS + torch.arange(B, dtype=torch.int32) % 4)   # staggered: envs spawned together do not end together
dev, cfg = env.device, env.eng.shaper.cfg
torch.manual_seed(0)
agent = SACAgent(action_dim=AD, rows=cfg.rows, cols=cfg.cols, device=dev, **(dict(alpha='auto') if AUTO else {}),
                 **(dict(draws='device', seed=0) if DEVICE else {}), nstep=NSTEP, per=PER, **(dict(stack=STACK) if STACK else {}),
                 max_grad_norm=CLIP)
raw = torch.zeros((B, AD), dtype=torch.float64, device=dev)                    # the policy's action, written in place
obs, reward, done, info = env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=dev))
total = torch.zeros((B,), dtype=torch.float64, device=dev)
updates = printed = 0
for step in range(1, STEPS + 1):
    if STACK:
        agent.act_from(env.replay, out=raw)                                    # the newest STACK frames of every env, from the ring
    else:
        agent.select_action(info['lidar_bitmap'], out=raw)
    obs, reward, done, info = env.step(env.path_actions(raw))
    total += reward
    if step > UPDATE_AFTER and step % UPDATE_EVERY == 0:
        if updates == 0:
            agent.capture_update(env.replay, BATCH)
        losses = agent.update_graph()
        updates += 1
        if updates % 4 == 1:
            print('step %3d, update %2d: losses (actor, critic 1, critic 2) %s%s%s%s%s%s' % (
                step, updates, ' '.join('%.6f' % v for v in losses.tolist()), ', alpha %.9f' % agent.alpha.item() if AUTO else '',
                ', mean span %.3f of %d' % (agent.sample['span'].double().mean().item(), NSTEP) if NSTEP > 1 else '',
                ', mean weight %.4f, beta %.6f' % (agent.sample['weight'].mean().item(), env.replay.priorities.beta) if PER else '',
                ', mean depth %.3f of %d' % (agent.sample['depth'].double().mean().item(), STACK) if STACK > 1 else '',
                ', gradient norms %s clipped at %g, steps skipped %s' % (' '.join('%.4g' % v for v in agent.grad_stats()['norm'].tolist()), CLIP,
                                                                        agent.grad_stats()['steps_skipped'].tolist()) if CLIP else ''))
            count = int(info['episodes_finished'].item())
            rec = {k: v.tolist() for k, v in env.episodes.finished(last=min(count - printed, 4)).items()}   # (a few of the new ones)
            for i in range(len(rec['env'])):
                print('Episode %d Reward=%.2f  (env %d, %d steps, %s)' % (count - len(rec['env']) + i, rec['ret'][i], rec['env'][i], rec['length'][i],
                                                                        REASONS[rec['reason'][i]]))
            printed = count
print('%d steps of %d envs, %d updates of batch %d, captures %d; %d of %d transitions valid; mean reward per step %.4f' % (
    STEPS, B, updates, BATCH, agent.captures, len(env.replay), env.replay.steps * B, float(total.mean()) / STEPS))
if DEVICE:
    print('draws made on the device: calls (acting, next_action, new_action, unused) %s' % agent.source.calls())
s = env.episodes.summary(last=100)
print('episodes: %d finished; the last %d: mean return %.3f, mean length %.1f; done %.0f %%, limit %.0f %%, reset %.0f %%'
      % (s['count'], s['n'], s['mean_return'], s['mean_length'], 100 * s['done'], 100 * s['limit'], 100 * s['reset']))
path = os.path.join(tempfile.mkdtemp(), 'sac_actor.pth')
torch.save({k: v.cpu() for k, v in agent.actor_state_dict().items()}, path)
print('actor saved as %s (%d tensors under the reference\'s keys)' % (path, len(torch.load(path))))
env.close()
