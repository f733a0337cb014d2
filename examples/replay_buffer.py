"""Closed loop of shaper + path follower + replay buffer on the GPU: what the training loop of the reference's RL consumer does
around `replay_buffer.push(obs, action, reward, next_obs, done)` (src/SAL.py:996-1001), for many envs at once.
    python examples/replay_buffer.py [envs] [steps]
A random policy stands in for the SAC actor: its raw action goes through path_actions (which also hands it to the buffer), the
step pushes the transition behind the shaper, and sample() returns a batch as device tensors."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import F110VecEnv, workload

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.shape_rewards()
env.follow_paths()
env.record_replay(capacity=16 * B)              # 16 step slots for all envs
env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
gen = torch.Generator(device=env.device).manual_seed(0)
for k in range(STEPS):
    raw = torch.rand((B, 16), dtype=torch.float64, device=env.device, generator=gen) * 2.0 - 1.0
    obs, reward, done, info = env.step(env.path_actions(raw))
    if k % 10 == 9:
        print('step %3d: %d pushes, %d of %d transitions valid' % (k + 1, int(info['replay_count']), len(env.replay), env.replay.steps * B))
s, a, r, ns, d, ok = env.replay.sample(64)
print('batch: s %s %s, a %s, r %s, ns %s, d %s, ok %d of %d' % (tuple(s.shape), s.dtype, tuple(a.shape), tuple(r.shape), tuple(ns.shape),
                                                              tuple(d.shape), int(ok.sum()), ok.numel()))
s32 = env.replay.sample(64, dtype=torch.float32, scale=1.0 / 255.0)[0]
print('for the convolutions: s %s %s, max %.1f' % (tuple(s32.shape), s32.dtype, float(s32.max())))
held, raw_bytes = env.replay.bytes_held(), env.replay.bytes_raw()
print('bytes held %.1f MB against %.1f MB raw (%.1f x)' % (held / 1e6, raw_bytes / 1e6, raw_bytes / held))
env.close()
