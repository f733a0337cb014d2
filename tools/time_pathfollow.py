"""Times the path follower's two kernels at 65 536 envs x 1 agent and 4 096 x 1: (a) the act kernel (f110_pathfollow_act) with every
env decoding a new path and with none, (b) the advance kernel (f110_pathfollow_update), (c) a step with the follower on
(path_actions + step) against the plain step:
    python tools/time_pathfollow.py [launches]
hipEvents around `launches` back-to-back calls after a warm-up, one process; the median of 5 such windows is reported and the 5
values are printed.  Results: profiles/r08_pathfollow.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from red_gym_amd import F110VecEnv, workload
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100


for B in (65536, 4096):
    env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True, timestep=0.015)
    env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
    env.follow_paths()
    raw = torch.as_tensor(np.random.default_rng(0).uniform(-1, 1, (B, 16)), device=env.device)
    out = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    fo = env.eng.follower
    for _ in range(30):                       # moving cars: the QPs see velocities and paths of a run
        env.step(env.path_actions(raw, out=out))
    idx = fo.buf['path_index']

    def act_all():
        idx.fill_(-1)                         # (the fill is ~2 us)
        fo.act(raw, out)

    report({'%5d x 1 (a) act, every env decodes (+ index fill)' % B: act_all}, N, 20, 5)
    idx.zero_()
    report({'%5d x 1 (a) act, no env decodes' % B: lambda: fo.act(raw, out)}, N, 20, 5)

    def advance():
        env.eng.t['current_time'].add_(env.timestep)   # (the kernel skips an env whose clock stands still; the add is ~2 us)
        fo.kernel()

    report({'%5d x 1 (b) advance (+ clock add)' % B: advance}, N, 20, 5)
    env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
    acts = env.path_actions(raw).clone()
    report({'%5d x 1 (c) path_actions + step, follower on' % B: lambda: env.step(env.path_actions(raw, out=out))}, N, 20, 3)
    env.follow_paths(False)
    report({'%5d x 1 (c) step, follower off' % B: lambda: env.step(acts)}, N, 20, 3)
    assert env.eng.device_errors() == 0
    env.close()
print('%d launches per window' % N)
