"""The reward of the reference's RL consumer (src/SAL.py, SACF110Env._calculate_rewards) for every env, computed on the GPU:
the batched pure-pursuit planner drives every env round the example track while the reward shaper pays, per step, a
collision term and a centering term read off the FILL bitmap of the previous scan and a progress term for the metres moved.

    python examples/bitmap_rewards.py [num_envs] [steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gym_amd import F110VecEnv, workload  # noqa: E402


def main():
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    env = F110VecEnv(num_envs, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    rl = workload.load_waypoints(workload.RACELINE)
    waypoints = torch.as_tensor(np.ascontiguousarray(rl[:, [1, 2, 5]]), device=env.device)   # x, y, speed
    env.shape_rewards()                                   # SAL's numbers: 256 x 256 image, 10 px / m, weights -100 / 10 / 2
    obs, reward, done, info = env.reset(torch.as_tensor(workload.spawn_poses(num_envs, 1), device=env.device))
    sums = {k: torch.zeros(num_envs, dtype=torch.float64, device=env.device)
            for k in ('reward_collision', 'reward_progress', 'reward_centering')}
    ret = torch.zeros(num_envs, dtype=torch.float64, device=env.device)
    for _ in range(steps):
        actions = env.pure_pursuit(waypoints, 0.82461887897713965, 1.375)
        obs, reward, done, info = env.step(actions)       # reward [num_envs]: the shaped total; info['lidar_bitmap']: the observation
        ret += reward
        for k in sums:
            sums[k] += info[k]
    for e in range(num_envs):
        print('env %d: mean reward %.3f per step (collision %.3f, progress %.3f, centering %.3f)'
              % (e, float(ret[e]) / steps, float(sums['reward_collision'][e]) / steps, float(sums['reward_progress'][e]) / steps,
                 float(sums['reward_centering'][e]) / steps))
    env.close()


if __name__ == '__main__':
    main()
