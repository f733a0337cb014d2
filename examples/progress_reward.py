"""Metres driven per env, measured on the GPU: the batched pure-pursuit planner drives every env round the example track
while the progress tracker follows the cars along the raceline.  `progress_delta` is what a learning loop would pay as a
reward (the reference's own reward is the constant time step, f110_env.py:292).

    python examples/progress_reward.py [num_envs] [steps]
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
    env.track_progress(waypoints)
    obs, _, done, info = env.reset(torch.as_tensor(workload.spawn_poses(num_envs, 1), device=env.device))
    ret = torch.zeros(num_envs, dtype=torch.float64, device=env.device)
    for _ in range(steps):
        actions = env.pure_pursuit(waypoints, 0.82461887897713965, 1.375)
        obs, _, done, info = env.step(actions)
        ret += info['progress_delta'][:, 0]          # the reward: metres along the raceline this step
    lap = info['lap_length'].cpu().numpy()
    for e in range(num_envs):
        print('env %d: %.2f m since its last reset (%.2f laps of %.2f m), %.3f m off the line, return %.2f m'
              % (e, float(info['progress'][e, 0]), float(info['progress'][e, 0]) / lap[e], lap[e],
                 float(info['frenet_d'][e, 0]), float(ret[e])))
    env.close()


if __name__ == '__main__':
    main()
