"""The SAC wrapper's whole step on the GPU (src/SAL.py, SACF110Env.step) for a batch of envs, closed loop: the policy's 16 numbers
per env -- random here -- become a path, the path an MPC action, the action a step, the step a FILL bitmap and a shaped reward.
Time step 0.015 as in SAL's main.
    python examples/path_actions.py [envs] [steps]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import F110VecEnv, workload

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 300
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, timestep=0.015, autoreset=True)
env.shape_rewards()
env.follow_paths()
obs, reward, done, info = env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
gen = torch.Generator(device=env.device).manual_seed(0)
raw = torch.empty((B, 16), dtype=torch.float64, device=env.device)
total = torch.zeros((B,), dtype=torch.float64, device=env.device)
replans = torch.zeros((B,), dtype=torch.int64, device=env.device)
for k in range(STEPS):
    raw.uniform_(-1.0, 1.0, generator=gen)          # the policy: info['lidar_bitmap'] -> 16 numbers
    obs, reward, done, info = env.step(env.path_actions(raw))
    total += reward
    replans += info['path_replanned']
print('%d envs, %d steps: mean return %.2f, paths decoded per env %.2f, mean waypoint index %.2f, mean |mpc_accel| %.2f'
      % (B, STEPS, float(total.mean()), float(replans.double().mean()), float(info['path_index'].double().mean()),
         float(info['mpc_accel'].abs().mean())))
assert env.eng.device_errors() == 0
env.close()
