"""Times the reward shaper at 65 536 envs x 1 agent: (a) the reward kernel alone (f110_shaping_update), (b) the FILL render of
every ego scan alone, (c) a step with shaping on against a step plus the same render with shaping off:
    python tools/time_shaping.py [envs] [launches]
hipEvents around `launches` back-to-back calls after a warm-up, one process; the median of 5 such windows is reported and the
5 values are printed, the two forms of (c) alternating, so that the spread is visible.  Results: profiles/r07_shaping.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from red_gym_amd import F110VecEnv, workload
from red_gym_amd.lidar import LidarBitmap
from timing import report

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100
TLAD, VGAIN = 0.82461887897713965, 1.375
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
rl = workload.load_waypoints(workload.RACELINE)
wp = torch.as_tensor(np.ascontiguousarray(rl[:, [1, 2, 5]]), device=env.device)
for _ in range(150):   # spread the cars along the track
    env.step(env.pure_pursuit(wp, TLAD, VGAIN))
acts = env.pure_pursuit(wp, TLAD, VGAIN).clone()


env.shape_rewards()
for _ in range(3):
    env.step(acts)


def update_stepped():
    env.eng.t['current_time'].add_(env.timestep)   # (the kernel skips an env whose clock stands still; the add is ~2 us)
    env.eng.shaper.kernel()


a = report({'reward kernel alone (+ clock add)': update_stepped,
            'clock add alone': lambda: env.eng.t['current_time'].add_(env.timestep)}, N, 20, 5, name='(a) ')
b = report({'FILL render alone': env.eng.shaper.render}, N, 20, 5, name='(b) ')
env.shape_rewards(False)
to_img = LidarBitmap(1080, bg_color='black', draw_mode='FILL')
imgs = torch.empty((B, 256, 256), dtype=torch.uint8, device=env.device)


def off_step():
    obs = env.step(acts)[0]
    to_img(obs['scans'][:, 0], out=imgs)


off = report({'step + render, shaping off': off_step}, N, 20, 3, name='(c) ')
env.shape_rewards()
on = report({'step, shaping on': lambda: env.step(acts)}, N, 20, 3, name='(c) ')
env.shape_rewards(False)
off2 = report({'step + render, shaping off (again)': off_step}, N, 20, 3, name='(c) ')
print('%d envs x 1, %d launches per window' % (B, N))
assert env.eng.device_errors() == 0
env.close()
