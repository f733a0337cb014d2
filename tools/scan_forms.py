"""Times the step path with the scan form this process was started with (F110_SCAN_FORM = classic | compact256 | compact512,
or unset: the rule of csrc/f110_scan_plan.h decides) and the fp32 rows it was started with (F110_SCAN_ROWS = lds | direct, or
unset: staged in LDS wherever the compact form of 256 slots runs), on a bundled map, optionally re-installed at another resolution (the
compact forms apply to power-of-two resolutions only; the bundled tracks but example_map are 0.05 m):
    F110_SCAN_FORM=compact256 python tools/scan_forms.py maps/berlin [--envs B] [--agents A] [--res 0.0625]
    F110_SCAN_FORM=compact256 F110_SCAN_ROWS=direct python tools/scan_forms.py     (compact256 has two columns: lds | direct)
    F110_SCAN_FORM=compact256 F110_SCAN_CODES=word python tools/scan_forms.py      (and, with its rows in LDS, byte | word cell codes)
Prints one line: map, form launched, how its fp32 rows are stored, which cell table its march reads, the map's shares of free cells behind the 256- and 512-slot images, ms/step, scan ms."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from red_gym_amd import F110VecEnv, workload  # noqa: E402
from red_gym_amd.maps import ASSETS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('map', nargs='?', default='example_map')
ap.add_argument('--envs', type=int, default=65536)
ap.add_argument('--agents', type=int, default=1)
ap.add_argument('--res', type=float, default=None, help='re-install the map\'s occupancy at this resolution')
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=50)
a = ap.parse_args()
B, A = a.envs, a.agents
env = F110VecEnv(B, map=os.path.join(ASSETS, a.map), num_agents=A, autoreset=True, count_lookups=True)
m = env.eng.map
res = m.resolution
if a.res is not None:
    res = a.res
    env.update_map_occupancy(m.free, res, m.orig_x, m.orig_y, 0.0)
if a.map == 'example_map' and a.res is None:
    poses = workload.spawn_poses(B, A)
else:  # random free cells with eight cells of clearance
    dt = env.eng.get_map_dt()
    rng = np.random.default_rng(0)
    free = np.argwhere(dt > 8 * res)
    pick = free[rng.integers(0, len(free), B * A)]
    poses = np.zeros((B, A, 3))
    poses[..., 0] = (m.orig_x + (pick[:, 1] + 0.5) * res).reshape(B, A)
    poses[..., 1] = (m.orig_y + (pick[:, 0] + 0.5) * res).reshape(B, A)
    poses[..., 2] = rng.uniform(0, 6.28, (B, A))
acts = torch.as_tensor(workload.action_pool(8, B, A), device=env.device)
env.reset(poses)
for k in range(a.warmup):
    env.step(acts[k % 8])
env.eng.t['lookups'].zero_()
env.eng.profile_begin(a.steps)
torch.cuda.synchronize()
t0 = time.perf_counter()
for k in range(a.steps):
    env.step(acts[k % 8])
torch.cuda.synchronize()
dt_s = time.perf_counter() - t0
ms, n = env.eng.profile_end()
lk = env.eng.t['lookups'].to(torch.int64).sum().item() / (a.steps * B * A)
form, share = env.eng.scan_form()
rows = 'lds' if env.eng.scan_rows() else 'direct'
codes = 'byte' if env.eng.scan_codes() else 'word'
print('%-12s res %.4f %6d x %d  asked %-10s form %3d  rows %-6s (asked %s)  codes %-4s (asked %s)  out256 %.4f out512 %.4f reach256 %.4f reach512 %.4f  ms/step %.4f scan_ms %.4f '
      'lookups/car-step %.0f' % (a.map, res, B, A, os.environ.get('F110_SCAN_FORM', '-'), form, rows, os.environ.get('F110_SCAN_ROWS', '-'), codes, os.environ.get('F110_SCAN_CODES', '-'), share[0], share[1], share[2], share[3],
                                 dt_s / a.steps * 1e3, ms / n, lk), flush=True)
env.close()
