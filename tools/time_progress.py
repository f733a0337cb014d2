"""Times the progress tracker (f110_progress_update) beside the planner's grid kernel, and the step with tracking on and off:
    python tools/time_progress.py [envs] [launches]
hipEvents around `launches` back-to-back launches after a warm-up, one process; every figure is printed twice (two rounds in
turn) so that the spread is visible.  Results: profiles/r06_progress.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from red_gym_amd import F110VecEnv, workload
from timing import window

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
TLAD, VGAIN = 0.82461887897713965, 1.375
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
rl = workload.load_waypoints(workload.RACELINE)
wp_np = np.ascontiguousarray(rl[:, [1, 2, 5]])
wp = torch.as_tensor(wp_np, device=env.device)
for _ in range(150):   # spread the cars along the track (the planner prepares its grid on the second call)
    env.step(env.pure_pursuit(wp, TLAD, VGAIN))
assert env.eng._plan_key is not None


def timed(fn, n=N, warm=20):
    for _ in range(warm):
        fn()
    return window(fn, n)


def kernels():
    out = torch.empty((B, 2), dtype=torch.float64, device=env.device)
    res = {}
    res['planner grid kernel'] = timed(lambda: env.eng.pure_pursuit(wp, TLAD, VGAIN, out=out))
    env.eng.tracker.install(wp_np)
    res['tracker, grid (1 raceline)'] = timed(env.eng.tracker.update)
    env.eng.tracker.install([wp_np], np.zeros(B, dtype=np.int32), grid=False)
    res['tracker, every segment, K = 1'] = timed(env.eng.tracker.update)
    env.eng.tracker.install([wp_np] * 8, np.arange(B, dtype=np.int32) % 8, grid=False)
    res['tracker, every segment, K = 8'] = timed(env.eng.tracker.update)
    env.eng.tracker.remove()
    return res


def steps():
    res = {}
    acts = env.pure_pursuit(wp, TLAD, VGAIN).clone()
    for tracking in (False, True):
        env.track_progress(wp_np if tracking else None)
        res['eager step, tracking %s' % ('on' if tracking else 'off')] = timed(lambda: env.step(acts), n=max(N, 300), warm=30) / 1e3
        env.capture_step()
        res['step_graph, tracking %s' % ('on' if tracking else 'off')] = timed(lambda: env.step_graph(acts), n=max(N, 300), warm=30) / 1e3
    env.track_progress(None)
    return res


for rnd in range(2):
    for name, us in kernels().items():
        print('round %d: %-34s %8.1f us per launch (%d cars, %d waypoints, %d launches)' % (rnd, name, us, B, wp.shape[0], N), flush=True)
for rnd in range(2):
    for name, ms in steps().items():
        print('round %d: %-34s %8.4f ms per step (%d envs x 1)' % (rnd, name, ms, B), flush=True)
assert env.eng.device_errors() == 0
env.close()
