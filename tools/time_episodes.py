"""Times the episode tracker's update (f110_episodes_update: three kernels) at 4 096 and 65 536 envs x 1 agent with none, a few per
cent and all of the envs closing their episode in the update, and beside it the reward shaper's kernel from the same process:
    python tools/time_episodes.py [launches] [windows] [envs ...]
hipEvents around `launches` back-to-back calls, `windows` windows per contestant (default 21) in turn after a warm-up of 20 calls
each; the median of the windows is reported, every window is printed.  No step runs between the calls: what makes an update do its
work is put there by two small fills in front of it (the clocks move on, every episode is open again; `done` holds the closing
pattern), which are timed alone as well.  Results: profiles/r21_episodes.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from red_gym_amd import F110VecEnv, workload
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 21
SIZES = [int(v) for v in sys.argv[3:]] or [4096, 65536]
for B in SIZES:
    env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
    acts = torch.as_tensor(workload.action_pool(1, B, 1)[0], device=env.device)
    env.shape_rewards()
    env.track_episodes(0, log=4096)
    for _ in range(3):
        env.step(acts)
    clock, done, is_open = env.eng.t['current_time'], env.eng.t['done'], env.episodes.buf['ep_open']
    e = torch.arange(B, device=env.device)
    patterns = {'none closing': e < 0, '3 %% closing (every 32nd env)': e % 32 == 0, 'all closing': e >= 0}

    def fills():
        clock.add_(env.timestep)
        is_open.fill_(1)

    def update():
        fills()
        env.episodes.kernel()

    def shaper():
        clock.add_(env.timestep)
        env.eng.shaper.kernel()

    print('%d envs x 1, %d launches per window, %d windows' % (B, N, ROUNDS))
    for label, mask in patterns.items():
        done.copy_(mask)
        count0 = int(env.episodes.buf['count'].item())
        report({'episodes update, %s (+ 2 fills)' % (label % ()): update}, N, 20, ROUNDS, name='%6d ' % B)
        closed = int(env.episodes.buf['count'].item()) - count0
        assert closed == int(mask.sum().item()) * (20 + N * ROUNDS), (label, closed)
    done.zero_()
    report({'the 2 fills alone': fills, 'shaper kernel (+ clock add)': shaper, 'clock add alone': lambda: clock.add_(env.timestep)},
           N, 20, ROUNDS, name='%6d ' % B)
    assert env.eng.device_errors() == 0
    env.close()
