"""Times the replay buffer at 65 536 and 4 096 envs x 1 agent, 256 x 256 images, beside a plain-torch baseline doing the same job
in the same process:
    python tools/time_replay.py [launches] [envs ...]
(a) the push (f110_replay_update: pack kernel + counter) against `copy_` of the raw lidar_bitmap into a [T + 1, B, rows, cols] uint8
ring, and against its byte floor: 72 KiB per env (64 read, 8 written) at the bandwidth a same-size `copy_` reaches in this run;
(b) draw + gather at n = 64 and n = 4 096, uint8 and fp32, against index_select of both frames from the raw ring (+ .float() * scale).
hipEvents around `launches` back-to-back calls after a warm-up; the median of 5 alternating windows is reported and the 5 values
are printed.  Results: profiles/r09_replay.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from red_gym_amd import F110VecEnv, workload
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
SIZES = [int(a) for a in sys.argv[2:]] or [65536, 4096]
T = 3            # step slots: the raw baseline ring costs (T + 1) * B * 64 KiB (17 GB at 65 536 envs)
ROWS = COLS = 256


for B in SIZES:
    env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.shape_rewards(rows=ROWS, cols=COLS)
    env.record_replay(steps=T)
    env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for _ in range(T + 2):
        env.step(acts)
    rp = env.replay
    bitmap = env.eng.shaper.buf['bitmap']
    raw_ring = torch.zeros((T + 1, B, ROWS, COLS), dtype=torch.uint8, device=env.device)
    packed_like = torch.empty((B, ROWS, COLS // 8), dtype=torch.uint8, device=env.device)
    half_a, half_b = torch.empty((B * 36 * 1024,), dtype=torch.uint8, device=env.device), torch.empty((B * 36 * 1024,), dtype=torch.uint8, device=env.device)
    state = {'k': 0}

    def push():
        env.eng.t['current_time'].add_(env.timestep)   # (a clock that stands still marks the env as not stepped; ~2 us)
        rp.kernel()

    def torch_push():
        env.eng.t['current_time'].add_(env.timestep)
        raw_ring[state['k'] % (T + 1)].copy_(bitmap)
        state['k'] += 1

    print('---- %d envs x 1, %d x %d, T = %d, %d launches per window' % (B, ROWS, COLS, T, N))
    a = report({'push: pack kernel + counter (+ clock add)': push, 'torch: copy_ of the raw bitmap into the ring (+ clock add)': torch_push,
                'copy_ of 36 KiB per env (reads + writes 72 KiB per env)': lambda: half_b.copy_(half_a),
                'clock add alone': lambda: env.eng.t['current_time'].add_(env.timestep)}, N, 10, 5, name='(a) ')
    moved = B * 72 * 1024
    copy_us = a['copy_ of 36 KiB per env (reads + writes 72 KiB per env)']
    bw = moved / (copy_us * 1e-6) / 1e12
    push_us = a['push: pack kernel + counter (+ clock add)'] - a['clock add alone']
    print('    copy bandwidth %.2f TB/s; byte floor of the push %.1f us; push without the clock add %.1f us = %.2f x the floor; torch baseline %.1f us'
          % (bw, copy_us, push_us, push_us / copy_us, a['torch: copy_ of the raw bitmap into the ring (+ clock add)'] - a['clock add alone']), flush=True)
    assert len(rp) > 0
    for n in (64, 4096):
        ridx = torch.randint(0, T * B, (n,), device=env.device)
        fr, env_i = ridx // B, ridx % B

        def torch_gather(f32):
            flat = raw_ring.view((T + 1) * B, ROWS, COLS)
            s, ns = flat.index_select(0, fr * B + env_i), flat.index_select(0, ((fr + 1) % (T + 1)) * B + env_i)
            if f32:
                s, ns = s.float().mul_(1.0 / 255.0).unsqueeze(1), ns.float().mul_(1.0 / 255.0).unsqueeze(1)
            return s, ns
        report({'draw + gather, uint8': lambda: rp.sample(n), 'draw + gather, fp32 * scale': lambda: rp.sample(n, dtype=torch.float32, scale=1.0 / 255.0),
                'torch: index_select of both frames, uint8': lambda: torch_gather(False),
                'torch: index_select + .float() * scale': lambda: torch_gather(True)}, max(N // 2, 5), 10, 5, name='(b) n = %4d ' % n)
    print('    bytes held %.1f MB against %.1f MB raw (%.1f x)' % (rp.bytes_held() / 1e6, rp.bytes_raw() / 1e6, rp.bytes_raw() / rp.bytes_held()), flush=True)
    assert env.eng.device_errors() == 0
    del raw_ring, half_a, half_b, packed_like
    env.close()
    del env, rp, bitmap
    torch.cuda.empty_cache()
