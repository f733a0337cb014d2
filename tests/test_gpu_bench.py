"""bench.py's plain run on the GPU: the line carries the headline only, and --dump-outputs holds exactly what the last
timed step returned (replayed here, in this process, from the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_dumps_what_its_last_timed_step_returned(tmp_path):
    import torch
    from red_gym_amd import F110VecEnv, workload
    B, A, K, W = 512, 2, 3, 2
    out_dir = str(tmp_path / 'out')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT', 'F110_BENCH_BACKEND')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--envs', str(B), '--agents', str(A),
                        '--steps', str(K), '--warmup', str(W), '--dump-outputs', out_dir],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out['steps'] == K and out['warmup'] == W and out['ms_per_step'] > 0
    assert abs(out['value'] - B / (out['ms_per_step'] * 1e-3)) < 1e-6 * out['value']
    assert out['roofline'] is None and out['sustained'] is None and out['steady_state'] is None and 'cpu_baseline' not in out
    got = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    assert sum(a.nbytes for a in got.values()) <= 64 * 10 ** 6

    # the same workload in this process: reset, W warm-up steps, K steps, from the rank-0 shard's seeded inputs
    poses, acts = bench.rank_workload(0, B, A, 16)
    e = F110VecEnv(B, map=workload.EXAMPLE_MAP, map_ext='.png', num_agents=A, timestep=0.01, seed=12345, device=0,
                   autoreset=True)
    e.reset(torch.as_tensor(poses, device='cuda:0'))
    acts = torch.as_tensor(acts, device='cuda:0')
    for k in range(W + K):
        res = e.step(acts[k % 16])
    want = bench.sample_outputs(bench.step_outputs(res))
    e.close()
    assert sorted(got) == sorted(want) and 'obs_scans' in got
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name
