"""bench.py --dump-outputs on CPU tensors: what a step hands its caller, converted to float32 / float64 without loss,
every env when it fits and otherwise the same fixed sample of envs in every array, under 64 MB in all."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def fake_result(B, A=1, nb=1080, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = {'ego_idx': 0, 'scans': torch.rand((B, A, nb), generator=g),
           'poses_x': torch.rand((B, A), generator=g, dtype=torch.float64),
           'collisions': torch.randint(0, 2, (B, A), generator=g, dtype=torch.uint8),
           'lap_counts': torch.randint(0, 5, (B, A), generator=g, dtype=torch.int32)}
    info = {'checkpoint_done': torch.randint(0, 2, (B, A), generator=g).bool(),
            'collision_idx': torch.randint(-1, A, (B, A), generator=g, dtype=torch.int32)}
    return obs, torch.full((B,), 0.01, dtype=torch.float64), torch.randint(0, 2, (B,), generator=g).bool(), info


def test_small_batch_is_dumped_whole_and_exact(tmp_path):
    res = fake_result(64, A=2)
    arrays = bench.sample_outputs(bench.step_outputs(res))
    assert sorted(arrays) == ['done', 'info_checkpoint_done', 'info_collision_idx', 'obs_collisions', 'obs_lap_counts',
                              'obs_poses_x', 'obs_scans', 'reward']
    assert arrays['obs_scans'].dtype == np.float32 and arrays['obs_poses_x'].dtype == np.float64
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert np.array_equal(arrays['obs_scans'], res[0]['scans'].numpy())
    assert np.array_equal(arrays['info_collision_idx'], res[3]['collision_idx'].numpy())
    assert np.array_equal(arrays['done'], res[2].numpy())
    bench.write_outputs(str(tmp_path / 'out'), arrays)
    for name, a in arrays.items():
        assert np.array_equal(np.load(str(tmp_path / 'out' / (name + '.npy'))), a)


def test_large_batch_is_a_fixed_sample_under_the_limit():
    for B, with_bitmaps in ((32768, False), (1024, True)):
        res = fake_result(B)
        bitmaps = torch.randint(0, 256, (B, 256, 256), dtype=torch.uint8) if with_bitmaps else None
        outs = bench.step_outputs(res, bitmaps)
        a1, a2 = bench.sample_outputs(outs), bench.sample_outputs(outs)
        assert sum(a.nbytes for a in a1.values()) <= 64 * 10 ** 6
        n = len(a1['reward'])
        assert 0 < n < B and all(len(a) == n for a in a1.values())
        assert all(np.array_equal(a1[k], a2[k]) for k in a1)           # the same rows every time
        # the same rows in every array: find them from the poses, check the scans against them
        rows = [int(np.flatnonzero(res[0]['poses_x'][:, 0].numpy() == x)[0]) for x in a1['obs_poses_x'][:3, 0]]
        assert rows == sorted(rows)
        assert np.array_equal(a1['obs_scans'][:3], res[0]['scans'][rows].numpy())
        if bitmaps is not None:
            assert a1['bitmaps'].dtype == np.float32 and np.array_equal(a1['bitmaps'][:3], bitmaps[rows].numpy())
