"""The cases of tests/test_gpu_scan_rowbuf.py: the roll-out of scan_compact_cases.py on the shapes at which the row buffer of
the compact form (csrc/f110_scan_plan.h: scan_rowbuf_plan) takes another path.  F110_SCAN_FORM and F110_SCAN_ROWS are read once
per process, so each setting runs the whole list in a child process of its own:  python scan_rowbuf_cases.py OUT.npz [case,..]"""
import sys

import numpy as np

import scan_compact_cases as base

ROWBUF_CHUNKS = 11      # SCAN_ROWBUF_CHUNKS (tests/test_scan_rowbuf_plan_cpu.py holds the header to it)
CAP = 64 * ROWBUF_CHUNKS

# name -> (cars, beams, kind); kinds as in scan_compact_cases.rollout, 'd0' besides (see d0_poses)
CASES = {
    # up to 1 024 cars run 8 waves per car: every wave stages all its chunks
    'cars2': (2, 1080, 'plain'), 'cars3': (3, 1080, 'plain'),
    # launches with reset_only (steps 7 and 13): early returns
    'cars129': (129, 1080, 'masked_resets'),
    # whole cars (17 chunks: 6 direct, 11 staged) and the tail of 4-wave cars: part != 0, everything staged
    'cars4100': (4100, 1080, 'plain'),
    # a short last chunk: the end of a car's row abuts its neighbour's
    'beams64': (129, 64, 'plain'), 'beams65': (129, 65, 'plain'), 'beams1081': (129, 1081, 'masked_resets'),
    # at the buffer's capacity, one beam under, one over (one chunk more), one whole chunk more; MAX_CHUNKS
    'beams%d' % (CAP - 1): (129, CAP - 1, 'plain'), 'beams%d' % CAP: (129, CAP, 'plain'), 'beams%d' % (CAP + 1): (129, CAP + 1, 'plain'),
    'beams768': (129, 768, 'plain'), 'beams4096': (129, 4096, 'plain'),
    # the same counts on whole cars (above 2 048 cars a car is one wave), where the capacity decides what is staged:
    # j0 = 0, 0, 1, 1 and 53
    'whole%d' % (CAP - 1): (4100, CAP - 1, 'plain'), 'whole%d' % CAP: (4100, CAP, 'plain'), 'whole%d' % (CAP + 1): (4100, CAP + 1, 'plain'),
    'whole768': (4100, 768, 'plain'), 'whole4096': (2100, 4096, 'plain'),
    'side_tables': base.CASES['side_tables'], 'boundary': base.CASES['boundary'], 'noise_per_env': base.CASES['noise_per_env'],
    # cars whose own cell ends every beam at once (the loop in front of the march: direct stores, no write-out)
    'd0': (131, 1080, 'd0'),
}
D0_OCCUPIED, D0_OFF_MAP, D0_NAN = slice(1, None, 4), slice(2, None, 4), 7


def d0_poses(B):
    """The spawn poses with every fourth car on an occupied cell of the map, every fourth off the map and one on a NaN pose."""
    from red_gym_amd import workload
    from red_gym_amd.maps import load_map
    p = SPAWN(B, 1)
    m = load_map(workload.EXAMPLE_MAP + '.yaml', '.png')
    occ = np.argwhere(m.free[8:-8, 8:-8] == 0) + 8
    n_occ = len(range(B)[D0_OCCUPIED])
    pick = occ[np.linspace(0, len(occ) - 1, n_occ).astype(int)]
    p[D0_OCCUPIED, 0, 0] = m.orig_x + (pick[:, 1] + 0.5) * m.resolution
    p[D0_OCCUPIED, 0, 1] = m.orig_y + (pick[:, 0] + 0.5) * m.resolution
    p[D0_OFF_MAP, 0, 0] = m.orig_x - 40.0 - np.arange(len(range(B)[D0_OFF_MAP]))
    p[D0_NAN, 0, 0] = np.nan
    return p


SPAWN = None


def rollout(name):
    """scan_compact_cases.rollout on a case of this module."""
    global SPAWN
    from red_gym_amd import workload
    B, nb, kind = CASES[name]
    saved, SPAWN = dict(base.CASES), workload.spawn_poses
    try:
        base.CASES[name] = (B, nb, 'plain' if kind == 'd0' else kind)
        if kind == 'd0':
            workload.spawn_poses = lambda n, a, rank=0: d0_poses(n)
        return base.rollout(name)
    finally:
        workload.spawn_poses = SPAWN
        base.CASES.clear()
        base.CASES.update(saved)


if __name__ == '__main__':
    sys.path.insert(0, base.ROOT)
    res = {}
    for name in (sys.argv[2].split(',') if len(sys.argv) > 2 else CASES):
        for k, v in rollout(name).items():
            res['%s/%s' % (name, k)] = v
    from red_gym_amd import F110VecEnv, workload  # noqa: E402
    env = F110VecEnv(2, map=workload.EXAMPLE_MAP, num_agents=1)       # what this process was asked for, as the library read it
    res['rows_lds'] = int(env.eng.scan_rows(65536))
    env.close()
    np.savez(sys.argv[1], **res)
