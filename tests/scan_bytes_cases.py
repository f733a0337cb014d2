"""The cases of tests/test_gpu_scan_bytes.py: the roll-out of scan_compact_cases.py on the shapes at which the byte cell table
of the compact form of 256 slots (csrc/f110_map.h: cell_elem_b; csrc/f110_scan.h: scan_kernel<.., 256, true, true>) can go
wrong.  F110_SCAN_FORM and F110_SCAN_CODES are read once per process, so each setting runs the whole list in a child process
of its own:  python scan_bytes_cases.py OUT.npz [case,..]"""
import sys

import numpy as np

import scan_rowbuf_cases as rb

base = rb.base
RES = 0.125             # the hand-made maps' resolution, 2^-3
WIDTHS, HEIGHTS = (15, 16, 17, 31, 33), (9, 23)     # around one and two 16-column strips; 16 and 32 padded rows
CARS = 64

# from the row buffer's list: 8 waves per car, masked resets, whole cars plus the 4-wave tail, a short last chunk, the ranks
# around both markers with the escape cell (a map installed from a host table), cars whose own cell ends every beam
FROM_ROWBUF = ('cars2', 'cars3', 'cars129', 'cars4100', 'beams65', 'boundary', 'd0')
# name -> (cars, beams, kind); 'widths': edge_poses on hand_map(H, W), 'far_car': far_poses on it
CASES = {name: rb.CASES[name] for name in FROM_ROWBUF}
for _h in HEIGHTS:
    for _w in WIDTHS:
        CASES['widths_w%d_h%d' % (_w, _h)] = (CARS, 1080, 'widths')
    CASES['far_car_h%d' % _h] = (CARS, 1080, 'far_car')
FAR_W = 17


def case_map(name):
    return (FAR_W if name.startswith('far_car') else int(name.split('_w')[1].split('_')[0])), int(name.split('_h')[1])


def hand_map(H, W):
    """(d2, dt, None) of an H x W map with one occupied cell in the middle: every other cell is free, the last one included, so
    dt[-1, -1] > eps and a ray that leaves the map keeps marching, dt[-1, -1] at a time, until max_range (240 cells)."""
    r, c = np.mgrid[0:H, 0:W]
    d2 = ((r - H // 2) ** 2 + (c - W // 2) ** 2).astype(np.int64)
    assert d2[-1, -1] > 0 and len(np.unique(d2)) < 254                # every rank inside the 256-slot image
    return d2, RES * np.sqrt(d2.astype(np.float64)), None


def edge_poses(H, W, n=CARS):
    """n cars on the cell centres of the first and last column and the first and last row, yaw anywhere: their rays leave the
    map on all four sides, through columns -1 and W, the border strips and the columns beyond +-16 (the range check's)."""
    rng = np.random.default_rng(H * 100 + W)
    p = np.zeros((n, 1, 3))
    for i in range(n):
        side, t = i % 4, rng.random()
        col = (0, W - 1, int(t * W), int(t * W))[side]
        row = (int(t * H), int(t * H), 0, H - 1)[side]
        p[i, 0, 0], p[i, 0, 1] = (col + 0.5) * RES, (row + 0.5) * RES
    p[:, 0, 2] = rng.uniform(-np.pi, np.pi, n)
    p[:4, 0, 2] = (np.pi, 0.0, -np.pi / 2, np.pi / 2)                 # straight out through each side
    return p


def far_poses(H, W, n=CARS):
    """Poses 10^6 m (the fast march: offsets outside the table on either side, negative ones wrapped) and 10^12 m (the clamped
    twin) from the map, on both axes and both signs, among cars on the map's edge."""
    p = edge_poses(H, W, n)
    k = 0
    for dist in (1e6, 1e12):
        for axis in (0, 1):
            for sign in (-1.0, 1.0):
                for both in (False, True):
                    p[4 + k, 0, axis] = sign * dist
                    if both:
                        p[4 + k, 0, 1 - axis] = -sign * dist
                    k += 1
    return p


def rollout(name):
    """scan_compact_cases.rollout on a case of this module."""
    B, nb, kind = CASES[name]
    if kind not in ('widths', 'far_car'):
        return rb.rollout(name)
    W, H = case_map(name)
    saved = dict(base.CASES), base.RES, base.boundary_map, base.boundary_poses
    try:
        base.CASES[name] = (B, nb, 'boundary')                        # a map installed from a host table, cars that stand still
        base.RES = RES
        base.boundary_map = lambda: hand_map(H, W)
        base.boundary_poses = (lambda n: far_poses(H, W, n)) if kind == 'far_car' else (lambda n: edge_poses(H, W, n))
        return base.rollout(name)
    finally:
        base.CASES.clear()
        base.CASES.update(saved[0])
        base.RES, base.boundary_map, base.boundary_poses = saved[1:]


if __name__ == '__main__':
    sys.path.insert(0, base.ROOT)
    res = {}
    for name in (sys.argv[2].split(',') if len(sys.argv) > 2 else CASES):
        for k, v in rollout(name).items():
            res['%s/%s' % (name, k)] = v
    from red_gym_amd import F110VecEnv, workload  # noqa: E402
    env = F110VecEnv(2, map=workload.EXAMPLE_MAP, num_agents=1)       # what this process was asked for, as the library read it
    res['rows_lds'] = int(env.eng.scan_rows(65536))
    res['codes_byte'] = int(env.eng.scan_codes(65536))
    env.close()
    np.savez(sys.argv[1], **res)
