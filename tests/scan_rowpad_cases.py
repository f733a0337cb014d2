"""The cases of tests/test_gpu_scan_rowpad.py: short roll-outs of cars that stand still on hand-made maps at 2^-3 m, on the
shapes at which the row-padded byte cell table (csrc/f110_map.h: cell_elem_bp) and the march without a row clamp
(csrc/f110_scan.h: march_ident_pow2_fast<true>) can go wrong.  F110_SCAN_FORM and F110_SCAN_CODES are read once per process, so
each setting runs the whole list in a child process of its own:  python scan_rowpad_cases.py OUT.npz
One engine per max_range (the padding rows are the handle's); the maps are installed into it one after the other."""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
RES = 0.125             # 2^-3 m: 30 m are 240 cells, P = 248; 5 m are 40 cells, P = 48
CARS, BEAMS, T = 64, 1080, 3
HEIGHTS, WIDTHS = (1, 7, 8, 9, 23), (17, 33)
FIELD = 64

# name -> (max_range, H, W, map kind, poses kind)
CASES = {}
for _h in HEIGHTS:
    for _w in WIDTHS:
        CASES['free_h%d_w%d' % (_h, _w)] = (30.0, _h, _w, 'free', 'edge')
        CASES['zero_h%d_w%d' % (_h, _w)] = (30.0, _h, _w, 'zero', 'edge')
CASES['field'] = (30.0, FIELD, FIELD, 'field', 'field')
CASES['short_range'] = (5.0, 9, 17, 'free', 'edge')
# a max_range of 8 * 10^7 cells: no padding that large, so no byte table -- the launch asked for byte codes reads word codes
# (dt[-1, -1] = 0: a ray that leaves the map ends there instead of marching 10^7 m)
CASES['no_table'] = (1e7, 9, 17, 'zero', 'edge')
PAD_ROWS = {30.0: 248, 5.0: 48, 1e7: -1}     # the smallest multiple of 8 >= ceil(max_range / RES) + 2; -1: no byte table

# edge poses: the car of each index (the rest stands on the map's first and last row, yaw anywhere)
OUT_DOWN, OUT_UP = 0, 1             # on rows 0 and H - 1, facing straight out through rows -1 and H
ROW_M1, ROW_H = 2, 3                # standing on the border rows -1 and H: the march without a row clamp
ROW_M2, ROW_H1 = 4, 5               # on rows -2 and H + 1: the clamped twin
FAR_X = (6, 7)                      # 10^6 m away in x only, the row on the map: the column's range check, no row clamp
FAR_Y = (8, 9)                      # 10^6 m away in y: the clamped twin
N_SPECIAL = 10


def hand_map(H, W, kind):
    """dt of an H x W map with one occupied cell.  'free': in the middle, so dt[-1, -1] > eps and a ray that leaves the map keeps
    marching, dt[-1, -1] at a time, until max_range.  'zero': the last cell itself, dt[-1, -1] = 0: a ray that leaves the map
    ends there.  'field': on the middle of row 0 of a 64 x 64 field -- well over 254 distinct distances, so the cells of the
    upper half lie behind the 256-slot marker, and a ray that starts there takes a far step of ~60 cells."""
    r, c = np.mgrid[0:H, 0:W]
    r0, c0 = {'free': (H // 2, W // 2), 'zero': (H - 1, W - 1), 'field': (0, W // 2)}[kind]
    d2 = ((r - r0) ** 2 + (c - c0) ** 2).astype(np.int64)
    assert (d2[-1, -1] == 0) == (kind == 'zero') and (len(np.unique(d2)) > 600) == (kind == 'field')
    return RES * np.sqrt(d2.astype(np.float64))


def edge_poses(H, W):
    rng = np.random.default_rng(H * 100 + W)
    p = np.zeros((CARS, 1, 3))
    col = rng.integers(0, W, CARS)
    row = np.where(np.arange(CARS) % 2 == 0, 0, H - 1)
    p[:, 0, 0], p[:, 0, 1] = (col + 0.5) * RES, (row + 0.5) * RES
    p[:, 0, 2] = rng.uniform(-np.pi, np.pi, CARS)
    p[:N_SPECIAL, 0, 0] = 0.5 * RES                                    # (column 0: never the occupied cell's)
    p[OUT_DOWN, 0, 1], p[OUT_UP, 0, 1] = 0.5 * RES, (H - 0.5) * RES
    p[OUT_DOWN, 0, 2], p[OUT_UP, 0, 2] = -np.pi / 2, np.pi / 2
    for i, r_ in ((ROW_M1, -1), (ROW_H, H), (ROW_M2, -2), (ROW_H1, H + 1)):
        p[i, 0, 1] = (r_ + 0.5) * RES
    for i, sign in zip(FAR_X, (-1.0, 1.0)):
        p[i, 0, 0] = sign * 1e6
    for i, sign in zip(FAR_Y, (-1.0, 1.0)):
        p[i, 0, 1] = sign * 1e6
    return p


def field_poses():
    """Cars all over the field; car 0 near the top edge facing up: its own cell lies behind the marker (~60 cells from the
    obstacle), and the far step carries its rays vertically out of the map, into the padding rows."""
    rng = np.random.default_rng(64)
    p = np.zeros((CARS, 1, 3))
    p[:, 0, 0] = rng.uniform(1, FIELD - 1, CARS) * RES
    p[:, 0, 1] = rng.uniform(1, FIELD - 1, CARS) * RES
    p[:, 0, 2] = rng.uniform(-np.pi, np.pi, CARS)
    p[0, 0] = ((FIELD // 2 + 0.5) * RES, (FIELD - 3.5) * RES, np.pi / 2)
    return p


def rollout(eng, name):
    import torch
    _, H, W, kind, pk = CASES[name]
    eng.set_map_dt(hand_map(H, W, kind), RES, 0.0, 0.0)
    poses = torch.as_tensor(field_poses() if pk == 'field' else edge_poses(H, W), device='cuda')
    acts = torch.zeros((CARS, 1, 2), dtype=torch.float64, device='cuda')
    out = {'pad_rows': eng.scan_pad_rows()}
    eng.reset(poses)
    out['form'], out['codes_byte'], out['rows_lds'] = eng.scan_form()[0], int(eng.scan_codes()), int(eng.scan_rows())
    scans, col, ittc, dn, lk = [], [], [], [], []
    for _ in range(T):
        eng.step(acts)
        torch.cuda.synchronize()
        scans.append(eng.t['scans'].reshape(CARS, BEAMS).cpu().numpy().copy())
        col.append(eng.t['collisions'].cpu().numpy().copy())
        ittc.append(eng.t['in_collision'].cpu().numpy().copy())
        dn.append(eng.t['done'].cpu().numpy().copy())
        lk.append(eng.t['lookups'].cpu().numpy().copy())
    out.update(scans=np.stack(scans), sums=np.stack(scans).view(np.uint32).astype(np.int64).sum(2), col=np.stack(col), ittc=np.stack(ittc),
               done=np.stack(dn), lookups=np.stack(lk), rows=eng.t['noise_step'].cpu().numpy().copy(), err=eng.device_errors())
    return out


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    from red_gym_amd.engine import Engine
    res = {}
    for mr in sorted(PAD_ROWS):
        eng = Engine(num_envs=CARS, num_agents=1, num_beams=BEAMS, max_range=mr, autoreset=True, count_lookups=True)
        for name in CASES:
            if CASES[name][0] == mr:
                for k, v in rollout(eng, name).items():
                    res['%s/%s' % (name, k)] = v
        eng.close()
    np.savez(sys.argv[1], **res)
