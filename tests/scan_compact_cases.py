"""The cases of tests/test_gpu_scan_compact.py.  F110_SCAN_FORM is read once per process, so each form runs the whole list in
a child process of its own:  python scan_compact_cases.py OUT.npz [case,case..]  rolls the cases out under the form of its
environment (unset: the rule decides) and records, per case, what a caller sees (fp32 scans, collisions, done, the look-up
counts), the device error word, and the form, the shares and the launch epoch before and after the first reset."""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
T = 40
RES = 0.0625

# name -> (cars, beams, kind)
CASES = {
    'cars2': (2, 1080, 'plain'), 'cars3': (3, 1080, 'plain'), 'cars129': (129, 1080, 'masked_resets'), 'cars4100': (4100, 1080, 'plain'),
    'beams64': (129, 64, 'plain'), 'beams65': (129, 65, 'plain'), 'beams1081': (129, 1081, 'masked_resets'),
    'side_tables': (12, 1080, 'side'), 'boundary': (48, 1080, 'boundary'),
    # every env on its own noise generator (ScanArgs::env_noise), an odd car count with a split tail
    'noise_per_env': (4099, 1080, 'noise_per_env'),
    # a handle the rule can route: at 32 768 cars the first reset of all envs learns the map's shares
    'cars32768': (32768, 1080, 'plain'),
}
# the rule's child runs these: example_map, which it routes, and berlin re-installed at 0.0625 m, whose road is too wide
RULE_CASES = ('cars32768', 'wide')
WIDE = (32768, 1080, 'wide')
HEAD = 128      # cars whose scans are kept at the KEEP steps
KEEP = (0, 1, 7, 8, 13, 14, 20, T - 1)   # steps whose scans are kept (the first HEAD cars; every step and car: one sum of bit patterns)


def boundary_map():
    """A 96 x 96 table of squared distances (in cells) whose distinct values are 0 .. 599, so that a cell's rank IS its value:
    the first rows hold every value once, the rest cycles through the ranks around both compact markers (S - 2 is the first
    rank behind the marker of S) and the classic form's, with one escape cell (not resolution * sqrt(integer)); a border of 0."""
    H = W = 96
    targets = np.array([252, 253, 254, 255, 256, 508, 509, 510, 511, 512, 40, 130])
    d2 = targets[(np.arange(H * W) * 5 + np.arange(H * W) // W) % len(targets)].reshape(H, W).astype(np.int64)
    d2[0, :] = d2[-1, :] = 0
    d2[:, 0] = d2[:, -1] = 0
    d2[2:10, 4:79] = np.arange(600).reshape(8, 75)
    dt = RES * np.sqrt(d2.astype(np.float64))
    esc = (40, 41)
    dt[esc] = 0.7123
    return d2, dt, esc


def boundary_poses(n):
    rng = np.random.default_rng(5)
    p = np.zeros((n, 1, 3))
    p[:, 0, 0] = rng.uniform(20, 76, n) * RES
    p[:, 0, 1] = rng.uniform(20, 76, n) * RES
    p[:, 0, 2] = rng.uniform(-np.pi, np.pi, n)
    p[0, 0, :2] = (41.5 * RES, 40.5 * RES)   # a car ON the escape cell: every beam's first look-up reads it
    return p


def rollout(name):
    import torch
    from red_gym_amd import F110VecEnv, workload
    B, nb, kind = WIDE if name == 'wide' else CASES[name]
    kw = {}
    steps = 3 if kind == 'wide' else T
    if kind == 'side':
        sys.path.insert(0, TESTS)
        from side_distance_cases import batch
        env_par, poses, acts = batch(B, 1)
        kw = dict(params=env_par, side_distances='per_env')
    else:
        poses, acts = workload.spawn_poses(B, 1), workload.action_pool(8, B, 1)
    if kind == 'noise_per_env':
        kw = dict(noise_source='per_env', seed=[1000 + 7 * e for e in range(B)])
    map_path = workload.EXAMPLE_MAP
    if kind == 'wide':
        from red_gym_amd.maps import ASSETS
        map_path = os.path.join(ASSETS, 'maps', 'berlin')
    env = F110VecEnv(B, map=map_path, num_agents=1, autoreset=True, num_beams=nb, count_lookups=True, **kw)
    if kind == 'boundary':
        env.eng.set_map_dt(boundary_map()[1], RES, 0.0, 0.0)
        poses = boundary_poses(B)
        acts = acts * 0.0
    if kind == 'wide':      # the same mask at a power-of-two resolution; cars on random free cells with eight cells of clearance
        m = env.eng.map
        env.update_map_occupancy(m.free, RES, m.orig_x, m.orig_y, 0.0)
        rng = np.random.default_rng(0)
        free = np.argwhere(env.eng.get_map_dt() > 8 * RES)
        pick = free[rng.integers(0, len(free), B)]
        poses = np.zeros((B, 1, 3))
        poses[:, 0, 0], poses[:, 0, 1] = m.orig_x + (pick[:, 1] + 0.5) * RES, m.orig_y + (pick[:, 0] + 0.5) * RES
        poses[:, 0, 2] = rng.uniform(0, 6.28, B)
    before = env.eng.scan_form()
    epoch0 = env.eng.launch_epoch()
    env.reset(poses)
    form, shares = env.eng.scan_form()
    out = {'form': form, 'form_before': before[0], 'shares_before': np.array(before[1]), 'shares': np.array(shares),
           'epoch_moved': int(env.eng.launch_epoch() != epoch0)}
    sums, col, dn, lk = [], [], [], []
    for k in range(steps):
        if kind == 'masked_resets' and k in (7, 13):     # a launch with reset_only: a third of the envs go back to their spawn
            mask = torch.as_tensor(((np.arange(B) + k) % 3 == 0).astype(np.uint8), device='cuda')   # (and onto noise row 0)
            env.reset(poses, mask)
        obs, _, done, _ = env.step(torch.as_tensor(acts[k % 8], device='cuda'))
        sc = obs['scans'].reshape(B, nb)
        sums.append(sc.view(torch.int32).to(torch.int64).sum(1).cpu().numpy())   # (summed on the device: 141 MB a step at 32 768 cars)
        if k in KEEP:
            out['scans%d' % k] = sc[:HEAD].cpu().numpy().copy()
        col.append(np.stack([obs['collisions'].cpu().numpy(), env.eng.t['in_collision'].cpu().numpy().astype(np.float64)]))
        dn.append(done.cpu().numpy().copy())
        lk.append(env.eng.t['lookups'].cpu().numpy().copy())
    out.update(sums=np.stack(sums), col=np.stack(col), done=np.stack(dn), lookups=np.stack(lk),
               rows=env.eng.t['noise_step'].cpu().numpy().copy(), err=env.eng.device_errors())
    env.close()
    return out


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    res = {}
    for name in (sys.argv[2].split(',') if len(sys.argv) > 2 else CASES):
        for k, v in rollout(name).items():
            res['%s/%s' % (name, k)] = v
    np.savez(sys.argv[1], **res)
