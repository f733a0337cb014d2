"""GPU parity tests proper: every call goes through the C ABI (libf110_hip.so) and
is compared with the CPU oracle on the same seeded inputs and with the golden
fixtures generated from the reference.

Tolerances (north_star: bit-exact collision/index, 1e-5 dynamics/scans):
  * ray march, iTTC, LUT indices, GJK booleans, collision_idx, blocked-view
    indices, lap toggles/counts: exact (==)
  * anything through device sin/cos/tan/atan2: 1e-9 absolute (far inside 1e-5)
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (test infrastructure)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def eng(assets):
    from red_gym_amd.engine import Engine
    e = Engine(num_envs=1, num_agents=1, noise_std=0)
    e.set_map(os.path.join(assets, 'example_map.yaml'), '.png')
    yield e
    e.close()


@pytest.fixture(scope='module')
def ex_oracle(assets):
    s = oracle.Scanner(1080, 2 * np.pi)
    s.set_map(os.path.join(assets, 'example_map.yaml'), '.png')
    return s


def test_map_table_bit_exact(eng, ex_oracle, golden):
    dt = eng.get_map_dt()
    assert np.array_equal(dt, ex_oracle.map['dt'])
    g = golden('g1_scan.npz')
    assert np.array_equal(dt[g['ex_dt_rows'], g['ex_dt_cols']], g['ex_dt_vals'])


def test_scan_golden_bit_exact(eng, golden):
    g = golden('g1_scan.npz')
    out, out32, lk = eng.scan(g['ex_poses'], want_f32=True, want_lookups=True)
    assert np.array_equal(_np(out), g['ex_scans'])
    assert np.array_equal(_np(lk).astype(np.int64), g['ex_lookups'])
    assert np.array_equal(_np(out32), g['ex_scans'].astype(np.float32))


def test_scan_random_poses_vs_oracle(eng, ex_oracle, assets):
    rl = np.loadtxt(os.path.join(assets, 'example_waypoints.csv'), delimiter=';', skiprows=3)
    rng = np.random.default_rng(11)
    n = 1500
    rows = rng.integers(0, rl.shape[0], n)
    poses = np.stack([rl[rows, 1] + rng.normal(0, 0.25, n), rl[rows, 2] + rng.normal(0, 0.25, n),
                      rng.uniform(-1, 8, n)], axis=1)
    poses[:20, :2] = rng.uniform(-100, 100, (20, 2))  # far off the track / off the map
    ref, rlk = ex_oracle.scan_batch(poses, return_lookups=True)
    out, lk = eng.scan(poses, want_lookups=True)
    assert np.array_equal(_np(out), ref)
    assert np.array_equal(_np(lk).astype(np.int64), rlk)


@pytest.mark.parametrize('name', ['berlin', 'skirk', 'vegas'])
def test_scan_other_maps(assets, golden, name):
    """resolution 0.05 (not a power of two): exercises the guarded-reciprocal index path;
    dt[-1,-1] = 0 there, so rays leaving the map stop instead of jumping to max range."""
    from red_gym_amd.engine import Engine
    g = golden('g1_scan.npz')
    e = Engine(num_envs=1, num_agents=1, fov=4.7, noise_std=0)
    e.set_map(os.path.join(assets, 'maps', name + '.yaml'), '.png')
    assert np.array_equal(_np(e.scan(g[name + '_poses'])), g[name + '_scans'])
    s = oracle.Scanner(1080, 4.7)
    s.set_map(os.path.join(assets, 'maps', name + '.yaml'), '.png')
    rng = np.random.default_rng(3)
    H, W, res = s.map['height'], s.map['width'], s.map['resolution']
    n = 300
    poses = np.stack([s.map['orig_x'] + rng.uniform(-2, W * res + 2, n), s.map['orig_y'] + rng.uniform(-2, H * res + 2, n),
                      rng.uniform(0, 6.3, n)], axis=1)
    assert np.array_equal(_np(e.scan(poses)), s.scan_batch(poses))
    e.close()


@pytest.mark.parametrize('name', ['berlin', 'vegas'])
def test_scan_quotients_on_cell_boundaries_other_maps(assets, name):
    """Resolution 0.05: the march computes (x - ox) * (1 / res) and must fall back to the reference's own division
    (laser_models.py:83-84) whenever that quotient lies within 1e-9 of an integer.  Poses whose y (or x) sits exactly on
    a cell boundary, looking exactly along the other axis (yaw = pi with fov 2 pi puts beam 0 on LUT entry 0: cos 1, sin 0;
    beam 270 / 540 / 810 on the other axes' entries): that beam's every look-up has an integer quotient in one coordinate, so
    every march iteration of the wave takes the exit.  Poses far from the map take the clamped loop.  `==` the oracle, look-up
    counts included."""
    from red_gym_amd.engine import Engine
    e = Engine(num_envs=1, num_agents=1, fov=2 * np.pi, noise_std=0)
    e.set_map(os.path.join(assets, 'maps', name + '.yaml'), '.png')
    s = oracle.Scanner(1080, 2 * np.pi)
    s.set_map(os.path.join(assets, 'maps', name + '.yaml'), '.png')
    m = s.map
    dt, res, ox, oy = m['dt'], m['resolution'], m['orig_x'], m['orig_y']
    rng = np.random.default_rng(17)
    free = np.argwhere(dt > 0.4)
    pick = free[rng.integers(0, len(free), 200)]
    poses = []
    for (r, c) in pick:
        for yaw in (np.pi, 0.0, 0.5 * np.pi, 1.2345):
            poses.append((ox + (c + 0.37) * res, oy + r * res, yaw))            # y on a boundary
            poses.append((ox + c * res, oy + (r + 0.61) * res, yaw))            # x on a boundary
            poses.append((ox + c * res, oy + r * res, yaw))                     # a cell corner
    poses += [(ox + 3e6, oy + 1.0, 0.3), (ox - 2.5e7, oy - 4e6, 2.0), (1e12, -1e12, 1.0)]   # far away: the clamped loop
    poses = np.array(poses)
    ref, rlk = s.scan_batch(poses, return_lookups=True)
    out, lk = e.scan(poses, want_lookups=True)
    assert np.array_equal(_np(out), ref) and np.array_equal(_np(lk).astype(np.int64), rlk)
    e.close()


def test_scan_odd_config_and_fov47(assets, golden):
    from red_gym_amd.engine import Engine
    g = golden('g1_scan.npz')
    e = Engine(num_envs=1, num_agents=1, fov=4.7, noise_std=0)
    e.set_map(os.path.join(assets, 'example_map.yaml'), '.png')
    assert np.array_equal(_np(e.scan(g['ex47_poses'])), g['ex47_scans'])
    e.close()
    e = Engine(num_envs=1, num_agents=1, fov=4.7, num_beams=271, eps=0.001, theta_dis=1500, max_range=12.0, noise_std=0)
    e.set_map(os.path.join(assets, 'example_map.yaml'), '.png')
    assert np.array_equal(_np(e.scan(g['exx_poses'])), g['exx_scans'])
    e.close()


def test_scan_rotated_origin_vs_oracle(ex_oracle):
    """origin yaw != 0 (general rotation path) and a user table that is not an EDT
    (escape cells served from the fp64 table)."""
    from red_gym_amd.engine import Engine
    rng = np.random.default_rng(8)
    dt = ex_oracle.map['dt'][600:1000, 500:1100].copy()
    dt[::7, ::5] *= 1.000001  # no longer resolution*sqrt(int): escape path
    oc, os_ = float(np.cos(0.3)), float(np.sin(0.3))
    m = {'height': dt.shape[0], 'width': dt.shape[1], 'resolution': 0.07, 'orig_x': -3.0, 'orig_y': 2.0,
         'orig_c': oc, 'orig_s': os_, 'dt': np.ascontiguousarray(dt)}
    s = oracle.Scanner(1080, 2 * np.pi)
    s.set_map_dict(m)
    e = Engine(num_envs=1, num_agents=1, noise_std=0)
    e.set_map_dt(dt, 0.07, -3.0, 2.0, oc, os_)
    n = 200
    u, v = rng.uniform(0, dt.shape[1] * 0.07, n), rng.uniform(0, dt.shape[0] * 0.07, n)
    poses = np.stack([-3.0 + oc * u - os_ * v, 2.0 + os_ * u + oc * v, rng.uniform(0, 6.3, n)], axis=1)
    assert np.array_equal(_np(e.scan(poses)), s.scan_batch(poses))
    e.close()


def test_scan_empty_and_errors(eng):
    from red_gym_amd.engine import Engine
    assert eng.scan(np.zeros((0, 3))).shape == (0, 1080)
    e = Engine(num_envs=1, num_agents=1, noise_std=0)
    with pytest.raises(ValueError, match='Map is not set'):
        e.scan(np.zeros((1, 3)))
    e.close()
    with pytest.raises(SyntaxError):
        Engine(num_envs=1, num_agents=1, integrator=7)
    with pytest.raises(ValueError):
        Engine(num_envs=1, num_agents=33)  # F110_MAX_AGENTS = 32


@pytest.mark.parametrize('tag,integ', [('rk4', 1), ('euler', 2)])
def test_update_pose_golden_and_oracle(assets, golden, tag, integ):
    from red_gym_amd.engine import Engine
    g = golden('g3_dynamics.npz')
    e = Engine(num_envs=1, num_agents=1, integrator=integ, noise_std=0)
    buf = g['buf'] * (np.arange(2)[None, :] < g['cnt'][:, None])
    ns, nb, nc = e.update_pose(g['state'], buf, g['cnt'], g['action'])
    ns, nb, nc = _np(ns), _np(nb), _np(nc)
    assert np.array_equal(nc, g[tag + '_cnt'])
    assert np.array_equal(nb * (np.arange(2)[None, :] < nc[:, None]), g[tag + '_buf'])
    assert np.allclose(ns, g[tag + '_state'], rtol=0, atol=1e-9)
    assert np.array_equal(ns[:, 2], g[tag + '_state'][:, 2])  # steer: no libm involved
    os_, ob, oc = oracle.update_pose_batch(g['state'], buf, g['cnt'], g['action'], oracle.params_vec(), 0.01, integ)
    assert np.allclose(ns, os_, rtol=0, atol=1e-9) and np.array_equal(nc, oc)
    e.close()


def test_vertices_gjk_golden(eng, golden):
    g = golden('g4_gjk.npz')
    va = _np(eng.get_vertices(g['pose_a']))
    assert np.allclose(va, g['verts_a'], rtol=0, atol=1e-12)
    hit = _np(eng.gjk_pairs(g['verts_a'], g['verts_b'])).astype(bool)
    assert np.array_equal(hit, g['hit'])
    for A in (2, 3, 4):
        poses = g['multi%d_poses' % A]
        verts = np.stack([[oracle.get_vertices(poses[k, a], 0.58, 0.31) for a in range(A)] for k in range(poses.shape[0])])
        col, idx = eng.collision_multiple(verts)
        assert np.array_equal(_np(col).astype(np.float64), g['multi%d_col' % A])
        assert np.array_equal(_np(idx).astype(np.float64), g['multi%d_idx' % A])
    col, idx = eng.collision_multiple(g['kat_verts'][None])  # collision_models.py:313-324
    assert np.array_equal(_np(col)[0], [1, 1, 1, 1, 1, 1, 0]) and np.array_equal(_np(idx)[0], [5, 5, 5, 5, 5, 4, -1])


def test_ttc_golden(golden):
    from red_gym_amd.engine import Engine
    g = golden('g5_ttc.npz')
    e = Engine(num_envs=1, num_agents=1, noise_std=0)
    assert np.array_equal(e.beam_cosines, g['cosines']) and np.array_equal(e.side_distances, g['side_distances'])
    scans = g['scans_f32'].astype(np.float64)
    for i in range(scans.shape[0]):
        if g['ov_beam'][i] >= 0:
            scans[i, g['ov_beam'][i]] = g['ov_val'][i]
    assert np.array_equal(_np(e.check_ttc(scans, g['vel'])).astype(bool), g['hit'])
    e.close()


def test_raycast_golden(eng, golden):
    g = golden('g6_raycast.npz')
    assert np.array_equal(eng.scan_angles, g['scan_angles'])
    scans_in = g['scans_in_f32'].astype(np.float64)
    out, span = eng.ray_cast(g['ego'], g['verts'], scans_in)
    out, span = _np(out), _np(span)
    assert np.array_equal(span, g['span'])
    assert np.allclose(out, g['scans_out'], rtol=0, atol=1e-9)
    assert np.array_equal(out != scans_in, g['scans_out'] != scans_in)


def test_scan_yaw_extremes_vs_oracle(eng, ex_oracle):
    """fmod / LUT-index start for yaws far outside [0, 2pi), exact multiples of the LUT
    step and sign changes (laser_models.py:167-172)."""
    rng = np.random.default_rng(21)
    yaws = np.concatenate([[0.0, -0.0, np.pi, -np.pi, 2 * np.pi, -2 * np.pi, 1e-300, -1e-300, 1e6, -1e6, 12345.678, -9876.54],
                           2 * np.pi * rng.integers(-50, 50, 20) / 2000.0 + np.pi,   # exact LUT-bin boundaries
                           rng.uniform(-200, 200, 60)])
    poses = np.stack([np.full_like(yaws, 0.7), np.zeros_like(yaws), yaws], axis=1)
    assert np.array_equal(_np(eng.scan(poses)), ex_oracle.scan_batch(poses))


def test_scan_rays_leaving_through_every_border(eng, ex_oracle):
    """Poses just inside each edge of the map looking outwards and just outside looking in:
    the clamped border lookups (dt[-1,-1], laser_models.py:80-81,:103) on all four sides and
    the corners."""
    m = ex_oracle.map
    x0, y0 = m['orig_x'], m['orig_y']
    x1, y1 = x0 + m['width'] * m['resolution'], y0 + m['height'] * m['resolution']
    e = 0.03
    pts = []
    for x in (x0 - 5, x0 - e, x0 + e, 0.5 * (x0 + x1), x1 - e, x1 + e, x1 + 5):
        for y in (y0 - 5, y0 - e, y0 + e, 0.5 * (y0 + y1), y1 - e, y1 + e, y1 + 5):
            for yaw in (0.0, 1.0, 2.5, 4.0, 5.5):
                pts.append((x, y, yaw))
    poses = np.array(pts)
    ref, rlk = ex_oracle.scan_batch(poses, return_lookups=True)
    out, lk = eng.scan(poses, want_lookups=True)
    assert np.array_equal(_np(out), ref) and np.array_equal(_np(lk).astype(np.int64), rlk)


# ---- map pipeline on the device: exact EDT and the tables built from it
def _edt_host(mask):
    import ctypes as C
    from red_gym_amd import _lib
    H, W = mask.shape
    d2 = np.empty((H, W), np.uint32)
    _lib.check(_lib.load().f110_edt_squared(mask.ctypes.data_as(C.c_void_p), H, W, d2.ctypes.data_as(C.c_void_p)))
    return d2


def _edt_dev(mask):
    import torch
    from red_gym_amd import _lib
    H, W = mask.shape
    m = torch.as_tensor(mask, device='cuda')
    d2 = torch.empty((H, W), dtype=torch.int32, device='cuda')
    _lib.check(_lib.load().f110_edt_squared_dev(m.data_ptr(), H, W, d2.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return d2.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('shape,density', [((64, 64), 0.02), ((37, 201), 0.005), ((301, 17), 0.1), ((1, 50), 0.1),
                                           ((50, 1), 0.1), ((257, 513), 0.0003), ((600, 600), 0.5), ((128, 4100), 0.001),
                                           # rows of more than 64 KiB of LDS (edt_rows_kernel through hipFuncSetAttribute)
                                           ((3, 16385), 0.002), ((3, 20000), 0.001), ((3, 32768), 0.0005)])
def test_edt_device_matches_host_and_scipy(shape, density):
    from scipy.ndimage import distance_transform_edt
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    mask = (rng.random(shape) >= density).astype(np.uint8)
    mask[rng.integers(shape[0]), rng.integers(shape[1])] = 0         # at least one occupied cell
    if shape[1] > 8:
        mask[:, 3] = 1                                               # a column without any occupied cell
    got = _edt_dev(mask)
    assert np.array_equal(got, _edt_host(mask))
    assert np.array_equal(got, np.rint(distance_transform_edt(mask) ** 2).astype(np.uint32))


def test_edt_device_single_obstacle_and_full_maps():
    mask = np.ones((200, 300), np.uint8)
    mask[150, 20] = 0
    yy, xx = np.mgrid[0:200, 0:300]
    assert np.array_equal(_edt_dev(mask), ((yy - 150) ** 2 + (xx - 20) ** 2).astype(np.uint32))
    assert not _edt_dev(np.zeros((40, 40), np.uint8)).any()


def test_device_map_pipeline_equals_reference_distance_table():
    """set_map through the device pipeline: the fp64 table equals the reference's resolution * scipy EDT
    (laser_models.py:40-53) on every shipped map; maps of different sizes replace each other on one handle."""
    from scipy.ndimage import distance_transform_edt
    from red_gym_amd import F110VecEnv, workload, maps
    env = F110VecEnv(4, map=workload.EXAMPLE_MAP, num_agents=1)
    for name in ['berlin', 'vegas', 'skirk']:
        y = maps.builtin_map_yaml(name)
        m = maps.load_map(y, '.png')
        env.update_map(y, '.png')
        want = m.resolution * distance_transform_edt(m.free)
        assert np.array_equal(env.eng.get_map_dt(), want), name
    m = maps.load_map(workload.EXAMPLE_MAP + '.yaml', '.png')
    env.update_map(workload.EXAMPLE_MAP + '.yaml', '.png')
    assert np.array_equal(env.eng.get_map_dt(), m.resolution * distance_transform_edt(m.free))
    env.close()


def test_device_mask_map_matches_file_map_scans():
    """A mask handed over as a CUDA tensor builds the same map as the file loader: identical scans."""
    import torch
    from red_gym_amd import F110VecEnv, workload, maps
    m = maps.load_map(workload.EXAMPLE_MAP + '.yaml', '.png')
    a = F110VecEnv(64, map=workload.EXAMPLE_MAP, num_agents=1)
    b = F110VecEnv(64, map='berlin', num_agents=1)
    b.update_map_occupancy(torch.as_tensor(m.free, device='cuda'), m.resolution, m.orig_x, m.orig_y,
                           float(np.arctan2(m.orig_s, m.orig_c)))
    poses = workload.spawn_poses(64, 1)
    oa, ob = a.reset(poses)[0], b.reset(poses)[0]
    assert torch.equal(oa['scans'], ob['scans'])
    assert np.array_equal(a.eng.get_map_dt(), b.eng.get_map_dt())
    with pytest.raises(ValueError):
        b.update_map_occupancy(torch.ones((32, 32), dtype=torch.uint8, device='cuda'), 0.05, 0., 0.)
    a.close(); b.close()


def test_edt_device_fuzz_small_shapes():
    """Every shape from 1x1 to 9x13 and a few hundred random masks of random density: device EDT == host EDT."""
    rng = np.random.default_rng(31)
    cases = 0
    for H in range(1, 10):
        for W in (1, 2, 3, 5, 8, 13):
            for dens in (0.05, 0.5, 0.95):
                mask = (rng.random((H, W)) >= dens).astype(np.uint8)
                mask[rng.integers(H), rng.integers(W)] = 0
                assert np.array_equal(_edt_dev(mask), _edt_host(mask)), (H, W, dens)
                cases += 1
    for _ in range(60):
        H, W = int(rng.integers(10, 90)), int(rng.integers(10, 140))
        mask = (rng.random((H, W)) >= rng.choice([0.001, 0.01, 0.2, 0.8])).astype(np.uint8)
        mask[rng.integers(H), rng.integers(W)] = 0
        if rng.random() < 0.3:
            mask[:, rng.integers(W)] = 1            # obstacle-free column
        if rng.random() < 0.3:
            mask[rng.integers(H), :] = 1            # obstacle-free row
        if not (mask == 0).any():
            mask[0, 0] = 0
        assert np.array_equal(_edt_dev(mask), _edt_host(mask)), (H, W)
        cases += 1
    assert cases > 200
