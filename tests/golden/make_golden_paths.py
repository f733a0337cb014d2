"""Generates g17_paths.npz: the reference's OWN path code -- compute_vectors_with_angle_clamp (src/SAL.py:585-608),
SACF110Env._calculate_global_path (:157-181), _update_path_index (:252-259), MPC_converter (:741-764) and the part of
MPC_controller (:615-687) in front of its first cvxpy call: `dists` and `ref_traj` -- on the cases of tests/path_cases.py.

Run through make_golden.py, with g16's loader of src/SAL.py (reference.load_sal(): stand-in modules for cv2, cvxpy, gym,
pyglet) and BLAS guard (np.linalg.norm is in `dists` and in _update_path_index).  cvxpy and OSQP are absent here, so the QP's
solution cannot be recorded: the stand-in cvxpy's Variable raises a private exception at MPC_controller's first use of it, and
`ref_traj` and `dists` are read from MPC_controller's frame in the traceback -- everything up to that line is NumPy and scipy.
The accelerations MPC_converter is recorded on are (a) the optimum the enumerator of tests/path_cases.py finds for the case and
(b) designed pairs.  The fixture holds inputs and recorded results only.

The reference has three discontinuities -- the +-pi wrap of the clamp, the wrap of the converter and dist < DIST_THRESHOLD; the
generator asserts, on the reference's values, that every case stays at least 1e-6 away from each, so that no test needs to
leave a case out.
"""
import os
import sys

import numpy as np

import reference
import path_cases as pc

N = 780
MARGIN = 1e-6


class _Stop(Exception):
    pass


def _raise(*a, **k):
    raise _Stop()


def controller_frame(sal, path, vx, vy, cfg=None):
    """(dists, ref_traj) of MPC_controller with SAL's MPC_PARAMS, or with the options of a tests/path_cases.py config."""
    p = sal.SACF110Env.MPC_PARAMS
    if cfg is not None:
        p = dict(p, desired_velocity=cfg['desired_velocity'], timestep=cfg['timestep'], horizon_length=cfg['horizon'],
                 state_cost=np.diag(cfg['q']), input_cost=np.diag(cfg['r']), terminal_cost=np.diag(cfg['p']))
    try:
        sal.MPC_controller(path=path, desiredVelocity=p['desired_velocity'], timeStep=p['timestep'], totalSteps=p['total_steps'],
                           horizonLength=p['horizon_length'], stateCost=p['state_cost'], inputCost=p['input_cost'],
                           terminalCost=p['terminal_cost'], current_vel_x=vx, current_vel_y=vy)
    except _Stop:
        tb = sys.exc_info()[2]
        while tb.tb_next is not None and tb.tb_frame.f_code.co_name != 'MPC_controller':
            tb = tb.tb_next
        loc = tb.tb_frame.f_locals
        assert tb.tb_frame.f_code.co_name == 'MPC_controller'
        return np.array(loc['dists'], dtype=np.float64), np.array(loc['ref_traj'], dtype=np.float64)
    raise AssertionError('MPC_controller did not reach cvxpy')


def away(values, period):
    """Distance of every value from the nearest multiple of `period`."""
    r = np.mod(values, period)
    return np.minimum(r, period - r)


def g17_paths():
    reference.require_unfused_dot()
    sal = reference.load_sal()
    sal.cp.Variable = _raise
    env = sal.SACF110Env.__new__(sal.SACF110Env)
    env.car_length, env.vector_length = 0.3, 0.5
    raw, poses, vels = pc.designed_raw(N, 1700), pc.designed_poses(N, 1701), pc.designed_vels(N, 1702)
    rng = np.random.default_rng(1703)
    inc, paths, dists, ref = np.zeros((N, 8, 2)), np.zeros((N, 8, 2)), np.zeros((N, 8)), np.zeros((N, 9, 4))
    index, xy, index_out = rng.integers(0, 8, N).astype(np.int32), np.zeros((N, 2)), np.zeros(N, dtype=np.int32)
    for i in range(N):
        inc[i] = sal.compute_vectors_with_angle_clamp(raw[i].copy())       # (it normalises its argument in place)
        paths[i] = np.array(env._calculate_global_path(inc[i], {'x': poses[i, 0], 'y': poses[i, 1], 'theta': poses[i, 2]}))
        dists[i], r = controller_frame(sal, paths[i], vels[i, 0], vels[i, 1])
        assert r.shape == (16, 4)
        ref[i] = r[:9]
        # the new pose: at a distance around DIST_THRESHOLD from the waypoint, either side
        rad = rng.uniform(0.0, 0.199) if i % 2 else rng.uniform(0.201, 0.6)
        phi = rng.uniform(0, 2 * np.pi)
        xy[i] = paths[i, index[i]] + rad * np.array([np.cos(phi), np.sin(phi)])
        env.path_points, env.sub_index = [tuple(p) for p in paths[i]], int(index[i])
        env._update_path_index({'poses_x': np.array([xy[i, 0]]), 'poses_y': np.array([xy[i, 1]])})
        index_out[i] = env.sub_index
        assert abs(np.linalg.norm(xy[i] - paths[i, index[i]]) - sal.SACF110Env.DIST_THRESHOLD) >= MARGIN
    # the converter: (a) on the enumerator's optimum of every case, (b) on designed pairs
    accel = pc.mpc_accel(paths, vels)[0]
    m = 260
    extra = rng.uniform(-1.0, 1.0, (m, 2))
    small = rng.uniform(0.0, 0.4, m) * rng.choice([-1.0, 1.0], m)
    extra[::2] = np.stack([np.cos(small[::2]), np.sin(small[::2])], axis=1) * rng.uniform(0.05, 1.0, (m // 2, 1))
    conv_in = np.concatenate([accel, extra])
    conv_out = np.array([sal.MPC_converter(ax, ay, 1.0, 0.0, 0.4189, 3.0, 8.0, -4.0) for ax, ay in conv_in])
    # discontinuities, on the reference's values: the clamp's wrap argument desired - prev + pi against multiples of 2 pi, with
    # prev = the heading of the reference's own previous increment; the converter's likewise
    v = raw.reshape(N, 8, 2)
    v = v / (np.linalg.norm(v, axis=2, keepdims=True) + 1e-8)
    desired = np.arctan2(v[:, 1:, 1], v[:, 1:, 0])
    prev = np.arctan2(inc[:, :-1, 1], inc[:, :-1, 0])
    arg = desired - prev + np.pi
    assert away(arg, 2 * np.pi).min() >= MARGIN, away(arg, 2 * np.pi).min()
    carg = np.arctan2(conv_in[:, 1], conv_in[:, 0]) + np.pi
    assert away(carg, 2 * np.pi).min() >= MARGIN, away(carg, 2 * np.pi).min()
    # coverage, on the reference's results
    lim = np.deg2rad(10.0)
    turned = np.arctan2(inc[:, 1:, 1], inc[:, 1:, 0]) - prev
    clamped = np.abs(np.abs(turned) - lim) < 1e-12
    cover = {'segment clamped': clamped, 'segment not clamped': ~clamped, 'index advanced': index_out == index + 1,
             'index kept': index_out == index, 'steer clipped': np.abs(conv_out[:, 0]) == 0.4189,
             'steer not clipped': np.abs(conv_out[:, 0]) < 0.4189,
             'steer not clipped, on a case\'s optimum': np.abs(conv_out[:N, 0]) < 0.4189}
    for name, mk in cover.items():
        print('%-40s %6d (%.1f %%)' % (name, mk.sum(), 100.0 * mk.mean()))
        assert mk.mean() >= 0.05, name
    assert ((index_out == index) | (index_out == index + 1)).all()
    size = reference.save('g17_paths.npz', raw=raw, poses=poses, vels=vels, increments=inc, paths=paths, dists=dists, ref_traj=ref,
                          index=index, xy=xy, index_out=index_out, conv_in=conv_in, conv_out=conv_out)
    print('  %d cases, %d converter records' % (N, conv_in.shape[0]))
    assert size < os.path.getsize(reference.fixture('g6_raycast.npz')) // 2
