"""Generates g19_path_configs.npz: the reference's OWN path code at the off-default configurations CONFIGS of
tests/path_cases.py -- compute_vectors_with_angle_clamp (src/SAL.py:585-608, its max_diff_deg is an argument),
SACF110Env._calculate_global_path (:157-181, car_length and vector_length are attributes), `dists` and the first horizon + 1
rows of `ref_traj` of MPC_controller (:615-687, read from its frame as in make_golden_paths.py, whose controller_frame is
reused with the config's velocity, timestep, horizon and weights) and MPC_converter (:741-764, max_steer is an argument) on the
enumerator's optimum of each case.  Every option is one the reference takes as an argument or an attribute: no record comes from
the NumPy checker.  Per config: path_cases.designed_raw / poses / vels on the config's own seeds, G19_CASES cases.

Run through make_golden.py, like g17 (same loader of src/SAL.py, same BLAS guard).  The fixture holds inputs and
recorded results only; keys are '<config>/<record>'.

Asserted here, on the reference's values: every case stays at least 1e-6 from the wrap of the clamp, the wrap of the converter
and the speed > 1e-3 switch of the reference states (the third discontinuity of g17, dist < DIST_THRESHOLD, is not recorded
here); in the first config every reference state is at least 1e-6 from a knot of the spline, and every spline piece 0..6 and
the end clamp occur in at least 5 % of the (case, k) pairs.
"""
import os

import numpy as np

import reference
import make_golden_paths as mgp
import path_cases as pc

MARGIN = 1e-6


def g19_path_configs():
    reference.require_unfused_dot()
    sal = reference.load_sal()
    sal.cp.Variable = mgp._raise
    env = sal.SACF110Env.__new__(sal.SACF110Env)
    n = pc.G19_CASES
    store = {}
    for ci, (name, entry) in enumerate(pc.CONFIGS.items()):
        c = pc.config(**entry['cfg'])
        H = c['horizon']
        env.car_length, env.vector_length = c['car_length'], c['vector_length']
        raw, poses, vels = pc.g19_inputs(name)
        inc, paths, dists, ref = np.zeros((n, 8, 2)), np.zeros((n, 8, 2)), np.zeros((n, 8)), np.zeros((n, H + 1, 4))
        for i in range(n):
            inc[i] = sal.compute_vectors_with_angle_clamp(raw[i].copy(), c['max_diff_deg'])
            paths[i] = np.array(env._calculate_global_path(inc[i], {'x': poses[i, 0], 'y': poses[i, 1], 'theta': poses[i, 2]}))
            dists[i], r = mgp.controller_frame(sal, paths[i], vels[i, 0], vels[i, 1], c)
            assert r.shape == (10 + H + 1, 4)
            ref[i] = r[:H + 1]
        conv_in = pc.mpc_accel(paths, vels, c)[0]
        conv_out = np.array([sal.MPC_converter(ax, ay, 1.0, 0.0, c['max_steer'], 3.0, 8.0, -4.0) for ax, ay in conv_in])
        # discontinuities, on the reference's values
        v = raw.reshape(n, 8, 2)
        v = v / (np.linalg.norm(v, axis=2, keepdims=True) + 1e-8)
        prev = np.arctan2(inc[:, :-1, 1], inc[:, :-1, 0])
        arg = np.arctan2(v[:, 1:, 1], v[:, 1:, 0]) - prev + np.pi
        assert mgp.away(arg, 2 * np.pi).min() >= MARGIN, (name, mgp.away(arg, 2 * np.pi).min())
        carg = np.arctan2(conv_in[:, 1], conv_in[:, 0]) + np.pi
        assert mgp.away(carg, 2 * np.pi).min() >= MARGIN, (name, mgp.away(carg, 2 * np.pi).min())
        moving = (ref[:, :, 2:] != 0.0).any(axis=2)
        assert moving.all(), name                              # speed > 1e-3 everywhere: |rv| = desired_velocity, far from the switch
        assert np.abs(np.hypot(ref[:, :, 2], ref[:, :, 3]) - c['desired_velocity']).max() <= 1e-9
        sk = c['desired_velocity'] * (np.arange(H + 1) * c['timestep'])
        gap = np.abs(sk[None, 1:, None] - dists[:, None, 1:]).min()
        assert gap >= MARGIN or ci > 0, (name, gap)             # (short_chords puts k = 5 on the knot x[4] = 1.0: the spline is C2 there)
        # coverage, on the reference's results: the piece of sk among the reference's own knots
        clamped = sk[None] > dists[:, -1:]
        piece = (dists[:, 1:-1, None] <= np.minimum(sk[None], dists[:, -1:])[:, None, :]).sum(axis=1)
        turned = np.arctan2(inc[:, 1:, 1], inc[:, 1:, 0]) - prev
        seg = np.abs(np.abs(mgp.away(turned + np.pi, 2 * np.pi) - np.pi) - np.deg2rad(c['max_diff_deg'])) < 1e-9
        steer = np.abs(conv_out[:, 0]) == c['max_steer']
        print('%-15s pieces %s  clamp %5.1f %%  segments clamped %5.1f %%  steer clipped %5.1f %%  nearest knot %.2g'
              % (name, ' '.join('%4.1f' % (100.0 * (piece == j).mean()) for j in range(7)), 100.0 * clamped.mean(), 100.0 * seg.mean(),
                 100.0 * steer.mean(), gap))
        if ci == 0:
            for j in range(7):
                assert ((piece == j) & ~clamped).mean() >= 0.05, j
            assert clamped.mean() >= 0.05
        if name == 'nothing_clamps':
            assert not seg.any() and steer.mean() >= 0.5
        if name == 'all_clamps':
            assert seg.mean() >= 0.9 and not steer.any()
        for key, val in (('increments', inc), ('paths', paths), ('dists', dists), ('ref_traj', ref), ('conv_in', conv_in), ('conv_out', conv_out)):
            store['%s/%s' % (name, key)] = val
    size = reference.save('g19_path_configs.npz', **store)
    print('  %d configs of %d cases' % (len(pc.CONFIGS), n))
    assert size < os.path.getsize(reference.fixture('g17_paths.npz'))
