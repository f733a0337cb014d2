"""Generates g15_nearest.npz: the reference's OWN nearest_point_on_trajectory (examples/waypoint_follow.py:16-47) on the
pose sets of tests/progress_cases.py, against the shipped example raceline.

Run through make_golden.py: the reference is loaded by file path (reference.load_planner(), identity-njit stand-in: numba
is absent; same source, same IEEE-754 double operations) without running its main.  The fixture holds recorded
numbers only: the extra poses, and per pose (g8's 3 329 first, then the extra ones) projection, dist, t, i.

The reference forms its dot product with np.dot, which NumPy hands to the BLAS, and what a BLAS does with a 2-element
vector is the host's business: OpenBLAS's SkylakeX kernel returns fma(x1, y1, x0 * y0), its Haswell and older kernels the two
rounded products and their sum.  The fixture records the reference under IEEE arithmetic without contraction -- the
numerics contract of the project and what the reference gives on any host whose BLAS does not fuse --
so the row runs under reference.BLAS_PIN, and the generator refuses to run if np.dot still fuses.
"""
import numpy as np

import reference
import progress_cases as pc


def g15_nearest():
    reference.require_unfused_dot()
    mod = reference.load_planner()[0]
    xy = np.ascontiguousarray(pc.example_raceline()[:, :2])
    g8 = np.load(reference.fixture('g8_env.npz'))
    extra = pc.g15_extra_poses(xy)
    poses = np.concatenate([np.stack([g8['x'], g8['y']], axis=1), extra], axis=0)
    n = poses.shape[0]
    proj, dist, t, seg = np.zeros((n, 2)), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    for k in range(n):
        proj[k], dist[k], t[k], seg[k] = mod.nearest_point_on_trajectory(poses[k].copy(), xy)
    reference.save('g15_nearest.npz', poses=extra, n_g8=np.int64(g8['x'].shape[0]), projection=proj, dist=dist, t=t, i=seg)
    print('  %d poses (%d of g8 + %d)' % (n, g8['x'].shape[0], extra.shape[0]))
