"""Generates g15_nearest.npz: the reference's OWN nearest_point_on_trajectory (examples/waypoint_follow.py:16-47) on the
pose sets of tests/progress_cases.py, against the shipped example raceline.

Dev-container only, like make_golden.py: the reference is loaded by file path through ref_loader's identity-njit stand-in
(numba is absent; same source, same IEEE-754 double operations) without running its main.  The fixture holds recorded
numbers only: the extra poses, and per pose (g8's 3 329 first, then the extra ones) projection, dist, t, i.

The reference forms its dot product with np.dot, which NumPy hands to the BLAS, and what a BLAS does with a 2-element
vector is the host's business: OpenBLAS's SkylakeX kernel returns fma(x1, y1, x0 * y0), its Haswell and older kernels the two
rounded products and their sum.  The fixture records the reference under IEEE arithmetic without contraction -- the
numerics contract of the project and what the reference gives on any host whose BLAS does not fuse --
so the BLAS kernel set is pinned before NumPy loads, and the generator refuses to run if np.dot still fuses.

    python tests/golden/make_golden_progress.py
"""
import importlib.util
import os
import sys

os.environ.setdefault('OPENBLAS_CORETYPE', 'Haswell')   # must precede the first import of numpy

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import ref_loader  # noqa: E402
import progress_cases as pc  # noqa: E402


def load_reference_planner():
    ref_loader.load_env()    # the numba / gym / pyglet stand-ins the example's imports need
    spec = importlib.util.spec_from_file_location('ref_waypoint_follow', ref_loader.REF_ROOT + '/examples/waypoint_follow.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dot_is_unfused():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-3, 3, (4096, 2)), rng.uniform(-3, 3, (4096, 2))
    return all(np.dot(a[k], b[k]) == a[k, 0] * b[k, 0] + a[k, 1] * b[k, 1] for k in range(4096))


def main():
    if not dot_is_unfused():
        raise SystemExit('np.dot fuses its multiply-add on this host (BLAS kernel): the fixture would record the host, not the reference')
    mod = load_reference_planner()
    xy = np.ascontiguousarray(pc.example_raceline()[:, :2])
    g8 = np.load(os.path.join(HERE, 'g8_env.npz'))
    extra = pc.g15_extra_poses(xy)
    poses = np.concatenate([np.stack([g8['x'], g8['y']], axis=1), extra], axis=0)
    n = poses.shape[0]
    proj, dist, t, seg = np.zeros((n, 2)), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    for k in range(n):
        proj[k], dist[k], t[k], seg[k] = mod.nearest_point_on_trajectory(poses[k].copy(), xy)
    out = os.path.join(HERE, 'g15_nearest.npz')
    np.savez_compressed(out, poses=extra, n_g8=np.int64(g8['x'].shape[0]), projection=proj, dist=dist, t=t, i=seg)
    print('wrote %s: %d poses (%d of g8 + %d), %d bytes' % (out, n, g8['x'].shape[0], extra.shape[0], os.path.getsize(out)))


if __name__ == '__main__':
    main()
