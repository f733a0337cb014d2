"""Progress tracker, the part that needs no GPU: the NumPy checker pinned on the reference's own nearest point (g15), the
host tables, the checker along the reference's 3 329-step lap run (g8), and the refusals of the tracker's entry points."""
import ctypes as C

import numpy as np
import pytest

import progress_cases as pc
from red_gym_amd import _lib, build, progress


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _lib.load()


@pytest.fixture(scope='module')
def example():
    return pc.FrenetChecker(pc.example_raceline())


def test_checker_equals_reference_nearest_point(golden, example):
    """checker (i, t, dist, projection) == the reference's nearest_point_on_trajectory on all 8 548 poses of g15: this
    pins the checker on the reference.  The fixture records the reference under arithmetic without contraction: its dot
    product is np.dot, and the generator pins a BLAS kernel set that does not fuse a 2-element dot (a fusing one returns
    fma(r1, s1, r0 * s0), which moves t in the last place on a third of the poses and flips the tie on waypoint 29 -- a
    property of a host's BLAS, not of the reference; tests/golden/make_golden.py g15)."""
    P, g = pc.g15_poses(golden), golden('g15_nearest.npz')
    assert P.shape[0] == g['i'].shape[0] == int(g['n_g8']) + g['poses'].shape[0]
    got = [example.nearest(x, y) for x, y in P]
    i = np.array([r[0] for r in got])
    t = np.array([r[1] for r in got])
    dist = np.array([r[2] for r in got])
    proj = np.array([r[3] for r in got])
    print('g15: %d poses; differing i %d, t %d (max %.3g), dist %d (max %.3g), projection %d (max %.3g)'
          % (P.shape[0], (i != g['i']).sum(), (t != g['t']).sum(), np.abs(t - g['t']).max(), (dist != g['dist']).sum(),
             np.abs(dist - g['dist']).max(), (proj != g['projection']).any(axis=1).sum(), np.abs(proj - g['projection']).max()))
    assert np.array_equal(i, g['i'])
    assert np.array_equal(t, g['t'])
    assert np.array_equal(dist, g['dist'])
    assert np.array_equal(proj, g['projection'])


def test_raceline_tables_equal_the_checkers(example):
    xy = pc.example_raceline()
    length, cum, psi, L = progress.raceline_tables(xy)          # [M, 3] in: columns 0, 1 are read
    assert np.array_equal(length, example.len) and np.array_equal(cum, example.cum) and np.array_equal(psi, example.psi)
    assert L == example.L
    assert xy.shape[0] == 783 and np.array_equal(xy[0, :2], xy[-1, :2])   # a closed file: no gap
    assert abs(L - 156.35611902054) < 5e-12                      # the polyline's length, not the CSV's own s_m column (156.3586)
    for line in (pc.circle_raceline(), pc.stadium_raceline(), pc.l_shape_raceline()):
        ck = pc.FrenetChecker(line)
        length, cum, psi, L = progress.raceline_tables(line)
        assert np.array_equal(length, ck.len) and np.array_equal(cum, ck.cum) and np.array_equal(psi, ck.psi) and L == ck.L
    assert pc.FrenetChecker(pc.stadium_raceline()).L > pc.FrenetChecker(pc.stadium_raceline()).cum[-1]   # an open line: the gap counts
    pk = progress.PackedRacelines([pc.circle_raceline(), pc.l_shape_raceline()])
    assert pk.K == 2 and list(pk.offsets) == [0, 201, 246] and pk.xy.shape == (246, 2)
    ck = pc.FrenetChecker(pc.l_shape_raceline())
    assert np.array_equal(pk.len[201:245], ck.len) and np.array_equal(pk.cum[201:246], ck.cum) and pk.lap_length[1] == ck.L


def test_checker_along_the_reference_lap_run(golden, example):
    """g8: the reference's closed loop of 3 329 steps, two laps of the example track.  Every step moves forward; the
    figures are those of the definition (computed when the issue was written: min delta 0.00128, max 0.110, progress 155.98
    at step 1 687 and 312.287 = 1.9973 L at step 3 328, the steps where lap_counts rises -- the lap counter's start zone
    fires a little before a full L, so progress >= k L is NOT asserted there)."""
    g8 = golden('g8_env.npz')
    poses = np.stack([g8['x'], g8['y'], g8['theta']], axis=1)
    trk = pc.ProgressChecker([example], [0])
    delta, prog = np.zeros(poses.shape[0]), np.zeros(poses.shape[0])
    for k in range(poses.shape[0]):
        out = trk.update(poses[k:k + 1], [False])
        delta[k], prog[k] = out['delta'][0], out['progress'][0]
    assert delta[0] == 0.0 and prog[0] == 0.0                     # the first call places the car
    assert (delta[1:] > 0).all()
    print('g8: min delta %.6f max %.6f progress[1687] %.4f progress[3328] %.4f' % (delta[1:].min(), delta[1:].max(), prog[1687], prog[3328]))
    assert abs(delta[1:].min() - 0.00128) < 5e-6 and abs(delta[1:].max() - 0.110) < 5e-4
    rises = np.flatnonzero(np.diff(g8['lap_c']) > 0) + 1
    assert list(rises) == [1687, 3328]
    assert abs(prog[1687] - 155.98) < 5e-3 and abs(prog[3328] - 312.287) < 5e-4
    assert abs(prog[3328] / example.L - 1.9973) < 5e-5
    assert prog[3328] == np.cumsum(delta)[-1] or abs(prog[3328] - delta.sum()) < 1e-9   # progress telescopes


def test_array_checker_equals_the_scalar_checker(golden, example):
    """The array forms the GPU tests use on their large pose sets are the scalar checker, bit for bit: on g15's poses
    (NaN and infinite ones mixed in), and as a tracker over a sequence of updates with restarts."""
    P = pc.g15_poses(golden)[::3]
    poses = pc.with_yaws(P, example.psi[np.array([example.nearest(x, y)[0] for x, y in P])], 7)
    poses[5::97, 0] = np.nan
    poses[11::89, 1] = np.inf
    seg, t, dist, s, d, e = pc.frenet_many(example, poses)
    for k in range(poses.shape[0]):
        r = example.frenet(*poses[k])
        assert r[0] == seg[k] and np.array_equal(np.array(r[1:]), np.array([s[k], d[k], e[k]]), equal_nan=True), k
    n = 300
    lines = [example, pc.FrenetChecker(pc.stadium_raceline())]
    of_car = np.arange(n) % 2
    a, b = pc.ProgressChecker(lines, of_car), pc.ProgressCheckerMany(lines, of_car)
    rng = np.random.default_rng(3)
    for step in range(6):
        q = poses[rng.integers(0, poses.shape[0], n)]
        reset = rng.uniform(size=n) < 0.2
        ra, rb = a.update(q, reset), b.update(q, reset)
        for key in ra:
            assert np.array_equal(ra[key], rb[key], equal_nan=True), (step, key)
        assert np.array_equal(a.seen, b.seen) and np.array_equal(a.s_prev, b.s_prev)


# ---------------------------------------------------------------------------------------------- ABI
def test_tracker_outputs_are_no_field_of_the_step_buffers():
    # (the declarations, exports and layouts themselves: tests/test_abi_cpu.py)  The step's own struct is untouched
    assert len(_lib.PROGRESS_FIELDS) == 8 and not set(_lib.PROGRESS_FIELDS) & set(_lib.BUFFER_FIELDS)


def _validate(lib, lines, assign=None, num_envs=4, tables=None):
    xy = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)[:, :2]) for a in lines]
    off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([a.shape[0] for a in xy])]), dtype=np.int32)
    total = int(off[-1])
    allxy = np.ascontiguousarray(np.concatenate(xy, axis=0))
    ln, cum, psi, lap = np.ones(total), np.zeros(total), np.zeros(total), np.ones(len(xy))
    if tables:
        ln, cum, psi, lap = (np.ascontiguousarray(t, dtype=np.float64) for t in tables)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    a32 = None if assign is None else np.ascontiguousarray(assign, dtype=np.int32)
    return lib.f110_progress_validate(p(allxy), p(off), len(xy), p(ln), p(cum), p(psi), p(lap), None if a32 is None else p(a32), num_envs)


def test_refusals_come_with_code_and_message_without_a_device(lib):
    sq = np.array([[0., 0.], [1., 0.], [1., 1.], [0., 1.]])
    assert _validate(lib, [sq]) == 0
    assert _validate(lib, [sq, sq + 3.0], assign=[0, 1, 1, 0]) == 0
    cases = [
        ([np.array([[0., 0.], [1., 0.], [1., 0.], [0., 1.]])], {}, b'zero-length'),
        ([np.array([[2., 2.]])], {}, b'at least 2'),
        ([np.array([[0., 0.], [np.nan, 0.], [1., 1.]])], {}, b'non-finite'),
        ([np.array([[0., 0.], [np.inf, 0.], [1., 1.]])], {}, b'non-finite'),
        ([sq], {'tables': (np.ones(4), np.zeros(4), np.zeros(4), np.zeros(1))}, b'lap length'),
        ([sq], {'tables': (np.ones(4), np.zeros(4), np.zeros(4), np.array([-2.0]))}, b'lap length'),
        ([sq], {'tables': (np.ones(4), np.zeros(4), np.zeros(4), np.array([np.nan]))}, b'lap length'),
        ([sq], {'tables': (np.array([1., 0., 1., 0.]), np.zeros(4), np.zeros(4), np.ones(1))}, b'zero-length'),
        ([sq], {'tables': (np.ones(4), np.array([0., 1., np.nan, 3.]), np.zeros(4), np.ones(1))}, b'not finite'),
        ([sq, sq], {'assign': [0, 2, 0, 0]}, b'raceline 2'),
        ([sq, sq], {'assign': [0, -1, 0, 0]}, b'raceline -1'),
    ]
    for lines, kw, word in cases:
        rc = _validate(lib, lines, **kw)
        assert rc == _lib.E_INVALID and word in lib.f110_last_error(), (word, lib.f110_last_error())
        with pytest.raises(ValueError):
            _lib.check(rc)
    # K < 1, null arrays, offsets that do not start at 0
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    xy, one = np.ascontiguousarray(sq), np.ones(4)
    assert lib.f110_progress_validate(p(xy), p(np.array([0, 4], dtype=np.int32)), 0, p(one), p(one), p(one), p(one), None, 1) == _lib.E_INVALID
    assert b'K=0' in lib.f110_last_error()
    assert lib.f110_progress_validate(p(xy), p(np.array([0, 4], dtype=np.int32)), 1, None, p(one), p(one), p(one), None, 1) == _lib.E_INVALID
    assert b'null' in lib.f110_last_error()
    assert lib.f110_progress_validate(p(xy), p(np.array([1, 4], dtype=np.int32)), 1, p(one), p(one), p(one), p(one), None, 1) == _lib.E_INVALID
    assert b'offsets[0]' in lib.f110_last_error()
    # the handle-taking entry points check their arguments before any HIP call
    for rc in (lib.f110_progress_install(None, p(xy), p(np.array([0, 4], dtype=np.int32)), 1, p(one), p(one), p(one), p(one), None, 1),
               lib.f110_progress_update(None, None), lib.f110_progress_bind(None, None)):
        assert rc == _lib.E_INVALID and b'null' in lib.f110_last_error()


def test_python_side_refusals():
    with pytest.raises(ValueError):
        progress.raceline_tables(np.zeros((1, 2)))
    with pytest.raises(ValueError):
        progress.raceline_xy(np.zeros(5))
    with pytest.raises(ValueError):
        progress.PackedRacelines([])
