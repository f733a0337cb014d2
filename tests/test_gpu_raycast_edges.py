"""Both GPU implementations of the opponent ray cast at the reference's edge geometries (g13,
tests/golden/make_golden.py g13; the oracle is pinned to the same fixture in tests/test_oracle_raycast_edges.py):

  * the function-level path (ray_cast_wave behind f110_ray_cast / Engine.ray_cast) against g13 itself: spans ==,
    modified-beam sets ==, values <= 1e-9;
  * the step path (opp_setup_body + opp_apply_kernel, what reset() and step() run) against the oracle at the same
    geometries: one env per geometry in an open room (every beam that misses the opponents reads max_range), reset()
    with the geometry's poses (the zero-action step leaves them bit-identical), then per car and beam the modified set
    ==, f64 ranges <= 1e-9 and the fp32 observation == float32 of the f64 one, bit for bit.

Rounding-decided beams (tests/raycast_edges.py) must be answered as one of the reference's evaluations of its dot
products would, with a normal at most 1 ulp per component from the reference's (the device's sin / cos); a corner within
4 ulp of the +-pi wrap may sit on either side of it (the span and every beam then as the reference's formula gives them
for that side); in the step path, which forms the opponent's vertices itself, a beam may also be answered as the
reference would for vertices from a sin / cos of the opponent's yaw 1 ulp away.  Every other beam and span is pinned exactly.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from raycast_edges import cast_over, g13_expected, g13_scan2, unexplained, vertices_1ulp, wrap_spans  # noqa: E402

L, W = 0.58, 0.31


def _check_car(out, want, base, pose, opponents, scan_angles, span=None, want_span=None, alt_opponents=()):
    """Differences of one scan that the module docstring's rules do not explain: [] if none."""
    if span is None or span == want_span:
        u = unexplained(out, want, base, pose, opponents, scan_angles, 1e-9, libm=True, alt_opponents=alt_opponents)
        if not u:
            return []
    else:
        u = [('span', span, want_span)]
    if len(opponents) == 1:
        # a corner at the +-pi wrap on the other side: the reference's formula over that span
        for alt in wrap_spans(pose, opponents[0], scan_angles):
            if span is not None and span != alt:
                continue
            if not unexplained(out, cast_over(pose, opponents[0], scan_angles, base, alt), base, pose, opponents,
                               scan_angles, 1e-9, libm=True):
                return []
    return u[:3]


def _np(t):
    return t.detach().cpu().numpy()


def test_function_level_vs_g13(golden):
    from red_gym_amd.engine import Engine
    g = golden('g13_raycast_edges.npz')
    names = list(g['tag_names'])
    bad = []
    for ci in range(len(g['cfg_nb'])):
        nb, fov = int(g['cfg_nb'][ci]), float(g['cfg_fov'][ci])
        e = Engine(num_envs=1, num_agents=1, noise_std=0, num_beams=nb, fov=fov)
        assert np.array_equal(e.scan_angles, -fov / 2. + np.arange(nb) * (fov / (nb - 1)))
        cases = np.nonzero(g['cfg'] == ci)[0]
        for scan_in in (30.0, g13_scan2(g, ci)):
            want = g13_expected(g, ci, cases, scan_in)
            base = np.array(np.broadcast_to(scan_in, (nb,)))
            out, span = e.ray_cast(g['ego'][cases], g['verts'][cases], np.tile(base, (len(cases), 1)))
            out, span = _np(out), _np(span)
            for k, c in enumerate(cases):
                u = _check_car(out[k], want[k], base, g['ego'][c], [g['verts'][c]], e.scan_angles,
                               tuple(int(x) for x in span[k]), tuple(int(x) for x in g['span'][c]))
                if u:
                    bad.append((names[g['tag'][c]], int(c), nb, 'span or beams (beam, gpu, reference)', u))
        e.close()
    assert not bad, '%d mismatches, first: %s' % (len(bad), bad[:8])


def _room(half=80.0, res=0.25):
    """An empty square room, walls more than max_range (30 m) from every car of g13 (all within 10 m of the origin)."""
    from scipy.ndimage import distance_transform_edt
    n = int(2 * half / res)
    free = np.ones((n, n), np.uint8)
    free[[0, -1], :] = 0
    free[:, [0, -1]] = 0
    m = {'height': n, 'width': n, 'resolution': res, 'orig_x': -half, 'orig_y': -half, 'orig_s': 0.0, 'orig_c': 1.0,
         'dt': np.ascontiguousarray(res * distance_transform_edt(free)), 'img': free * 255.}
    return free, m


def _step_path_vs_oracle(poses, nb, fov, sizes=None, check_env=4):
    """reset(poses) of one F110VecEnv [B, A] in the open room against the oracle: per car a's scan = the map scan plus
    noise row 0, then ray_cast against every other car in agent order with vertices of car a's OWN length / width
    (base_classes.py:204-225, 221).  sizes: [A] (length, width) per agent (update_params per agent) or None."""
    from red_gym_amd import F110VecEnv
    from red_gym_amd.engine import DEFAULT_PARAMS
    B, A = poses.shape[:2]
    free, m = _room()
    env = F110VecEnv(B, num_agents=A, num_beams=nb, fov=fov, autoreset=False, keep_f64_scans=True)
    env.update_map_occupancy(free, m['resolution'], m['orig_x'], m['orig_y'])
    if sizes is not None:
        for a in range(A):
            p = dict(DEFAULT_PARAMS)
            p['length'], p['width'] = sizes[a]
            env.update_params(p, a)
    obs, _, _, _ = env.reset(poses)
    st, s64, s32 = _np(env.state), _np(obs['scans_f64']), _np(obs['scans'])
    env.close()
    # the zero-action step of reset leaves the poses bit-identical (yaws in [0, 2pi]: no wrap)
    assert np.array_equal(st[..., [0, 1, 4]], poses)
    assert np.array_equal(s32.view(np.uint32), s64.astype(np.float32).view(np.uint32))
    sc = oracle.Scanner(nb, fov)
    sc.set_map_dict(m)
    noise = oracle.noise_table(12345, 2, num_beams=nb)
    base = sc.scan_batch(poses.reshape(-1, 3)).reshape(B, A, nb) + noise[0]
    lw = [(L, W)] * A if sizes is None else sizes
    want = base.copy()
    verts = {}
    for b in range(B):
        for a in range(A):
            for j in range(A):
                if j != a:
                    verts[b, a, j] = oracle.get_vertices(poses[b, j], *lw[a])
                    want[b, a] = sc.ray_cast(poses[b, a], want[b, a], verts[b, a, j])
    if sizes is None:
        # the composition above is the oracle's own Env.reset (Simulator.step with noise)
        for b in range(min(B, check_env)):
            o = oracle.Env(sc, A, noise=noise).reset(poses[b])
            assert np.array_equal(o['scans'], want[b])
    bad = []
    for b in range(B):
        for a in range(A):
            alt = [[v] for v in vertices_1ulp(poses[b, 1 - a], *lw[a])] if A == 2 else []
            u = _check_car(s64[b, a], want[b, a], base[b, a], poses[b, a], [verts[b, a, j] for j in range(A) if j != a],
                           sc.scan_angles, alt_opponents=alt)
            if u:
                bad.append((b, a, u[:3]))
    return bad


@pytest.mark.parametrize('ci', range(8))
def test_step_path_two_agents_vs_oracle(golden, ci):
    """Every g13 geometry of one configuration as one env of two cars (B in the hundreds in one launch: short and long
    interval lists, more than OPP_GROUP_MAX beams, in the same wave).  Both cars are checked: each is the other's
    opponent."""
    g = golden('g13_raycast_edges.npz')
    names = list(g['tag_names'])
    nb, fov = int(g['cfg_nb'][ci]), float(g['cfg_fov'][ci])
    cases = np.nonzero(g['cfg'] == ci)[0]
    poses = np.stack([g['ego'][cases], g['opp'][cases]], axis=1)
    # a corner contact puts the ego on the corner the reference computed with ndarray.dot; the step path and the oracle
    # compute the vertices as plain sums of products: the ego goes on THAT corner (the nearest one)
    for k, c in enumerate(cases):
        if names[g['tag'][c]] == 'corner':
            v = oracle.get_vertices(poses[k, 1], L, W)
            poses[k, 0, :2] = v[np.argmin(np.hypot(*(v - poses[k, 0, :2]).T))]
    bad = _step_path_vs_oracle(poses, nb, fov)
    bad = [(names[g['tag'][cases[b]]], int(cases[b]), a, u) for b, a, u in bad]
    assert not bad, '%d cars differ (nb %d, fov %.4f), first: %s' % (len(bad), nb, fov, bad[:8])


def test_step_path_many_agents_occluding_vs_oracle():
    """32 cars per env in a ring and in a line, occluding one another: the in-place minimum over the opponents in
    agent order, on 1081 beams (a beam at exactly 0 rad) with yaws of exactly 0 among them."""
    rng = np.random.default_rng(7)
    A, envs = 32, []
    for k in range(6):
        r = 1.2 + 0.8 * k
        th = 2 * np.pi * np.arange(A) / A
        ring = np.stack([r * np.cos(th), r * np.sin(th), (th + np.pi / 2) % (2 * np.pi) if k % 2 else np.zeros(A)], axis=1)
        envs.append(ring)
        line = np.stack([0.7 * (np.arange(A) - 3) + 0.01 * k, np.full(A, 0.0 if k < 3 else W / 2 * (k - 3)),
                         np.zeros(A) if k % 2 == 0 else rng.uniform(0, 2 * np.pi, A)], axis=1)
        envs.append(line)
    poses = np.array(envs)
    bad = _step_path_vs_oracle(poses, 1081, 2 * np.pi)
    assert not bad, '%d cars differ, first: %s' % (len(bad), bad[:8])


def test_step_path_own_sizes_vs_oracle(golden):
    """update_params per agent: a car sizes its opponents with its OWN length and width (base_classes.py:221)."""
    g = golden('g13_raycast_edges.npz')
    ci = 0
    cases = np.nonzero((g['cfg'] == ci) & (g['tag'] != list(g['tag_names']).index('corner')))[0]
    poses = np.stack([g['ego'][cases], g['opp'][cases]], axis=1)
    bad = _step_path_vs_oracle(poses, int(g['cfg_nb'][ci]), float(g['cfg_fov'][ci]), sizes=[(0.9, 0.5), (0.4, 0.2)])
    assert not bad, '%d cars differ, first: %s' % (len(bad), bad[:8])
