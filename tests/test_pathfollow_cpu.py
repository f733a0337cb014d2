"""Path follower without a GPU: the NumPy checker of tests/path_cases.py against every record of g17 (the reference's own
outputs), the enumerator's answers against the KKT conditions, f110_pathfollow_validate's refusals, the ABI's symbols and the
state machine on a scripted clock."""
import numpy as np
import pytest

import path_cases as pc


def _report(what, got, want):
    ok, worst = pc.close(got, want)
    print('%-12s largest |got - want| / max(1, |want|) = %.3g' % (what, worst))
    assert ok, (what, worst)


def test_checker_against_every_record_of_g17(golden):
    g = golden('g17_paths.npz')
    n = g['raw'].shape[0]
    assert n >= 700
    inc = pc.clamp_angles(g['raw'])[0]
    _report('increments', inc, g['increments'])
    _report('paths', pc.global_path(g['increments'], g['poses']), g['paths'])
    _report('decode', pc.decode(g['raw'], g['poses']), g['paths'])
    x, ref = pc.reference_states(g['paths'], pc.config(horizon=8))
    _report('dists', x, g['dists'])
    _report('ref_traj', ref, g['ref_traj'])
    new, dist = pc.advance(g['paths'], g['index'], g['xy'])
    assert np.array_equal(new, g['index_out']) and np.abs(dist - 0.2).min() >= 1e-6
    _report('converter', pc.convert(g['conv_in'])[0], g['conv_out'])
    # the fixture demonstrates every branch (the generator asserted 5 % each on the reference's results)
    assert 0.05 <= (g['index_out'] != g['index']).mean() <= 0.95
    clipped = np.abs(g['conv_out'][:, 0]) == 0.4189
    assert 0.05 <= clipped.mean() <= 0.95 and (~clipped[:n]).mean() >= 0.05
    assert (np.abs(g['raw']) <= 1.0).all() and (g['raw'].reshape(n, 8, 2) == 0).all(axis=2).mean() >= 0.02
    assert g['vels'][:, 0].min() < -4.0 and g['vels'][:, 0].max() > 19.0 and np.abs(g['poses'][:, :2]).max() > 90.0


@pytest.mark.parametrize('cfg', [dict(), dict(horizon=1), dict(horizon=3, q=(2.0, 0.5, 0.0, 0.3), r=(0.05, 0.2), p=(4.0, 20.0, 0.5, 2.0)),
                                 dict(horizon=8, timestep=0.05, desired_velocity=3.0)])
def test_enumerator_satisfies_kkt(golden, cfg):
    """The enumerator's optimum satisfies the KKT conditions of its QP to rounding, on g17's cases and on scaled linear terms
    that make bounds bind; for a strictly convex QP that makes it THE optimum."""
    g = golden('g17_paths.npz')
    c = pc.config(**cfg)
    m = slice(0, 780 if c['horizon'] <= 5 else 60)
    _, ref = pc.reference_states(g['paths'][m], c)
    for axis in range(2):
        Hm, f = pc.qp_terms(ref, g['paths'][m, 0, axis], g['vels'][m, axis], axis, c)
        assert np.allclose(Hm, Hm.T) and np.linalg.eigvalsh(Hm).min() >= c['r'][axis] * (1 - 1e-12)
        for scale in (1.0, 0.05):
            u, pat, viol = pc.solve_box_qp(Hm, f * scale)
            tol = 1e-12 * max(1.0, np.abs(f * scale).max())
            assert viol.max() <= tol and pc.kkt_violation(Hm, f * scale, u).max() <= 1e-9
            assert (np.abs(u) <= 1.0).all() and ((np.abs(u) == 1.0) >= (pat != 0)).all()


def test_validate_accepts_and_refuses():
    from red_gym_amd import _lib, build, pathfollow
    build.build()
    pathfollow.validate(num_agents=1)
    pathfollow.validate(num_agents=3, agent=2, horizon=8, replan_at=1, q=(0, 0, 0, 0), p=(0, 0, 0, 0), r=(1e-6, 5.0), dist_threshold=0.0)
    pathfollow.validate(num_agents=1, car_length=-0.3, desired_velocity=-2.0, max_diff_deg=0.0, max_steer=0.0)   # (the GPU test runs these)
    for name, entry in pc.CONFIGS.items():
        pathfollow.validate(num_agents=1, **entry['cfg'])
    pathfollow.validate(num_agents=1, **pc.EDGE_DIAGONAL)
    pathfollow.validate(num_agents=1, **pc.EDGE_STIFF)
    for bad in (dict(agent=1), dict(agent=-1), dict(horizon=0), dict(horizon=9), dict(replan_at=0), dict(replan_at=9),
                dict(r=(0.0, 0.1)), dict(r=(0.1, -1.0)), dict(q=(-1.0, 1, 1, 1)), dict(q=(1, 1, 1, -0.1)), dict(p=(1, -2.0, 1, 1)),
                dict(p=(1, 1, -1e-9, 1)), dict(r=(float('nan'), 0.1)), dict(max_steer=float('inf')), dict(car_length=float('nan')),
                dict(vector_length=0.0), dict(timestep=0.0), dict(desired_velocity=float('inf')),
                dict(max_diff_deg=-10.0), dict(max_diff_deg=-1e-300), dict(max_steer=-0.4189), dict(dist_threshold=-0.2), dict(vector_length=-0.5)):
        with pytest.raises(ValueError):
            pathfollow.validate(num_agents=1, **bad)
    with pytest.raises(TypeError):
        pathfollow.make_config(no_such_option=1)
    with pytest.raises(ValueError):
        pathfollow.make_config(q=(1.0, 1.0))
    assert _lib.load().f110_pathfollow_validate(None, 1) == _lib.E_INVALID
    c = pathfollow.make_config()
    got = {k: (tuple(getattr(c, k)) if isinstance(v, tuple) else getattr(c, k)) for k, v in pathfollow.DEFAULTS.items()}
    assert got == pc.DEFAULTS == pathfollow.DEFAULTS


def test_state_machine_on_a_scripted_clock():
    """Three envs: 0 drives on and reaches its waypoints; 1 is reset; 2 is left alone by a masked reset."""
    dt = 0.01
    ck = pc.FollowChecker(3, dt, replan_at=2)
    raw = np.tile(np.r_[1.0, 0.0], 8)[None].repeat(3, axis=0)
    poses = np.zeros((3, 3))
    act, acc, rep = ck.act(raw, poses, np.full(3, 2.0))
    assert rep.tolist() == [1, 1, 1] and ck.index.tolist() == [0, 0, 0]
    assert np.allclose(ck.paths[0, :, 0], 0.3 + 0.5 * np.arange(1, 9)) and np.allclose(ck.paths[0, :, 1], 0.0)
    assert np.allclose(acc, 0.0, atol=1e-9)               # on the path at the desired velocity: nothing to correct
    ck.update(np.array([[0.75, 0.0], [0.0, 0.0], [0.0, 0.0]]), np.array([2 * dt, 2 * dt, 2 * dt]))
    assert ck.index.tolist() == [1, 0, 0]
    assert ck.act(raw, poses, np.full(3, 2.0))[2].tolist() == [0, 0, 0]
    ck.update(np.array([[1.25, 0.0], [0.8, 0.0], [0.8, 0.0]]), np.array([3 * dt, dt, 2 * dt]))   # 1: reset; 2: clock stands still
    assert ck.index.tolist() == [2, -1, 0]
    assert ck.act(raw, poses, np.full(3, 2.0))[2].tolist() == [1, 1, 0] and ck.index.tolist() == [0, 0, 0]
    assert ck.replans.tolist() == [2, 2, 1] and ck.advances.tolist() == [2, 0, 0]


# ---------------------------------------------------------------- off the defaults: g19 and the case families of path_cases
def test_checker_against_every_record_of_g19(golden):
    """The reference's records at the off-default configurations (tests/golden/make_golden.py g19)."""
    g = golden('g19_path_configs.npz')
    assert {k.split('/')[0] for k in g.files} == set(pc.CONFIGS)
    for name, entry in pc.CONFIGS.items():
        c = pc.config(**entry['cfg'])
        raw, poses, vels = pc.g19_inputs(name)
        rec = {k: g['%s/%s' % (name, k)] for k in ('increments', 'paths', 'dists', 'ref_traj', 'conv_in', 'conv_out')}
        assert rec['paths'].shape == (pc.G19_CASES, 8, 2) and rec['ref_traj'].shape == (pc.G19_CASES, c['horizon'] + 1, 4)
        _report(name + ' inc', pc.clamp_angles(raw, c['max_diff_deg'])[0], rec['increments'])
        _report(name + ' paths', pc.decode(raw, poses, c), rec['paths'])
        x, ref = pc.reference_states(rec['paths'], c)
        _report(name + ' dists', x, rec['dists'])
        _report(name + ' ref', ref, rec['ref_traj'])
        _report(name + ' accel', pc.mpc_accel(rec['paths'], vels, c)[0], rec['conv_in'])
        _report(name + ' conv', pc.convert(rec['conv_in'], c['max_steer'])[0], rec['conv_out'])


def _config_features(name, g):
    """What a g19 config demonstrates, read off the reference's records."""
    c = pc.config(**pc.CONFIGS[name]['cfg'])
    vl, H = c['vector_length'], c['horizon']
    piece, clamped, _ = pc.spline_pieces(g[name + '/paths'], c)
    feats = {('g19 horizon', H)}
    feats |= {('piece', j, vl) for j in range(7) if ((piece == j) & ~clamped).mean() >= 0.05}
    if clamped.mean() >= 0.05:
        feats.add(('end clamp', vl, int(np.flatnonzero(clamped.all(axis=0))[0])))
    if c['car_length'] != 0.3:
        feats.add(('car_length', c['car_length']))
    inc = g[name + '/increments']
    head = np.arctan2(inc[..., 1], inc[..., 0])
    turn = np.abs(np.mod(head[:, 1:] - head[:, :-1] + np.pi, 2 * np.pi) - np.pi)
    at_limit = np.abs(turn - np.deg2rad(c['max_diff_deg'])) < 1e-9
    if c['max_diff_deg'] != 10.0:
        feats.add(('segments at the limit', c['max_diff_deg'], 'none' if not at_limit.any() else 'nearly all' if at_limit.mean() >= 0.9 else 'some'))
    steer = np.abs(g[name + '/conv_out'][:, 0])
    if c['max_steer'] != 0.4189:
        feats.add(('steer clipped', c['max_steer'], 'never' if (steer < c['max_steer']).all() else 'mostly' if (steer == c['max_steer']).mean() >= 0.5 else 'some'))
    if c['q'][0] != c['q'][1] and c['r'][0] != c['r'][1] and c['p'][0] != c['p'][1]:
        feats.add(('weights differ per axis', H))
    return feats


def _family_features(name):
    f = pc.family(name)
    H = f['cfg']['horizon']
    feats = {(name, k) for k in pc.walk_classes(f['info'], H)}
    if name == 'release_order':
        agree = f['info']['stable'] & f['tells'] & (f['info']['steps'] != f['first'])
        feats |= {(name, 'first and worst release differ in steps')} if agree.sum() >= 6 else set()
    if name.startswith('bound'):
        for kind in (0, 1):
            feats |= {('on a bound', H, kind)} if (f['kind'] == kind).sum() >= 20 else set()
    return feats


REQUIRED = (
    {('piece', j, 0.5) for j in range(7)} | {('end clamp', 0.5, 8)}                                  # late_pieces
    | {('piece', j, 0.25) for j in range(7)}                                                            # short_chords
    | {('end clamp', 0.125, 5), ('car_length', 0.0)}                                                    # short_clamped
    | {('piece', 0, 1.5), ('car_length', 0.55), ('g19 horizon', 6)}                                     # long_chords
    | {('segments at the limit', 180.0, 'none'), ('steer clipped', 0.1, 'mostly')}                      # nothing_clamps
    | {('segments at the limit', 0.5, 'nearly all'), ('steer clipped', 3.2, 'never')}                   # all_clamps
    | {('g19 horizon', 2), ('g19 horizon', 4), ('g19 horizon', 7), ('weights differ per axis', 4)}      # horizon_2, _4, _7
    | {('qp horizon', H) for H in range(1, 9)}                                                          # QP_CONFIGS
    | {('on a bound', H, kind) for H in pc.BOUND_HORIZONS for kind in (0, 1)}                           # bound2, bound5, bound8
    | {('bound%d' % H, k) for H in pc.BOUND_HORIZONS for k in ('blocks only', 'all bound', 'none bound', 'mixed')}
    | {('stiff', k) for k in ('blocks only', 'a release', 'blocks and releases', 'all bound', 'none bound', 'mixed')}
    | {('release_order', 'first and worst release differ in steps')}
    | {('diagonal', 'none bound')})


def test_case_tables_cover_the_kernels_paths(golden):
    """Every spline piece and the end clamp, every horizon, every arm of the walk and every kind of optimum occur in the tables the
    follower's tests run -- and each config and family is needed: without any one of them something REQUIRED is missing."""
    g = golden('g19_path_configs.npz')
    parts = {'config ' + n: _config_features(n, g) for n in pc.CONFIGS}
    parts.update({'family ' + n: _family_features(n) for n in pc.FAMILIES})
    parts.update({'qp config %d' % i: {('qp horizon', pc.config(**c)['horizon'])} for i, c in enumerate(pc.QP_CONFIGS)})
    have = set().union(*parts.values())
    for name, feats in sorted(parts.items()):
        print('%-22s %s' % (name, sorted(feats, key=str)))
    assert REQUIRED <= have, REQUIRED - have
    for name in parts:
        if name in ('qp config 0', 'qp config 3'):       # (horizons 5 and 8 of the first tests: the g19 configs run them too)
            continue
        rest = set().union(*(f for n, f in parts.items() if n != name))
        assert not REQUIRED <= rest, '%s demonstrates nothing of its own' % name
    assert {pc.config(**c)['horizon'] for c in pc.QP_CONFIGS} == set(range(1, 9))
    # the stationary point, non-uniform chords and exact directions are what they are called
    paths, cfg, k = pc.stationary_case()
    _, ref = pc.reference_states(paths, cfg)
    x = pc.chord_lengths(paths[:1])
    s, dx, sl = pc.notaknot_slopes(x, paths[:1, :, 0])
    assert abs(pc.spline_eval(x, paths[:1, :, 0], s, dx, sl, np.array([cfg['desired_velocity'] * (k * cfg['timestep'])]))[1][0]) < 1e-6
    assert (ref[:, k, 2:] == 0.0).all() and (np.abs(ref[:, [j for j in range(6) if j != k], 2:]).max(axis=2) > 1.0).all()
    d = np.diff(pc.chord_lengths(pc.nonuniform_paths(pc.g17_paths())), axis=1)
    ratio = d[:, 1:] / d[:, :-1]
    for col in (0, 5):                                    # the not-a-knot rows: both ends, both ways
        assert ratio[:, col].max() >= pc.CHORD_RATIO * (1 - 1e-9) and ratio[:, col].min() <= (1 + 1e-9) / pc.CHORD_RATIO
    raw, _ = pc.exact_direction_cases()
    _, diffs, args = pc.clamp_angles(raw)
    assert (args == 2 * np.pi).any() and (args == 0.0).any() and (diffs == -np.pi).sum() >= 2 * 6 * 10


def test_walk_agrees_with_the_enumerator_and_the_families_are_well_posed():
    """walk() -- the classifier -- ends on the enumerator's optimum to 1e-9 on every family, within the kernel's step bound;
    at most 5 % of the on-a-bound designs were dropped as ill-posed; the designs are on their bounds."""
    for name in pc.FAMILIES:
        f = pc.family(name)
        H, info = f['cfg']['horizon'], f['info']
        for axis, (Hm, fl) in enumerate(pc.qp_of(f['paths'], f['vels'], f['cfg'])):
            u, blocks, rels, steps, done = pc.walk(Hm, fl)
            err = np.abs(u - info['u'][:, axis]).max()
            print('%-9s axis %d: |walk - enumerator| %.3g, steps <= %d, blocks <= %d, releases <= %d' % (name, axis, err, steps.max(), blocks.max(), rels.max()))
            assert done.all() and err <= 1e-9 and steps.min() >= 1 and steps.max() <= 4 * H + 2
            assert pc.kkt_violation(Hm, fl, info['u'][:, axis]).max() <= 1e-9 * max(1.0, np.abs(fl).max())
        if name.startswith('bound'):
            assert f['dropped'] <= 0.05 and (info['spread'] <= 1e-9).all()
            slack, mult = [], []
            for axis, (Hm, fl) in enumerate(pc.qp_of(f['paths'], f['vels'], f['cfg'])):
                un = -fl @ np.linalg.inv(Hm).T
                slack.append(np.abs(np.abs(un) - 1.0).min(axis=1))
                u = info['u'][:, axis]
                gr = np.abs(u @ Hm.T + fl) / np.maximum(1.0, np.abs(fl).max(axis=1))[:, None]
                mult.append(np.where(np.abs(u) == 1.0, gr, np.inf).min(axis=1))
            assert (np.maximum(*slack)[f['kind'] == 0] <= 1.1e-8).all()         # both axes of every design of kind (a)
            assert (np.minimum(*mult)[f['kind'] == 1] <= 1.1e-8).sum() >= 6     # kind (b): the designs whose face is the optimum's
            for d in (-1e-13, -1e-11, -1e-8):                                   # either side of PF_TOL_G, each at every horizon
                hit = (f['kind'] == 1) & (f['delta'] == d) & (np.minimum(*mult) <= 1.1 * abs(d))
                assert hit.sum() >= 1, (name, d)
    # the per-set enumerator that mpc_accel uses from horizon 6 on is the per-pattern one: same patterns, same u
    c6 = pc.config(horizon=6, p=(30.0, 30.0, 3.0, 3.0))
    p6 = pc.g17_paths()[:40]
    for Hm, fl in pc.qp_of(p6, pc.built_cases(p6, c6, 2140), c6):
        a, b = pc.solve_box_qp(Hm, fl), pc.solve_box_qp_by_sets(Hm, fl)
        assert np.array_equal(a[1], b[1]) and np.abs(a[0] - b[0]).max() <= 1e-13 and len(set(map(tuple, a[1]))) >= 5
    st = pc.family('stiff')
    print('stiff: e_ref = %.3g' % st['e_ref'])
    assert 0.0 < st['e_ref'] < 1e-9 / 16                                     # so the device's bound max(1e-9, 16 e_ref) is 1e-9
    e_exact = pc.stiff_cases(pc.g17_paths(), 8, exact=True)[3]              # what a host without a wider float would use: four cases, exact
    print('stiff: e_ref from exact rationals on four cases = %.3g' % e_exact)
    assert 0.0 < e_exact < 1e-9 / 16
    dg = pc.family('diagonal')
    for axis, (Hm, fl) in enumerate(pc.qp_of(dg['paths'], dg['vels'], dg['cfg'])):
        assert np.array_equal(Hm, np.diag(np.diag(Hm))) and np.array_equal(dg['info']['u'][:, axis], np.clip(-fl / np.diag(Hm), -1.0, 1.0))


def test_nonuniform_chords_are_within_the_checkers_own_rounding():
    """reference_states on the non-uniform paths in fp64 and in np.longdouble differ by less than 1e-10 at CHORD_RATIO, so
    the 1e-9 rule holds for them with the dense fp64 solve as the expectation."""
    paths = pc.nonuniform_paths(pc.g17_paths())
    c = pc.config(horizon=8)
    x, ref = pc.reference_states(paths, c)
    xl, refl = pc.reference_states(paths.astype(np.longdouble), c)
    err = float(np.abs(ref - refl).max())
    print('ratio %g: fp64 against longdouble %.3g' % (pc.CHORD_RATIO, err))
    assert np.finfo(np.longdouble).eps < 1e-18 and err <= 1e-10
