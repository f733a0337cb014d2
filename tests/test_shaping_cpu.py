"""Reward shaper without a GPU: the NumPy checker of tests/shaping_cases.py `==` the reference's own reward code on every
case of g16 (every recorded intermediate too), f110_shaping_validate's refusals, and the episode rules on a scripted clock."""
import numpy as np
import pytest

import shaping_cases as sc


def test_checker_equals_the_reference_on_g16(golden):
    g = golden('g16_shaping.npz')
    imgs = {k: sc.unpack_images(g, grp) for k, grp in enumerate(sc.GROUPS)}
    n = g['group'].shape[0]
    assert n >= 5000 and int(g['n_real']) == 36
    keys = ('px', 'py', 'collided', 'dist') + sc.TERMS
    got = {k: np.zeros(n) for k in keys}
    for i in range(n):
        r = sc.reward_terms(imgs[int(g['group'][i])][int(g['img'][i])], g['xy'][i, 0], g['xy'][i, 1], g['prev'][i, 0], g['prev'][i, 1])
        for k in keys:
            got[k][i] = r[k]
    bad = {k: int((~sc.same(got[k], g[k].astype(np.float64))).sum()) for k in keys}
    print('g16: %d cases, differing:' % n, bad)
    assert not any(bad.values()), bad
    # the fixture demonstrates every branch (the generator asserted 5 % each on the reference's results)
    reward = g['centering_term'] / 2.0
    assert (g['collided'] == 1).mean() >= 0.05 and (g['collided'] == 0).mean() >= 0.05
    assert ((reward > 0) & (reward < 1)).mean() >= 0.05 and (reward == 0.0).mean() >= 0.05 and (reward == -1.0).mean() >= 0.10
    assert np.isinf(g['xy']).sum() == 0 and (np.abs(g['xy']) == 1e300).any()
    assert {tuple(g['shape_' + grp]) for grp in sc.GROUPS} == {(256, 256), (75, 100), (40, 300)}


def test_world_to_pixel_for_every_finite_value():
    for v, want in ((0.0, 128), (-12.8, 0), (-12.85, 0), (-12.75, 0), (-12.7, 1), (12.7, 255), (12.65, 254), (1e300, 255), (-1e300, 0),
                    (1.7e308, 255), (-1.7e308, 0), (-0.04, 127), (np.nextafter(0.0, -1), 128), (0.05, 128)):
        assert sc.world_to_pixel(v, 128.0, 10.0, 255) == want, v


def test_validate_accepts_and_refuses():
    from red_gym_amd import build, shaping
    build.build()
    shaping.validate(num_agents=1)
    shaping.validate(num_agents=3, agent=2, rows=75, cols=100, neighborhood=0, scale=0.0, w_collision=0.0, clip_max=0)
    for bad in (dict(rows=0), dict(cols=-1), dict(agent=1), dict(agent=-1), dict(neighborhood=-1), dict(clip_max=-1),
                dict(scale=float('nan')), dict(origin_x=float('inf')), dict(origin_y=float('-inf')), dict(w_collision=float('nan')),
                dict(w_progress=float('inf')), dict(w_centering=float('nan')), dict(max_lane_halfwidth=0.0),
                dict(max_lane_halfwidth=-50.0), dict(max_lane_halfwidth=float('inf'))):
        with pytest.raises(ValueError):
            shaping.validate(num_agents=1, **bad)
    with pytest.raises(TypeError):
        shaping.make_config(no_such_option=1)
    from red_gym_amd import _lib
    assert _lib.load().f110_shaping_validate(None, 1) == _lib.E_INVALID
    assert {k: getattr(shaping.make_config(), k) for k in shaping.DEFAULTS} == sc.DEFAULTS


def test_episode_rules_on_a_scripted_clock():
    """Four envs: 0 steps on; 1 is reset (clock == timestep) twice in a row; 2 is left alone by a masked reset (its clock
    stands still); 3 gets a pose that is not finite."""
    dt = 0.01
    img = sc.hand_images(256, 256)[4]                      # everything filled
    imgs = np.stack([img] * 4)
    ck = sc.ShapingChecker(4, dt)
    xy = np.array([[130.0, 5.0], [131.0, 5.0], [132.0, 5.0], [133.0, 5.0]])
    out = ck.update(imgs, xy, np.full(4, dt))              # the reset: nothing paid, prev_xy taken
    assert all((out[k] == 0).all() for k in sc.TERMS) and (out['collided'] == 0).all() and np.array_equal(ck.prev_xy, xy)
    xy2 = xy + [[0.25, 0.5]]
    xy2[3, 0] = np.nan
    out = ck.update(imgs, xy2, np.array([2 * dt, dt, 2 * dt, 2 * dt]))
    assert out['progress_term'][0] == np.sqrt(0.25 * 0.25 + 0.5 * 0.5) * 10.0 == out['progress_term'][2]
    assert out['total'][1] == 0 and np.array_equal(ck.prev_xy[1], xy2[1])          # reset again: zeros, prev_xy follows
    assert all(np.isnan(out[k][3]) for k in sc.TERMS) and out['collided'][3] == 0 and np.array_equal(ck.prev_xy[3], xy[3])
    assert out['centering_term'][0] == sc.reward_terms(img, xy2[0, 0], xy2[0, 1], 0, 0)['centering_term'] == 2.0 * (1.0 - 2.5 / 50)
    xy3 = xy2 + 1.0
    xy3[3] = (140.0, 6.0)
    out3 = ck.update(imgs, xy3, np.array([3 * dt, 2 * dt, 2 * dt, 3 * dt]))         # env 2's clock stands still
    assert all(out3[k][2] == out[k][2] for k in sc.TERMS) and np.array_equal(ck.prev_xy[2], xy2[2])
    assert out3['progress_term'][0] == np.sqrt(2.0) * 10.0
    assert out3['progress_term'][3] == np.sqrt(7.0 * 7.0 + 1.0) * 10.0               # from the last finite position
    # a fresh checker (t_seen = -1) in the middle of a run pays no progress on its first update
    ck2 = sc.ShapingChecker(1, dt)
    o = ck2.update(imgs[:1], np.array([[135.0, 5.0]]), np.array([0.37]))
    assert o['progress_term'][0] == 0.0 and o['centering_term'][0] != 0.0 and np.array_equal(ck2.prev_xy[0], [135.0, 5.0])
