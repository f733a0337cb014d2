"""The oracle's opponent ray cast (oracle/f110_oracle.c: orc_get_blocked_view_indices, orc_ray_cast) against the
reference at its edge geometries (g13, tests/golden/make_golden.py g13): beams at exactly 0 rad with yaw 0, the +-pi
wrap, contacts on an edge's line and on the corners, the ego inside the box, silhouette corners, opponents outside a
narrow fov, in eight (num_beams, fov) configurations.  This is what makes the oracle a valid referee for the GPU's
two implementations at these edges (tests/test_gpu_raycast_edges.py).

Spans ==; modified-beam sets == and values within 1e-11 (libm against NumPy, as test_raycast_golden), except on
rounding-decided silhouette beams, which must be answered as one of the reference's evaluations would
(tests/raycast_edges.py).
"""
import numpy as np

import oracle
from raycast_edges import g13_expected, g13_scan2, unexplained


def test_g13_covers_the_edges(golden):
    g = golden('g13_raycast_edges.npz')
    names = list(g['tag_names'])
    for t in range(len(names)):
        # every geometry class in more than one configuration
        assert len(np.unique(g['cfg'][g['tag'] == t])) >= 2, names[t]
    # corner contacts: the reference's NaN corner angle gives np.argmin's 0, a span from beam 0 and zero distances
    corner = g['tag'] == names.index('corner')
    assert (g['span'][corner, 0] == 0).all()
    assert (g['mod_val'][np.isin(g['mod_case'], np.nonzero(corner)[0])] == 0.0).all()
    # the zero-yaw alignment (ego at the origin, yaw 0, an opponent at yaw 0 whose lower edge lies on the x axis):
    # the reference leaves the beam at exactly 0 rad alone, in front of the car and behind it
    for ci in np.nonzero(g['cfg_nb'] % 2 == 1)[0]:
        nb, fov = int(g['cfg_nb'][ci]), float(g['cfg_fov'][ci])
        zero = (nb - 1) // 2
        assert -fov / 2. + zero * (fov / (nb - 1)) == 0.0
        for ox in (1.0, -1.0):
            c = np.nonzero((g['cfg'] == ci) & (g['ego'] == 0.0).all(axis=1) & (g['opp'][:, 0] == ox) &
                           (g['opp'][:, 1] == 0.31 / 2) & (g['opp'][:, 2] == 0.0))[0]
            assert len(c) >= 1
            assert not (np.isin(g['mod_case'], c) & (g['mod_beam'] == zero)).any()
    # pairs with more modified beams than one group of lanes holds (OPP_GROUP_MAX = 256) and pairs with few
    counts = np.bincount(g['mod_case'], minlength=len(g['tag']))
    assert (counts > 256).sum() > 50 and ((counts > 0) & (counts < 16)).sum() > 500


def test_oracle_raycast_edges(golden):
    g = golden('g13_raycast_edges.npz')
    names = list(g['tag_names'])
    bad, decided = [], 0
    for ci in range(len(g['cfg_nb'])):
        nb, fov = int(g['cfg_nb'][ci]), float(g['cfg_fov'][ci])
        s = oracle.Scanner(nb, fov)
        # the oracle's beam table is the reference's (-fov/2 + i * fov/(nb-1), base_classes.py:131)
        assert np.array_equal(s.scan_angles, -fov / 2. + np.arange(nb) * (fov / (nb - 1)))
        cases = np.nonzero(g['cfg'] == ci)[0]
        for scan_in in (30.0, g13_scan2(g, ci)):
            want = g13_expected(g, ci, cases, scan_in)
            base = np.array(np.broadcast_to(scan_in, (nb,)))
            for k, c in enumerate(cases):
                ego, verts = g['ego'][c], g['verts'][c]
                span = s.blocked_view_indices(ego, verts)
                if span != tuple(g['span'][c]):
                    bad.append((names[g['tag'][c]], int(c), 'span', span, tuple(g['span'][c])))
                out = s.ray_cast(ego, base, verts)
                u = unexplained(out, want[k], base, ego, [verts], s.scan_angles, 1e-11)
                if u:
                    bad.append((names[g['tag'][c]], int(c), 'beams', u[:4]))
                decided += int(((out != base) != (want[k] != base)).sum())
    assert not bad, '%d mismatches, first: %s' % (len(bad), bad[:6])
    assert decided < 100  # rounding-decided beams stay a handful among ~170 000 modified ones
