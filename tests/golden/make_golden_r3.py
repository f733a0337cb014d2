"""Round-3 golden fixture, generated in the dev container by RUNNING THE REFERENCE's own code (never shipped;
/root/reference does not exist on the GPU box):

    python tests/golden/make_golden_r3.py

  g13_raycast_edges.npz  get_vertices (collision_models.py:237-260), get_blocked_view_indices and ray_cast
                     (laser_models.py:283-346) at the geometries where an opponent ray cast goes wrong: exact
                     alignments, contacts, the +-pi wrap, beams at exactly 0 rad, silhouette corners, opponents outside
                     a narrow fov -- in several (num_beams, fov) configurations.  Per case: the ego pose, the opponent
                     pose and the vertices the reference computed from it, the configuration, a class tag and the span.
                     The scans are stored as the modified beams only: (case, beam, value) for a constant 30.0 input,
                     plus, per beam, whether a second, f32-exact input of the configuration (`scan2`) was modified too
                     (a modified beam takes the ray-cast distance whatever the input, asserted below).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

L, W = 0.58, 0.31   # the default length / width (base_classes.py:84, f110_env.py:125)
PI = np.pi

# (num_beams, fov): three odd counts with a beam at exactly 0 rad (asserted), even counts without one
CONFIGS = [(1081, 2 * PI), (1080, 2 * PI), (1079, 4.7), (271, 2 * PI), (271, 3.0), (64, 1.0), (4096, 2 * PI),
           (271, 1.0)]
ZERO_BEAM = {(1081, 2 * PI), (1079, 4.7), (271, 2 * PI), (271, 3.0), (271, 1.0)}

# class tags (the tests report failures per class)
BEARING, CASE1, EDGE_LINE, CORNER, INSIDE, SILHOUETTE, OUTSIDE_FOV = range(7)
TAGS = ['bearing', 'zero_yaw_aligned', 'edge_line', 'corner', 'inside', 'silhouette', 'outside_fov']


def scan_angles(nb, fov):
    # base_classes.py:131-132 with get_increment() = fov / (num_beams - 1) (laser_models.py:372,465)
    incr = fov / (nb - 1)
    return np.array([-fov / 2. + i * incr for i in range(nb)])


def cases_for(nb, fov, rng, cm):
    """[(tag, ego pose, opponent pose)] of one configuration; cm: the reference's collision_models."""
    out = []
    big = nb / fov > 150   # dense beams: near opponents fill hundreds of them, so they are sampled more thinly (fixture size)
    # ---- bearing sweep: opponent centre at bearing b (ego frame) and distance d
    special = [0.0, PI / 2, -PI / 2, PI, -PI, PI - 1e-12, -PI + 1e-12, PI + 1e-12, -PI - 1e-12]
    h = fov / 2
    special += [h, -h, h - 1e-3, -(h - 1e-3), h + 1e-3, -(h + 1e-3)]
    near_bearings = (0.0, PI, PI - 1e-12, -PI + 1e-12, h)
    grid = list(np.linspace(-PI, PI, 9 if big else 17)[1:-1])
    k = 0
    for b in special + grid:
        for d in (0.1, 0.3, 1.0, 5.0, 25.0, 35.0):
            near = d < 1.0
            if near and (nb == 4096 or b not in near_bearings):
                continue
            if near and big and not (b == 0.0 or (b == PI - 1e-12 and d == 0.3)):
                continue
            if nb == 4096 and d < 5.0 and b not in near_bearings:
                continue
            yaws = (0.0, rng.uniform(0, 2 * PI))
            if big and b != 0.0:
                yaws = yaws[len(out) % 2:][:1]
            for ego_yaw in yaws:
                oy_opts = [0.0, PI / 2, PI, ego_yaw, rng.uniform(0, 2 * PI)]
                opp_yaw = oy_opts[k % 5]
                k += 1
                ang = ego_yaw + b
                ego = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), ego_yaw])
                if d == 0.1 and b == 0.0:
                    ego[:2] = 0.0
                opp = np.array([ego[0] + d * np.cos(ang), ego[1] + d * np.sin(ang), opp_yaw])
                out.append((BEARING, ego, opp))
    # coincident centres
    for ego_yaw in (0.0, rng.uniform(0, 2 * PI)):
        for opp_yaw in ((0.0,) if big else (0.0, PI / 2, PI, ego_yaw, rng.uniform(0, 2 * PI))):
            ego = np.array([0.25, -0.5, ego_yaw])
            out.append((BEARING, ego, np.array([0.25, -0.5, opp_yaw])))
    # ---- the zero-yaw alignment: horizontal edges parallel to the beam at exactly 0 rad
    for ox in ((3.0, -3.0) if nb == 4096 else (1.0, -1.0, 3.0, -3.0, 0.5)):
        for oy in (W / 2, -W / 2, W, 0.05):
            out.append((CASE1, np.array([0.0, 0.0, 0.0]), np.array([ox, oy, 0.0])))
            out.append((CASE1, np.array([2.0, -1.0, 0.0]), np.array([2.0 + ox, -1.0 + oy, PI])))
    # ---- ego centre on an opponent edge's line (both at yaw 0), and around the collinear tolerance 1e-8
    for ox in ((2.5,) if nb == 4096 else (1.0, -1.0, 0.2, 2.5) if big else (1.0, -1.0, 0.2, -0.1, 0.29, 2.5)):
        for off in (0.0, 3e-9, -3e-9, 3e-8, -3e-8):
            out.append((EDGE_LINE, np.array([0.0, 0.0, 0.0]), np.array([ox, W / 2 + off, 0.0])))
            if ox in (1.0, 0.2) and not big:
                out.append((EDGE_LINE, np.array([0.0, 0.0, rng.uniform(0, 2 * PI)]), np.array([ox, W / 2 + off, 0.0])))
                out.append((EDGE_LINE, np.array([0.0, 0.0, 0.0]), np.array([ox, -W / 2 - off, 0.0])))
    # ---- ego centre exactly on each corner (the vertices as the reference computes them)
    opps = [np.array([1.0, 0.5, 0.0]), np.array([-0.4, 2.0, 0.0]), np.array([0.3, -0.7, rng.uniform(0, 2 * PI)]),
            np.array([5.0, 1.0, PI / 2])]
    for opp in (opps[:0] if nb == 4096 else opps[:2] if big else opps):
        v = cm.get_vertices(opp, L, W)
        for c in range(4):
            for ego_yaw in ((0.0,) if big else (0.0, rng.uniform(0, 2 * PI))):
                out.append((CORNER, np.array([v[c, 0], v[c, 1], ego_yaw]), opp.copy()))
    # ---- ego inside the box, centred and off-centre
    for opp_yaw in (() if nb == 4096 else (0.7,) if big else (0.0, 0.7, PI / 2)):
        for (fx, fy) in (((0.2, 0.1), (-0.25, -0.14)) if big else ((0.0, 0.0), (0.2, 0.1), (-0.25, -0.14), (0.28, 0.0), (0.0, -0.15))):
            c, s = np.cos(opp_yaw), np.sin(opp_yaw)
            opp = np.array([1.5, -2.0, opp_yaw])
            ego = np.array([opp[0] + c * fx - s * fy, opp[1] + s * fx + c * fy, 0.0 if fx == 0.2 else rng.uniform(0, 2 * PI)])
            out.append((INSIDE, ego, opp))
    # ---- silhouette corners: corner c on beam i's ray, one adjacent edge facing the ego, the other facing away
    sa = scan_angles(nb, fov)
    hx = np.array([-L / 2, -L / 2, L / 2, L / 2])
    hy = np.array([W / 2, -W / 2, -W / 2, W / 2])
    beams = sorted(set([0, nb - 1, (nb - 1) // 2, nb // 2] + list(rng.integers(0, nb, 8))))
    n_sil = 0
    for i in beams:
        for r in ((3.0,) if big else (0.7, 3.0)):
            for ego_yaw in (0.0, rng.uniform(0, 2 * PI)):
                ego = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), ego_yaw])
                th = ego_yaw + sa[i]
                P = np.array([ego[0] + r * np.cos(th), ego[1] + r * np.sin(th)])
                for opp_yaw_kind in ('zero', 'random'):
                    for tries in range(64):
                        oyaw = 0.0 if opp_yaw_kind == 'zero' else rng.uniform(0, 2 * PI)
                        c = int(rng.integers(0, 4))
                        co, so = np.cos(oyaw), np.sin(oyaw)
                        opp = np.array([P[0] - (co * hx[c] - so * hy[c]), P[1] - (so * hx[c] + co * hy[c]), oyaw])
                        v = cm.get_vertices(opp, L, W)
                        # facing of the two edges at corner c: edge (c-1 -> c) and (c -> c+1)
                        orient = (v[2, 0] - v[0, 0]) * (v[3, 1] - v[1, 1]) - (v[2, 1] - v[0, 1]) * (v[3, 0] - v[1, 0])
                        front = []
                        for e in ((c - 1) % 4, c):
                            va, vb = v[e], v[(e + 1) % 4]
                            cr = (vb[0] - va[0]) * (ego[1] - va[1]) - (vb[1] - va[1]) * (ego[0] - va[0])
                            front.append(cr * orient < 0)
                        if front[0] != front[1]:
                            out.append((SILHOUETTE, ego, opp))
                            n_sil += 1
                            break
    assert n_sil > len(beams) * 2
    # ---- opponents outside a narrow fov: fully outside and half outside (the span clamps to the end beams)
    if fov < 2 * PI:
        for side in (1, -1):
            for d in (1.0, 4.0):
                for extra in (0.6, 0.0, 0.02, -0.02):
                    for ego_yaw in (0.0, rng.uniform(0, 2 * PI)):
                        ang = ego_yaw + side * (h + extra)
                        ego = np.array([0.5, 0.5, ego_yaw])
                        opp = np.array([ego[0] + d * np.cos(ang), ego[1] + d * np.sin(ang), rng.uniform(0, 2 * PI)])
                        out.append((OUTSIDE_FOV, ego, opp))
    return out


def main():
    import ref_loader
    lm, dm, cm, bc = ref_loader.load()
    rng = np.random.default_rng(1313)
    np.seterr(all='ignore')  # the corner contacts divide 0 / 0 in get_blocked_view_indices, as the reference does
    cfg_nb, cfg_fov, scan2, scan2_off = [], [], [], [0]
    ego_a, opp_a, vert_a, cfg_a, tag_a, span_a = [], [], [], [], [], []
    m_case, m_beam, m_val, m_in2 = [], [], [], []
    n = 0
    for ci, (nb, fov) in enumerate(CONFIGS):
        sa = scan_angles(nb, fov)
        zero = sa[(nb - 1) // 2] == 0.0 if nb % 2 == 1 else False
        assert bool(zero) == ((nb, fov) in ZERO_BEAM), (nb, fov)
        assert (sa == 0.0).sum() == (1 if zero else 0)
        s2 = rng.uniform(0.05, 30.0, nb).astype(np.float32)
        s2[::17] = 30.0
        cfg_nb.append(nb); cfg_fov.append(fov)
        scan2.append(s2); scan2_off.append(scan2_off[-1] + nb)
        s2 = s2.astype(np.float64)
        for tag, ego, opp in cases_for(nb, fov, rng, cm):
            v = cm.get_vertices(opp, L, W)
            lo, hi = lm.get_blocked_view_indices(ego, v, sa)
            out30 = lm.ray_cast(ego, np.full(nb, 30.0), sa, v)
            out2 = lm.ray_cast(ego, s2.copy(), sa, v)
            mod = np.nonzero(out30 != 30.0)[0]
            mod2 = np.nonzero(out2 != s2)[0]
            assert np.all(np.isin(mod2, mod)) and np.array_equal(out2[mod2], out30[mod2])
            assert np.all((mod >= lo) & (mod <= hi))
            ego_a.append(ego); opp_a.append(opp); vert_a.append(v); cfg_a.append(ci); tag_a.append(tag)
            span_a.append((lo, hi))
            m_case.append(np.full(len(mod), n)); m_beam.append(mod); m_val.append(out30[mod])
            m_in2.append(np.isin(mod, mod2))
            n += 1
        print('  config %d: nb %d fov %.4f, cases so far %d, modified beams so far %d' % (
            ci, nb, fov, n, sum(len(x) for x in m_beam)), flush=True)
    tag_a = np.array(tag_a, np.int8)
    m_val = np.concatenate(m_val)
    for t, name in enumerate(TAGS):
        sel = tag_a == t
        print('  %-18s %5d cases' % (name, sel.sum()))
    print('  zero-distance hits (corner contacts):', int((m_val == 0).sum()))
    path = os.path.join(HERE, 'g13_raycast_edges.npz')
    np.savez_compressed(path, cfg_nb=np.array(cfg_nb, np.int32), cfg_fov=np.array(cfg_fov),
                        scan2=np.concatenate(scan2), scan2_off=np.array(scan2_off, np.int64),
                        ego=np.array(ego_a), opp=np.array(opp_a), verts=np.array(vert_a), cfg=np.array(cfg_a, np.int8),
                        tag=tag_a, tag_names=np.array(TAGS), span=np.array(span_a, np.int32),
                        mod_case=np.concatenate(m_case).astype(np.int32), mod_beam=np.concatenate(m_beam).astype(np.int16),
                        mod_val=m_val, mod_in2=np.concatenate(m_in2))
    print('wrote g13_raycast_edges.npz %.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
