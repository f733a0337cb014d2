"""Shared by the tests of the opponent ray cast at its edge geometries (g13, tests/golden/make_golden.py g13):
the reference's scans rebuilt from the fixture's modified-beam triplets, and the one place where the reference's
answer is not a function of its inputs alone.

get_range (laser_models.py:250-280) forms denom and d2 with ndarray.dot, which NumPy hands to BLAS: whether the
two-term sum is evaluated with a fused multiply-add is the BLAS build's choice, not the reference's.  At a silhouette
corner d2 sits at 0 or 1 up to that last rounding, so a beam can hit with one BLAS and miss with another.  Such a beam
is "rounding-decided": an implementation passes on it if its answer is the reference's under ONE of the IEEE
evaluations of those dot products (plain, or fused in either order).

Two more answers depend on the last ulp of a libm function, which no device library reproduces bit for bit.  The GPU
decides a borderline beam with the reference's own normal cos / sin(fl(fl(yaw + angle) + pi/2)), but from the device's
sin / cos: the GPU tests (libm=True) accept on such a beam the reference's answer under a normal whose components are
each at most 1 ulp from the reference's.  And a corner whose direction lies within 4 ulp of the +-pi wrap takes the
first or the last beam as its index by the last ulp of atan2 / sin / cos: there the span may be the one the reference
would get with that corner on the other side of the wrap (wrap_spans), with every beam then checked against the
reference's formula over that span.
"""
from fractions import Fraction

import numpy as np


def g13_scan2(g, ci):
    return g['scan2'][g['scan2_off'][ci]:g['scan2_off'][ci + 1]].astype(np.float64)


def g13_expected(g, ci, cases, scan_in):
    """The reference's output scans [len(cases), nb] for configuration ci from g13's modified-beam triplets.
    scan_in: 30.0 (the constant input) or the configuration's second input (g13_scan2)."""
    nb = int(g['cfg_nb'][ci])
    pos = np.full(len(g['tag']), -1, np.int64)
    pos[cases] = np.arange(len(cases))
    out = np.tile(np.broadcast_to(np.asarray(scan_in, np.float64), (nb,)), (len(cases), 1))
    sel = pos[g['mod_case']] >= 0
    if not np.isscalar(scan_in):
        sel &= g['mod_in2']
    out[pos[g['mod_case'][sel]], g['mod_beam'][sel].astype(np.int64)] = g['mod_val'][sel]
    return out


def _dot(a, b, how):
    p0, p1 = a[0] * b[0], a[1] * b[1]
    if how == 0:
        return p0 + p1
    if how == 1:   # fma(a1, b1, a0 * b0), correctly rounded
        return float(Fraction(a[1]) * Fraction(b[1]) + Fraction(p0))
    return float(Fraction(a[0]) * Fraction(b[0]) + Fraction(p1))


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _get_range(pose, angle, va, vb, how, nudge=(0, 0)):
    """laser_models.py:250-280 with the dot products evaluated as `how` says, the normal's components moved by
    `nudge` ulps."""
    o = np.asarray(pose[:2], np.float64)
    v1, v2 = o - va, vb - va
    beam_theta = pose[2] + angle
    v3 = np.array([_ulps(np.cos(beam_theta + np.pi / 2.), nudge[0]), _ulps(np.sin(beam_theta + np.pi / 2.), nudge[1])])
    denom = _dot(v2, v3, how)
    if abs(denom) > 0.0:
        d1 = (v2[0] * v1[1] - v2[1] * v1[0]) / denom
        d2 = _dot(v1, v3, how) / denom
        return d1 if (d1 >= 0.0 and d2 >= 0.0 and d2 <= 1.0) else np.inf
    ba, ca = va - o, o - vb
    if abs(ba[0] * ca[1] - ba[1] * ca[0]) < 1e-8:
        return min(np.sqrt(_dot(va - o, va - o, 0)), np.sqrt(_dot(vb - o, vb - o, 0)))
    return np.inf


NUDGES = [(a, b) for a in (0, -1, 1) for b in (0, -1, 1)]


def beam_variants(pose, angle, opponents, scan_value, libm=False):
    """The beam's output under each evaluation of the dot products (and, with libm=True, of normals at most 1 ulp per
    component from the reference's): ray_cast's loop (laser_models.py:336-344) over the opponents in order."""
    out = []
    for nudge in (NUDGES if libm else NUDGES[:1]):
        for how in range(3):
            s = scan_value
            for verts in opponents:
                for j in range(4):
                    r = _get_range(pose, angle, verts[j], verts[(j + 1) % 4], how, nudge)
                    if r < s:
                        s = r
            out.append(s)
    return out


def wrap_spans(pose, verts, scan_angles):
    """The spans get_blocked_view_indices (laser_models.py:283-315) would give with one corner whose wrapped angle lies
    within 4 ulp of +-pi moved to the other side of the wrap (empty: no such corner)."""
    vecs = verts - pose[:2]
    with np.errstate(invalid='ignore'):   # a corner on the ego: 0 / 0, as in the reference
        u = vecs / np.sqrt(vecs[:, 0] ** 2 + vecs[:, 1] ** 2)[:, None]
    ang = np.arctan2(np.sin(pose[2]), np.cos(pose[2])) - np.arctan2(u[:, 1], u[:, 0])
    ang = np.where(ang > np.pi, ang - 2 * np.pi, np.where(ang < -np.pi, ang + 2 * np.pi, ang))
    idx = [int(np.argmin(np.abs(scan_angles - (-a)))) for a in ang]
    out = []
    for c in range(4):
        if abs(abs(ang[c]) - np.pi) <= 4 * np.spacing(np.pi):
            alt = list(idx)
            alt[c] = int(np.argmin(np.abs(scan_angles - ang[c])))   # -angle on the other side: +-pi swapped
            out.append((min(alt), max(alt)))
    return out


def cast_over(pose, verts, scan_angles, base, span):
    """ray_cast's loop (laser_models.py:336-344) over the beams of a given span, plain dot products."""
    out = np.array(base, np.float64)
    for i in range(span[0], span[1] + 1):
        out[i] = beam_variants(pose, scan_angles[i], [verts], base[i])[0]
    return out


def vertices_1ulp(opp_pose, length, width):
    """The opponent's vertices as get_vertices forms them (oracle / step path: plain sums of products) from cos / sin of
    its yaw each moved by at most 1 ulp: what a device sin / cos within 1 ulp of glibc's may compute."""
    hx = np.array([-length / 2, -length / 2, length / 2, length / 2])
    hy = np.array([width / 2, -width / 2, -width / 2, width / 2])
    out = []
    for dc, ds in NUDGES[1:]:
        c, s = _ulps(np.cos(opp_pose[2]), dc), _ulps(np.sin(opp_pose[2]), ds)
        out.append(np.stack([((c * hx + (-s) * hy) + 0. * 0.) + opp_pose[0] * 1.,
                             ((s * hx + c * hy) + 0. * 0.) + opp_pose[1] * 1.], axis=1))
    return out


def unexplained(out, want, base, pose, opponents, scan_angles, tol, libm=False, alt_opponents=()):
    """Beams where `out` differs from the reference's `want` (modified or not, or by more than tol) and the difference
    is not a rounding-decided beam answered as one of the reference's evaluations would.  opponents: the [4, 2]
    vertex arrays ray-cast in order.  Returns [(beam, out, want)]."""
    bad = []
    for i in np.nonzero(((out != base) != (want != base)) | ~(np.abs(out - want) <= tol))[0]:
        var = beam_variants(pose, scan_angles[i], opponents, base[i], libm)
        mods = {v != base[i] for v in var}
        ok = len(mods) == 2 and any((v != base[i]) == (out[i] != base[i]) and abs(v - out[i]) <= tol for v in var)
        for alt in alt_opponents:   # libm: the opponents' vertices from a sin / cos 1 ulp away
            if ok:
                break
            var = beam_variants(pose, scan_angles[i], alt, base[i], libm)
            ok = any((v != base[i]) == (out[i] != base[i]) and abs(v - out[i]) <= tol for v in var)
        if not ok:
            bad.append((int(i), float(out[i]), float(want[i])))
    return bad
