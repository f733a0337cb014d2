"""CHECKER and pose sets for the progress tracker (csrc/f110_progress.h) -- test infrastructure, never imported by the
product.  The checker restates DESIGN.md section 3 "Progress along the raceline" line by line in NumPy scalars, on top of
oracle.planner.Raceline.nearest (the reference's nearest_point_on_trajectory expression, pinned on the reference itself by
tests/golden/g15_nearest.npz); the tests demand `==` of it for every output of the kernel."""
import os

import numpy as np

from oracle.planner import Raceline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_WAYPOINTS = os.path.join(ROOT, 'red_gym_amd', 'assets', 'example_waypoints.csv')


def example_raceline():
    """[783, 3] = (x, y, speed) of the shipped raceline, the columns the reference's planner reads."""
    w = np.loadtxt(EXAMPLE_WAYPOINTS, delimiter=';', skiprows=3)
    return np.ascontiguousarray(w[:, [1, 2, 5]])


class FrenetChecker(object):
    """One raceline: tables and the per-pose quantities, each line the definition's."""

    def __init__(self, xy):
        self.line = Raceline(np.asarray(xy, dtype=np.float64)[:, :2])
        p = self.line.xy
        dx, dy = p[1:, 0] - p[:-1, 0], p[1:, 1] - p[:-1, 1]
        self.dx, self.dy = dx, dy
        self.len = np.sqrt(dx * dx + dy * dy)
        self.cum = np.concatenate([[0], np.cumsum(self.len)])
        self.psi = np.arctan2(dy, dx)
        ex, ey = p[0, 0] - p[-1, 0], p[0, 1] - p[-1, 1]
        self.L = self.cum[p.shape[0] - 1] + np.sqrt(ex * ex + ey * ey)

    def nearest(self, px, py):
        """(i, t, dist, projection) of the reference's nearest_point_on_trajectory."""
        dist, t, i = self.line.nearest(np.array([px, py]))
        return i, t, dist, self.line.xy[i] + t * self.line.seg[i]

    def frenet(self, px, py, yaw):
        """(seg, s, d, heading_error) -- steps 1 to 4; a non-finite px or py gives (0, nan, nan, nan) (step 6)."""
        if not (np.isfinite(px) and np.isfinite(py)):
            return 0, np.nan, np.nan, np.nan
        i, t, dist, _ = self.nearest(px, py)
        s = self.cum[i] + t * self.len[i]
        x0, y0 = self.line.xy[i]
        cross = self.dx[i] * (py - y0) - self.dy[i] * (px - x0)
        d = dist if cross >= 0 else -dist
        e = yaw - self.psi[i]
        if e > np.pi:
            e -= 2 * np.pi
        if e <= -np.pi:
            e += 2 * np.pi
        return i, s, d, e


def frenet_many(ck, poses, chunk=2048):
    """FrenetChecker.frenet for poses [n, 3] at once: the same expressions element by element on [chunk, segments] arrays
    (tests/test_progress_cpu.py holds it `==` the scalar form).  Returns (seg, t, dist, s, d, heading_error) arrays [n]."""
    poses = np.asarray(poses, dtype=np.float64)
    n = poses.shape[0]
    seg, t_out, dist = np.zeros(n, dtype=np.int32), np.full(n, np.nan), np.full(n, np.nan)
    a, sg, l2 = ck.line.xy[:-1], ck.line.seg, ck.line.len2
    fin = np.isfinite(poses[:, 0]) & np.isfinite(poses[:, 1])
    idx = np.flatnonzero(fin)
    for lo in range(0, idx.shape[0], chunk):
        k = idx[lo:lo + chunk]
        px, py = poses[k, 0][:, None], poses[k, 1][:, None]
        rx, ry = px - a[None, :, 0], py - a[None, :, 1]
        t = np.clip((rx * sg[None, :, 0] + ry * sg[None, :, 1]) / l2[None, :], 0.0, 1.0)
        ox, oy = px - (a[None, :, 0] + t * sg[None, :, 0]), py - (a[None, :, 1] + t * sg[None, :, 1])
        dd = np.sqrt(ox * ox + oy * oy)
        i = np.argmin(dd, axis=1)
        r = np.arange(k.shape[0])
        seg[k], t_out[k], dist[k] = i, t[r, i], dd[r, i]
    px, py, yaw = poses[:, 0], poses[:, 1], poses[:, 2]
    with np.errstate(invalid='ignore'):
        s = ck.cum[seg] + t_out * ck.len[seg]
        cross = ck.dx[seg] * (py - a[seg, 1]) - ck.dy[seg] * (px - a[seg, 0])
        d = np.where(cross >= 0, dist, -dist)
        e = yaw - ck.psi[seg]
        e = np.where(e > np.pi, e - 2 * np.pi, e)
        e = np.where(e <= -np.pi, e + 2 * np.pi, e)
    s, d, e = np.where(fin, s, np.nan), np.where(fin, d, np.nan), np.where(fin, e, np.nan)
    return seg, t_out, dist, s, d, e


class ProgressCheckerMany(object):
    """ProgressChecker on arrays (the same steps 5 and 6 with np.where), for the large pose sets of the GPU tests."""

    def __init__(self, checkers, of_car):
        self.checkers, self.of_car = list(checkers), np.asarray(of_car)
        n = self.of_car.shape[0]
        self.progress, self.s_prev, self.seen = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)

    def update(self, poses, reset):
        poses, reset = np.asarray(poses, dtype=np.float64), np.asarray(reset, dtype=bool)
        n = self.of_car.shape[0]
        seg, s, d, e, L = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        for k, ck in enumerate(self.checkers):
            m = self.of_car == k
            if m.any():
                seg[m], _, _, s[m], d[m], e[m] = frenet_many(ck, poses[m])
                L[m] = ck.L
        fin = np.isfinite(poses[:, 0]) & np.isfinite(poses[:, 1])
        restart = reset | ~self.seen
        with np.errstate(invalid='ignore'):
            delta = s - self.s_prev
            delta = np.where(delta >= L / 2, delta - L, delta)
            delta = np.where(delta < -L / 2, delta + L, delta)
        delta = np.where(restart, 0.0, delta)
        progress = np.where(restart, 0.0, self.progress + delta)
        self.progress = np.where(fin, progress, self.progress)
        self.s_prev = np.where(fin, s, self.s_prev)
        self.seen = np.where(fin, True, np.where(restart, False, self.seen))
        delta = np.where(fin, delta, np.nan)
        return {'seg': seg, 's': s, 'd': d, 'heading_error': e, 'delta': delta, 'progress': self.progress.copy()}


class ProgressChecker(object):
    """The tracker of n cars: car c drives on checkers[of_car[c]]; update() is one f110_progress_update."""

    def __init__(self, checkers, of_car):
        self.checkers, self.of_car = list(checkers), np.asarray(of_car)
        n = self.of_car.shape[0]
        self.progress, self.s_prev, self.seen = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)

    def update(self, poses, reset):
        """poses [n, 3] = (x, y, yaw); reset [n] bool = the car's env was reset by its last step.  Returns a dict of
        arrays [n]: seg, s, d, heading_error, delta, progress."""
        n = self.of_car.shape[0]
        out = {'seg': np.zeros(n, dtype=np.int32), 's': np.zeros(n), 'd': np.zeros(n), 'heading_error': np.zeros(n),
               'delta': np.zeros(n)}
        for c in range(n):
            ck = self.checkers[self.of_car[c]]
            px, py, yaw = poses[c]
            seg, s, d, e = ck.frenet(px, py, yaw)
            restart = bool(reset[c]) or not self.seen[c]
            if not (np.isfinite(px) and np.isfinite(py)):
                delta = np.nan                      # step 6: progress and s_prev stay
                if restart:
                    self.seen[c] = False            # the restart is taken at the next finite pose
            else:
                if restart:                         # step 5
                    delta, self.progress[c] = 0.0, 0.0
                else:
                    L = ck.L
                    delta = s - self.s_prev[c]
                    if delta >= L / 2:
                        delta -= L
                    if delta < -L / 2:
                        delta += L
                    self.progress[c] += delta
                self.s_prev[c], self.seen[c] = s, True
            out['seg'][c], out['s'][c], out['d'][c], out['heading_error'][c], out['delta'][c] = seg, s, d, e, delta
        out['progress'] = self.progress.copy()
        return out


# ---------------------------------------------------------------------------------------------- pose sets
def scattered_poses(xy, n, radius, seed):
    """n points uniformly in discs of `radius` metres around random waypoints."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, xy.shape[0], n)
    r, a = radius * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    return np.stack([xy[k, 0] + r * np.cos(a), xy[k, 1] + r * np.sin(a)], axis=1)


def tie_poses(xy, every=4, min_gap=60):
    """Points (nearly) equally far from two stretches of the raceline: for every `every`-th waypoint i the nearest
    waypoint j at least min_gap indices away (either way round), their midpoint and points along the perpendicular
    bisector of the two; and, for the corners, points behind each waypoint on the outer bisector of its two segments
    (nearest to the waypoint itself, which ends one segment at t = 1 and starts the next at t = 0)."""
    M = xy.shape[0]
    out = []
    idx = np.arange(M)
    for i in range(0, M, every):
        gap = np.minimum(np.abs(idx - i), M - np.abs(idx - i))
        d2 = (xy[:, 0] - xy[i, 0]) ** 2 + (xy[:, 1] - xy[i, 1]) ** 2
        d2[gap < min_gap] = np.inf
        j = int(np.argmin(d2))
        mid, v = 0.5 * (xy[i] + xy[j]), xy[j] - xy[i]
        perp = np.array([-v[1], v[0]]) / np.sqrt(v[0] * v[0] + v[1] * v[1])
        for k in (-0.5, -0.125, 0.0, 0.125, 0.5):
            out.append(mid + k * perp)
    for i in range(1, M - 1, every):
        a, b = xy[i] - xy[i - 1], xy[i + 1] - xy[i]
        a, b = a / np.hypot(a[0], a[1]), b / np.hypot(b[0], b[1])
        turn = a[0] * b[1] - a[1] * b[0]
        n = np.array([a[1] + b[1], -(a[0] + b[0])]) * (1.0 if turn > 0 else -1.0)   # outer side of the corner
        n = n / np.hypot(n[0], n[1])
        for k in (0.25, 1.0):
            out.append(xy[i] + k * n)
    return np.array(out)


def far_poses(xy, radius=50.0, n=64):
    c = xy.mean(axis=0)
    a = np.arange(n) * (2 * np.pi / n)
    return np.stack([c[0] + radius * np.cos(a), c[1] + radius * np.sin(a)], axis=1)


def g15_extra_poses(xy):
    """The poses g15 stores beside g8's own: scattered up to 5 m, exactly on waypoints, ties, 50 m away."""
    return np.concatenate([scattered_poses(xy, 3000, 5.0, 1501), xy.copy(), tie_poses(xy), far_poses(xy)], axis=0)


def g15_poses(golden):
    """All poses of g15 in its row order: g8's 3 329 (read from g8_env.npz), then the stored extra ones."""
    g8, g15 = golden('g8_env.npz'), golden('g15_nearest.npz')
    return np.concatenate([np.stack([g8['x'], g8['y']], axis=1), g15['poses']], axis=0)


def with_yaws(xy_poses, psi_of_pose, seed):
    """[n, 3] poses: yaw uniform in [0, 2 pi], with the values 0, pi, 2 pi and psi +- pi (psi_of_pose [n]: the heading of
    each pose's nearest segment, so that heading_error lands exactly on the wrap's edges) dealt to every 16th pose in turn."""
    rng = np.random.default_rng(seed)
    n = xy_poses.shape[0]
    yaw = rng.uniform(0, 2 * np.pi, n)
    k = np.arange(n)
    yaw[k % 16 == 0] = 0.0
    yaw[k % 16 == 1] = np.pi
    yaw[k % 16 == 2] = 2 * np.pi
    m = k % 16 == 3
    yaw[m] = psi_of_pose[m] + np.pi
    m = k % 16 == 4
    yaw[m] = psi_of_pose[m] - np.pi
    return np.concatenate([xy_poses, yaw[:, None]], axis=1)


def circle_raceline(radius=6.0, n=200, centre=(1.0, -2.0)):
    a = np.arange(n + 1) * (2 * np.pi / n)
    a[-1] = 0.0                                       # closed: the last point repeats the first
    return np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1)


def stadium_raceline(straight=10.0, radius=3.0, n_arc=40, n_straight=25):
    pts = []
    for k in range(n_straight):
        pts.append([-straight / 2 + straight * k / n_straight, -radius])
    for k in range(n_arc):
        a = -np.pi / 2 + np.pi * k / n_arc
        pts.append([straight / 2 + radius * np.cos(a), radius * np.sin(a)])
    for k in range(n_straight):
        pts.append([straight / 2 - straight * k / n_straight, radius])
    for k in range(n_arc):
        a = np.pi / 2 + np.pi * k / n_arc
        pts.append([-straight / 2 + radius * np.cos(a), radius * np.sin(a)])
    return np.array(pts)                              # open: the gap back to the first point counts into L


def l_shape_raceline():
    """An open L: 12 m east, then 7 m north, in uneven steps."""
    xs = np.concatenate([np.linspace(0, 12, 31)[:-1], np.full(15, 12.0)])
    ys = np.concatenate([np.zeros(30), np.linspace(0, 7, 15) ** 1.0])
    return np.stack([xs + 3.0, ys - 1.0], axis=1)
