"""NumPy restatement of the action side of the reference's RL consumer (src/SAL.py, SACF110Env.step) -- the checker of the path
follower's tests -- and the designed cases of g17 (tests/golden/make_golden_paths.py records the reference's own results on them).

decode (:585-608), global path (:157-181), chord lengths and the not-a-knot cubic spline of MPC_controller (:615-687; scipy's
system written out, solved with np.linalg.solve), the first QP (:693-722) as two box QPs solved by ENUMERATION of the 3^H
patterns (every variable at -1, free or at +1: a small solve plus a sign check each), MPC_converter (:741-764) and
_update_path_index (:252-259); FollowChecker is the wrapper's state machine with the follower's replan_at rule.  All arrays
carry a leading case dimension."""
import itertools

import numpy as np

DEFAULTS = dict(agent=0, car_length=0.3, vector_length=0.5, max_diff_deg=10.0, dist_threshold=0.2, replan_at=8,
                desired_velocity=2.0, timestep=0.1, horizon=5, q=(1.0, 1.0, 0.1, 0.1), r=(0.1, 0.1), p=(10.0, 10.0, 1.0, 1.0),
                max_steer=0.4189)
POINTS = 8


def config(**kw):
    assert set(kw) <= set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def close(got, want, rel=1e-9):
    """|got - want| <= rel * max(1, |want|) element by element; returns (ok, largest |got - want| / max(1, |want|))."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    worst = float(np.nanmax(err)) if err.size else 0.0
    return bool(np.all(err <= rel)), worst


# ---------------------------------------------------------------- decode
def clamp_angles(raw, max_diff_deg=10.0):
    """compute_vectors_with_angle_clamp: raw [n, 16] -> (increments [n, 8, 2], diff [n, 7] before the clip, wrap argument [n, 7])."""
    v = np.array(raw, dtype=np.float64).reshape(-1, POINTS, 2)
    v = v / (np.sqrt(v[..., 0:1] ** 2 + v[..., 1:2] ** 2) + 1e-8)
    n = v.shape[0]
    inc = np.zeros((n, POINTS, 2))
    inc[:, 0, 0] = 1.0
    prev = np.zeros(n)
    lim = np.deg2rad(max_diff_deg)
    diffs, args = np.zeros((n, POINTS - 1)), np.zeros((n, POINTS - 1))
    for i in range(1, POINTS):
        desired = np.arctan2(v[:, i, 1], v[:, i, 0])
        args[:, i - 1] = desired - prev + np.pi
        diff = np.mod(args[:, i - 1], 2 * np.pi) - np.pi
        diffs[:, i - 1] = diff
        prev = prev + np.clip(diff, -lim, lim)
        inc[:, i, 0], inc[:, i, 1] = np.cos(prev), np.sin(prev)
    return inc, diffs, args


def global_path(inc, poses, car_length=0.3, vector_length=0.5):
    """_calculate_global_path: increments [n, 8, 2], poses [n, 3] -> paths [n, 8, 2]."""
    x, y, th = poses[:, 0], poses[:, 1], poses[:, 2]
    ct, st = np.cos(th), np.sin(th)
    px, py = x + car_length * ct, y + car_length * st
    out = np.zeros((inc.shape[0], POINTS, 2))
    for i in range(POINTS):
        dxs, dys = inc[:, i, 0] * vector_length, inc[:, i, 1] * vector_length
        px = px + (dxs * ct - dys * st)
        py = py + (dxs * st + dys * ct)
        out[:, i, 0], out[:, i, 1] = px, py
    return out


def decode(raw, poses, cfg=DEFAULTS):
    return global_path(clamp_angles(raw, cfg['max_diff_deg'])[0], poses, cfg['car_length'], cfg['vector_length'])


# ---------------------------------------------------------------- spline and reference states
def chord_lengths(paths):
    d = paths[:, 1:] - paths[:, :-1]
    return np.concatenate([np.zeros((paths.shape[0], 1)), np.cumsum(np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2), axis=1)], axis=1)


def notaknot_slopes(x, y):
    """First derivatives at the knots of the not-a-knot cubic spline through (x, y), x, y [n, 8]: scipy.interpolate.
    CubicSpline's tridiagonal system, assembled densely."""
    n, N = x.shape
    dx = x[:, 1:] - x[:, :-1]
    sl = (y[:, 1:] - y[:, :-1]) / dx
    A, b = np.zeros((n, N, N)), np.zeros((n, N))
    for i in range(1, N - 1):
        A[:, i, i - 1], A[:, i, i], A[:, i, i + 1] = dx[:, i], 2.0 * (dx[:, i - 1] + dx[:, i]), dx[:, i - 1]
        b[:, i] = 3.0 * (dx[:, i] * sl[:, i - 1] + dx[:, i - 1] * sl[:, i])
    d = x[:, 2] - x[:, 0]
    A[:, 0, 0], A[:, 0, 1] = dx[:, 1], d
    b[:, 0] = ((dx[:, 0] + 2.0 * d) * dx[:, 1] * sl[:, 0] + dx[:, 0] ** 2 * sl[:, 1]) / d
    d = x[:, -1] - x[:, -3]
    A[:, -1, -1], A[:, -1, -2] = dx[:, -2], d
    b[:, -1] = (dx[:, -1] ** 2 * sl[:, -2] + (2.0 * d + dx[:, -1]) * dx[:, -2] * sl[:, -1]) / d
    return np.linalg.solve(A, b[..., None])[..., 0], dx, sl


def spline_eval(x, y, s, dx, sl, at):
    """Value and first derivative at `at` [n] of the spline with knot derivatives s."""
    piece = np.clip((x[:, 1:-1] <= at[:, None]).sum(axis=1), 0, x.shape[1] - 2)
    r = np.arange(x.shape[0])
    xj, yj, sj, sj1, dxj, slj = x[r, piece], y[r, piece], s[r, piece], s[r, piece + 1], dx[r, piece], sl[r, piece]
    t = (sj + sj1 - 2.0 * slj) / dxj
    c0, c1 = t / dxj, (slj - sj) / dxj - t
    z = at - xj
    return ((c0 * z + c1) * z + sj) * z + yj, (3.0 * c0 * z + 2.0 * c1) * z + sj


def reference_states(paths, cfg=DEFAULTS):
    """(dists [n, 8], ref_traj [n, H + 1, 4]) of MPC_controller."""
    H, v, dt = cfg['horizon'], cfg['desired_velocity'], cfg['timestep']
    x = chord_lengths(paths)
    fits = [notaknot_slopes(x, paths[..., k]) for k in range(2)]
    ref = np.zeros((paths.shape[0], H + 1, 4))
    for i in range(H + 1):
        at = np.minimum(v * (i * dt), x[:, -1])
        (rx, dxv), (ry, dyv) = [spline_eval(x, paths[..., k], *fits[k], at) for k in range(2)]
        speed = np.hypot(dxv, dyv)
        ok = speed > 1e-3
        safe = np.where(ok, speed, 1.0)
        ref[:, i, 0], ref[:, i, 1] = rx, ry
        ref[:, i, 2], ref[:, i, 3] = np.where(ok, v * dxv / safe, 0.0), np.where(ok, v * dyv / safe, 0.0)
    return x, ref


# ---------------------------------------------------------------- the QP
def qp_terms(ref, p0, v0, axis, cfg=DEFAULTS):
    """The QP of one axis, minimise 1/2 u'Hu + f'u over -1 <= u <= 1 (the reference's cost, halved, without its constant): with
    x_0 = (p0, v0), p_k = p0 + k dt v0 + sum_j A[k, j] u_j, v_k = v0 + sum_j B[k, j] u_j from x_{k+1} = A x_k + B u_k (:648-655),
    cost = sum_{k=1..H} wp_k (p_k - rp_k)^2 + wv_k (v_k - rv_k)^2 + r |u|^2 (the k = 0 term is a constant).  Returns (Hm [H, H],
    f [n, H])."""
    H, dt = cfg['horizon'], cfg['timestep']
    A, B = np.zeros((H + 1, H)), np.zeros((H + 1, H))
    for k in range(1, H + 1):
        for j in range(k):
            A[k, j], B[k, j] = dt * dt * (k - j - 0.5), dt
    Hm = cfg['r'][axis] * np.eye(H)
    f = np.zeros((ref.shape[0], H))
    for k in range(1, H + 1):
        wp, wv = (cfg['q'][axis], cfg['q'][2 + axis]) if k < H else (cfg['p'][axis], cfg['p'][2 + axis])
        Hm += wp * np.outer(A[k], A[k]) + wv * np.outer(B[k], B[k])
        f += wp * (p0 + k * dt * v0 - ref[:, k, axis])[:, None] * A[k][None] + wv * (v0 - ref[:, k, 2 + axis])[:, None] * B[k][None]
    return Hm, f


def kkt_violation(Hm, f, u):
    """Per case the largest violation of the KKT conditions of the box QP at u [n, H]: bounds, and per component the
    gradient's sign and size -- 0 where u_i is strictly inside, <= 0 at +1, >= 0 at -1."""
    g = u @ Hm.T + f
    inside = np.abs(u) < 1.0
    v = np.where(inside, np.abs(g), np.where(u >= 1.0, np.maximum(g, 0.0), np.maximum(-g, 0.0)))
    return np.maximum(v.max(axis=1), np.maximum(np.abs(u) - 1.0, 0.0).max(axis=1))


def solve_box_qp(Hm, f):
    """The optimum u* [n, H] by enumeration of the 3^H patterns, and the pattern found (-1 / 0 / +1 per variable).  For each
    pattern the free variables solve H_FF u_F = -(f_F + H_FB u_B); the pattern whose KKT violation is smallest is taken
    (exactly one pattern has violation ~ 0 unless a multiplier or a free variable's slack is 0, where the neighbours agree)."""
    n, H = f.shape
    best_u, best_v = np.zeros((n, H)), np.full(n, np.inf)
    best_pat = np.zeros((n, H), dtype=np.int8)
    for pat in itertools.product((-1, 0, 1), repeat=H):
        pat = np.array(pat)
        F, Bd = np.flatnonzero(pat == 0), np.flatnonzero(pat != 0)
        u = np.tile(pat.astype(np.float64), (n, 1))
        if F.size:
            rhs = -f[:, F]
            if Bd.size:
                rhs = rhs - (Hm[np.ix_(F, Bd)] @ pat[Bd].astype(np.float64))[None]
            u[:, F] = np.linalg.solve(Hm[np.ix_(F, F)], rhs.T).T
        g = u @ Hm.T + f
        viol = np.zeros(n)
        if F.size:
            viol = np.maximum(viol, np.maximum(np.abs(u[:, F]) - 1.0, 0.0).max(axis=1))
        for i in Bd:
            viol = np.maximum(viol, np.maximum(g[:, i] * pat[i], 0.0))
        better = viol < best_v
        best_u[better], best_v[better], best_pat[better] = u[better], viol[better], pat
    return np.clip(best_u, -1.0, 1.0), best_pat, best_v


def mpc_accel(paths, vels, cfg=DEFAULTS):
    """(accel [n, 2], active [n, 2] = bounds active per axis, dists, ref_traj): u_0 of the two QPs by enumeration."""
    x, ref = reference_states(paths, cfg)
    acc, act = np.zeros((paths.shape[0], 2)), np.zeros((paths.shape[0], 2), dtype=np.int32)
    for axis in range(2):
        Hm, f = qp_terms(ref, paths[:, 0, axis], vels[:, axis], axis, cfg)
        u, pat, viol = solve_box_qp(Hm, f)
        assert viol.max() <= 1e-12 * max(1.0, np.abs(f).max()), viol.max()
        acc[:, axis], act[:, axis] = u[:, 0], (pat != 0).sum(axis=1)
    return acc, act, x, ref


def convert(accel, max_steer=0.4189):
    """MPC_converter with current_steer = 0.0: (actions [n, 2] = (steer, speed), wrapped angle before the clip, wrap argument)."""
    arg = np.arctan2(accel[:, 1], accel[:, 0]) - 0.0 + np.pi
    ang = np.mod(arg, 2 * np.pi) - np.pi
    thr = accel[:, 0] * np.cos(0.0) + accel[:, 1] * np.sin(0.0)
    return np.stack([np.clip(ang, -max_steer, max_steer), np.clip(thr, -1.0, 1.0)], axis=1), ang, arg


def advance(paths, index, xy, dist_threshold=0.2):
    """_update_path_index for index in 0..7: (new index, distance to the waypoint)."""
    r = np.arange(paths.shape[0])
    d = xy - paths[r, np.clip(index, 0, POINTS - 1)]
    dist = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    ok = (index >= 0) & (index < POINTS)
    return np.where(ok & (dist < dist_threshold), index + 1, index).astype(np.int32), dist


class FollowChecker(object):
    """SACF110Env.step's path management for B envs with the follower's rules: act() decodes where there is no path or the
    index has reached replan_at; update() advances the index and reads resets off the clock (clock == timestep: the path is
    dropped; clock unchanged since the previous update: the env is left alone)."""

    def __init__(self, B, timestep, **cfg):
        self.cfg, self.dt = config(**cfg), timestep
        self.paths = np.zeros((B, POINTS, 2))
        self.index = np.full(B, -1, dtype=np.int32)
        self.t_seen = np.full(B, -1.0)
        self.replans = np.zeros(B, dtype=np.int64)      # paths decoded per env
        self.advances = np.zeros(B, dtype=np.int64)     # index advances per env
        self.reached = np.zeros(B, dtype=np.int64)      # paths decoded because the index had reached replan_at

    def act(self, raw, poses, vx):
        """raw [B, 16], poses [B, 3], vx [B] -> (actions [B, 2], accel [B, 2], replanned [B] uint8)."""
        c = self.cfg
        need = (self.index < 0) | (self.index >= c['replan_at'])
        self.reached += self.index >= c['replan_at']
        if need.any():
            self.paths[need] = decode(raw[need], poses[need], c)
            self.index[need] = 0
            self.replans[need] += 1
        acc = mpc_accel(self.paths, np.stack([vx, np.zeros_like(vx)], axis=1), c)[0]
        return convert(acc, c['max_steer'])[0], acc, need.astype(np.uint8)

    def update(self, xy, clock):
        reset = clock == self.dt
        moved = ~reset & (clock != self.t_seen)
        new, _ = advance(self.paths, self.index, xy, self.cfg['dist_threshold'])
        self.advances += moved & (new != self.index)
        self.index = np.where(reset, -1, np.where(moved, new, self.index)).astype(np.int32)
        self.t_seen = np.where(reset | moved, clock, self.t_seen)
        return reset


# ---------------------------------------------------------------- the cases of g17
def designed_raw(n, seed):
    """n raw actions in [-1, 1]^16: random ones, and designed ones -- zero rows, rows that turn hard one way and the other (the
    clamp on every segment), rows that barely turn (no clamp), rows that straddle the +-pi wrap."""
    rng = np.random.default_rng(seed)
    raw = rng.uniform(-1.0, 1.0, (n, 16))
    kind = np.arange(n) % 8
    ang = np.zeros((n, POINTS))
    for i in range(n):
        k = kind[i]
        if k == 1 or (k == 6 and i % 16 != 6):        # gentle: every heading within 8 degrees of the one before
            k = 1
            ang[i] = np.cumsum(rng.uniform(-8.0, 8.0, POINTS)) * np.pi / 180
        elif k == 2:      # hard left, clamped on every segment
            ang[i] = rng.uniform(1.6, 3.0, POINTS)
        elif k == 3:      # hard right
            ang[i] = -rng.uniform(1.6, 3.0, POINTS)
        elif k == 4:      # behind the car: the wrap's neighbourhood, at least 1e-3 rad off
            ang[i] = np.pi - rng.uniform(1e-3, 0.4, POINTS) * rng.choice([-1.0, 1.0], POINTS)
        if 1 <= k <= 4:
            length = rng.uniform(0.05, 1.0, POINTS)
            raw[i] = np.stack([np.cos(ang[i]) * length, np.sin(ang[i]) * length], axis=1).reshape(-1)
        elif k == 5:      # some rows zero
            raw[i].reshape(POINTS, 2)[rng.uniform(size=POINTS) < 0.4] = 0.0
        elif k == 6:
            raw[i] = 0.0
    return raw


def gentle_cases(n):
    """The cases whose raw action designed_raw makes gentle."""
    i = np.arange(n)
    return (i % 8 == 1) | ((i % 8 == 6) & (i % 16 != 6))


def designed_poses(n, seed):
    """Poses over the extent of the reference's maps (+-100 m), theta over the full circle and beyond it."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-2 * np.pi, 2 * np.pi, n)
    ahead = gentle_cases(n)
    th[ahead] = rng.uniform(-0.15, 0.15, int(ahead.sum()))   # with a gentle path and a slow car: an acceleration within max_steer of +x
    return np.stack([rng.uniform(-100.0, 100.0, n), rng.uniform(-100.0, 100.0, n), th], axis=1)


def designed_vels(n, seed):
    """(vx, vy): vx from -5 to 20 m/s; vy is 0 (as in the observation) for half the cases, -5 .. 5 for the others."""
    rng = np.random.default_rng(seed)
    vx = rng.uniform(-5.0, 20.0, n)
    vx[::3] = rng.uniform(0.5, 3.5, vx[::3].shape)            # around the desired velocity: bounds inactive
    vy = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(-5.0, 5.0, n))
    vy[1::6] = rng.uniform(-0.3, 0.3, vy[1::6].shape)
    ahead = gentle_cases(n)
    vx[ahead], vy[ahead] = rng.uniform(0.3, 1.8, int(ahead.sum())), rng.uniform(-0.05, 0.05, int(ahead.sum()))
    return np.stack([vx, vy], axis=1)
