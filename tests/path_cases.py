"""NumPy restatement of the action side of the reference's RL consumer (src/SAL.py, SACF110Env.step) -- the checker of the path
follower's tests -- and the designed cases of g17 (tests/golden/make_golden.py g17 records the reference's own results on them).

decode (:585-608), global path (:157-181), chord lengths and the not-a-knot cubic spline of MPC_controller (:615-687; scipy's
system written out, solved with np.linalg.solve), the first QP (:693-722) as two box QPs solved by ENUMERATION of the 3^H
patterns (every variable at -1, free or at +1: a small solve plus a sign check each), MPC_converter (:741-764) and
_update_path_index (:252-259); FollowChecker is the wrapper's state machine with the follower's replan_at rule.  All arrays
carry a leading case dimension."""
import fractions
import functools
import itertools
import os

import numpy as np

DEFAULTS = dict(agent=0, car_length=0.3, vector_length=0.5, max_diff_deg=10.0, dist_threshold=0.2, replan_at=8,
                desired_velocity=2.0, timestep=0.1, horizon=5, q=(1.0, 1.0, 0.1, 0.1), r=(0.1, 0.1), p=(10.0, 10.0, 1.0, 1.0),
                max_steer=0.4189)
POINTS = 8
TOL_U = TOL_G = 1e-12        # PF_TOL_U, PF_TOL_G of csrc/f110_pathfollow.h
QP_LIMIT = 64                # PF_QP_LIMIT
DEVERR_QP_LIMIT = 4
NEAR = 1e-11                 # ten times the walk's tolerances: see solve_box_qp(spread=True)


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
    return np.concatenate([np.zeros((paths.shape[0], 1), dtype=paths.dtype), np.cumsum(np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2), axis=1)], axis=1)


def gauss_solve(A, b):
    """A [n, m, m], b [n, m] -> x [n, m] by Gaussian elimination with partial pivoting in the arrays' own type: np.linalg has no
    np.longdouble.  Only the extended-precision runs that measure the checker's own rounding use it."""
    A, b = A.copy(), b.copy()
    n, m = b.shape
    r = np.arange(n)
    for c in range(m):
        piv = c + np.abs(A[:, c:, c]).argmax(axis=1)
        A[r, c], A[r, piv] = A[r, piv].copy(), A[r, c].copy()
        b[r, c], b[r, piv] = b[r, piv].copy(), b[r, c].copy()
        for i in range(c + 1, m):
            fct = A[:, i, c] / A[:, c, c]
            A[:, i] = A[:, i] - fct[:, None] * A[:, c]
            b[:, i] = b[:, i] - fct * b[:, c]
    x = np.zeros_like(b)
    for i in range(m - 1, -1, -1):
        x[:, i] = (b[:, i] - (A[:, i, i + 1:] * x[:, i + 1:]).sum(axis=1)) / A[:, i, i]
    return x


def notaknot_slopes(x, y):
    """First derivatives at the knots of the not-a-knot cubic spline through (x, y), x, y [n, 8]: scipy.interpolate.
    CubicSpline's tridiagonal system, assembled densely (in x's type: fp64 goes through np.linalg.solve)."""
    n, N = x.shape
    dx = x[:, 1:] - x[:, :-1]
    sl = (y[:, 1:] - y[:, :-1]) / dx
    A, b = np.zeros((n, N, N), dtype=x.dtype), np.zeros((n, N), dtype=x.dtype)
    for i in range(1, N - 1):
        A[:, i, i - 1], A[:, i, i], A[:, i, i + 1] = dx[:, i], 2.0 * (dx[:, i - 1] + dx[:, i]), dx[:, i - 1]
        b[:, i] = 3.0 * (dx[:, i] * sl[:, i - 1] + dx[:, i - 1] * sl[:, i])
    d = x[:, 2] - x[:, 0]
    A[:, 0, 0], A[:, 0, 1] = dx[:, 1], d
    b[:, 0] = ((dx[:, 0] + 2.0 * d) * dx[:, 1] * sl[:, 0] + dx[:, 0] ** 2 * sl[:, 1]) / d
    d = x[:, -1] - x[:, -3]
    A[:, -1, -1], A[:, -1, -2] = dx[:, -2], d
    b[:, -1] = (dx[:, -1] ** 2 * sl[:, -2] + (2.0 * d + dx[:, -1]) * dx[:, -2] * sl[:, -1]) / d
    if x.dtype != np.float64:
        return gauss_solve(A, b), dx, sl
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
    ref = np.zeros((paths.shape[0], H + 1, 4), dtype=paths.dtype)
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
    T = ref.dtype.type if ref.dtype != object else fractions.Fraction     # (object arrays hold exact Fractions: see stiff_cases)
    H, dt = cfg['horizon'], T(cfg['timestep'])
    A, B = np.zeros((H + 1, H), dtype=T), np.zeros((H + 1, H), dtype=T)
    for k in range(1, H + 1):
        for j in range(k):
            A[k, j], B[k, j] = dt * dt * T(k - j - 0.5), dt
    Hm = T(cfg['r'][axis]) * np.eye(H, dtype=T)
    f = np.zeros((ref.shape[0], H), dtype=T)
    for k in range(1, H + 1):
        wp, wv = (cfg['q'][axis], cfg['q'][2 + axis]) if k < H else (cfg['p'][axis], cfg['p'][2 + axis])
        wp, wv = T(wp), T(wv)
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


def solve_box_qp(Hm, f, spread=False):
    """The optimum u* [n, H] by enumeration of the 3^H patterns, and the pattern found (-1 / 0 / +1 per variable).  For each
    pattern the free variables solve H_FF u_F = -(f_F + H_FB u_B); the pattern whose KKT violation is smallest is taken
    (exactly one pattern has violation ~ 0 unless a multiplier or a free variable's slack is 0, where the neighbours agree).
    With spread=True a fourth result: per case the range of the clipped u_0 over the patterns whose violation is at most
    NEAR * max(1, |f|_inf) -- the patterns a solver with tolerances may end on; a case is well-posed at 1e-9 where it is <= 1e-9."""
    n, H = f.shape
    best_u, best_v = np.zeros((n, H)), np.full(n, np.inf)
    best_pat = np.zeros((n, H), dtype=np.int8)
    near = NEAR * np.maximum(1.0, np.abs(f).max(axis=1))
    lo0, hi0 = np.full(n, np.inf), np.full(n, -np.inf)
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
        if spread:
            u0 = np.clip(u[:, 0], -1.0, 1.0)
            lo0, hi0 = np.where(viol <= near, np.minimum(lo0, u0), lo0), np.where(viol <= near, np.maximum(hi0, u0), hi0)
    if spread:
        return np.clip(best_u, -1.0, 1.0), best_pat, best_v, hi0 - lo0
    return np.clip(best_u, -1.0, 1.0), best_pat, best_v


def solve_box_qp_by_sets(Hm, f):
    """solve_box_qp's enumeration with one solve per SET of free variables: the 2^|bound| sign assignments of a set are right-hand
    sides of one system.  The same patterns, the same choice (smallest violation), 3^H / 2^H times fewer calls: what the closed
    loops at horizon >= 6 use.  Returns (u*, pattern, violation)."""
    n, H = f.shape
    best_u, best_v, best_pat = np.zeros((n, H)), np.full(n, np.inf), np.zeros((n, H), dtype=np.int8)
    r = np.arange(n)
    for fm in range(1 << H):
        F = np.array([i for i in range(H) if (fm >> i) & 1], dtype=int)
        Bd = np.array([i for i in range(H) if not (fm >> i) & 1], dtype=int)
        signs = np.array(list(itertools.product((-1.0, 1.0), repeat=Bd.size))).reshape(1 << Bd.size, Bd.size)
        S = signs.shape[0]
        u = np.zeros((n, S, H))
        u[:, :, Bd] = signs[None]
        viol = np.zeros((n, S))
        if F.size:
            rhs = -f[:, None, F] - (signs @ Hm[np.ix_(Bd, F)])[None]
            u[:, :, F] = np.linalg.solve(Hm[np.ix_(F, F)], rhs.reshape(n * S, F.size).T).T.reshape(n, S, F.size)
            viol = np.maximum(np.abs(u[:, :, F]) - 1.0, 0.0).max(axis=2)
        if Bd.size:
            g = u @ Hm.T + f[:, None, :]
            viol = np.maximum(viol, np.maximum(g[:, :, Bd] * signs[None], 0.0).max(axis=2))
        k = viol.argmin(axis=1)
        better = viol[r, k] < best_v
        best_u[better], best_v[better] = u[r, k][better], viol[r, k][better]
        pat = np.zeros((n, H), dtype=np.int8)
        pat[:, Bd] = signs[k].astype(np.int8)
        best_pat[better] = pat[better]
    return np.clip(best_u, -1.0, 1.0), best_pat, best_v


def mpc_accel(paths, vels, cfg=DEFAULTS):
    """(accel [n, 2], active [n, 2] = bounds active per axis, dists, ref_traj): u_0 of the two QPs by enumeration."""
    x, ref = reference_states(paths, cfg)
    acc, act = np.zeros((paths.shape[0], 2)), np.zeros((paths.shape[0], 2), dtype=np.int32)
    for axis in range(2):
        Hm, f = qp_terms(ref, paths[:, 0, axis], vels[:, axis], axis, cfg)
        u, pat, viol = (solve_box_qp if cfg['horizon'] < 6 else solve_box_qp_by_sets)(Hm, f)
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


# ---------------------------------------------------------------- off-default configurations (g19) and the kernel's case analysis
# tests/golden/make_golden.py g19 records the reference on designed_raw / poses / vels(G19_CASES, seed .. seed + 2) per entry.
G19_CASES = 96
CONFIGS = {
    'late_pieces': dict(seed=1900, cfg=dict(desired_velocity=4.7, timestep=0.1, horizon=8)),                      # sk = 0.47 k: pieces 0 0 1 2 3 4 5 6, the clamp at k = 8
    'short_chords': dict(seed=1910, cfg=dict(vector_length=0.25, car_length=0.0, desired_velocity=2.0, timestep=0.1, horizon=8)),   # x[7] = 1.75, sk <= 1.6: short chords, no clamp
    'short_clamped': dict(seed=1915, cfg=dict(vector_length=0.125, car_length=0.0, desired_velocity=2.0, timestep=0.1, horizon=8)),   # x[7] = 0.875: the clamp from k = 5 on
    'long_chords': dict(seed=1920, cfg=dict(vector_length=1.5, car_length=0.55, horizon=6)),
    'nothing_clamps': dict(seed=1930, cfg=dict(max_diff_deg=180.0, max_steer=0.1)),
    'all_clamps': dict(seed=1940, cfg=dict(max_diff_deg=0.5, max_steer=3.2)),
    'horizon_2': dict(seed=1950, cfg=dict(horizon=2)),
    'horizon_4': dict(seed=1960, cfg=dict(horizon=4, q=(2.0, 0.5, 0.0, 0.3), r=(0.05, 0.2), p=(4.0, 20.0, 0.5, 2.0))),
    'horizon_7': dict(seed=1970, cfg=dict(horizon=7, timestep=0.08, desired_velocity=3.3)),
}


def g19_inputs(name):
    s = CONFIGS[name]['seed']
    return designed_raw(G19_CASES, s), designed_poses(G19_CASES, s + 1), designed_vels(G19_CASES, s + 2)


def spline_pieces(paths, cfg=DEFAULTS):
    """The kernel's piece and clamp arithmetic restated: (piece [n, H + 1] = the knots x[1..6] at or below sk, clamped [n, H + 1]
    = sk > x[7] before the clamp, margin [n, H + 1] = distance of the unclamped sk from the nearest of x[1..7])."""
    x = chord_lengths(np.asarray(paths, dtype=np.float64))
    sk = cfg['desired_velocity'] * (np.arange(cfg['horizon'] + 1) * cfg['timestep'])
    sk = np.broadcast_to(sk[None], (x.shape[0], sk.size))
    clamped = sk > x[:, -1:]
    margin = np.abs(sk[:, :, None] - x[:, None, 1:]).min(axis=2)
    sk = np.where(clamped, x[:, -1:], sk)
    return (x[:, 1:-1, None] <= sk[:, None, :]).sum(axis=1), clamped, margin


def walk(Hm, f, tol_u=TOL_U, release='worst', jitter=None):
    """NumPy transcription of the kernel's active-set walk, tolerances and step limit included: (u [n, H], blocks [n], releases [n],
    steps [n], done [n]).  It CLASSIFIES cases (which arms a case drives the kernel through); the expected u is the enumerator's.
    tol_u and release ('first': the first wrong-signed multiplier, not the worst) restate two mutations of the kernel, so that the
    tables can be held to cases that tell them apart; jitter = (rng, relative size for the inverses, relative size for f)
    perturbs the tables and f as another inversion and another order of sums would (see step_stable)."""
    n, H = f.shape
    every = (1 << H) - 1
    inv = {}
    if jitter is not None:
        f = f * (1.0 + jitter[2] * jitter[0].standard_normal(f.shape))

    def Z(fm):
        if fm not in inv:
            z, F = np.zeros((H, H)), [i for i in range(H) if (fm >> i) & 1]
            if F:
                z[np.ix_(F, F)] = np.linalg.inv(Hm[np.ix_(F, F)])
            if jitter is not None:
                e = jitter[1] * jitter[0].standard_normal((H, H))
                z = z * (1.0 + 0.5 * (e + e.T))
            inv[fm] = z
        return inv[fm]
    bit = 1 << np.arange(H)
    out_u, blocks, rels, steps, done = np.zeros((n, H)), np.zeros(n, int), np.zeros(n, int), np.zeros(n, int), np.zeros(n, bool)
    for c in range(n):
        fc = f[c]
        tolg = TOL_G * max(1.0, np.abs(fc).max())
        u = -Z(every) @ fc
        hi, lo = int(bit[u >= 1.0].sum()), int(bit[u <= -1.0].sum())
        u = np.clip(u, -1.0, 1.0)
        while steps[c] < QP_LIMIT and not done[c]:
            bound = hi | lo
            fm = every & ~bound
            held, free = (bound & bit) != 0, (fm & bit) != 0
            v = -Z(fm) @ (fc + Hm @ np.where(held, u, 0.0))
            t = np.where(free, v, u)
            alpha, blk = 1.0, -1
            for i in np.flatnonzero(free):
                for b in (1.0, -1.0):
                    if b * v[i] > 1.0 + tol_u:
                        al = (b - u[i]) / (v[i] - u[i])
                        if al < alpha:
                            alpha, blk = al, i
            if blk >= 0:
                up = t[blk] > u[blk]
                u = u + alpha * (t - u)
                u[blk] = 1.0 if up else -1.0
                hi, lo = (hi | (1 << blk), lo) if up else (hi, lo | (1 << blk))
                u = np.clip(u, -1.0, 1.0)
                blocks[c] += 1
            else:
                u = np.clip(t, -1.0, 1.0)
                g = fc + Hm @ u
                viol = np.where(held, np.where((hi & bit) != 0, g, -g), -np.inf)
                rel = int(viol.argmax()) if release == 'worst' else int((viol > tolg).argmax())
                if viol[rel] > tolg:
                    hi, lo = hi & ~(1 << rel), lo & ~(1 << rel)
                    rels[c] += 1
                else:
                    done[c] = True
            steps[c] += 1
        out_u[c] = u
    return out_u, blocks, rels, steps, done


STABLE_Z, STABLE_F = 1e-6, 1e-12


def step_stable(Hm, f, trials=3, seed=0):
    """[n] bool: the cases whose walk takes the same block, release and total step counts when every inverse of the table is
    perturbed by STABLE_Z (relative; the host's Gauss-Jordan against np.linalg.inv on a Hessian of condition 1e9 differ by up to
    cond * 2^-53 ~ 1e-7; ten times that) and f by STABLE_F (the device's order of sums).  On these the device's qp_steps must be the walk's."""
    base = walk(Hm, f)
    ok = base[4].copy()
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        w = walk(Hm, f, jitter=(rng, STABLE_Z, STABLE_F))
        ok &= (w[1] == base[1]) & (w[2] == base[2]) & (w[3] == base[3]) & w[4]
    return ok


def qp_of(paths, vels, cfg):
    """[(Hm, f) for the two axes] of mpc_accel's QPs."""
    _, ref = reference_states(paths, cfg)
    return [qp_terms(ref, paths[:, 0, axis], vels[:, axis], axis, cfg) for axis in range(2)]


def classify(paths, vels, cfg):
    """Per case and axis, from walk(): (blocks, releases, steps) [n, 2] each, and from the enumerator (u* [n, 2, H], bound variables
    [n, 2], spread of u_0 [n, 2]), and stable [n, 2] = step_stable."""
    n, H = paths.shape[0], cfg['horizon']
    blocks, rels, steps = (np.zeros((n, 2), int) for _ in range(3))
    ustar, nb, spread, stable = np.zeros((n, 2, H)), np.zeros((n, 2), int), np.zeros((n, 2)), np.zeros((n, 2), bool)
    for axis, (Hm, f) in enumerate(qp_of(paths, vels, cfg)):
        _, blocks[:, axis], rels[:, axis], steps[:, axis], done = walk(Hm, f)
        assert done.all()
        stable[:, axis] = step_stable(Hm, f)
        u, pat, _, spread[:, axis] = solve_box_qp(Hm, f, spread=True)
        ustar[:, axis], nb[:, axis] = u, (pat != 0).sum(axis=1)
    return dict(blocks=blocks, releases=rels, steps=steps, u=ustar, bound=nb, spread=spread, stable=stable)


# ---------------------------------------------------------------- case families off the reference's beaten track
DELTAS = (0.0, 1e-13, -1e-13, 1e-11, -1e-11, 1e-8, -1e-8)
BOUND_HORIZONS = (2, 5, 8)


def _linear_in_v0(paths, cfg, axis):
    """f = f0 + v0 * g for the QP of `axis` (the reference states do not depend on the velocity): (Hm, f0 [n, H], g [n, H])."""
    _, ref = reference_states(paths, cfg)
    z = np.zeros(paths.shape[0])
    Hm, f0 = qp_terms(ref, paths[:, 0, axis], z, axis, cfg)
    _, f1 = qp_terms(ref, paths[:, 0, axis], z + 1.0, axis, cfg)
    return Hm, f0, f1 - f0


def on_a_bound_cases(paths_pool, H):
    """Cases whose optimum sits on the edge of a bound, for horizon H, the other options at their defaults.  Per axis the velocity is
    solved for (f is linear in it) so that (a) component i of the UNCONSTRAINED optimum is sign * (1 + delta), or (b) with the
    variables j != i that are bound in the optimum at the case's base velocity held, the multiplier of variable i held at `sign`
    is delta * max(1, |f|_inf) on the wrong side -- for i = 0 and i = H - 1, both signs, every delta of DELTAS.  Returns (paths, vels,
    kind [n] = 0 for (a), 1 for (b), dropped = the share of designs that came out ill-posed (solve_box_qp's spread > 1e-9 on an axis),
    delta [n]).  In (b) only delta <= 0 can be the optimum's face: a multiplier of the wrong sign means the variable is not held
    there, and those designs end with variable i inside its bound by a hair instead."""
    cfg = config(horizon=H)
    designs = [(kind, i, sign, d) for kind in (0, 1) for i in sorted({0, H - 1}) for sign in (1.0, -1.0) for d in DELTAS]
    n = len(designs)
    rng = np.random.default_rng(2000 + H)
    paths = paths_pool[rng.choice(paths_pool.shape[0], n, replace=False)]
    _, ref = reference_states(paths, cfg)
    base = ref[:, 0, 2:4] + rng.normal(0.0, 0.6, (n, 2))
    vels = np.zeros((n, 2))
    for axis in range(2):
        Hm, f0, g = _linear_in_v0(paths, cfg, axis)
        Hinv = np.linalg.inv(Hm)
        pat = solve_box_qp(Hm, f0 + base[:, axis:axis + 1] * g)[1]
        for c, (kind, i, sign, d) in enumerate(designs):
            if kind == 0:
                # -(Hinv (f0 + v g))_i = sign (1 + d)
                vels[c, axis] = (-(Hinv[i] @ f0[c]) - sign * (1.0 + d)) / (Hinv[i] @ g[c])
                continue
            held = np.flatnonzero(pat[c] != 0)
            held = held[held != i]
            ub = np.zeros(H)
            ub[held], ub[i] = pat[c, held], sign
            B = np.append(held, i).astype(int)
            F = np.setdiff1d(np.arange(H), B)
            # gradient of variable i on that face, g_i = a + v b, to equal sign * delta * scale (wrong-signed where delta > 0)
            M = np.zeros((H, H))
            if F.size:
                M[np.ix_(F, F)] = np.linalg.inv(Hm[np.ix_(F, F)])
            # on that face u_F = -M (f + H u_B) and g_i = f_i + H_i u_B + H_i u_F = a + v b
            a_, b_ = (f0[c, i] + Hm[i] @ ub - Hm[i] @ M @ (f0[c] + Hm @ ub)), (g[c, i] - Hm[i] @ M @ g[c])
            v = base[c, axis]
            for _ in range(3):                             # the scale depends (weakly) on v itself
                scale = max(1.0, np.abs(f0[c] + v * g[c]).max())
                v = (sign * d * scale - a_) / b_
            vels[c, axis] = v
    info = classify(paths, vels, cfg)
    ok = (info['spread'] <= 1e-9).all(axis=1)
    return paths[ok], vels[ok], np.array([k for k, _, _, _ in designs])[ok], 1.0 - ok.mean(), np.array([d for _, _, _, d in designs])[ok]


EDGE_DIAGONAL = dict(r=(1e-6, 5.0), q=(0.0, 0.0, 0.0, 0.0), p=(0.0, 0.0, 0.0, 0.0))       # what validate accepts at its edge: u = clip(-f / r), f = 0
EDGE_STIFF = dict(r=(1e-6, 1e-6), p=(1e4, 1e4, 1e2, 1e2), horizon=8)


def built_cases(paths, cfg, seed):
    """Velocities around the first reference state's, so that some, all or no bounds bind (as the GPU test's own _built_cases)."""
    rng = np.random.default_rng(seed)
    _, ref = reference_states(paths, cfg)
    n = paths.shape[0]
    return ref[:, 0, 2:4] + rng.normal(0.0, 1.0, (n, 2)) * rng.choice([0.02, 0.3, 0.5, 0.8], (n, 1))


def stiff_cases(paths_pool, n=40, exact=None):
    """(paths, vels, u0* [n, 2], e_ref) for EDGE_STIFF: the enumerator's optimum in fp64, and e_ref = the largest difference of
    u_0 from the same pattern's solution in np.longdouble (whose KKT conditions are checked in np.longdouble: it IS the optimum).
    Where np.longdouble is no wider than fp64 (exact=None decides by its eps; True forces it), e_ref comes from exact rational
    arithmetic (fractions.Fraction) on the QPs of the first four cases instead, built from the fp64 reference states."""
    cfg = config(**EDGE_STIFF)
    paths = paths_pool[:n]
    vels = built_cases(paths, cfg, 2100)
    want, e_ref = np.zeros((n, 2)), 0.0
    if exact is None:
        exact = not np.finfo(np.longdouble).eps < 1e-18
    if exact:
        to = np.vectorize(fractions.Fraction, otypes=[object])
        m = 4
        pl, vl, ref_l = to(paths[:m]), to(vels[:m]), to(reference_states(paths[:m], cfg)[1])
    else:
        m = n
        pl, vl = paths.astype(np.longdouble), vels.astype(np.longdouble)
        _, ref_l = reference_states(pl, cfg)
    for axis, (Hm, f) in enumerate(qp_of(paths, vels, cfg)):
        u, pat, viol = solve_box_qp(Hm, f)
        want[:, axis] = u[:, 0]
        Hl, fl = qp_terms(ref_l, pl[:, 0, axis], vl[:, axis], axis, cfg)
        for c in range(m):
            F, Bd = np.flatnonzero(pat[c] == 0), np.flatnonzero(pat[c] != 0)
            ul = pat[c].astype(Hl.dtype)
            if F.size:
                rhs = -(fl[c, F] + Hl[np.ix_(F, Bd)] @ ul[Bd])
                ul[F] = gauss_solve(Hl[np.ix_(F, F)][None], rhs[None])[0]
            g = Hl @ ul + fl[c]
            assert (np.abs(ul) <= 1).all() and (g[Bd] * pat[c, Bd] <= 0).all(), 'the fp64 pattern is not the optimum in the wider arithmetic'
            e_ref = max(e_ref, float(abs(ul[0] - u[c, 0])))
    return paths, vels, want, e_ref


def release_order_cases(paths_pool, n=400):
    """EDGE_STIFF cases on which the ORDER of the releases shows: the walk that releases the worst wrong-signed multiplier and one
    that releases the first take different numbers of steps to the same optimum, on an axis where both counts are step-stable.
    Searched among n built cases with walk(); returns (paths, vels, first [m, 2] = the other walk's steps, tells [m, 2] bool)."""
    cfg = config(**EDGE_STIFF)
    paths = paths_pool[40:40 + n]
    vels = built_cases(paths, cfg, 2130)
    first, tells = np.zeros((n, 2), int), np.zeros((n, 2), bool)
    for axis, (Hm, f) in enumerate(qp_of(paths, vels, cfg)):
        worst, other = walk(Hm, f), walk(Hm, f, release='first')
        first[:, axis] = other[3]
        idx = np.flatnonzero(worst[3] != other[3])
        ok = step_stable(Hm, f[idx])
        rng = np.random.default_rng(1)
        for _ in range(4):
            ok &= walk(Hm, f[idx], release='first', jitter=(rng, STABLE_Z, STABLE_F))[3] == other[3][idx]
        tells[idx[ok], axis] = True
    keep = tells.any(axis=1)
    return paths[keep], vels[keep], first[keep], tells[keep]


CHORD_PATTERNS = ((1, 4, 1, 4, 1, 4, 1), (4, 1, 4, 1, 4, 1, 4), (1, 1, 4, 1, 4, 1, 1), (4, 4, 1, 4, 1, 4, 4), (1, 4, 4, 1, 1, 4, 1))
CHORD_RATIO = 4.0


def nonuniform_paths(paths_pool, n=40, ratio=CHORD_RATIO):
    """g17's paths with their points moved along the path: point i + 1 lies in the direction of the original chord i at a length
    from CHORD_PATTERNS (neighbouring chords 1 : ratio and ratio : 1, at both ends -- the not-a-knot rows -- and inside), the
    mean chord 0.5 as before."""
    out = np.zeros((n, POINTS, 2))
    for c in range(n):
        w = np.array(CHORD_PATTERNS[c % len(CHORD_PATTERNS)], dtype=np.float64)
        w = np.where(w > 1, ratio, 1.0)
        w = w * (0.5 * (POINTS - 1) / w.sum())
        d = paths_pool[c, 1:] - paths_pool[c, :-1]
        d = d / np.sqrt((d ** 2).sum(axis=1, keepdims=True))
        out[c] = paths_pool[c, 0] + np.concatenate([np.zeros((1, 2)), np.cumsum(d * w[:, None], axis=0)])
    return out


def stationary_case():
    """A path that runs out and back along one axis (once along x, once along y): the spline of that coordinate has a stationary
    point near the turn and the other coordinate is constant, so the reference speed there is 0 and the reference's `else` arm
    gives rv = (0, 0).  desired_velocity is found by bisection on the checker so that reference state STATIONARY_K falls on it.
    Returns (paths [2, 8, 2], cfg, k)."""
    k, dt = 3, 0.1
    run = np.array([0.5, 1.0, 1.5, 2.0, 1.5, 1.0, 0.5, 0.0])
    paths = np.zeros((2, POINTS, 2))
    paths[0, :, 0], paths[0, :, 1] = 3.0 + run, -7.25
    paths[1, :, 1], paths[1, :, 0] = -40.0 + run, 12.5
    x = chord_lengths(paths[:1])
    s, dx, sl = notaknot_slopes(x, paths[:1, :, 0])
    deriv = lambda at: spline_eval(x, paths[:1, :, 0], s, dx, sl, np.array([at]))[1][0]  # noqa: E731
    lo, hi = 1.0, 2.0
    assert deriv(lo) > 0.0 > deriv(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if deriv(mid) > 0.0 else (lo, mid)
    best = min((abs(deriv(v / (k * dt) * (k * dt))), v / (k * dt)) for v in (lo, hi, np.nextafter(lo, 0), np.nextafter(hi, 9)))
    return paths, config(desired_velocity=best[1], timestep=dt, horizon=5), k


def exact_direction_cases():
    """(raw [n, 16], poses [n, 3]): rows exactly ahead (a, 0), then one row exactly behind, (-a, +0.0) and (-a, -0.0) -- atan2 gives
    +pi and -pi, the wrap's argument is exactly 2 pi or 0 --, then rows ahead again; the same with a saturated a = 1; an all-zero
    raw action; a single zero row at i = 1.  Each at poses with |theta| up to 4 pi, the multiples of pi / 2 included."""
    rows = []
    for a in (0.37, 1.0):
        for at in (1, 3, 7):
            for zero in (0.0, -0.0):
                r = np.tile(np.array([a, 0.0]), (POINTS, 1))
                r[at] = (-a, zero)
                rows.append(r.reshape(-1))
    rows.append(np.zeros(2 * POINTS))
    r = np.tile(np.array([0.5, 0.25]), (POINTS, 1))
    r[1] = 0.0
    rows.append(r.reshape(-1))
    thetas = np.array([0.0, np.pi / 2, -np.pi, 2 * np.pi, 4 * np.pi, -4 * np.pi, 7.7, -11.3, 3 * np.pi / 2, 12.566])
    raw = np.repeat(np.array(rows), thetas.size, axis=0)
    th = np.tile(thetas, len(rows))
    rng = np.random.default_rng(2200)
    poses = np.stack([rng.uniform(-100, 100, th.size), rng.uniform(-100, 100, th.size), th], axis=1)
    return raw, poses


# ---------------------------------------------------------------- the tables the tests share (built once per process)
# The QP against the enumerator: the first four are the configurations the follower's first tests ran; with the others every
# horizon 1..8 occurs.
QP_CONFIGS = (dict(), dict(horizon=1, r=(0.02, 0.3)), dict(horizon=3, q=(2.0, 0.5, 0.0, 0.3), r=(0.05, 0.2), p=(4.0, 20.0, 0.5, 2.0)),
              dict(horizon=8, timestep=0.05, desired_velocity=3.0, p=(30.0, 30.0, 3.0, 3.0)),
              dict(horizon=2, r=(0.3, 0.02), p=(3.0, 30.0, 1.0, 0.0)), dict(horizon=4, timestep=0.2), dict(horizon=6, desired_velocity=4.7, q=(0.0, 3.0, 1.0, 0.0)),
              dict(horizon=7, timestep=0.15, r=(0.01, 1.0)))


@functools.lru_cache(maxsize=None)
def g17_paths():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g17_paths.npz'))['paths']


@functools.lru_cache(maxsize=None)
def family(name):
    """A case family by name, with its classification: dict(paths, vels, cfg, info=classify(...), ...).  'bound2' / 'bound5' /
    'bound8': on_a_bound_cases; 'stiff': stiff_cases (with want, e_ref); 'release_order': release_order_cases; 'diagonal': EDGE_DIAGONAL on built velocities."""
    pool = g17_paths()
    if name.startswith('bound'):
        H = int(name[5:])
        paths, vels, kind, dropped, delta = on_a_bound_cases(pool, H)
        out = dict(paths=paths, vels=vels, cfg=config(horizon=H), kind=kind, dropped=dropped, delta=delta)
    elif name == 'stiff':
        paths, vels, want, e_ref = stiff_cases(pool)
        out = dict(paths=paths, vels=vels, cfg=config(**EDGE_STIFF), want=want, e_ref=e_ref)
    elif name == 'release_order':
        paths, vels, first, tells = release_order_cases(pool)
        out = dict(paths=paths, vels=vels, cfg=config(**EDGE_STIFF), first=first, tells=tells)
    else:
        assert name == 'diagonal'
        cfg = config(**EDGE_DIAGONAL)
        out = dict(paths=pool[:65], vels=built_cases(pool[:65], cfg, 2110), cfg=cfg)
    out['info'] = classify(out['paths'], out['vels'], out['cfg'])
    return out


FAMILIES = ('bound2', 'bound5', 'bound8', 'stiff', 'release_order', 'diagonal')


def walk_classes(info, H):
    """The arms of the walk and the patterns of the optimum that a classified table drives the kernel through."""
    b, r, nb = info['blocks'], info['releases'], info['bound']
    names = {'blocks only': (b > 0) & (r == 0), 'a release': (r > 0) & (b == 0), 'blocks and releases': (b > 0) & (r > 0),
             'neither': (b == 0) & (r == 0), 'all bound': nb == H, 'none bound': nb == 0, 'mixed': (nb > 0) & (nb < H)}
    return {k for k, m in names.items() if m.any()}
