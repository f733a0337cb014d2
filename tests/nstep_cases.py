"""The checker of the n-step walk (csrc/f110_replay.h replay_walk, the contract of include/f110_hip.h), NumPy and Python numbers only,
in three statements: walk(), the contract over the ring's arrays (valid, dones, rewards [T, B] and count); brute(), the same quantities
from per-env lists of episodes, which never looks at a slot or a modulus until a frame row is named; and target_rows(), the one-step
target's arithmetic of tests/qhead_cases.py with a discount per row in gamma's place.  Python's and NumPy's fp64 products and sums are
rounded one by one, which is the contract's order."""
import numpy as np

import qhead_cases as qc
import replay_cases as rc

MAX_NSTEP = 64
GAMMA = 0.99
NSTEPS = (1, 2, 3, 5, 64)
ENDS = ('full', 'newest', 'invalid', 'done_inside', 'done_on_last_of_full')


def resolve(valid, count, idx):
    """replay_resolve: (ok, push c, env) of index = step slot * B + env as `count` stands."""
    T, B = valid.shape
    idx, count = int(idx), int(count)
    if not (0 <= idx < T * B and count >= 1):
        return False, 0, 0
    slot, env = divmod(idx, B)
    if not (slot <= count - 1 and valid[slot, env] != 0):
        return False, 0, env
    c = count - 1 - (count - 1 - slot) % T
    return c >= 1, c, env


def one_step(valid, dones, rewards, count, indices):
    """What f110_replay_locate / the gather's tail give: dict of s_frame, ns_frame [n] int64, r [n] fp64, d, ok [n] uint8."""
    T, B = valid.shape
    n = len(indices)
    out = dict(s_frame=np.full(n, -1, np.int64), ns_frame=np.full(n, -1, np.int64), r=np.zeros(n, np.float64), d=np.zeros(n, np.uint8),
               ok=np.zeros(n, np.uint8))
    for i, idx in enumerate(indices):
        ok, c, env = resolve(valid, count, idx)
        if ok:
            slot = int(idx) // B
            out['s_frame'][i], out['ns_frame'][i] = ((c - 1) % (T + 1)) * B + env, (c % (T + 1)) * B + env
            out['r'][i], out['d'][i], out['ok'][i] = rewards[slot, env], dones[slot, env], 1
    return out


def walk(valid, dones, rewards, count, indices, nstep, gamma):
    """The contract: dict of ns_frame [n] int64, ret [n] fp64, d [n] uint8, discount [n] fp64, span [n] int32 and, beside them, c0 [n]
    (the push, -1 for a refused row) and end [n] (one of ENDS, '' for a refused row): why the span is as long as it is."""
    assert 1 <= nstep <= MAX_NSTEP
    valid, dones, rewards = np.asarray(valid), np.asarray(dones), np.asarray(rewards, np.float64)
    T, B = valid.shape
    n = len(indices)
    gamma = np.float64(gamma)
    out = dict(ns_frame=np.full(n, -1, np.int64), ret=np.zeros(n, np.float64), d=np.zeros(n, np.uint8), discount=np.full(n, gamma, np.float64),
               span=np.zeros(n, np.int32), c0=np.full(n, -1, np.int64), end=[''] * n)
    for i, idx in enumerate(indices):
        ok, c0, env = resolve(valid, count, idx)
        if not ok:
            continue
        # the span: the largest m whose pushes are all stored and valid, with no done in front of the last one
        m = 1
        while m < nstep and c0 + m <= count - 1 and valid[(c0 + m) % T, env] != 0 and dones[(c0 + m - 1) % T, env] == 0:
            m += 1
        R, g = np.float64(rewards[c0 % T, env]), gamma
        for k in range(1, m):
            R = R + g * rewards[(c0 + k) % T, env]
            g = g * gamma
        last = c0 + m - 1
        d = int(dones[last % T, env] != 0)
        out['ns_frame'][i], out['ret'][i], out['d'][i], out['discount'][i], out['span'][i], out['c0'][i] = (last % (T + 1)) * B + env, R, d, g, m, c0
        if m == nstep:
            out['end'][i] = 'done_on_last_of_full' if d else 'full'
        elif d:
            out['end'][i] = 'done_inside'
        else:
            out['end'][i] = 'newest' if last == count - 1 else 'invalid'
            assert last == count - 1 or valid[(last + 1) % T, env] == 0
    return out


# ---------------------------------------------------------------------------------------------- the brute-force statement
def pushes_of_arrays(valid, dones, rewards, count):
    """The stored pushes, oldest first: [(c, [None | (reward, done) per env])] -- what a deque(maxlen=T) of pushes holds."""
    T, B = np.asarray(valid).shape
    return [(c, [(float(rewards[c % T, e]), int(dones[c % T, e] != 0)) if valid[c % T, e] else None for e in range(B)])
            for c in range(max(0, int(count) - T), int(count))]


def pushes_of_mirror(mirror):
    """The same from a replay_cases.Mirror (its records are (s, a, r, ns, d) or None)."""
    return [(c, [None if t is None else (t[2], t[4]) for t in rec]) for c, rec in mirror.steps]


def episodes(pushes, B):
    """Per env, the stored transitions cut into runs of consecutive pushes that belong together: a run ends behind a done and in front
    of a push without a transition.  -> [env][run] = [(c, reward, done), ...]"""
    out = []
    for e in range(B):
        runs, cur = [], []
        for c, rec in pushes:
            if rec[e] is None:
                if cur:
                    runs.append(cur)
                cur = []
                continue
            assert not cur or cur[-1][0] + 1 == c
            cur.append((c, rec[e][0], rec[e][1]))
            if rec[e][1]:
                runs.append(cur)
                cur = []
        if cur:
            runs.append(cur)
        out.append(runs)
    return out


def brute(pushes, T, B, indices, nstep, gamma):
    """The n-step quantities of `indices` from episodes(): a transition's successors inside its run, at most nstep - 1 of them, summed
    with the running product.  The same dict as walk() without c0 and end."""
    n = len(indices)
    gamma = np.float64(gamma)
    out = dict(ns_frame=np.full(n, -1, np.int64), ret=np.zeros(n, np.float64), d=np.zeros(n, np.uint8), discount=np.full(n, gamma, np.float64),
               span=np.zeros(n, np.int32))
    where = {}
    for e, runs in enumerate(episodes(pushes, B)):
        for run in runs:
            for p, (c, _, _) in enumerate(run):
                if c >= 1:                                    # (push 0 has no frame before it)
                    where[(c % T) * B + e] = (e, run, p)
    for i, idx in enumerate(indices):
        if int(idx) not in where:
            continue
        e, run, p = where[int(idx)]
        steps = run[p:p + nstep]
        R, g = np.float64(steps[0][1]), gamma
        for _, r, _ in steps[1:]:
            R = R + g * np.float64(r)
            g = g * gamma
        out['ns_frame'][i], out['ret'][i], out['d'][i], out['discount'][i], out['span'][i] = (steps[-1][0] % (T + 1)) * B + e, R, steps[-1][2], g, len(steps)
    return out


# ---------------------------------------------------------------------------------------------- the scripted rings
def _rewards(T, B, seed):
    """Rewards of mixed magnitude, so that the order of the sums shows in the last bits."""
    rng = np.random.default_rng([T, B, seed])
    return rng.normal(size=(T, B)) * 10.0 ** rng.integers(-3, 3, (T, B))


def census_ring():
    """The base ring: DRAW_CASE's shape (T = 5, B = 7, count = 13: pushes 8 .. 12 are stored in step slots 3, 4, 0, 1, 2 and frame slots
    2, 3, 4, 5, 0) with one column of (valid, done) per env, push 8 first, chosen so that at nstep = 3 every way a span ends occurs
    at least three times (test_nstep_cpu.py counts them from walk() alone).  -> (valid, dones, rewards, count)"""
    c = rc.DRAW_CASE
    T, B, count = c['T'], c['B'], c['count']
    # per env: valid of pushes 8 .. 12, then the pushes that are done
    script = [((1, 1, 1, 1, 1), ()),          # 8, 9, 10 full; 11, 12 cut by the newest push
              ((1, 1, 1, 0, 1), (10,)),       # 8: done on the last step of a full span; 9, 10: cut by the done; 11 is the reset; 12: newest
              ((1, 1, 1, 1, 1), (12,)),       # 8, 9 full; 10: done on the last step; 11, 12: cut by the done
              ((1, 1, 0, 1, 1), ()),          # 8, 9: cut by the invalid push 10; 11, 12: newest
              ((1, 0, 1, 1, 1), (12,)),       # 8: cut by the invalid push 9; 10: done on the last step; 11, 12: cut by the done
              ((1, 1, 1, 1, 1), ()),          # as env 0
              ((0, 1, 1, 1, 0), ())]          # 9: full; 10, 11: cut by the invalid push 12
    valid, dones = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8)
    for e, (v, done_at) in enumerate(script):
        for k, c0 in enumerate(range(count - T, count)):
            valid[c0 % T, e] = v[k]
            dones[c0 % T, e] = int(c0 in done_at)
    return valid, dones, _rewards(T, B, 1), count


def random_ring(T, B, count, seed):
    """A ring after `count` pushes with 75 % of the stored transitions valid and a fifth of those done; push 0 (no frame before it)
    and the slots no push has reached are invalid.  -> (valid, dones, rewards, count)"""
    rng = np.random.default_rng([T, B, count, seed])
    valid = (rng.random((T, B)) < 0.75).astype(np.uint8)
    dones = ((rng.random((T, B)) < 0.2) & (valid != 0)).astype(np.uint8)
    for slot in range(T):
        if slot > count - 1 or (count <= T and slot == 0):
            valid[slot] = 0
    return valid, dones, _rewards(T, B, seed), count


def rings():
    """name -> ring: the census ring, one that has not wrapped (count < T) and one of count = 2 T + 1."""
    c = rc.DRAW_CASE
    return {'census': census_ring(), 'not_wrapped': random_ring(c['T'], c['B'], 3, 2), 'two_wraps': random_ring(c['T'], c['B'], 2 * c['T'] + 1, 3)}


def all_indices(T, B):
    """Every index of the ring, and one on either side."""
    return np.arange(-1, T * B + 1, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- the target with a discount per row
def target_rows(inp, discount, alpha, C=None, fp32_action=False, bias=True):
    """tv [n] float32 of qc.inputs()-shaped `inp`: qc.forward's q and qmin, then the two fp64 lines of its target with discount[b]
    where gamma stands: tq = qmin - alpha * nlp; tv = reward + ((1.0 - done) * discount) * tq, rounded once."""
    fwd = qc.forward(inp, C=C, fp32_action=fp32_action, bias=bias, target=False)
    nlp = np.asarray(inp['nlp'], np.float64)
    if fp32_action:
        nlp = nlp.astype(np.float32).astype(np.float64)
    tq = fwd['qmin'].astype(np.float64) - np.float64(alpha) * nlp
    keep = (1.0 - inp['done'].astype(np.float64)) * np.asarray(discount, np.float64)
    return (np.asarray(inp['reward'], np.float64) + keep * tq).astype(np.float32), fwd
