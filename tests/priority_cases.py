"""Prioritized replay (red_gym_amd/csrc/f110_priority.h, include/f110_hip.h) restated from the header's contract: the level layout of
the integer sum tree, the rebuild, the set with its maximum rule, the pick, the quantisation of a TD error in NumPy fp64, the importance
weights and the weighted critic loss in the order of tests/sacloss_cases.py.  Words are uint32 and sums uint64 (L * 2^32 < 2^64 for every
L the contract admits), so NumPy's integer arithmetic is exact and `==` is the comparison; the descent itself runs in Python ints."""
import numpy as np

import replay_cases as rc
import sacloss_cases as sl

FANOUT, SHIFT, QMAX_WORD, MAX_LEAVES, STATE_BYTES = 64, 16, 2 ** 32 - 1, 2 ** 31, 64
ONE = 1 << SHIFT
CPU_L = (1, 63, 64, 65, 4095, 4096, 4097, 262144, 262145)          # the layout is also taken at 2^26
GPU_L = (1, 63, 64, 65, 4097, 262145)


def layout(L):
    """levels (0: the leaves are the top), the node count and the offset of every level, and the words of node[]."""
    counts, offsets, words, cur = [], [], 0, int(L)
    while cur > FANOUT:
        cur = -(-cur // FANOUT)
        counts.append(cur)
        offsets.append(words)
        words += cur
    return dict(levels=len(counts), count=counts, offset=offsets, words=words)


def rebuild(leaf):
    """node[] (uint64, level 1 first) for the leaves."""
    lay = layout(len(leaf))
    out, cur = np.zeros(lay['words'], np.uint64), np.asarray(leaf).astype(np.uint64)
    for k in range(lay['levels']):
        pad = np.zeros(lay['count'][k] * FANOUT, np.uint64)
        pad[:len(cur)] = cur
        cur = pad.reshape(-1, FANOUT).sum(axis=1, dtype=np.uint64)
        out[lay['offset'][k]:lay['offset'][k] + lay['count'][k]] = cur
    return out


def set_max(leaf, idx, q):
    """The leaves after f110_ptree_set: rows outside 0 .. L - 1 are skipped, a leaf several rows name becomes the maximum of their q."""
    leaf, idx, q = np.array(leaf, np.uint32), np.asarray(idx, np.int64), np.asarray(q, np.uint32)
    inside = (idx >= 0) & (idx < len(leaf))
    best = np.zeros(len(leaf), np.uint32)
    np.maximum.at(best, idx[inside], q[inside])
    named = np.unique(idx[inside])
    leaf[named] = best[named]
    return leaf


def draw_bits(seed, j):
    """Attempt 0 of the uniform draw j."""
    return rc.splitmix64(seed + rc.GOLDEN * (1 + j * rc.TRIES))


def pick(leaf, node, seed, first, n):
    """(idx [n] int64, q [n] uint32, path [n, levels + 1] int64) of draws first .. first + n - 1 by the descent of the contract; path holds
    the node taken on every level from the top down (its last column is idx); -1 everywhere for an empty tree."""
    leaf = np.asarray(leaf)
    lay = layout(len(leaf))
    level = [leaf.astype(np.uint64)] + [np.asarray(node)[lay['offset'][k]:lay['offset'][k] + lay['count'][k]] for k in range(lay['levels'])]
    top = level[-1][:FANOUT]
    total = sum(int(x) for x in top)
    idx, q = np.full(n, -1, np.int64), np.zeros(n, np.uint32)
    path = np.full((n, lay['levels'] + 1), -1, np.int64)
    if total == 0:
        return idx, q, path
    for i in range(n):
        u = (draw_bits(seed, first + i) * total) >> 64
        nd, children = 0, top
        for lev in range(lay['levels'], -1, -1):
            pre = np.cumsum(children, dtype=np.uint64)                    # the inclusive prefix sums across the lanes
            c = int(np.searchsorted(pre, np.uint64(u), side='right'))     # the first child whose prefix exceeds u
            assert c < len(children), 'a node is not the sum of its children'
            u -= int(pre[c]) - int(children[c])
            nd = nd * FANOUT + c
            path[i, lay['levels'] - lev] = nd
            if lev > 0:
                children = level[lev - 1][nd * FANOUT:nd * FANOUT + FANOUT]
        idx[i], q[i] = nd, leaf[nd]
    return idx, q, path


def pick_flat(leaf, seed, first, n):
    """The same draws over the flat leaves: searchsorted(cumsum(leaf), u, 'right')."""
    cum = np.cumsum(np.asarray(leaf).astype(np.uint64), dtype=np.uint64)
    total = int(cum[-1])
    if total == 0:
        return np.full(n, -1, np.int64)
    u = np.array([(draw_bits(seed, first + i) * total) >> 64 for i in range(n)], np.uint64)
    return np.searchsorted(cum, u, side='right').astype(np.int64)


def random_leaves(L, seed=0):
    """Words of one magnitude (every child of a node is drawn about as often as its siblings), the last leaf heavy: with L = 64^k + 1 it
    is alone in the last node of every level, and the draws must reach it."""
    leaf = np.random.default_rng([L, seed]).integers(1 << 19, 1 << 20, L).astype(np.uint32)
    leaf[-1] = min(max(int(leaf.astype(np.uint64).sum()) // 8, int(leaf[-1])), QMAX_WORD)
    return leaf


def sparse_leaves(L, seed=0):
    """Mostly zero, with runs of zeros at both ends (where L has the room); a handful of words up to 2^32 - 1."""
    rng = np.random.default_rng([L, seed, 1])
    leaf = np.where(rng.random(L) < 0.02, rng.integers(1, 1 << 32, L), 0).astype(np.uint32)
    edge = L // 5
    leaf[:edge] = 0
    leaf[L - edge:] = 0
    if not leaf.any():
        leaf[L // 2] = QMAX_WORD
    return leaf


def quantise(td, exponent, eps):
    """q [n] uint32 and p * 2^16 [n] fp64 of the TD errors td [n] fp32."""
    td = np.asarray(td, np.float32)
    with np.errstate(all='ignore'):
        s = td.astype(np.float64) + np.float64(eps)
        x = (s if exponent == 1.0 else np.power(s, np.float64(exponent))) * 65536.0         # (exponent 1: the sum itself, no pow)
        q = np.where(~(x < 4294967295.0), float(QMAX_WORD), np.where(~(x >= 1.0), 1.0, np.rint(x)))
    q = np.where(np.isnan(td) | (td == np.inf), float(QMAX_WORD), q)
    return q.astype(np.uint64).astype(np.uint32), x


def weights(prio, ok, beta):
    """fp32 [n]: (qmin / prio)^beta over the rows with ok, 0 elsewhere; qmin the smallest word of a row with ok."""
    prio, ok = np.asarray(prio, np.uint32), np.asarray(ok) != 0
    live = ok & (prio > 0)
    out = np.zeros(len(prio), np.float32)
    if live.any():
        qmin = np.float64(prio[live].min())
        out[live] = np.power(qmin / prio[live].astype(np.float64), np.float64(beta)).astype(np.float32)
    return out


def weighted_critic(q1, q2, tv, w):
    """-> (loss [2] fp32, grad_q1, grad_q2, td [n] fp32): t_i = double(w) * (e * e) summed in sacloss_cases' order."""
    n = tv.shape[0]
    assert q1.dtype == q2.dtype == tv.dtype == w.dtype == np.float32
    k2n = np.float32(2.0 / float(n))
    loss = np.array([np.float32(np.float64(sl.ordered_sum(w.astype(np.float64) * sl.critic_terms(q, tv))) / np.float64(n)) for q in (q1, q2)], np.float32)
    td = np.maximum(np.abs(q1 - tv), np.abs(q2 - tv))
    return loss, ((q1 - tv) * k2n) * w, ((q2 - tv) * k2n) * w, td


def state_words(state):
    """The fields of the 64 bytes of an f110_priority_state ([8] int64 as the device holds them)."""
    raw = np.ascontiguousarray(state).view(np.uint8)
    assert raw.size == STATE_BYTES
    return dict(qmax=int(raw[:4].view(np.uint32)[0]), reserved0=int(raw[4:8].view(np.uint32)[0]), beta=float(raw[8:16].view(np.float64)[0]),
                beta_step=float(raw[16:24].view(np.float64)[0]), beta_end=float(raw[24:32].view(np.float64)[0]), reserved=raw[32:].view(np.uint64).tolist())
