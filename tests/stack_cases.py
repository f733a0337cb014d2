"""The checker of the frame stacks (csrc/f110_replay.h replay_stack_kernel and csrc/f110_bitconv.h's stacked kernels; the contracts
of include/f110_hip.h), NumPy and Python numbers only, in three statements: stack(), the walk's contract over the ring's valid array
and count; brute(), the same rows from nstep_cases.episodes(), which never looks at a slot or a modulus until a frame row is named; and
forward_stack(), bitconv_cases.forward with the frames of a stack added one behind the other in float32.  base_ring() is the scripted
ring the census is taken on: the n-step census ring has five step slots, too few for a stack of four."""
import numpy as np

import bitconv_cases as bc
import nstep_cases as nc

MAX_STACK = 8
STACKS = (1, 2, 3, 4, 8)
ENDS = ('full', 'reset', 'unstepped', 'chain_start', 'oldest')


# ---------------------------------------------------------------------------------------------- the contract
def links(valid, count, p, env):
    """Push p of env links frame p to frame p - 1: its step slot is still the ring's and its transition is valid."""
    T = valid.shape[0]
    return p >= max(int(count) - T, 0) and valid[p % T, env] != 0


def stack(valid, count, frame_rows, k):
    """The contract: dict of rows [n, k] int64, depth [n] int32 and, beside them, c [n] (the push the row stands for, -1 for a refused
    row), cut [n] (the push that did not link, -1 for a full or refused stack) and loaded [n] (the pushes whose link was asked, newest
    first).  frame_rows None: the latest mode, row i = env i's newest frame."""
    assert 1 <= k <= MAX_STACK
    valid, count = np.asarray(valid), int(count)
    T, B = valid.shape
    F = T + 1
    latest = frame_rows is None
    n = B if latest else len(frame_rows)
    out = dict(rows=np.full((n, k), -1, np.int64), depth=np.zeros(n, np.int32), c=np.full(n, -1, np.int64), cut=np.full(n, -1, np.int64),
               loaded=[[] for _ in range(n)])
    for i in range(n):
        if latest:
            if count < 1:
                continue
            c, env = count - 1, i
        else:
            row = int(frame_rows[i])
            if not (0 <= row < F * B and count >= 1):
                continue
            slot, env = divmod(row, B)
            if slot > count - 1:
                continue
            c = max(p for p in range(max(count - F, 0), count) if p % F == slot)   # the newest push of the slot: one of the F live frames
        rows, depth = [(c % F) * B + env], 1
        for j in range(1, k):
            p = c - j + 1
            out['loaded'][i].append(p)
            if not links(valid, count, p, env):
                out['cut'][i] = p
                break
            assert p >= 1, 'push 0 has no frame before it and is never valid'
            rows.append(((c - j) % F) * B + env)
            depth += 1
        rows += [rows[-1]] * (k - depth)
        out['rows'][i], out['depth'][i], out['c'][i] = rows, depth, c
    return out


# ---------------------------------------------------------------------------------------------- the brute-force statement
def brute(pushes, T, B, count, frame_rows, k):
    """The stacks of `frame_rows` from nstep_cases.episodes(): the stored transitions of an env cut into runs of consecutive pushes
    (a stack does not ask whether a step was terminal -- the reset behind it is what cuts -- so every done is handed over as 0).  The
    frames of a run are the frame before its first push and the frame of each of its pushes; a frame's predecessors are those inside
    its run, a frame no run holds stands alone.  -> (rows [n, k] int64, depth [n] int32)."""
    plain = [(c, [None if t is None else (t[0], 0) for t in rec]) for c, rec in pushes]
    first = {}                                              # (env, frame) -> the oldest frame of its run
    for e, runs in enumerate(nc.episodes(plain, B)):
        for run in runs:
            assert run[0][0] >= 1
            for c, _, _ in run:
                first[(e, c)] = run[0][0] - 1
    where = {}
    for f in range(max(0, count - 1 - T), count):           # the T + 1 live frames; only here a slot is named
        for e in range(B):
            where[(f % (T + 1)) * B + e] = (e, f)
    n = len(frame_rows)
    rows, depth = np.full((n, k), -1, np.int64), np.zeros(n, np.int32)
    for i, row in enumerate(frame_rows):
        if int(row) not in where:
            continue
        e, f = where[int(row)]
        frames = list(range(f, first.get((e, f), f) - 1, -1))[:k]
        depth[i] = len(frames)
        frames += [frames[-1]] * (k - len(frames))
        rows[i] = [(g % (T + 1)) * B + e for g in frames]
    return rows, depth


def all_rows(T, B):
    """Every row of the frame tensor, and one on either side."""
    return np.arange(-1, (T + 1) * B + 1, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- the scripted rings
BASE = dict(T=9, B=8, count=22)
# per env the pushes 13 .. 21 (count - T .. count - 1): v a valid step, r the env's reset (the push before it is done), u the env was not
# stepped by the call, c the chain break (chain_start: every env at once)
BASE_SCRIPT = ('vcvvvvvvv',     # frames 12, 13 end at the ring's oldest frame, 14 .. 16 at the chain break, 17 .. 21 are full
               'vcvvvrvvv',     # the reset is push 18, in step slot 0: frames 18 .. 20 end in front of it
               'vcvvvvuuv',     # not stepped at pushes 19 and 20
               'vcvvrvvvv',     # the reset is push 17, in step slot T - 1: the stacks of frames 18 and 19 ask across the step-slot seam
               'vcvvvvvrv',     # the reset is push 20: its spawn frame is frame slot 0, frame 21 stacks over it and no further
               'vcuvvvvvv',     # not stepped at push 15
               'rcvvvvvvv',     # reset at the oldest stored push
               'vcvvvvvvr')     # reset at the newest push: the spawn frame stacks over itself


def base_ring():
    """The base ring (T = 9, B = 8, count = 22: one wrap and four pushes into the next; pushes 13 .. 21 are stored in step slots 4 .. 8,
    0 .. 3 and frames 12 .. 21 in frame slots 2 .. 9, 0, 1).  -> (valid, dones, rewards, count)"""
    T, B, count = BASE['T'], BASE['B'], BASE['count']
    valid, dones = np.zeros((T, B), np.uint8), np.zeros((T, B), np.uint8)
    for e, script in enumerate(BASE_SCRIPT):
        assert len(script) == T
        for k, p in enumerate(range(count - T, count)):
            valid[p % T, e] = script[k] == 'v'
            dones[p % T, e] = script[k] == 'v' and k + 1 < T and script[k + 1] == 'r'
    return valid, dones, nc._rewards(T, B, 4), count


def base_why(p, env):
    """Why push p of the base ring does not link."""
    count, T = BASE['count'], BASE['T']
    if p < count - T:
        return 'oldest'
    return {'r': 'reset', 'u': 'unstepped', 'c': 'chain_start'}[BASE_SCRIPT[env][p - (count - T)]]


def rings():
    """name -> ring: the base ring and the three of nstep_cases.rings() (T = 5: the census ring, one that has not wrapped, one of count
    = 2 T + 1)."""
    out = {'base': base_ring()}
    out.update({'nstep_' + k: v for k, v in nc.rings().items()})
    return out


def census(k=4):
    """How the stacks of every frame row of the base ring end at stack = k, counted from stack() alone: {end: count} over ENDS, and
    under 'step_seam' / 'frame_seam' the ends of the stacks that ask the link of push p and of push p - 1 with p % T == 0 (step slot 0,
    then T - 1) / that hold frames f and f - 1 with f % (T + 1) == 0 (frame slot 0, then T)."""
    valid, _, _, count = base_ring()
    T, B = valid.shape
    rows = np.arange((T + 1) * B, dtype=np.int64)
    s = stack(valid, count, rows, k)
    out = {e: 0 for e in ENDS}
    out['step_seam'], out['frame_seam'] = [], []
    for i in range(len(rows)):
        assert s['depth'][i] >= 1
        env, c, depth = int(rows[i]) % B, int(s['c'][i]), int(s['depth'][i])
        end = 'full' if depth == k else base_why(int(s['cut'][i]), env)
        out[end] += 1
        loaded = s['loaded'][i]
        if any(p % T == 0 and p - 1 in loaded for p in loaded):
            out['step_seam'].append(end)
        if any(f % (T + 1) == 0 for f in range(c, c - depth + 1, -1)):
            out['frame_seam'].append(end)
    return out


# ---------------------------------------------------------------------------------------------- the stacked convolution
def params_stack(kernel, channels, k, seed=0):
    """weight [C, k, K, K] and bias [C] in fp32 of mixed sign and magnitude, as bitconv_cases.params."""
    rng = np.random.default_rng([kernel, channels, k, seed])
    shape = (channels, k, kernel, kernel)
    w = (rng.normal(size=shape) * 10.0 ** rng.integers(-2, 2, shape)).astype(np.float32)
    return w, rng.normal(size=channels).astype(np.float32)


def stack_index(n, k, frames, seed=0):
    """index [n, k] over `frames` frames: seeded draws, with a -1, an entry beyond the frames and a repeat within a row."""
    idx = np.random.default_rng([n, k, frames, seed]).integers(0, frames, (n, k)).astype(np.int64)
    idx[0, -1] = -1
    idx[-1, 0] = frames + 2
    if k > 1:
        idx[n // 2, 1] = idx[n // 2, 0] = 0
    return idx


def forward_stack(imgs, index, weight, bias, stride, on, relu):
    """bitconv_cases.forward for nn.Conv2d(k, C, K, stride): imgs [m, rows, cols] uint8, index [n, k] (an entry outside 0 .. m - 1 reads
    an empty frame), weight [C, k, K, K].  acc = 0; frames j major, then ky, then kx minor: acc = acc + w[c][j][ky][kx] where that tap of
    frame index[i][j] is set, in float32; out = (acc * on) + bias; the relu.  -> [n, C, OH, OW] float32"""
    w = np.asarray(weight, np.float32)
    index = np.asarray(index)
    ch, k, K, _ = w.shape
    assert index.shape[1] == k
    zero = np.float32(0.0)
    acc = None
    for j in range(k):
        sel = bc.taps(bc.pick(imgs, index[:, j]) == 255, K, stride)
        if acc is None:
            acc = np.zeros((index.shape[0], ch) + sel[0].shape[1:], np.float32)
        for t, s in enumerate(sel):
            wt = w[:, j, t // K, t % K]
            acc = acc + np.where(s[:, None], wt[None, :, None, None], zero).astype(np.float32)
            assert acc.dtype == np.float32
    b = np.zeros(ch, np.float32) if bias is None else np.asarray(bias, np.float32)
    out = (acc * np.float32(on)).astype(np.float32) + b[None, :, None, None]
    assert out.dtype == np.float32
    if relu:
        out = np.where(out < 0, zero, out).astype(np.float32)
    return out


def unpacked_stack(imgs, index):
    """[n, k, rows, cols] uint8: what a framework would stack for nn.Conv2d(k, ...)."""
    index = np.asarray(index)
    return np.stack([bc.pick(imgs, index[:, j]) for j in range(index.shape[1])], axis=1)
