"""The NumPy checker of gradient clipping (csrc/f110_adam_clip.h, the contract "Gradient clipping" of include/f110_hip.h) and the shape
tables of its tests.  Every addition is one fp64 addition in the contract's order: 256 chains by element index within a chunk, the
losses' tree, 256 chains over the chunk partials, the tree again; the square of an fp32 value is exact in fp64; sqrt and the division
are NumPy's float64 ones, which are correctly rounded.  The update itself is tests/optim_cases.py on g * coef."""
import numpy as np

import optim_cases as oc

CHUNK, THREADS, MAX_TENSORS = oc.CHUNK, oc.THREADS, oc.MAX_TENSORS
CLIP_STATE_BYTES = 64
NORM_EPS = 1e-6

# one tensor of 257 chunks: lane 0 of the step sum adds two partials, lane 1 one; and one of 257 whole chunks and 5 elements, 258
# chunks: lanes 0 and 1 add two
BIG_257 = 256 * CHUNK + 5
BIG = 257 * CHUNK + 5
# more tensors than a call holds: the step takes two calls, the second with a chunk_base
MANY = [1] * (MAX_TENSORS + 1) + [CHUNK + 1]
# max_norm far above every norm of these tests, far below, and the guard alone
FAR_ABOVE, FAR_BELOW, INF = 1e30, 1e-3, float('inf')


def chain_of(j):
    """The chain of a chunk's sum that takes element j of the chunk."""
    return (np.asarray(j) >> 2) & (THREADS - 1)


def chunk_numbers(sizes, base=0):
    """The number of every tensor's first chunk, numbered from `base` (an empty tensor owns none) -> (list, chunks)."""
    first, chunks = [], 0
    for n in sizes:
        first.append(base + chunks)
        chunks += (n + CHUNK - 1) // CHUNK
    return first, chunks


def tree(s):
    s = np.array(s, np.float64)
    assert s.shape == (THREADS,)
    w = THREADS // 2
    while w >= 1:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return s[0]


def chunk_partial(g):
    """P_c of one chunk's elements g (1 .. CHUNK of them, fp32).  A missing element is added as 0.0, which changes no bit: every
    term and every partial sum is +0.0 or larger, or NaN."""
    g = np.asarray(g, np.float32)
    assert 1 <= g.size <= CHUNK
    sq = np.zeros(CHUNK, np.float64)
    g64 = g.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        sq[:g.size] = g64 * g64
        sq = sq.reshape(CHUNK // (4 * THREADS), THREADS, 4)             # [round, chain, element of the quad]: j = 4 (chain + 256 round) + e
        s = np.zeros(THREADS, np.float64)
        for k in range(sq.shape[0]):
            for e in range(4):
                s = s + sq[k, :, e]
        return tree(s)


def partials(grads):
    """The chunk partials of one step: grads in table order, None for a parameter without a gradient (its chunks are not numbered)."""
    out = []
    for g in grads:
        if g is None:
            continue
        g = np.asarray(g, np.float32).reshape(-1)
        out += [chunk_partial(g[at:at + CHUNK]) for at in range(0, g.size, CHUNK)]
    return np.array(out, np.float64)


def step_sum(p):
    p = np.asarray(p, np.float64)
    padded = np.zeros((p.size + THREADS - 1) // THREADS * THREADS, np.float64)
    padded[:p.size] = p
    s = np.zeros(THREADS, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for row in padded.reshape(-1, THREADS):
            s = s + row
        return tree(s)


def new_clip():
    return dict(sumsq=np.float64(0), norm=np.float64(0), coef=np.float32(0), skip=0, steps_clipped=0, steps_skipped=0)


def clip(S, max_norm, before=None):
    """adam_clip_kernel's lane 0 on the step sum S -> the new clip state (the counters continue `before`'s)."""
    c = dict(new_clip() if before is None else before)
    S = np.float64(S)
    finite = bool(S < np.inf)
    if finite:
        norm = np.sqrt(S)
        q = np.float64(max_norm) / (norm + np.float64(NORM_EPS))
        coef = np.float32(q) if q < 1.0 else np.float32(1.0)
        c.update(sumsq=S, norm=norm, coef=coef, skip=0)
    else:
        c.update(sumsq=np.float64(np.inf), norm=np.float64(np.inf), coef=np.float32(1.0), skip=1)
    c['steps_clipped'] += int(finite and c['coef'] < np.float32(1.0))
    c['steps_skipped'] += int(not finite)
    return c


def clip_words(c):
    """f110_adam_clip_state as eight int64 words, for a bitwise comparison with the device's."""
    w = np.zeros(CLIP_STATE_BYTES // 8, np.int64)
    w.view(np.float64)[0:2] = c['sumsq'], c['norm']
    w.view(np.float32)[4] = c['coef']
    w.view(np.int32)[5] = c['skip']
    w[3], w[4] = c['steps_clipped'], c['steps_skipped']
    return w


def same_partials(got, want):
    """Bit for bit where the checker's partial is finite; a non-finite one must be non-finite of the same kind (a NaN's payload is no
    part of the contract)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return False
    fin = np.isfinite(want)
    return (bool((got[fin].view(np.uint64) == want[fin].view(np.uint64)).all()) and bool((np.isnan(got[~fin]) == np.isnan(want[~fin])).all())
            and bool((np.isposinf(got[~fin]) == np.isposinf(want[~fin])).all()))


def run(params, grads, max_norm, targets=None, state=None, moments=None, clip_state=None, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, tau=oc.TAU):
    """len(grads) clipped steps on lists of arrays, as optim_cases.run takes them -> (params, exp_avg, exp_avg_sq, targets or None,
    state, clip state, the last step's partials).  A step without any gradient leaves the clip state alone; a skipped step leaves
    params, moments and state alone and still moves the targets.  The inputs are left unchanged."""
    ps = [np.array(p, np.float32) for p in params]
    ms = [np.zeros_like(p) for p in ps] if moments is None else [np.array(m, np.float32) for m in moments[0]]
    vs = [np.zeros_like(p) for p in ps] if moments is None else [np.array(v, np.float32) for v in moments[1]]
    ts = None if targets is None else [np.array(t, np.float32) for t in targets]
    state = dict(oc.new_state(betas) if state is None else state)
    cs = dict(new_clip() if clip_state is None else clip_state)
    last = np.zeros(0, np.float64)
    for gs in grads:
        stepping = any(g is not None for g in gs)
        if stepping:
            last = partials(gs)
            cs = clip(step_sum(last), max_norm, cs)
            stepping = not cs['skip']
        if stepping:
            oc.advance(state, lr, betas)
        for i, g in enumerate(gs):
            if g is not None and stepping:
                gc = np.asarray(g, np.float32) * cs['coef']
                assert gc.dtype == np.float32
                ps[i], ms[i], vs[i] = oc.adam(ps[i], gc, ms[i], vs[i], state, betas, eps)
            if ts is not None:
                ts[i] = oc.lerp(ts[i], ps[i], tau)
    return ps, ms, vs, ts, state, cs, last
