"""The NumPy float32 checker of the parameter update (csrc/f110_adam.h, the contract of include/f110_hip.h) and the size lists of its
tests.  Every line of the update is one correctly rounded fp32 operation (NumPy's float32 +, -, *, / and sqrt are; fma32 is the exact
fused step), the step state is fp64 advanced by one multiplication per step, and k2 and a are formed in fp64 and rounded once."""
import numpy as np

from bitconv2_cases import fma32

# csrc/f110_adam.h, include/f110_hip.h
CHUNK, MAX_TENSORS, THREADS, STATE_BYTES = 4096, 64, 256, 32

# one tensor of each: below, at and above a float4, a wave, a workgroup's round of vectors and a chunk; several chunks; an empty one
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 0]
MISALIGNED_SIZES = [5, CHUNK + 1]
# SAL's critic (src/SAL.py:424-433): conv1-3 weight and bias, fc1 [512, 25104], fc2
SAL_CRITIC = [(16, 1, 8, 8), (16,), (32, 16, 4, 4), (32,), (32, 32, 3, 3), (32,), (512, 25104), (512,), (1, 512), (1,)]
LR, BETAS, EPS, TAU = 3e-4, (0.9, 0.999), 1e-8, 0.005


def new_state(betas=BETAS, t=0):
    """The device state after t steps: the powers computed once on the host, as load_state_dict does."""
    return dict(t=int(t), pow1=float(betas[0]) ** int(t), pow2=float(betas[1]) ** int(t), k2=np.float32(0), a=np.float32(0))


def advance(state, lr=LR, betas=BETAS):
    """adam_advance_kernel: in place."""
    state['t'] += 1
    state['pow1'] = float(np.float64(state['pow1']) * np.float64(betas[0]))
    state['pow2'] = float(np.float64(state['pow2']) * np.float64(betas[1]))
    state['k2'] = np.float32(np.sqrt(np.float64(1.0) - np.float64(state['pow2'])))
    state['a'] = np.float32(np.float64(lr) / (np.float64(1.0) - np.float64(state['pow1'])))
    return state


def state_words(state):
    """f110_adam_state as four int64 words, for a bitwise comparison with the device's."""
    w = np.zeros(4, np.int64)
    w[0] = state['t']
    w.view(np.float64)[1:3] = state['pow1'], state['pow2']
    w.view(np.float32)[6:8] = state['k2'], state['a']
    return w


def adam(p, g, m, v, state, betas=BETAS, eps=EPS):
    """One element-wise Adam update with the advanced `state` -> (p', m', v'), all float32."""
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    c1, c2, b2, e = np.float32(1.0 - betas[0]), np.float32(1.0 - betas[1]), np.float32(betas[1]), np.float32(eps)
    d = g - m
    m1 = fma32(c1, d, m)
    t1 = g * g
    t2 = t1 * c2
    v1 = fma32(b2, v, t2)
    s = np.sqrt(v1)
    r = s / state['k2']
    den = r + e
    q = m1 / den
    p1 = fma32(-state['a'], q, p)
    for x in (d, t1, t2, s, r, den, q):
        assert x.dtype == np.float32
    return p1, m1, v1


def lerp(tp, p, tau=TAU):
    """The target rule: u = p - tp; tp' = fmaf(float(tau), u, tp)."""
    tp, p = np.asarray(tp, np.float32), np.asarray(p, np.float32)
    u = p - tp
    assert u.dtype == np.float32
    return fma32(np.float32(tau), u, tp)


def values(rng, n, scale=1.0):
    return (rng.normal(size=n) * scale).astype(np.float32)


def gradients(rng, n):
    """Magnitudes from 1e-3 to 1e3 with both signs, exact zeros, and (where there is room) values whose square is a denormal that
    survives the multiplication by 1 - beta2 (1e-20) and one that does not (1e-22)."""
    g = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(np.float32)
    if n >= 8:
        g[rng.integers(0, n, size=max(1, n // 16))] = 0.0
        g[n // 2], g[n // 2 + 1], g[n // 2 + 2] = 1e-20, -1e-22, -0.0
    return g


def run(params, grads, targets=None, state=None, moments=None, lr=LR, betas=BETAS, eps=EPS, tau=TAU):
    """len(grads) steps on lists of arrays; grads[k][i] None: parameter i has no gradient at step k (untouched, its target still
    moved) -> (params, exp_avg, exp_avg_sq, targets or None, state).  The inputs are left unchanged."""
    ps = [np.array(p, np.float32) for p in params]
    ms = [np.zeros_like(p) for p in ps] if moments is None else [np.array(m, np.float32) for m in moments[0]]
    vs = [np.zeros_like(p) for p in ps] if moments is None else [np.array(v, np.float32) for v in moments[1]]
    ts = None if targets is None else [np.array(t, np.float32) for t in targets]
    state = dict(new_state(betas) if state is None else state)
    for gs in grads:
        if any(g is not None for g in gs):
            advance(state, lr, betas)
        for i, g in enumerate(gs):
            if g is not None:
                ps[i], ms[i], vs[i] = adam(ps[i], g, ms[i], vs[i], state, betas, eps)
            if ts is not None:
                ts[i] = lerp(ts[i], ps[i], tau)
    return ps, ms, vs, ts, state


def adam64(params, grads, lr=LR, betas=BETAS, eps=EPS):
    """torch.optim.Adam's formula in fp64 from the same fp32 gradients -> params after len(grads) steps."""
    ps = [np.array(p, np.float64) for p in params]
    ms, vs = [np.zeros_like(p) for p in ps], [np.zeros_like(p) for p in ps]
    for k, gs in enumerate(grads):
        t = k + 1
        for i, g in enumerate(gs):
            g = np.asarray(g, np.float64)
            ms[i] = ms[i] + (1.0 - betas[0]) * (g - ms[i])
            vs[i] = betas[1] * vs[i] + (1.0 - betas[1]) * g * g
            den = np.sqrt(vs[i]) / np.sqrt(1.0 - betas[1] ** t) + eps
            ps[i] = ps[i] - (lr / (1.0 - betas[0] ** t)) * (ms[i] / den)
    return ps


def ulp32(x):
    """The spacing of float32 at |x| (x fp64)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def ulps_apart(a, b):
    """How many float32 values lie between a and b, element by element (same-sign finite values or zeros)."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
