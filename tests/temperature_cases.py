"""The temperature step (red_gym_amd/csrc/f110_temperature.h, include/f110_hip.h) restated in NumPy from the header's contract, composed
of the checkers it shares its arithmetic with: sacloss_cases.ordered_sum for the sum, optim_cases.advance and optim_cases.adam for the
state and the one element.  Everything but alpha is `==` material: NumPy's fp32 and fp64 arithmetic is correctly rounded.  alpha is one
fp64 exp: the device's library against NumPy's, judged with alpha_bound."""
import numpy as np

import optim_cases as oc
import policyhead_cases as ph
import sacloss_cases as sl

N = sl.GPU_N                                   # chains without a term, one term per chain, a chain of two, a long tail
MAX_ROWS = 2 ** 24
STATE_BYTES = 64
LR, BETAS, EPS, TARGET_ENTROPY, INIT_ALPHA = 3e-4, oc.BETAS, oc.EPS, -16.0, 0.2
CFG = dict(betas=BETAS, eps=EPS, target_entropy=TARGET_ENTROPY)


def new_state(init_alpha=INIT_ALPHA, betas=BETAS, t=0, log_alpha=None, m=0.0, v=0.0):
    """The state as the host writes it: alpha = init_alpha exactly, log_alpha = float(log(init_alpha)) unless given."""
    la = np.float32(np.log(np.float64(init_alpha))) if log_alpha is None else np.float32(log_alpha)
    return dict(adam=oc.new_state(betas, t), alpha=float(init_alpha), log_alpha=la, m=np.float32(m), v=np.float32(v),
                grad=np.float32(0), loss=np.float32(0))


def resumed_state():
    """A state at t = 7 with non-zero moments and a log_alpha off its start."""
    return new_state(init_alpha=0.37, t=7, log_alpha=np.float32(-0.99341), m=-3.1234567, v=41.87654)


def mean_of(logp, target_entropy):
    """t_i = double(logp[i]) + target_entropy; S_0 in the losses' order; mean = S_0 / double(n)."""
    t = np.asarray(logp).astype(np.float64) + np.float64(target_entropy)
    return np.float64(sl.ordered_sum(t)) / np.float64(t.shape[0]), t


def step(logp, state, cfg=CFG, lr=LR):
    """One f110_temperature_step -> the new state (the input is left unchanged)."""
    mean, _ = mean_of(logp, cfg['target_entropy'])
    s = dict(state, adam=dict(state['adam']))
    s['loss'] = np.float32(-(np.float64(state['log_alpha']) * mean))
    s['grad'] = np.float32(-mean)
    oc.advance(s['adam'], lr, cfg['betas'])
    p, m, v = oc.adam(state['log_alpha'], s['grad'], state['m'], state['v'], s['adam'], cfg['betas'], cfg['eps'])
    s['log_alpha'], s['m'], s['v'] = np.float32(p), np.float32(m), np.float32(v)
    s['alpha'] = float(np.exp(np.float64(s['log_alpha'])))
    return s


def state_words(state):
    """f110_temperature_state as eight int64 words."""
    w = np.zeros(8, np.int64)
    w[:4] = oc.state_words(state['adam'])
    w.view(np.float64)[4] = state['alpha']
    w.view(np.float32)[10:15] = state['log_alpha'], state['m'], state['v'], state['grad'], state['loss']
    return w


def exact_words(words):
    """The words of a state without alpha (word 4), the one field that is not bit-exact."""
    return np.delete(np.asarray(words, np.int64), 4)


def alpha_of(words):
    return float(np.asarray(words, np.int64).view(np.float64)[4])


def alpha_bound(log_alpha):
    """One device exp against NumPy's: the project's bound for that pair (tests/policyhead_cases.py)."""
    return (ph.ULP_EXP + ph.ULP_NUMPY) * ph._ulp(np.exp(np.float64(log_alpha)))


def inputs(n, dtype=np.float64, seed=0):
    """log_prob for n rows: sacloss_cases.case's (in the tens, nothing a multiple of a power of two) and, where there is room,
    sacloss_cases.cancelling's +-2^60 pair in one chain added on top, so that a sum in another order gives other bits."""
    logp = sl.case(n, seed=seed, logp_dtype=np.float64)['logp'].copy()
    if n > 256:
        logp = logp + sl.cancelling(n, False)['logp']
    return logp.astype(dtype)
