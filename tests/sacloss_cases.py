"""The two SAC losses (red_gym_amd/csrc/f110_sacloss.h, include/f110_hip.h) restated in NumPy from the header's contract: the terms
in fp64, 256 chains over i = l mod 256 ascending, the tree over the chains with strides 128 .. 1, one fp64 division by n, one rounding to
fp32; the gradients one correctly rounded fp32 (or fp64) operation per line.  NumPy's element-wise fp32 and fp64 arithmetic is
correctly rounded and keeps denormals, so `==` is the comparison."""
import numpy as np

SL_THREADS, SL_MAX_GRID, MAX_ROWS = 256, 64, 2 ** 24
GPU_N = (1, 3, 63, 64, 65, 257, 4097)          # one lane, a partial wave, the wave boundary, more than one workgroup, a tail
CPU_N = GPU_N + (2, 16, 255, 256, 512, 1000, 4096, 70000)


def ordered_sum(t):
    """S_0 of the contract for the fp64 terms t [n]."""
    t = np.asarray(t, np.float64)
    chains = np.zeros(SL_THREADS, np.float64)
    for first in range(0, t.shape[0], SL_THREADS):
        seg = t[first:first + SL_THREADS]
        chains[:seg.shape[0]] = chains[:seg.shape[0]] + seg
    w = SL_THREADS // 2
    while w >= 1:
        chains[:w] = chains[:w] + chains[w:2 * w]
        w //= 2
    return chains[0]


def _mean32(s, n):
    return np.float32(np.float64(s) / np.float64(n))


def critic_terms(q, tv):
    e = q.astype(np.float64) - tv.astype(np.float64)
    return e * e


def critic(q1, q2, tv):
    """-> (loss [2] fp32, grad_q1, grad_q2 [n] fp32)."""
    n = tv.shape[0]
    assert q1.dtype == q2.dtype == tv.dtype == np.float32
    k2n = np.float32(2.0 / float(n))
    loss = np.array([_mean32(ordered_sum(critic_terms(q, tv)), n) for q in (q1, q2)], np.float32)
    return loss, (q1 - tv) * k2n, (q2 - tv) * k2n


def actor_terms(logp, qn, alpha):
    m = np.float64(alpha) * logp.astype(np.float64)
    return m - qn.astype(np.float64)


def actor(logp, qn, alpha):
    """-> (loss [1] fp32, grad_logp [n] of logp's dtype, grad_qn [n] fp32)."""
    n = qn.shape[0]
    assert logp.dtype in (np.float64, np.float32) and qn.dtype == np.float32
    loss = np.array([_mean32(ordered_sum(actor_terms(logp, qn, alpha)), n)], np.float32)
    g = np.float64(alpha) / np.float64(n)
    return loss, np.full(n, g, np.float64).astype(logp.dtype), np.full(n, np.float32(-1.0 / float(n)), np.float32)


def plan(n, actor_kernel=False, logp_fp64=False, alpha=0.0):
    """What f110_sacloss_plan.h plans for n rows: the launch and the scalars of the gradients."""
    g = np.float64(alpha) / np.float64(n)
    return dict(grid=min(-(-n // SL_THREADS), SL_MAX_GRID), block=SL_THREADS, lds=0, inst=(1 + int(logp_fp64)) if actor_kernel else 0,
                k2n=np.float32(2.0 / float(n)), glp64=g, glp32=np.float32(g), gqn=np.float32(-1.0 / float(n)))


def case(n, seed=0, logp_dtype=np.float64):
    """Inputs of both kernels for n rows: q's and a target a few units apart, a log_prob in the tens, and values that are no
    multiples of a power of two, so that every addition rounds."""
    rng = np.random.default_rng([seed, n])
    tv = (3.0 * rng.normal(size=n)).astype(np.float32)
    q1, q2 = ((tv + rng.normal(size=n)).astype(np.float32) for _ in range(2))
    logp = (10.0 * rng.normal(size=n) - 5.0).astype(logp_dtype)
    qn = np.minimum(q1, q2) + rng.normal(size=n).astype(np.float32)
    return dict(q1=q1, q2=q2, tv=tv, logp=logp, qn=qn.astype(np.float32))


def cancelling(n, apart):
    """An actor case (alpha = 1) whose loss shows the order in fp32: qn = 1 everywhere and log_prob = 0 but for +2^60 in row 0 and
    -2^60 in row 256 (one chain: they cancel exactly before any one is added, the loss is -(n - 2) / n) or, `apart`, in row 1 (two
    chains that absorb their ones into 2^60 before the tree lets them cancel).  The same rows, permuted."""
    assert n > 256
    logp, qn = np.zeros(n, np.float64), np.ones(n, np.float32)
    logp[0], logp[1 if apart else 256] = 2.0 ** 60, -2.0 ** 60            # (their own -1 is below half a unit of 2^60: t = -+2^60)
    return dict(logp=logp, qn=qn)


def butterfly(n, m):
    """The permutation i -> i ^ m for a power of two m < 256 and n a multiple of 256: it swaps whole chains that the tree adds to one
    another at stride m, and fp64 addition commutes, so the contract gives the same loss."""
    assert n % SL_THREADS == 0 and m in (1, 2, 4, 8, 16, 32, 64, 128)
    return np.arange(n) ^ m
