"""The checker of the two SAC losses (tests/sacloss_cases.py) on the CPU: its sums against math.fsum, its gradients against torch's
autograd on the CPU for the framework's own expressions, and the launch plan header (red_gym_amd/csrc/f110_sacloss_plan.h) compiled for
the host against the checker's restatement, as tests/test_launch_plans_cpu.py does for the other policy kernels.

Bounds.  The loss: the checker adds n fp64 terms in some order, so it lies within n * 2^-53 * sum|t_i| of the exact sum of those terms
(math.fsum); that is far below half an fp32 ulp of the loss unless the terms cancel, and the rounding to fp32 adds at most half an ulp:
one fp32 ulp of the loss in all, as long as sum|t_i| <= 2^20 |sum t_i| (asserted: the cases do not cancel).  The gradients: for n a power
of two 2 / n, 1 / n and alpha / n are exact scalings, every route rounds the same one number, and `==` is required.  For other n the
checker's (q - tv) * float(2 / n) and the framework's 2 (q - tv) / n each round the factor and the product once: 4 * 2^-24 relative (and
one denormal step) covers both; alpha / n against alpha * (1 / n) likewise in the dtype of log_prob."""
import ctypes
import math

import numpy as np
import pytest

import host_build
import sacloss_cases as sl

ALPHAS = (0.2, 1.0, 0.013)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize('n', sl.CPU_N)
def test_sums_against_fsum(n):
    c = sl.case(n)
    loss, _, _ = sl.critic(c['q1'], c['q2'], c['tv'])
    for k, q in enumerate((c['q1'], c['q2'])):
        t = sl.critic_terms(q, c['tv'])
        want = math.fsum(t.tolist()) / n
        assert abs(float(loss[k]) - want) <= _ulp32(want), (n, k, float(loss[k]), want)
    for dt in (np.float64, np.float32):
        c = sl.case(n, logp_dtype=dt)
        for alpha in ALPHAS:
            t = sl.actor_terms(c['logp'], c['qn'], alpha)
            exact, mass = math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())
            assert mass <= 2.0 ** 20 * abs(exact)
            got = float(sl.actor(c['logp'], c['qn'], alpha)[0][0])
            assert abs(got - exact / n) <= _ulp32(exact / n), (n, dt, alpha, got, exact / n)


def test_the_order_is_the_contracts():
    """Chains of i mod 256 and a tree: on terms chosen so that the order shows (2^53 and ones), the value is the contract's, and
    another order's is another."""
    t = np.ones(512)
    t[0] = 2.0 ** 53
    # chain 0 = (0 + 2^53) + 1 = 2^53 (the one is lost); every other chain = 2; the tree adds 255 chains of 2 to it pairwise
    assert sl.ordered_sum(t) == 2.0 ** 53 + 510.0 and float(np.sum(t[::-1].cumsum()[-1:])) != sl.ordered_sum(t)
    assert sl.ordered_sum(np.array([1.5])) == 1.5 and sl.ordered_sum(np.array([])) == 0.0
    n = 4096
    c = sl.case(n)
    base = sl.critic(c['q1'], c['q2'], c['tv'])[0]
    for m in (1, 4, 128):
        p = sl.butterfly(n, m)
        assert np.array_equal(sl.critic(c['q1'][p], c['q2'][p], c['tv'][p])[0], base)
    # an order that shows in the fp32 loss: a pair that cancels inside one chain, or across two chains that have absorbed their ones
    for n in (257, 4097):
        one, two = sl.cancelling(n, False), sl.cancelling(n, True)
        a, b = sl.actor(one['logp'], one['qn'], 1.0)[0], sl.actor(two['logp'], two['qn'], 1.0)[0]
        assert a[0] == np.float32(-(n - 2) / n) and a[0] != b[0], (n, a, b)


@pytest.mark.parametrize('n', sl.CPU_N)
def test_gradients_against_autograd(n):
    import torch
    import torch.nn.functional as F
    pow2 = n & (n - 1) == 0
    c = sl.case(n)
    _, g1, g2 = sl.critic(c['q1'], c['q2'], c['tv'])
    tv = torch.as_tensor(c['tv'])
    for q, g in ((c['q1'], g1), (c['q2'], g2)):
        x = torch.as_tensor(q).requires_grad_()
        F.mse_loss(x, tv).backward()
        want = x.grad.numpy()
        if pow2:
            assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), n
        else:
            assert (np.abs(g.astype(np.float64) - want) <= 4 * 2.0 ** -24 * np.abs(want) + 2.0 ** -149).all(), n
    for dt, eps in ((np.float64, 2.0 ** -53), (np.float32, 2.0 ** -24)):
        c = sl.case(n, logp_dtype=dt)
        for alpha in ALPHAS:
            _, glp, gqn = sl.actor(c['logp'], c['qn'], alpha)
            lp, qn = torch.as_tensor(c['logp']).requires_grad_(), torch.as_tensor(c['qn']).requires_grad_()
            (alpha * lp - qn).mean().backward()
            wlp, wqn = lp.grad.numpy(), qn.grad.numpy()
            assert glp.dtype == wlp.dtype == dt and gqn.dtype == wqn.dtype == np.float32
            if pow2:
                assert np.array_equal(glp, wlp) and np.array_equal(gqn, wqn), (n, dt, alpha)
            else:
                assert (np.abs(glp.astype(np.float64) - wlp) <= 4 * eps * np.abs(wlp)).all(), (n, dt, alpha)
                assert (np.abs(gqn.astype(np.float64) - wqn) <= 4 * 2.0 ** -24 * np.abs(wqn)).all(), (n, dt, alpha)


# ---------------------------------------------------------------- the launch plan header, compiled for the host
SHIM = r'''
#include "f110_sacloss_plan.h"
using namespace f110;
typedef long long ll;
extern "C" ll shim_constant(int which) { const ll v[] = {SL_THREADS, SL_MAX_GRID, SL_MAX_ROWS}; return v[which]; }
// o: grid x, y, z, block, lds, inst;  f: k2n, glp32, gqn;  d: glp64, alpha
extern "C" void shim_sacloss(ll n, int actor, int logp_fp64, double alpha, ll *o, float *f, double *d)
{
    const SaclossPlan p = sacloss_plan(n, actor != 0, logp_fp64 != 0, alpha);
    o[0] = p.l.gx; o[1] = p.l.gy; o[2] = p.l.gz; o[3] = p.l.block; o[4] = (ll)p.l.lds; o[5] = p.l.inst; o[6] = p.a.n; o[7] = p.a.logp_fp64;
    f[0] = p.a.k2n; f[1] = p.a.glp32; f[2] = p.a.gqn;
    d[0] = p.a.glp64; d[1] = p.a.alpha;
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('sacloss_plan'), 'saclossplan', SHIM)
    L.shim_constant.restype = ctypes.c_longlong
    L.shim_sacloss.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_longlong),
                               ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
    L.shim_sacloss.restype = None
    return L


def test_plan_header_against_the_checker(lib):
    assert [lib.shim_constant(k) for k in range(3)] == [sl.SL_THREADS, sl.SL_MAX_GRID, sl.MAX_ROWS]
    from red_gym_amd import sacloss
    assert sacloss.MAX_ROWS == sl.MAX_ROWS
    rng = np.random.default_rng(7)
    ns = sorted(set(sl.CPU_N) | {sl.SL_THREADS * sl.SL_MAX_GRID, sl.SL_THREADS * sl.SL_MAX_GRID + 1, sl.MAX_ROWS}
                | set(int(x) for x in rng.integers(1, sl.MAX_ROWS, 200)))
    grids = set()
    for n in ns:
        for kind in ((0, 0), (1, 0), (1, 1)):
            for alpha in ALPHAS:
                o, f, d = (ctypes.c_longlong * 8)(), (ctypes.c_float * 3)(), (ctypes.c_double * 2)()
                lib.shim_sacloss(n, kind[0], kind[1], alpha, o, f, d)
                w = sl.plan(n, bool(kind[0]), bool(kind[1]), alpha)
                assert list(o) == [w['grid'], 1, 1, w['block'], w['lds'], w['inst'], n, kind[1]], (n, kind)
                got = np.array(list(f), np.float32)
                want = np.array([w['k2n'], w['glp32'], w['gqn']], np.float32)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, alpha)
                assert (d[0], d[1]) == (float(w['glp64']), alpha), (n, alpha)
                assert 1 <= o[0] <= sl.SL_MAX_GRID and o[0] * sl.SL_THREADS >= min(n, sl.SL_THREADS * sl.SL_MAX_GRID)
                grids.add(int(o[0]))
    assert {1, 2, sl.SL_MAX_GRID} <= grids
    # the GPU cases reach one workgroup, a second one and a tail
    assert [sl.plan(n)['grid'] for n in sl.GPU_N] == [1, 1, 1, 1, 1, 2, 17]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from red_gym_amd import _lib
    lib = _lib.load()
    assert lib.f110_sac_critic_loss(None, None, None, 0, None, None, None, None) == _lib.E_INVALID and b'n=0' in lib.f110_last_error()
    assert lib.f110_sac_critic_loss(None, None, None, 4, None, None, None, None) == _lib.E_INVALID and b'null' in lib.f110_last_error()
    assert lib.f110_sac_actor_loss(None, 1, None, 0.2, sl.MAX_ROWS + 1, None, None, None, None) == _lib.E_INVALID
    with pytest.raises(ValueError):
        _lib.check(lib.f110_sac_actor_loss(None, 1, None, 0.2, 4, None, None, None, None))
    assert lib.f110_replay_sample(None, 0, None, 4, None, None, None, None, None, None, None, None) == _lib.E_INVALID
