"""No-GPU checks of the parameter update (csrc/f110_adam.h): what f110_adam_validate, f110_adam_step and f110_soft_update refuse on
the host, the mirrored constants and struct sizes, what SacAdam and soft_update refuse before they touch a device, the checker of
tests/optim_cases.py against torch.optim.Adam(foreach=False) and fp64 Adam over 50 steps, and its target rule against torch.lerp."""
import ctypes as C
import math

import numpy as np
import pytest

import optim_cases as oc

from red_gym_amd import _lib, build


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _lib.load()


def _cfg(beta1=0.9, beta2=0.999, eps=1e-8, tau=0.005, with_target=1, advance=1):
    c = _lib.AdamConfig()
    c.beta1, c.beta2, c.eps, c.tau, c.with_target, c.advance = beta1, beta2, eps, tau, with_target, advance
    return c


def _table(count=2, **holes):
    """count tensors of 8 elements at distinct non-null 16-byte aligned addresses (the checks come before any launch); holes: field
    -> value for tensor 1."""
    t = (_lib.AdamTensor * max(count, 1))()
    for i in range(count):
        t[i].p, t[i].g, t[i].m, t[i].v, t[i].target = (4096 * (5 * i + k + 1) for k in range(5))
        t[i].n = 8
    for k, val in holes.items():
        setattr(t[1], k, val)
    return t


def test_mirrored_constants_and_struct_sizes(lib):
    from red_gym_amd import optim
    assert (_lib.F110_ADAM_CHUNK, _lib.F110_ADAM_MAX_TENSORS) == (oc.CHUNK, oc.MAX_TENSORS) == (optim.CHUNK, optim.MAX_TENSORS)
    assert lib.f110_adam_state_bytes() == oc.STATE_BYTES == _lib.F110_ADAM_STATE_BYTES
    assert oc.CHUNK % (4 * oc.THREADS) == 0                                  # a chunk is whole float4 rounds of a workgroup
    assert oc.MAX_TENSORS * C.sizeof(_lib.AdamTensor) + oc.MAX_TENSORS * 4 + 24 + 8 <= 4096     # the table and the state pointer fit a kernel's arguments
    assert oc.MAX_TENSORS >= 12                                              # SAL's actor in one launch
    src = open(build.HEADERS[-1].replace('include/f110_hip.h', 'red_gym_amd/csrc/f110_adam.h')).read()
    assert 'AD_THREADS = %d' % oc.THREADS in src and '__shared__' not in src and 'atomic' not in src.split('#pragma once')[1]


def test_config_refusals(lib):
    assert lib.f110_adam_validate(None) == _lib.E_INVALID and b'null config' in lib.f110_last_error()
    assert lib.f110_adam_validate(C.byref(_cfg())) == 0
    assert lib.f110_adam_validate(C.byref(_cfg(beta1=0.0, beta2=0.0, tau=0.0))) == 0 and lib.f110_adam_validate(C.byref(_cfg(tau=1.0))) == 0
    nan, inf = float('nan'), float('inf')
    for kw, word in ([(dict(beta1=b), 'beta1') for b in (-0.1, 1.0, nan)] + [(dict(beta2=b), 'beta2') for b in (-1e-9, 1.0, 1.5, nan)]
                     + [(dict(eps=e), 'eps') for e in (0.0, -1e-8, inf, nan)] + [(dict(tau=t), 'tau') for t in (-0.1, 1.1, inf, nan)]):
        assert lib.f110_adam_validate(C.byref(_cfg(**kw))) == _lib.E_INVALID, kw
        assert word.encode() in lib.f110_last_error(), (kw, lib.f110_last_error())
        assert lib.f110_adam_step(C.byref(_cfg(**kw)), _table(), 2, 4096, 3e-4, None) == _lib.E_INVALID and word.encode() in lib.f110_last_error()
    assert lib.f110_adam_validate(C.byref(_cfg(tau=7.0, with_target=0))) == 0      # tau is read only with a target


def test_bad_calls_are_refused_before_any_launch(lib):
    """F110_E_INVALID on the host, with a word that names the culprit: no device is touched (this runs without one)."""
    state = 4096 * 100
    step = lambda table, n=2, cfg=None, st=state, lr=3e-4: lib.f110_adam_step(C.byref(cfg or _cfg()), table, n, st, lr, None)  # noqa: E731
    soft = lambda table, n=2, tau=0.005: lib.f110_soft_update(table, n, tau, None)  # noqa: E731

    def refused(rc, word):
        assert rc == _lib.E_INVALID, (rc, word)
        assert word.encode() in lib.f110_last_error(), (word, lib.f110_last_error())
    refused(lib.f110_adam_step(None, _table(), 2, state, 3e-4, None), 'null config')
    refused(step(None), 'null table')
    refused(soft(None), 'null table')
    refused(step(_table(), st=None), 'null state')
    for n in (-1, oc.MAX_TENSORS + 1):
        refused(step(_table(), n=n), 'n_tensors')
        refused(soft(_table(), n=n), 'n_tensors')
    for n in (-1, 2 ** 31 + 1):
        refused(step(_table(n=n)), 'tensor 1: n')
        refused(soft(_table(n=n)), 'tensor 1: n')
    for name in ('p', 'g', 'm', 'v', 'target'):
        refused(step(_table(**{name: None})), 'tensor 1: null ' + name)
    refused(soft(_table(p=None)), 'tensor 1: null p')
    refused(soft(_table(target=None)), 'tensor 1: null target')
    assert step(_table(target=None), cfg=_cfg(with_target=0)) != _lib.E_INVALID or b'null target' not in lib.f110_last_error()
    t = _table()
    t[1].target = t[1].p
    refused(step(t), 'target == p')
    refused(soft(t), 'target == p')
    for name in ('p', 'g', 'm', 'v', 'target'):
        for off in (1, 2, 3):
            refused(step(_table(**{name: 4096 * 50 + off})), 'tensor 1: a pointer is not 4-byte aligned')
    refused(soft(_table(p=4096 * 50 + 2)), 'not 4-byte aligned')
    refused(soft(_table(target=4096 * 50 + 1)), 'not 4-byte aligned')
    for lr in (float('inf'), float('nan')):
        refused(step(_table(), lr=lr), 'lr')
    for tau in (float('inf'), float('nan'), -0.5, 1.5):
        refused(soft(_table(), tau=tau), 'tau')
    # nothing to do is not an error; a null table with no tensors is none either
    t = _table(n=0, p=None, target=None)
    t[0].n = 0
    assert soft(None, n=0) == 0 and soft(t) == 0 and soft(_table(), n=0) == 0      # (empty tensors may have null pointers)
    # every pointer set and aligned, none of them device memory: refused on the host, by the check the policy head uses
    buf = np.zeros(64, np.float32)
    t = (_lib.AdamTensor * 1)()
    base = buf.ctypes.data
    t[0].p, t[0].g, t[0].m, t[0].v, t[0].target, t[0].n = base, base + 32, base + 64, base + 96, base + 128, 8
    st = np.zeros(4, np.int64)
    for rc in (lib.f110_adam_step(C.byref(_cfg()), t, 1, st.ctypes.data, 3e-4, None), lib.f110_soft_update(t, 1, 0.005, None)):
        assert rc in (_lib.E_INVALID, _lib.E_HIP), rc
        if rc == _lib.E_INVALID:
            assert b'not device memory' in lib.f110_last_error()
    assert not buf.any() and not st.any()


def test_python_refusals_need_no_device():
    import torch
    from red_gym_amd.optim import SacAdam, soft_update
    cpu = [torch.zeros(4)]
    with pytest.raises(ValueError, match='CPU'):
        SacAdam(cpu)
    with pytest.raises(ValueError, match='CPU'):
        soft_update(cpu, [torch.zeros(4)], 0.005)
    with pytest.raises(ValueError, match='float32'):
        SacAdam([torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(ValueError, match='2 targets for 1'):
        soft_update([torch.zeros(4), torch.zeros(4)], [torch.zeros(4)], 0.005)
    with pytest.raises(ValueError, match='shape'):
        soft_update([torch.zeros(5)], [torch.zeros(4)], 0.005)
    with pytest.raises(ValueError, match='not a tensor'):
        SacAdam([1.0])
    with pytest.raises(ValueError, match='one tensor'):
        SacAdam(torch.zeros(4))


def _fixed_case():
    """Parameters and 50 steps of gradients, the same on every side: zeros, magnitudes 1e-3 .. 1e3, and one tensor (the last, from p
    = 0) whose |g| = 1e-22 everywhere so that g * g is denormal."""
    rng = np.random.default_rng(16)
    sizes = [1, 5, 257, 1000]
    params = [oc.values(rng, n) for n in sizes] + [np.zeros(64, np.float32)]
    grads = []
    for k in range(50):
        gs = [oc.gradients(rng, n) for n in sizes]
        gs.append(np.where(rng.random(64) < 0.5, 1e-22, -1e-22).astype(np.float32))
        grads.append(gs)
    sq = grads[0][-1] * grads[0][-1]
    assert (sq > 0).all() and (sq < np.finfo(np.float32).tiny).all()          # denormal, and kept by NumPy
    assert any((g == 0).any() for g in grads[0][:-1])
    mags = np.abs(np.concatenate([g for g in grads[0][:-1]]))
    assert mags[mags > 1e-10].min() < 1e-2 and mags.max() > 1e2
    return params, grads


def test_checker_is_as_close_to_fp64_adam_as_torch_is():
    """50 steps.  Per element |checker - p64| <= 2 max|torch32 - p64| + 1 ulp32(p64), the maximum over the tensor: the checker and
    torch's fp32 Adam differ only in rounding order, so their errors against fp64 Adam are of one size, not equal."""
    import torch
    params, grads = _fixed_case()
    want = oc.adam64(params, grads)
    tp = [torch.tensor(p, requires_grad=True) for p in params]
    opt = torch.optim.Adam(tp, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, foreach=False)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = torch.tensor(g)
        opt.step()
    got, _, _, _, state = oc.run(params, grads)
    assert state['t'] == 50 and state['pow1'] == pytest.approx(0.9 ** 50, rel=1e-13) and state['pow2'] == pytest.approx(0.999 ** 50, rel=1e-13)
    for i in range(len(params)):
        e_torch = np.abs(tp[i].detach().numpy().astype(np.float64) - want[i])
        e_check = np.abs(got[i].astype(np.float64) - want[i])
        print('tensor %d (%d elements): max |torch32 - p64| %.3e, max |checker - p64| %.3e' % (i, params[i].size, e_torch.max(), e_check.max()))
        assert (e_check <= 2.0 * e_torch.max() + oc.ulp32(want[i])).all(), i
        assert not np.array_equal(got[i], params[i])
    assert (np.abs(got[-1]) > 0).all() and (np.abs(got[-1]) < 1e-12).all()    # the denormal tensor moved, by very little


def test_checker_target_rule_is_torch_lerp_within_one_ulp():
    """fmaf(tau, u, tp) against torch.lerp = tp + rn(tau u) (its form for a weight below 0.5) from the same u = rn(p - tp): the two differ
    by the one rounding of tau u, at most half an ulp of tau u before the last rounding.  So they are at most 1 ulp apart, the ulp being
    that of the result, or that of tau u where tp and tau u cancel and the result is the smaller of the two."""
    import torch
    rng = np.random.default_rng(5)
    for tau in (0.005, 0.3, 0.0):
        tp, p = oc.values(rng, 4099), oc.values(rng, 4099)
        p[:7] = tp[:7]
        got = oc.lerp(tp, p, tau)
        want = torch.lerp(torch.tensor(tp), torch.tensor(p), tau).numpy()
        tu = np.float64(np.float32(tau)) * (p - tp).astype(np.float64)
        ulp = np.maximum(oc.ulp32(want), oc.ulp32(tu))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print('tau %g: worst |checker - torch.lerp| %.3g ulp; %d of %d elements equal, at most %d ulp of the result apart' % (
            tau, float((err / ulp).max()), int((got == want).sum()), got.size, int(oc.ulps_apart(got, want).max())))
        assert (err <= ulp).all()
        assert np.array_equal(got[:7], tp[:7])
    assert np.array_equal(oc.lerp(tp, p, 0.0), tp)


def test_checker_state_is_one_multiplication_per_step():
    s = oc.new_state()
    assert oc.state_words(s).tolist()[0] == 0 and s['pow1'] == 1.0 and s['pow2'] == 1.0
    oc.advance(s)
    assert s['t'] == 1 and s['pow1'] == 0.9 and s['pow2'] == 0.999
    assert s['k2'] == np.float32(math.sqrt(1.0 - 0.999)) and s['a'] == np.float32(3e-4 / (1.0 - 0.9))
    oc.advance(s)
    assert s['pow1'] == 0.9 * 0.9 and s['pow2'] == 0.999 * 0.999
    r = oc.new_state(t=7)
    assert r['t'] == 7 and r['pow1'] == 0.9 ** 7 and r['pow2'] == 0.999 ** 7
