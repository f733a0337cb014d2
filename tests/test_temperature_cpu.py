"""No-GPU checks of the learnt temperature (csrc/f110_temperature.h): the checker of tests/temperature_cases.py against torch's
autograd in fp64 and against fp64 Adam over 50 steps, the host checks of csrc/f110_temperature_plan.h compiled for the host, the
library's own refusals before any launch, the mirrored structs against the C compiler, the fresh state's bytes, and the number / [1]
tensor dispatch of td_target and actor_loss.

Bounds.  mean: the checker adds n fp64 terms in some order and divides once, so it lies within gamma_n * sum|t_i| / n of the exact
mean, gamma_n = n u / (1 - n u), u = 2^-53; grad = float(-mean) adds one fp32 rounding (half an ulp32; a whole one is allowed).  loss =
float(-(log_alpha * mean)): |log_alpha| times the mean's bound, one fp64 rounding of the product and the fp32 rounding."""
import ctypes as C
import math

import numpy as np
import pytest

import host_build
import sacloss_cases as sl
import temperature_cases as tc

U64 = 2.0 ** -53


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize('n', sl.CPU_N)
def test_loss_and_gradient_against_autograd(n):
    import torch
    for dt in (np.float64, np.float32):
        for name, logp in (('case', sl.case(n, logp_dtype=dt)['logp']), ('cancelling', tc.inputs(n, dt))):
            for state in (tc.new_state(), tc.resumed_state()):
                got = tc.step(logp, state)
                la = torch.tensor(float(state['log_alpha']), dtype=torch.float64, requires_grad=True)
                x = torch.as_tensor(logp.astype(np.float64))
                loss = -(la * (x + tc.TARGET_ENTROPY)).mean()
                loss.backward()
                _, t = tc.mean_of(logp, tc.TARGET_ENTROPY)
                gamma = n * U64 / (1.0 - n * U64)
                dmean = gamma * math.fsum(np.abs(t).tolist()) / n
                wg, wl = float(la.grad), float(loss)
                eg, el = abs(float(got['grad']) - wg), abs(float(got['loss']) - wl)
                bg = dmean + _ulp32(wg)
                bl = abs(float(state['log_alpha'])) * dmean + U64 * abs(wl) + _ulp32(wl)
                print('n %d %s %s: grad %r (autograd %r, |diff| %.3e, bound %.3e)  loss %r (autograd %r, |diff| %.3e, bound %.3e)'
                      % (n, np.dtype(dt).name, name, float(got['grad']), wg, eg, bg, float(got['loss']), wl, el, bl))
                assert eg <= bg and el <= bl, (n, dt, name)
                assert got['grad'].dtype == got['loss'].dtype == np.float32


def test_the_order_is_the_losses():
    """The +-2^60 pair of sacloss_cases.cancelling in one chain cancels before anything is added to it; in two chains it absorbs."""
    for n in (257, 4097):
        one, two = sl.cancelling(n, False)['logp'], sl.cancelling(n, True)['logp']
        a, b = tc.step(one, tc.new_state()), tc.step(two, tc.new_state())
        assert a['grad'] == np.float32(-((n - 2) * tc.TARGET_ENTROPY / n)) and a['grad'] != b['grad'], (n, a['grad'], b['grad'])


def test_checker_is_as_close_to_fp64_adam_as_torch_is():
    """50 steps on seeded batches.  The gradient -mean does not depend on log_alpha, so the checker, torch's fp32 Adam and fp64 Adam
    take the same fp32 gradients; the checker's distance from the fp64 run is at most torch-fp32's plus one ulp32."""
    import torch
    state = tc.new_state()
    grads = []
    for k in range(50):
        logp = tc.inputs(64 if k % 2 else 257, seed=100 + k)
        state = tc.step(logp, state)
        grads.append(float(state['grad']))
    start = float(tc.new_state()['log_alpha'])
    runs = {}
    for dt in (torch.float32, torch.float64):
        p = torch.tensor([start], dtype=dt, requires_grad=True)
        opt = torch.optim.Adam([p], lr=tc.LR, betas=tc.BETAS, eps=tc.EPS, foreach=False)
        for g in grads:
            p.grad = torch.tensor([g], dtype=dt)
            opt.step()
        runs[dt] = float(p.detach()[0])
    want = runs[torch.float64]
    e_check, e_torch = abs(float(state['log_alpha']) - want), abs(runs[torch.float32] - want)
    print('50 steps: |checker - p64| %.3e, |torch32 - p64| %.3e, ulp32 %.3e; log_alpha %r -> %r, alpha %r'
          % (e_check, e_torch, _ulp32(want), start, float(state['log_alpha']), state['alpha']))
    assert e_check <= e_torch + _ulp32(want)
    assert state['adam']['t'] == 50 and float(state['log_alpha']) != start
    assert state['alpha'] == float(np.exp(np.float64(state['log_alpha'])))


# ---------------------------------------------------------------- the plan header, compiled for the host
SHIM = host_build.FAIL_SHIM + r'''
#include "f110_temperature_plan.h"
using namespace f110;
typedef long long ll;
extern "C" ll shim_constant(int which) { const ll v[] = {TP_THREADS, TP_MAX_ROWS, (ll)sizeof(f110_temperature_state)}; return v[which]; }
extern "C" int shim_validate(const f110_temperature_config *cfg) { return temperature_check(cfg, "validate"); }
extern "C" int shim_step_check(const f110_temperature_config *cfg, ll logp, int logp_fp64, ll n, ll state, double lr)
{
    return temperature_step_check("step", cfg, (const void *)(uintptr_t)logp, logp_fp64, n, (const f110_temperature_state *)(uintptr_t)state, lr);
}
// o: grid x, y, z, block, lds, inst, n, logp_fp64;  f: c1, c2, b2, eps;  d: target_entropy, beta1, beta2, lr
extern "C" void shim_plan(const f110_temperature_config *cfg, ll n, int logp_fp64, double lr, ll *o, float *f, double *d)
{
    const TemperaturePlan p = temperature_plan(*cfg, n, logp_fp64 != 0, lr);
    o[0] = p.l.gx; o[1] = p.l.gy; o[2] = p.l.gz; o[3] = p.l.block; o[4] = (ll)p.l.lds; o[5] = p.l.inst; o[6] = p.a.n; o[7] = p.a.logp_fp64;
    f[0] = p.a.c1; f[1] = p.a.c2; f[2] = p.a.b2; f[3] = p.a.eps;
    d[0] = p.a.target_entropy; d[1] = p.a.beta1; d[2] = p.a.beta2; d[3] = p.a.lr;
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('temperature_plan'), 'temperatureplan', SHIM)
    L.shim_constant.restype = C.c_longlong
    L.shim_message.restype = C.c_char_p
    L.shim_validate.argtypes = [C.c_void_p]
    L.shim_step_check.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_longlong, C.c_longlong, C.c_double]
    L.shim_plan.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.POINTER(C.c_longlong), C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.shim_plan.restype = None
    return L


def _cfg(**kw):
    from red_gym_amd import _lib
    c = _lib.TemperatureConfig()
    c.beta1, c.beta2, c.eps, c.target_entropy = tc.BETAS[0], tc.BETAS[1], tc.EPS, tc.TARGET_ENTROPY
    for k, v in kw.items():
        setattr(c, k, v)
    return c


NAN, INF = float('nan'), float('inf')
# (cfg fields, logp, logp_fp64, n, state, lr) -> the word the message names the culprit with
LOGP, STATE = 4096 * 100, 4096 * 200
REFUSED = [
    (None, LOGP, 1, 4, STATE, tc.LR, 'null config'),
    ({}, 0, 1, 4, STATE, tc.LR, 'null logp'),
    ({}, LOGP, 1, 4, 0, tc.LR, 'null state'),
    ({}, LOGP, 1, 0, STATE, tc.LR, 'n=0'),
    ({}, LOGP, 1, -1, STATE, tc.LR, 'n=-1'),
    ({}, LOGP, 1, tc.MAX_ROWS + 1, STATE, tc.LR, 'n=%d' % (tc.MAX_ROWS + 1)),
    (dict(beta1=1.0), LOGP, 1, 4, STATE, tc.LR, 'beta1'),
    (dict(beta1=-0.1), LOGP, 1, 4, STATE, tc.LR, 'beta1'),
    (dict(beta1=NAN), LOGP, 1, 4, STATE, tc.LR, 'beta1'),
    (dict(beta2=1.0), LOGP, 1, 4, STATE, tc.LR, 'beta2'),
    (dict(beta2=-1e-9), LOGP, 1, 4, STATE, tc.LR, 'beta2'),
    (dict(eps=0.0), LOGP, 1, 4, STATE, tc.LR, 'eps'),
    (dict(eps=-1e-8), LOGP, 1, 4, STATE, tc.LR, 'eps'),
    (dict(eps=INF), LOGP, 1, 4, STATE, tc.LR, 'eps'),
    (dict(eps=NAN), LOGP, 1, 4, STATE, tc.LR, 'eps'),
    (dict(target_entropy=NAN), LOGP, 1, 4, STATE, tc.LR, 'target_entropy'),
    (dict(target_entropy=-INF), LOGP, 1, 4, STATE, tc.LR, 'target_entropy'),
    ({}, LOGP, 1, 4, STATE, NAN, 'lr'),
    ({}, LOGP, 1, 4, STATE, INF, 'lr'),
    ({}, LOGP + 4, 1, 4, STATE, tc.LR, 'logp is not aligned'),
    ({}, LOGP + 2, 0, 4, STATE, tc.LR, 'logp is not aligned'),
    ({}, LOGP, 1, 4, STATE + 4, tc.LR, 'state is not 8-byte aligned'),
]


def _try(check, message, case):
    from red_gym_amd import _lib
    fields, logp, f64, n, state, lr, word = case
    cfg = None if fields is None else C.byref(_cfg(**fields))
    assert check(cfg, logp, f64, n, state, lr) == _lib.E_INVALID, case
    assert word.encode() in message(), (case, message())


def test_plan_header_refuses_and_plans(shim):
    assert [shim.shim_constant(k) for k in range(3)] == [sl.SL_THREADS, tc.MAX_ROWS, tc.STATE_BYTES]
    for case in REFUSED:
        _try(shim.shim_step_check, shim.shim_message, case)
    ok = C.byref(_cfg())
    assert shim.shim_step_check(ok, LOGP + 4, 0, 1, STATE, tc.LR) == 0 and shim.shim_step_check(ok, LOGP, 1, tc.MAX_ROWS, STATE + 8, 0.0) == 0
    assert shim.shim_validate(C.byref(_cfg(beta1=0.0, beta2=0.0, target_entropy=0.0))) == 0 and shim.shim_validate(None) == -1
    for n in (1, 64, 4097, tc.MAX_ROWS):
        for f64 in (0, 1):
            o, f, d = (C.c_longlong * 8)(), (C.c_float * 4)(), (C.c_double * 4)()
            shim.shim_plan(ok, n, f64, 1e-3, o, f, d)
            assert list(o) == [1, 1, 1, sl.SL_THREADS, 0, f64, n, f64]              # one workgroup whatever n
            want = np.array([1.0 - tc.BETAS[0], 1.0 - tc.BETAS[1], tc.BETAS[1], tc.EPS]).astype(np.float32)
            assert np.array_equal(np.array(list(f), np.float32).view(np.uint32), want.view(np.uint32))
            assert list(d) == [tc.TARGET_ENTROPY, tc.BETAS[0], tc.BETAS[1], 1e-3]


def test_library_refuses_before_any_launch():
    """The shipped entry points, without a device: the same cases, then a host pointer is no device memory."""
    from red_gym_amd import _lib
    lib = _lib.load()
    step = lambda cfg, logp, f64, n, state, lr: lib.f110_temperature_step(cfg, logp or None, f64, n, state or None, lr, None)  # noqa: E731
    for case in REFUSED:
        _try(step, lib.f110_last_error, case)
    assert lib.f110_temperature_validate(C.byref(_cfg())) == 0 and lib.f110_temperature_validate(None) == _lib.E_INVALID
    assert lib.f110_temperature_state_bytes() == tc.STATE_BYTES == C.sizeof(_lib.TemperatureState)
    assert lib.f110_sac_actor_loss_alpha_dev(4096, 1, 4096, None, 4, 4096, None, None, None) == _lib.E_INVALID and b'null alpha' in lib.f110_last_error()
    assert lib.f110_sac_actor_loss_alpha_dev(4096, 1, 4096, 4096, 0, 4096, None, None, None) == _lib.E_INVALID and b'n=0' in lib.f110_last_error()
    with pytest.raises(ValueError):
        _lib.check(lib.f110_temperature_step(None, None, 1, 4, None, 3e-4, None))


def test_mirrored_structs_against_the_compiler(tmp_path):
    """_lib.TEMPERATURE_STRUCTS (the header's tagged typedefs, one nested by value): sizes and every offset as strict C99 sees them,
    and the field names and order as the header spells them."""
    import re
    from red_gym_amd import _lib
    paths = {'f110_adam_state': ['t', 'pow1', 'pow2', 'k2', 'a'],
             'f110_temperature_config': ['beta1', 'beta2', 'eps', 'target_entropy'],
             'f110_temperature_state': ['adam', 'adam.t', 'adam.pow1', 'adam.pow2', 'adam.k2', 'adam.a', 'alpha', 'log_alpha', 'm', 'v', 'grad', 'loss', 'reserved']}
    assert set(paths) == set(_lib.TEMPERATURE_STRUCTS)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "f110_hip.h"', 'int main(void)', '{']
    for name, fields in sorted(paths.items()):
        lines.append('    printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f) for f in fields]
    got = dict(line.split() for line in host_build.run_c(tmp_path, 'layout', '\n'.join(lines + ['    return 0;', '}', ''])).splitlines())

    def offset(cls, path):
        off = 0
        for part in path.split('.'):
            off, cls = off + getattr(cls, part).offset, dict(cls._fields_)[part]
        return off
    for name, fields in paths.items():
        cls = _lib.TEMPERATURE_STRUCTS[name]
        assert int(got[name]) == C.sizeof(cls), name
        assert [f for f in fields if '.' not in f] == [f for f, _ in cls._fields_], name
        for f in fields:
            assert int(got['%s.%s' % (name, f)]) == offset(cls, f), (name, f)
    assert C.sizeof(_lib.TemperatureState) == 64 and C.sizeof(_lib.AdamState) == _lib.F110_ADAM_STATE_BYTES
    # the header declares exactly these fields, in this order
    text = re.sub(r'/\*.*?\*/', ' ', open(host_build.ROOT + '/include/f110_hip.h').read(), flags=re.S)
    for name in ('f110_temperature_config', 'f110_temperature_state'):
        body = re.search(r'typedef struct %s\s*\{(.*?)\}\s*%s\s*;' % (name, name), text, flags=re.S).group(1)
        declared = [f.strip() for decl in re.findall(r'\w+\s+([^;]+);', body) for f in decl.split(',')]
        assert declared == [f for f, _ in _lib.TEMPERATURE_STRUCTS[name]._fields_], (name, declared)


def test_fresh_state_bytes_are_the_structs():
    from red_gym_amd import _lib
    from red_gym_amd.temperature import STATE_BYTES, fresh_state_bytes
    assert STATE_BYTES == tc.STATE_BYTES
    for alpha in (0.2, 1.0, 0.013, 7.5):
        raw = fresh_state_bytes(alpha)
        assert len(raw) == 64 and np.array_equal(np.frombuffer(raw, np.int64), tc.state_words(tc.new_state(alpha)))
        s = _lib.TemperatureState.from_buffer_copy(raw)
        assert (s.adam.t, s.adam.pow1, s.adam.pow2, s.adam.k2, s.adam.a) == (0, 1.0, 1.0, 0.0, 0.0)
        assert s.alpha == alpha and s.log_alpha == float(np.float32(math.log(alpha))) and (s.m, s.v, s.grad, s.loss, s.reserved) == (0, 0, 0, 0, 0)
    r = tc.resumed_state()
    raw = fresh_state_bytes(r['alpha'], tc.BETAS, 7, float(r['log_alpha']), float(r['m']), float(r['v']))
    assert np.array_equal(np.frombuffer(raw, np.int64), tc.state_words(r))


def test_alpha_dispatch_raises_before_any_library_call(monkeypatch):
    """A [2] tensor, fp32 and a CPU tensor (and a non-finite number) are refused by the check td_target and actor_loss share, which
    needs no device and runs before the library is loaded."""
    import torch
    from red_gym_amd import _lib, qhead, sacloss
    from red_gym_amd.temperature import alpha_argument

    def no_library():
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'load', no_library)
    assert qhead.alpha_argument is alpha_argument and sacloss.alpha_argument is alpha_argument
    dev = torch.device('cuda', 0)
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(1, dtype=torch.float32), torch.zeros(1, dtype=torch.float64),
                torch.zeros((1, 1), dtype=torch.float64), NAN, INF, None, '0.2'):
        with pytest.raises(ValueError):
            alpha_argument('actor_loss', bad, dev)
    assert alpha_argument('actor_loss', 0.2, dev) == (0.2, None) and alpha_argument('td_target', 1, dev) == (1.0, None)
    good = torch.zeros(1, dtype=torch.float64)
    assert alpha_argument('actor_loss', good, torch.device('cpu'))[0] is None
    with pytest.raises(ValueError, match='no CPU path'):
        from red_gym_amd.temperature import Temperature
        Temperature(device='cpu')
