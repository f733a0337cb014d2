"""No-GPU checks of gradient clipping (csrc/f110_adam_clip.h): the checker of tests/clip_cases.py against math.fsum and against
torch.nn.utils.clip_grad_norm_ in fp64, its exact cases (coef == 1.0f, max_norm = inf, S = 0), the non-finite guard, the plan header
csrc/f110_adam_plan.h compiled for the host against the checker's chunk numbering and chain membership, the mirrored struct against
the C compiler, and what the three entry points and SacAdam refuse before they touch a device.

Bounds.  u = 2^-53, gamma_k = k u / (1 - k u).  Every term g_j^2 is exact in fp64 and non-negative, so a sum that reaches its result
through at most k additions on any path from a term lies within gamma_k * S_exact of the exact sum S_exact (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2: without cancellation the relative error of any summation order is bounded by gamma of
its longest path).  The longest path is a chunk chain (at most 16 additions, the first to 0.0), the 8 levels of the tree, a chain of
the step sum (ceil(chunks / 256) additions) and 8 levels again.  math.fsum returns S_exact rounded once: within u * S_exact."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import clip_cases as cc
import host_build
import optim_cases as oc

U64 = 2.0 ** -53


def _gamma(k):
    return k * U64 / (1.0 - k * U64)


def _path(sizes):
    chunks = sum((n + cc.CHUNK - 1) // cc.CHUNK for n in sizes)
    longest = min(max(sizes), cc.CHUNK) if sizes else 0
    chain = min(16, 4 * ((longest + 4 * cc.THREADS - 1) // (4 * cc.THREADS)))
    return chain + 8 + (chunks + cc.THREADS - 1) // cc.THREADS + 8


_cache = {}


def _cases():
    """name -> (sizes, gradients): computed once, left unchanged."""
    if not _cache:
        rng = np.random.default_rng(29)
        for name, sizes in (('sizes', oc.SIZES), ('big', [cc.BIG]), ('big_257', [cc.BIG_257]), ('many', cc.MANY), ('critic_like', [512, 16 * 64, 3 * cc.CHUNK + 17, 1])):
            gs = [oc.gradients(rng, n) for n in sizes]
            for g in gs:
                g.setflags(write=False)
            _cache[name] = (sizes, gs)
    return _cache


@pytest.mark.parametrize('name', ['sizes', 'big', 'big_257', 'many', 'critic_like'])
def test_sum_against_fsum(name):
    sizes, gs = _cases()[name]
    S = cc.step_sum(cc.partials(gs))
    exact = math.fsum(float(x) * float(x) for g in gs for x in g.astype(np.float64))      # each product is exact
    k = _path(sizes)
    bound = (_gamma(k) + U64) * exact / (1.0 - U64)
    print('%s: S %r, fsum %r, |diff| %.3e, bound %.3e (k = %d)' % (name, float(S), exact, abs(float(S) - exact), bound, k))
    assert abs(float(S) - exact) <= bound
    assert len(cc.partials(gs)) == cc.chunk_numbers(sizes)[1]


@pytest.mark.parametrize('name', ['sizes', 'critic_like', 'many'])
def test_coefficient_and_clipped_gradients_against_torch_fp64(name):
    """torch.nn.utils.clip_grad_norm_ on fp64 copies.  coef: float(c) is within 2^-24 of c; c = max_norm / (norm + 1e-6) carries the
    relative error of norm (half that of S: gamma_k / 2, and u for the root), u for the addition and u for the division; torch's fp64
    norm adds the n squares in an order of its own, within gamma_n.  Every clipped gradient g * coef is one fp32 multiplication: within
    one ulp32 (in fact half) of the fp64 product double(g) * double(coef).  Against what torch leaves in its fp64 .grad, g64 * coef64,
    one ulp32 cannot hold for an fp32 coefficient: coef's own relative error of up to 2^-24 is up to one ulp32 of a product with a
    mantissa near 2, and the multiplication's rounding adds half an ulp (measured here: up to 1.1 ulp32).  So that comparison takes
    the derived bound: half an ulp32 of the result plus |g64 * coef64| times coef's relative slack."""
    import torch
    sizes, gs = _cases()[name]
    n = sum(sizes)
    S = cc.step_sum(cc.partials(gs))
    norm = float(np.sqrt(S))
    for max_norm in (norm / 3.0, norm * 0.999, 1e-3, norm * 2.0):
        got = cc.clip(S, max_norm)
        ps = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in gs]
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g.astype(np.float64))
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        coef64 = min(1.0, max_norm / (total + 1e-6))
        slack = coef64 * (2.0 ** -24 + _gamma(_path(sizes)) + _gamma(n) + 4.0 * U64)
        print('%s max_norm %.6g: norm %r (torch %r), coef %r (fp64 %r), |diff| %.3e, bound %.3e' % (
            name, max_norm, norm, total, float(got['coef']), coef64, abs(float(got['coef']) - coef64), slack))
        assert abs(float(got['coef']) - coef64) <= slack
        assert (float(got['coef']) == 1.0) == (max_norm / (norm + 1e-6) >= 1.0)
        worst, worst_torch = 0.0, 0.0
        for p, g in zip(ps, gs):
            theirs = p.grad.numpy()
            mine = (g * got['coef']).astype(np.float64)
            assert (g * got['coef']).dtype == np.float32
            if g.size:
                product = g.astype(np.float64) * np.float64(got['coef'])          # the fp64 product of the two fp32 operands
                worst = max(worst, float((np.abs(mine - product) / oc.ulp32(product)).max()))
                assert (np.abs(mine - product) <= oc.ulp32(product)).all()
                worst_torch = max(worst_torch, float((np.abs(mine - theirs) / oc.ulp32(theirs)).max()))
                assert (np.abs(mine - theirs) <= 0.5 * oc.ulp32(mine) + np.abs(theirs) * slack / coef64).all()
        print('    worst |g * coef - fp64 product| = %.3f ulp32; against torch\'s fp64 .grad %.3f ulp32' % (worst, worst_torch))


def test_exact_cases():
    _, gs = _cases()['sizes']
    S = cc.step_sum(cc.partials(gs))
    norm = np.sqrt(S)
    one = np.float32(1.0)
    for max_norm in (float(norm) + 1e-6 + 1e-3, float(norm) * 2, 1e30, cc.INF):          # every case with c >= 1
        got = cc.clip(S, max_norm)
        assert np.float64(max_norm) / (norm + np.float64(1e-6)) >= 1.0
        assert got['coef'].dtype == np.float32 and got['coef'].view(np.uint32) == one.view(np.uint32) and got['steps_clipped'] == 0
    for huge in (1e300, np.finfo(np.float64).max):                                        # max_norm = inf: coef == 1.0f at any norm
        got = cc.clip(huge, cc.INF)
        assert got['coef'] == one and not got['skip'] and got['steps_clipped'] == 0 and got['norm'] == np.sqrt(np.float64(huge))
    # c just below 1 rounds to 1.0f: not counted as clipped (the decision is taken after rounding)
    got = cc.clip(np.float64(1.0), 1.0)
    assert np.float64(1.0) / (np.float64(1.0) + np.float64(1e-6)) < 1.0 and got['coef'] < one and got['steps_clipped'] == 1
    got = cc.clip(np.float64(1.0), 1.0 + 1e-6 - 1e-9)
    assert got['coef'] == one and got['steps_clipped'] == 0
    # S = 0: norm 0, coef 1.0f, no skip (max_norm / 1e-6 >= 1 for every max_norm >= 1e-6; below that the zero gradient is scaled: still zero)
    zeros = [np.zeros(n, np.float32) for n in (5, cc.CHUNK + 1)]
    zeros[0][1] = -0.0
    got = cc.clip(cc.step_sum(cc.partials(zeros)), 1.0)
    assert cc.clip_words(got).tolist() == cc.clip_words(dict(cc.new_clip(), coef=one)).tolist() and got['norm'] == 0.0 and not got['skip']
    assert cc.step_sum(cc.partials([])) == 0.0 and cc.partials([None, np.zeros(0, np.float32)]).size == 0
    # with coef == 1.0f the run is optim_cases.run, bit for bit
    rng = np.random.default_rng(3)
    sizes = [5, 257, cc.CHUNK + 1]
    p0, t0 = [oc.values(rng, n) for n in sizes], [oc.values(rng, n) for n in sizes]
    grads = [[oc.gradients(rng, n) for n in sizes] for _ in range(3)]
    want = oc.run(p0, grads, t0)
    for max_norm in (cc.FAR_ABOVE, cc.INF):
        got = cc.run(p0, grads, max_norm, t0)
        for a, b in zip(got[:4], want[:4]):
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
        assert np.array_equal(oc.state_words(got[4]), oc.state_words(want[4])) and got[5]['steps_clipped'] == 0
    low = cc.run(p0, grads, cc.FAR_BELOW, t0)
    assert low[5]['steps_clipped'] == 3 and low[5]['coef'] < one and not np.array_equal(low[0][1], want[0][1])


@pytest.mark.parametrize('bad', ['inf', '-inf', 'nan', 'both'])
def test_a_non_finite_gradient_skips_the_step(bad):
    """One inf, one -inf, one NaN, or both kinds, anywhere: a skip.  On a skip every word of params, moments and state is unchanged,
    the target equals optim_cases.lerp, steps_skipped goes up by one; the next finite step continues from the unskipped t."""
    rng = np.random.default_rng(11)
    sizes = [5, 257, 2 * cc.CHUNK + 3]
    p0, t0 = [oc.values(rng, n) for n in sizes], [oc.values(rng, n) for n in sizes]
    grads = [[oc.gradients(rng, n) for n in sizes] for _ in range(3)]
    first = cc.run(p0, grads[:1], 1.0, t0)
    places = [(0, 0), (1, 256), (2, 2 * cc.CHUNK + 2), (2, cc.CHUNK - 1)]
    for i, j in places:
        poisoned = [g.copy() for g in grads[1]]
        poisoned[i][j] = {'inf': np.inf, '-inf': -np.inf, 'nan': np.nan, 'both': np.nan}[bad]
        if bad == 'both':
            poisoned[(i + 1) % 3][0] = np.inf
        for max_norm in (1.0, cc.INF):
            start = cc.run(p0, grads[:1], max_norm, t0)
            ps, ms, vs, ts, state, cs, last = cc.run(start[0], [poisoned], max_norm, start[3], start[4], (start[1], start[2]), start[5])
            assert cs['skip'] == 1 and cs['steps_skipped'] == 1 and cs['steps_clipped'] == start[5]['steps_clipped']
            assert cs['coef'] == np.float32(1.0) and np.isposinf(cs['sumsq']) and np.isposinf(cs['norm'])
            assert not np.isfinite(last).all()
            for got, was in ((ps, start[0]), (ms, start[1]), (vs, start[2])):
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, was))
            assert np.array_equal(oc.state_words(state), oc.state_words(start[4])) and state['t'] == 1
            assert all(np.array_equal(ts[k], oc.lerp(start[3][k], start[0][k])) for k in range(3))
            # the next finite step: what an unskipped run makes of it from the same params, moments and t = 1 (its targets moved once more)
            after = cc.run(ps, [grads[2]], max_norm, ts, state, (ms, vs), cs)
            want = cc.run(start[0], [grads[2]], max_norm, ts, start[4], (start[1], start[2]), start[5])
            assert after[4]['t'] == 2 and after[5]['skip'] == 0 and after[5]['steps_skipped'] == 1
            for a, b in zip(after[:4], want[:4]):
                assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    assert first[5]['steps_skipped'] == 0


# ---------------------------------------------------------------- the plan header, compiled for the host
SHIM = host_build.FAIL_SHIM + r'''
#include "f110_adam_plan.h"
using namespace f110;
typedef long long ll;
extern "C" ll shim_constant(int which) { const ll v[] = {AC_THREADS, AC_CHUNK, AC_QUADS, (ll)sizeof(f110_adam_clip_state), F110_ADAM_MAX_TENSORS}; return v[which]; }
extern "C" ll shim_chunks(ll n) { return adam_chunks(n); }
extern "C" int shim_chain(unsigned j) { return adam_clip_chain(j); }
extern "C" unsigned shim_element(int l, int k) { return adam_clip_element(l, k); }
extern "C" int shim_partial_chain(ll c) { return adam_clip_partial_chain(c); }
extern "C" ll shim_number(const ll *n, int count, ll base, ll *first)
{
    static_assert(sizeof(ll) == sizeof(int64_t), "");
    return adam_clip_number((const int64_t *)n, count, base, (int64_t *)first);
}
extern "C" int shim_gradnorm_check(ll chunk_base, ll partials, ll partials_len, ll chunks)
{
    return adam_gradnorm_check("gradnorm", chunk_base, (const double *)(uintptr_t)partials, partials_len, chunks);
}
extern "C" int shim_clip_check(ll partials, ll n_chunks, double max_norm, ll clip)
{
    return adam_clip_check("clip", (const double *)(uintptr_t)partials, n_chunks, max_norm, (const f110_adam_clip_state *)(uintptr_t)clip);
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('adam_plan'), 'adamplan', SHIM)
    ll = C.c_longlong
    L.shim_constant.restype = L.shim_chunks.restype = L.shim_number.restype = ll
    L.shim_message.restype = C.c_char_p
    L.shim_chunks.argtypes = [ll]
    L.shim_chain.argtypes = [C.c_uint]
    L.shim_element.argtypes = [C.c_int, C.c_int]
    L.shim_element.restype = C.c_uint
    L.shim_partial_chain.argtypes = [ll]
    L.shim_number.argtypes = [C.POINTER(ll), C.c_int, ll, C.POINTER(ll)]
    L.shim_gradnorm_check.argtypes = [ll, ll, ll, ll]
    L.shim_clip_check.argtypes = [ll, ll, C.c_double, ll]
    return L


def _numbers(shim, sizes):
    """The header's numbering of a step's tensors, call by call of at most MAX_TENSORS -> (first chunk of every tensor, chunks)."""
    first, base = [], 0
    for at in range(0, len(sizes), cc.MAX_TENSORS):
        part = sizes[at:at + cc.MAX_TENSORS]
        n, out = (C.c_longlong * len(part))(*part), (C.c_longlong * len(part))()
        chunks = shim.shim_number(n, len(part), base, out)
        first += list(out)
        base += chunks
    return first, base


def test_plan_header_numbers_chunks_and_chains_as_the_checker(shim):
    assert [shim.shim_constant(k) for k in range(5)] == [cc.THREADS, cc.CHUNK, cc.CHUNK // (4 * cc.THREADS), cc.CLIP_STATE_BYTES, cc.MAX_TENSORS]
    for sizes in (oc.SIZES, [cc.BIG], [cc.BIG_257], cc.MANY, oc.MISALIGNED_SIZES):
        assert _numbers(shim, sizes) == cc.chunk_numbers(sizes), sizes
        assert all(shim.shim_chunks(n) == (n + cc.CHUNK - 1) // cc.CHUNK for n in sizes)
    assert cc.chunk_numbers([cc.BIG_257])[1] == 257 and cc.chunk_numbers([cc.BIG])[1] == 258 and len(cc.MANY) == cc.MAX_TENSORS + 2 and cc.chunk_numbers(cc.MANY) == (list(range(65)) + [65], 67)
    # chain membership: all 4 096 positions, by element index
    j = np.arange(cc.CHUNK)
    chains = np.array([shim.shim_chain(int(x)) for x in j])
    assert np.array_equal(chains, cc.chain_of(j)) and np.array_equal(np.bincount(chains), np.full(cc.THREADS, 16))
    # a chain's elements in the order it adds them: ascending j, every position exactly once, and the checker's [round, chain, e] layout
    order = np.array([[shim.shim_element(l, k) for k in range(16)] for l in range(cc.THREADS)])
    assert (np.diff(order, axis=1) > 0).all() and np.array_equal(np.sort(order.reshape(-1)), j)
    assert all((cc.chain_of(order[l]) == l).all() for l in range(cc.THREADS))
    layout = j.reshape(cc.CHUNK // (4 * cc.THREADS), cc.THREADS, 4)
    assert np.array_equal(order, layout.transpose(1, 0, 2).reshape(cc.THREADS, 16))
    # the step sum: partial c goes to chain c mod 256; with 257 chunks chain 0 adds two partials and chain 1 one
    assert [shim.shim_partial_chain(c) for c in (0, 1, 255, 256, 257, 2 ** 40 + 3)] == [0, 1, 255, 0, 1, 3]
    counts = np.bincount([shim.shim_partial_chain(c) for c in range(257)], minlength=cc.THREADS)
    assert counts[0] == 2 and (counts[1:] == 1).all()


NAN, INF = float('nan'), float('inf')
PARTIALS, CLIP = 4096 * 100, 4096 * 200
# (chunk_base, partials, partials_len, chunks) -> the word that names the culprit
GRADNORM_REFUSED = [
    ((0, 0, 8, 2), 'null partials'),
    ((0, PARTIALS + 4, 8, 2), 'partials is not 8-byte aligned'),
    ((-1, PARTIALS, 8, 2), 'chunk_base -1'),
    ((0, PARTIALS, -1, 0), 'partials_len'),
    ((0, PARTIALS, 1, 2), 'do not fit'),
    ((7, PARTIALS, 8, 2), 'do not fit'),
    ((9, PARTIALS, 8, 0), 'do not fit'),
    ((2 ** 62, PARTIALS, 2 ** 62 + 1, 2), 'do not fit'),
]
# (partials, n_chunks, max_norm, clip)
CLIP_REFUSED = [
    ((0, 2, 1.0, CLIP), 'null partials'),
    ((PARTIALS, 2, 1.0, 0), 'null clip'),
    ((PARTIALS + 4, 2, 1.0, CLIP), 'partials is not 8-byte aligned'),
    ((PARTIALS, 2, 1.0, CLIP + 4), 'clip is not 8-byte aligned'),
    ((PARTIALS, -1, 1.0, CLIP), 'n_chunks -1'),
    ((PARTIALS, 2, NAN, CLIP), 'max_norm'),
    ((PARTIALS, 2, 0.0, CLIP), 'max_norm'),
    ((PARTIALS, 2, -1.0, CLIP), 'max_norm'),
    ((PARTIALS, 2, -INF, CLIP), 'max_norm'),
]


def test_plan_header_refuses(shim):
    from red_gym_amd import _lib
    for args, word in GRADNORM_REFUSED:
        assert shim.shim_gradnorm_check(*args) == _lib.E_INVALID and word.encode() in shim.shim_message(), (args, shim.shim_message())
    for args, word in CLIP_REFUSED:
        assert shim.shim_clip_check(*args) == _lib.E_INVALID and word.encode() in shim.shim_message(), (args, shim.shim_message())
    assert shim.shim_gradnorm_check(6, PARTIALS, 8, 2) == 0 and shim.shim_gradnorm_check(8, PARTIALS + 8, 8, 0) == 0 and shim.shim_gradnorm_check(0, PARTIALS, 0, -1) == 0
    assert shim.shim_clip_check(PARTIALS, 0, INF, CLIP) == 0 and shim.shim_clip_check(PARTIALS + 8, 2 ** 40, 1e-300, CLIP + 8) == 0


def _table(count=2, **holes):
    from red_gym_amd import _lib
    t = (_lib.AdamTensor * max(count, 1))()
    for i in range(count):
        t[i].p, t[i].g, t[i].m, t[i].v, t[i].target = (4096 * (5 * i + k + 1) for k in range(5))
        t[i].n = 8
    for k, val in holes.items():
        setattr(t[1], k, val)
    return t


def test_library_refuses_before_any_launch():
    """The shipped entry points, without a device: the same cases, the table's own, and a host pointer is no device memory."""
    from red_gym_amd import _lib
    lib = _lib.load()
    assert lib.f110_adam_clip_state_bytes() == cc.CLIP_STATE_BYTES == _lib.F110_ADAM_CLIP_STATE_BYTES == C.sizeof(_lib.AdamClipState)

    def refused(rc, word):
        assert rc == _lib.E_INVALID, (rc, word)
        assert word.encode() in lib.f110_last_error(), (word, lib.f110_last_error())
    for (base, partials, length, chunks), word in GRADNORM_REFUSED:
        if chunks in (0, 2):
            refused(lib.f110_adam_gradnorm(_table(2 if chunks else 0), 2 if chunks else 0, base, partials or None, length, None), word)
    for (partials, n_chunks, max_norm, clip), word in CLIP_REFUSED:
        refused(lib.f110_adam_clip(partials or None, n_chunks, max_norm, clip or None, None), word)
    norm = lambda table, n=2: lib.f110_adam_gradnorm(table, n, 0, PARTIALS, 1 << 19, None)  # noqa: E731
    refused(norm(None), 'null table')
    for n in (-1, cc.MAX_TENSORS + 1):
        refused(norm(_table(), n), 'n_tensors')
    for n in (-1, 2 ** 31 + 1):
        refused(norm(_table(n=n)), 'tensor 1: n')
    refused(norm(_table(g=None)), 'tensor 1: null g')
    for off in (1, 2, 3):
        refused(norm(_table(g=4096 * 50 + off)), 'tensor 1: g is not 4-byte aligned')
    refused(norm(_table(n=2 ** 31)), 'do not fit')                             # 2^19 chunks and one more behind a partials_len of 2^19
    # it reads g and n only: null p, m, v and target are none of its business (what is left to refuse is the host pointer)
    rc = norm(_table(p=None, m=None, v=None, target=None))
    assert rc in (_lib.E_INVALID, _lib.E_HIP) and (rc == _lib.E_HIP or b'not device memory' in lib.f110_last_error())
    # the clipped step: f110_adam_step's refusals under its own name, and the clip pointer's
    cfg = _lib.AdamConfig()
    cfg.beta1, cfg.beta2, cfg.eps, cfg.tau, cfg.with_target, cfg.advance = 0.9, 0.999, 1e-8, 0.005, 1, 1
    step = lambda table, clip=CLIP, lr=3e-4, state=4096 * 300: lib.f110_adam_step_clipped(C.byref(cfg), table, 2, state, clip, lr, None)  # noqa: E731
    refused(step(_table(), clip=None), 'f110_adam_step_clipped: null clip')
    refused(step(_table(), clip=CLIP + 4), 'clip is not 8-byte aligned')
    refused(step(_table(), state=None), 'null state')
    refused(step(_table(), lr=NAN), 'lr')
    refused(step(_table(m=None)), 'tensor 1: null m')
    refused(lib.f110_adam_step_clipped(None, _table(), 2, 4096 * 300, CLIP, 3e-4, None), 'null config')
    # every pointer set and aligned, none of them device memory
    buf, state, clip, partials = np.zeros(64, np.float32), np.zeros(4, np.int64), np.zeros(8, np.int64), np.zeros(4, np.float64)
    t = (_lib.AdamTensor * 1)()
    b = buf.ctypes.data
    t[0].p, t[0].g, t[0].m, t[0].v, t[0].target, t[0].n = b, b + 32, b + 64, b + 96, b + 128, 8
    for rc in (lib.f110_adam_gradnorm(t, 1, 0, partials.ctypes.data, 4, None), lib.f110_adam_clip(partials.ctypes.data, 1, 1.0, clip.ctypes.data, None),
               lib.f110_adam_step_clipped(C.byref(cfg), t, 1, state.ctypes.data, clip.ctypes.data, 3e-4, None)):
        assert rc in (_lib.E_INVALID, _lib.E_HIP), rc
        if rc == _lib.E_INVALID:
            assert b'not device memory' in lib.f110_last_error()
    assert not buf.any() and not state.any() and not clip.any() and not partials.any()


def test_mirrored_struct_against_the_compiler(tmp_path):
    """_lib.ADAM_CLIP_STRUCTS (a tagged typedef of the header): size and every offset as strict C99 sees them, and the field names
    and order as the header spells them."""
    from red_gym_amd import _lib
    name, cls = 'f110_adam_clip_state', _lib.AdamClipState
    assert _lib.ADAM_CLIP_STRUCTS == {name: cls}
    fields = [f for f, _ in cls._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "f110_hip.h"', 'int main(void)', '{',
             '    printf("%s %%d\\n", (int)sizeof(%s));' % (name, name), '    printf("bytes %d\\n", F110_ADAM_CLIP_STATE_BYTES);']
    lines += ['    printf("%s %%d\\n", (int)offsetof(%s, %s));' % (f, name, f) for f in fields]
    got = dict(line.split() for line in host_build.run_c(tmp_path, 'layout', '\n'.join(lines + ['    return 0;', '}', ''])).splitlines())
    assert int(got[name]) == int(got['bytes']) == C.sizeof(cls) == cc.CLIP_STATE_BYTES
    assert all(int(got[f]) == getattr(cls, f).offset for f in fields)
    text = re.sub(r'/\*.*?\*/', ' ', open(host_build.ROOT + '/include/f110_hip.h').read(), flags=re.S)
    body = re.search(r'typedef struct %s\s*\{(.*?)\}\s*%s\s*;' % (name, name), text, flags=re.S).group(1)
    declared = [re.sub(r'\[.*\]', '', f).strip() for decl in re.findall(r'\w+\s+([^;]+);', body) for f in decl.split(',')]
    assert declared == fields, declared
    # the checker's words are the struct's
    c = dict(sumsq=np.float64(2.25), norm=np.float64(1.5), coef=np.float32(0.25), skip=1, steps_clipped=3, steps_skipped=4)
    s = cls.from_buffer_copy(cc.clip_words(c).tobytes())
    assert (s.sumsq, s.norm, s.coef, s.skip, s.steps_clipped, s.steps_skipped, list(s.reserved)) == (2.25, 1.5, 0.25, 1, 3, 4, [0, 0, 0])


def test_python_refusals_need_no_device():
    import torch
    from red_gym_amd.optim import SacAdam
    with pytest.raises(ValueError, match='CPU'):
        SacAdam([torch.zeros(4)], max_grad_norm=1.0)
    src = open(host_build.CSRC + '/f110_adam_clip.h').read().split('#pragma once')[1]
    assert 'atomic' not in src and src.count('__shared__ double s[AC_THREADS]') == 2 and src.count('__shared__') == 2     # 2 KiB: one tree each
