"""The dense layer (red_gym_amd/dense.py, csrc/f110_dense.h) without a GPU: every refusal of f110_dense_validate and the workspace
formula through the library's host code; the NumPy checkers of tests/dense_cases.py against fp64 within bounds derived from the
number of roundings; the proof that the GPU shape table reaches every path, and that on every shape a wrong segmentation gives
other bits; the launch plan (csrc/f110_dense_plan.h) compiled for the host with a small shim and compared with paths(), on the table,
on a seeded sample and, for what every launch must satisfy, on every accepted configuration of the sample; and the reference pin:
the checkers against the recording of the reference's own Actor.fc1 (tests/golden/g23_dense.npz)."""
import ctypes

import numpy as np
import pytest

import dense_cases as dc
import host_build


@pytest.fixture(scope='module')
def hip():
    from red_gym_amd import _lib
    return _lib, _lib.load()


# ---------------------------------------------------------------- f110_dense_validate and f110_dense_workspace
def test_validate_refusals(hip):
    from red_gym_amd import dense
    dense.validate(1, 1, 1, 4)
    dense.validate(dc.MAX_K, dc.MAX_H, dc.MAX_K, dc.MAX_S, True)
    dense.validate(25088, 512, 25104, 784)
    bad = [(0, 1, None, 4), (dc.MAX_K + 1, 1, None, 4), (-3, 1, None, 4), (1, 0, None, 4), (1, dc.MAX_H + 1, None, 4), (8, 1, 7, 4),
           (8, 1, -1, 4), (8, 1, None, 0), (8, 1, None, 3), (8, 1, None, 6), (8, 1, None, dc.MAX_S + 4), (8, 1, None, -4), (2 ** 40, 1, None, 4)]
    for k, h, ld, s in bad:
        with pytest.raises(ValueError):
            dense.validate(k, h, ld, s)
    _lib, lib = hip
    c = dense.make_config(8, 8)
    c.reserved = 1
    assert lib.f110_dense_validate(ctypes.byref(c)) == _lib.E_INVALID and b'reserved' in lib.f110_last_error()
    assert lib.f110_dense_validate(None) == _lib.E_INVALID


def test_workspace_formula(hip):
    from red_gym_amd import dense
    for n, K, H, S in dc.SHAPES + [dc.SAL, (64, 25088, 512, 784), (4096, 25088, 512, 784), (65536, 25088, 512, 784)]:
        p = dc.paths(n, K, H, S)
        for ld in (K, K + 3):
            assert dense.workspace_bytes(dense.make_config(K, H, ld, S), n) == p['workspace'] == (4 * -(-K // S) * n * H if p['split'] else 0), (n, K, H, S)
    cfg = dense.make_config(100, 130, None, 36)
    assert [dense.workspace_bytes(cfg, n) for n in (0, -1, dc.MAX_ROWS + 1, 2 ** 62)] == [0, 0, 0, 0]
    assert dense.workspace_bytes(dense.make_config(100, 130, 99, 36), 4) == 0            # an invalid configuration
    # SAL: the update's batch goes through the workspace, 4 MB; acting on 4 096 rows and more adds in registers
    assert dc.paths(64, 25088, 512, 784)['workspace'] == 32 * 64 * 512 * 4 and not dc.paths(4096, 25088, 512, 784)['split']


# ---------------------------------------------------------------- the shape table
def test_shape_table_reaches_every_path():
    ps = [dc.paths(*s) for s in dc.SHAPES]
    assert {p['path'] for p in ps} == {'split', 'registers', 'single'}
    for key in ('kpad', 'chunk_pad', 'partial_m', 'partial_n', 'gx_partial_n', 'gw_partial_m'):
        assert {p[key] for p in ps} == {False, True}, key
    assert max(p['chunks'] for p in ps) > 1 and max(p['segs'] for p in ps) > 2
    for key in ('mblocks', 'nblocks', 'gx_nblocks', 'gw_mblocks', 'gx_chunks', 'gw_chunks', 'sum_blocks', 'gb_blocks'):
        assert min(p[key] for p in ps) <= 1 < max(p[key] for p in ps), key
    # the pair either side of the plan's boundary: the same (K, H, S), n one apart, taken from paths()
    a, b = dc.SHAPES[-2], dc.SHAPES[-1]
    assert a[1:] == b[1:] == dc.EDGE and b[0] == a[0] + 1 and (dc.paths(*a)['path'], dc.paths(*b)['path']) == ('split', 'registers')
    assert dc.paths(*a)['workspace'] > 0 == dc.paths(*b)['workspace']
    # what the comments of the table claim
    want = {(1, 1, 1, 4): dict(segs=1, last_seg=1), (5, 7, 3, 4): dict(segs=2, last_seg=3, kpad=True), (17, 37, 33, 8): dict(segs=5, last_seg=5),
            (16, 64, 16, 64): dict(segs=1, chunks=2, chunk_pad=False, workspace=0), (33, 1572, 20, 784): dict(segs=3, last_seg=4, mblocks=2),
            (40, 100, 130, 36): dict(segs=3, nblocks=3, mblocks=2, chunks=2, gx_chunks=5)}
    for s, w in want.items():
        assert s in dc.SHAPES and {k: dc.paths(*s)[k] for k in w} == w, s
    assert dc.paths(*dc.SAL)['segs'] == 32 and dc.paths(*dc.SAL)['path'] == 'split'
    # no kernel walks a grid: every launch of every shape the limits admit stays inside the device's
    worst = dc.paths(dc.MAX_ROWS, dc.MAX_K, dc.MAX_H, 4)
    assert worst['gx'] <= dc.DN_MAX_GRID_X and max(worst['gy'], worst['gx_nblocks'], worst['gw_nblocks']) <= dc.DN_MAX_GRID_Y


@pytest.mark.parametrize('shape', dc.SHAPES, ids=str)
def test_a_wrong_segmentation_gives_other_bits(shape):
    """With another S -- or one chain over all of K -- at least one element of the forward differs, so a kernel that cuts K elsewhere
    cannot pass the GPU test of this shape.  (K <= 4 has one chain under every S.)"""
    n, K, H, S = shape
    r = dc.reference(shape)
    other = dc.other_segment(K, S)
    if other is None:
        assert K <= 4
        return
    assert (dc.chains(r['x'], r['w'], other).view(np.uint32) != r['sum'].view(np.uint32)).any()
    if K > S:
        one = dc.chains(r['x'], r['w'], 4 * -(-K // 4))
        assert (one.view(np.uint32) != r['sum'].view(np.uint32)).any()


# ---------------------------------------------------------------- the checkers against fp64
def close(v, ref, mag, t, factor=1.0):
    err = np.abs(np.asarray(v, np.float64) - ref)
    return bool((err <= factor * dc.gamma(t) * mag).all())


@pytest.mark.parametrize('shape', dc.SHAPES[:6], ids=str)
def test_checkers_against_fp64(shape):
    n, K, H, S = shape
    r = dc.reference(shape)
    v = (False, True)
    ref, mag = dc.forward_fp64(r['x'], r['w'], r['b'])
    assert close(r['out'][v], ref, mag, dc.forward_roundings(K, S))
    g = r['g'][(True, True)]
    assert (g == 0).any() and (g != 0).any() or n * H < 4
    assert close(r['grad_x'][(True, True)], *dc.grad_x_fp64(g, r['w']), H)
    assert close(r['grad_weight'][(True, True)], *dc.grad_weight_fp64(g, r['x']), n)
    assert close(r['grad_bias'][(True, True)], *dc.grad_bias_fp64(g), max(n - 1, 1))


# ---------------------------------------------------------------- the launch plan, compiled for the host
CONSTANTS = ('DN_MAX_K DN_MAX_H DN_MAX_S DN_MAX_ROWS DN_THREADS DN_BM DN_BN DN_KC DN_LDK DN_LDM DN_LDN DN_SPLIT_BELOW DN_MAX_GRID_X '
             'DN_MAX_GRID_Y DN_FORWARD_LDS DN_GRADX_LDS DN_GRADW_LDS DN_LDS_BYTES').split()
KEYS = ('segs chunks mblocks nblocks split gx gy block inst lds sum_blocks sum_block workspace gx_mblocks gx_nblocks gw_mblocks gw_nblocks '
        'gb_blocks gb_block').split()

SHIM = r'''
#include "f110_dense_plan.h"
using namespace f110;
typedef long long ll;

#define C(x) {#x, (ll)x}
static const struct { const char *name; ll value; } constants[] = {@CONSTANTS@};
#undef C
extern "C" int shim_constant(const char *name, ll *out)
{
    for (const auto &c : constants) if (!strcmp(c.name, name)) { *out = c.value; return 1; }
    return 0;
}

// s: (K, H, ld, S)
extern "C" int shim_dense(const int *s, ll n, ll *o)
{
    f110_dense_config c = {};
    c.in_features = s[0]; c.out_features = s[1]; c.ld = s[2]; c.segment = s[3];
    if (int rc = dense_check(&c, "shim")) return rc;
    if (n < 1 || !dense_rows_ok(n)) return -1;
    const DenseForwardPlan f = dense_forward_plan(c, n);
    const DenseBackwardPlan b = dense_backward_plan(c, n);
    const ll v[] = {f.a.segs, f.a.chunks, f.a.mblocks, f.a.nblocks, f.a.split, f.gemm.gx, f.gemm.gy, f.gemm.block, f.gemm.inst, (ll)f.gemm.lds,
                    f.sum.gx, f.sum.block, dense_workspace_bytes(c, n), b.gradx.gx, b.gradx.gy, b.gradw.gx, b.gradw.gy, b.gradb.gx, b.gradb.block};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
    // what the plans must agree on, and what never varies
    return (f.gemm.gz == 1 && f.sum.gy == 1 && b.gradx.gz == 1 && b.gradw.gz == 1 && b.gradb.gy == 1 && b.gradx.block == (unsigned)DN_THREADS
            && b.gradw.block == (unsigned)DN_THREADS && b.gradx.lds + b.gradw.lds + b.gradb.lds + f.sum.lds == 0 && f.a.n == n && b.a.n == n
            && b.gx_mblocks == (int)b.gradx.gx && b.gw_mblocks == (int)b.gradw.gx && f.a.K == s[0] && f.a.H == s[1] && f.a.ld == s[2] && f.a.S == s[3]) ? 0 : 100;
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('dense_plan'), 'denseplan',
                              host_build.FAIL_SHIM + SHIM.replace('@CONSTANTS@', ', '.join('C(%s)' % c for c in CONSTANTS)))
    L.shim_message.restype = ctypes.c_char_p
    L.shim_constant.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
    L.shim_dense.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    return L


def constant(L, name):
    v = ctypes.c_longlong()
    assert L.shim_constant(name.encode(), ctypes.byref(v)), name
    return v.value


def plan(L, K, H, ld, S, n):
    """The compiled plan as a dict, or None where the compiled check refuses the configuration or n."""
    s = (ctypes.c_int * 4)(K, H, ld, S)
    out = (ctypes.c_longlong * len(KEYS))()
    rc = L.shim_dense(s, n, out)
    assert rc in (0, -1), 'the plans of %r disagree among themselves' % ((K, H, ld, S, n),)
    return dict(zip(KEYS, out)) if rc == 0 else None


def check_plan(L, hip, K, H, ld, S, n):
    p = plan(L, K, H, ld, S, n)
    if p is None:
        return None
    w = dc.paths(n, K, H, S)
    both = sorted(set(p) & set(w))
    assert set('segs chunks mblocks nblocks split gx gy sum_blocks workspace gx_mblocks gx_nblocks gw_mblocks gw_nblocks gb_blocks'.split()) <= set(both)
    bad = {k: (p[k], w[k]) for k in both if p[k] != int(w[k])}
    assert not bad, ((K, H, ld, S, n), bad)
    # what every launch must satisfy: static LDS only, within the budget; a grid the device takes; workspace == 0 exactly on the in-register path
    assert p['lds'] == 0 and (p['block'], p['sum_block'], p['gb_block']) == (dc.DN_THREADS, dc.DN_THREADS, 64)
    assert p['inst'] == p['split'] and (p['workspace'] == 0) == (not p['split']) and (p['sum_blocks'] == 0) == (not p['split'])
    for gx, gy in ((p['gx'], p['gy']), (p['gx_mblocks'], p['gx_nblocks']), (p['gw_mblocks'], p['gw_nblocks']), (p['gb_blocks'], 1), (max(p['sum_blocks'], 1), 1)):
        assert 1 <= gx <= dc.DN_MAX_GRID_X and 1 <= gy <= dc.DN_MAX_GRID_Y, (K, H, ld, S, n)
    if hip:
        _lib, lib_ = hip
        assert lib_.f110_dense_workspace(ctypes.byref(_lib.DenseConfig(K, H, ld, S, 0, 0)), n) == p['workspace']
    return p


def test_constants_the_cases_file_types_again(lib):
    c = {name: constant(lib, name) for name in CONSTANTS}
    want = dict(DN_MAX_K=dc.MAX_K, DN_MAX_H=dc.MAX_H, DN_MAX_S=dc.MAX_S, DN_MAX_ROWS=dc.MAX_ROWS, DN_THREADS=dc.DN_THREADS, DN_BM=dc.DN_BM, DN_BN=dc.DN_BN,
                DN_KC=dc.DN_KC, DN_LDK=dc.DN_LDK, DN_LDM=dc.DN_LDM, DN_LDN=dc.DN_LDN, DN_SPLIT_BELOW=dc.DN_SPLIT_BELOW, DN_MAX_GRID_X=dc.DN_MAX_GRID_X,
                DN_MAX_GRID_Y=dc.DN_MAX_GRID_Y, DN_LDS_BYTES=dc.DN_LDS_BYTES)
    assert {k: c[k] for k in want} == want
    # the kernels' static LDS: the tiles of one chunk, well inside what a workgroup may ask for
    assert c['DN_FORWARD_LDS'] == (dc.DN_BM + dc.DN_BN) * dc.DN_LDK * 4 == 13824
    assert c['DN_GRADX_LDS'] == (dc.DN_BM * dc.DN_LDK + dc.DN_KC * dc.DN_LDN) * 4 == 14848
    assert c['DN_GRADW_LDS'] == (dc.DN_KC * dc.DN_LDM + dc.DN_KC * dc.DN_LDN) * 4 == 16384
    assert max(c['DN_FORWARD_LDS'], c['DN_GRADX_LDS'], c['DN_GRADW_LDS']) <= dc.DN_LDS_BYTES
    # a staged read's 64 addresses fall into 64 different banks: rows DN_LDK apart with 4 terms each; terms DN_LDM / DN_LDN apart with 16 columns each
    assert len({(col * dc.DN_LDK + q) % 64 for col in range(16) for q in range(4)}) == 64
    assert all(len({(q * ld + col) % 64 for col in range(16) for q in range(4)}) == 64 for ld in (dc.DN_LDM, dc.DN_LDN))
    from red_gym_amd import dense
    assert (dense.MAX_IN, dense.MAX_OUT, dense.MAX_SEGMENT, dense.MAX_ROWS, dense.DEFAULT_SEGMENT) == (dc.MAX_K, dc.MAX_H, dc.MAX_S, dc.MAX_ROWS, dc.DEFAULT_SEGMENT)


def test_plan_on_the_table(lib, hip):
    for n, K, H, S in dc.SHAPES + [dc.SAL, (64, 25088, 512, 784), (4096, 25088, 512, 784), (65536, 25088, 512, 784)]:
        for name, (ld, _) in dc.LAYOUTS.items():
            assert check_plan(lib, hip, K, H, ld(K), S, n)
    assert check_plan(lib, hip, dc.MAX_K, dc.MAX_H, dc.MAX_K, 4, dc.MAX_ROWS)
    assert check_plan(lib, hip, dc.MAX_K, 1, dc.MAX_K, 4, 1)['gx'] == dc.MAX_K // 4


def test_plan_on_a_seeded_sample(lib, hip):
    """2000 configurations the compiled check accepts, out of draws that reach a little past every limit."""
    rng = np.random.default_rng(43)
    ok = refused = 0
    while ok < 2000:
        assert refused < 20000
        K = int(rng.integers(0, dc.MAX_K + 2)) if rng.random() < 0.3 else int(rng.integers(0, 3000))
        H = int(rng.integers(0, dc.MAX_H + 2)) if rng.random() < 0.3 else int(rng.integers(0, 200))
        S = int(rng.integers(0, dc.MAX_S // 4 + 2)) * 4 + (int(rng.integers(1, 4)) if rng.random() < 0.05 else 0)
        ld = K + int(rng.integers(-1, 5))
        n = int(rng.choice([1, 3, 31, 32, 33, 67, 8160, 8161, 65536, dc.MAX_ROWS, dc.MAX_ROWS + 1, 0]))
        p = check_plan(lib, hip, K, H, ld, S, n)
        ok, refused = ok + (p is not None), refused + (p is None)
    assert refused > 0


# ---------------------------------------------------------------- the reference pin
def test_reference_pin():
    g, x, w, b = dc.golden_inputs()
    pre = dc.forward(x, w, b, dc.DEFAULT_SEGMENT, False)
    # the backward on the recording's own mask: a pre-activation within its bound of 0 may have the other sign in the checker, and
    # the backward's contract is stated on the forward's output it is given
    gm = dc.masked(g['pre'], g['cotangent'], True)
    dc.golden_check(g, x, w, b, pre, dc.grad_x(gm, w), dc.grad_weight(gm, x, g['cols']), dc.grad_bias(gm))
