"""No-GPU checks of prioritized replay (csrc/f110_priority.h): the level layout of csrc/f110_priority_plan.h compiled for the host
against the checker of tests/priority_cases.py, the checker's descent against the flat cumsum / searchsorted it must equal, the checker's
set and quantisation on hand-made rows, the ABI mirror of the new entries and structs against the header and the C compiler, the
library's refusals before any launch, and the host side's options."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_header
import host_build
import priority_cases as pc

LAYOUT_L = pc.CPU_L + (2 ** 26,)

SHIM = host_build.FAIL_SHIM + r'''
#include "f110_priority_plan.h"
using namespace f110;
typedef long long ll;
extern "C" ll shim_constant(int which) { const ll v[] = {PT_FANOUT, PT_MAX_LEVELS, PT_THREADS, F110_PRIORITY_SHIFT, (ll)F110_PRIORITY_MAX_LEAVES,
                                                         (ll)sizeof(f110_priority_state), F110_PRIORITY_STATE_BYTES}; return v[which]; }
// o: levels, words, then count[PT_MAX_LEVELS], offset[PT_MAX_LEVELS]
extern "C" void shim_layout(ll L, ll *o)
{
    const PriorityLayout p = priority_layout(L);
    o[0] = p.levels; o[1] = p.words;
    for (int k = 0; k < PT_MAX_LEVELS; k++) { o[2 + k] = p.count[k]; o[2 + PT_MAX_LEVELS + k] = p.offset[k]; }
}
extern "C" ll shim_node_words(ll L) { return priority_node_words(L); }
extern "C" int shim_tree_check(ll leaf, ll node, ll L) { return priority_tree_check("tree", (const void *)(uintptr_t)leaf, (const void *)(uintptr_t)node, L); }
extern "C" int shim_config_check(const f110_priority_config *cfg) { return priority_config_check("config", cfg); }
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('priority_plan'), 'priorityplan', SHIM)
    L.shim_constant.restype = L.shim_node_words.restype = C.c_longlong
    L.shim_node_words.argtypes = [C.c_longlong]
    L.shim_message.restype = C.c_char_p
    L.shim_layout.argtypes = [C.c_longlong, C.POINTER(C.c_longlong)]
    L.shim_layout.restype = None
    L.shim_tree_check.argtypes = [C.c_longlong] * 3
    L.shim_config_check.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope='module')
def lib():
    from red_gym_amd import _lib, build
    build.build()
    return _lib.load()


def test_plan_header_layout_equals_the_checker(shim):
    fan, max_levels = shim.shim_constant(0), shim.shim_constant(1)
    assert [shim.shim_constant(k) for k in range(7)] == [pc.FANOUT, max_levels, 256, pc.SHIFT, pc.MAX_LEAVES, pc.STATE_BYTES, pc.STATE_BYTES] and fan == 64
    seen = set()
    for L in LAYOUT_L + (pc.MAX_LEAVES,):
        o = (C.c_longlong * (2 + 2 * max_levels))()
        shim.shim_layout(L, o)
        w = pc.layout(L)
        assert w['levels'] <= max_levels
        assert (o[0], o[1]) == (w['levels'], w['words']), L
        assert list(o[2:2 + w['levels']]) == w['count'] and list(o[2 + max_levels:2 + max_levels + w['levels']]) == w['offset'], L
        assert shim.shim_node_words(L) == w['words']
        assert not w['count'] or (w['count'][-1] <= 64 and all(c > 64 for c in w['count'][:-1]))
        seen.add(w['levels'])
    assert seen == {0, 1, 2, 3, 4, 5}
    assert [pc.layout(L)['levels'] for L in pc.GPU_L] == [0, 0, 0, 1, 2, 3]                  # what the GPU cases reach
    assert pc.layout(65) == dict(levels=1, count=[2], offset=[0], words=2)
    assert pc.layout(262145) == dict(levels=3, count=[4097, 65, 2], offset=[0, 4097, 4162], words=4164)
    assert shim.shim_node_words(0) == -1 and shim.shim_node_words(pc.MAX_LEAVES + 1) == -1


def test_plan_header_refuses(shim):
    from red_gym_amd import _lib
    bad_tree = [((4096, 8192, 0), 'L=0'), ((4096, 8192, pc.MAX_LEAVES + 1), 'L='), ((0, 8192, 100), 'null leaf'), ((4098, 8192, 100), 'leaf is not 4-byte'),
                ((4096, 0, 100), 'null node'), ((4096, 8196, 100), 'node is not 8-byte')]
    for args, word in bad_tree:
        assert shim.shim_tree_check(*args) == _lib.E_INVALID and word.encode() in shim.shim_message(), (args, shim.shim_message())
    assert shim.shim_tree_check(4096, 0, 64) == 0 and shim.shim_tree_check(4100, 8192, 65) == 0
    nan, inf = float('nan'), float('inf')
    for exponent, eps, word in ((-0.1, 1e-6, 'exponent'), (8.5, 1e-6, 'exponent'), (nan, 1e-6, 'exponent'), (0.6, -1e-9, 'eps'), (0.6, inf, 'eps'), (0.6, nan, 'eps')):
        cfg = _lib.PriorityConfig(exponent, eps)
        assert shim.shim_config_check(C.byref(cfg)) == _lib.E_INVALID and word.encode() in shim.shim_message(), (exponent, eps)
    assert shim.shim_config_check(None) == _lib.E_INVALID and b'null config' in shim.shim_message()
    for exponent, eps in ((0.0, 0.0), (8.0, 1.0), (0.6, 1e-6)):
        assert shim.shim_config_check(C.byref(_lib.PriorityConfig(exponent, eps))) == 0


@pytest.mark.parametrize('L', pc.CPU_L)
def test_the_descent_equals_cumsum_searchsorted(L):
    n = 512 if L > 4097 else 2048
    for name, leaf in (('random', pc.random_leaves(L)), ('sparse', pc.sparse_leaves(L))):
        node = pc.rebuild(leaf)
        assert len(node) == pc.layout(L)['words']
        idx, q, path = pc.pick(leaf, node, 777, 5, n)
        assert np.array_equal(idx, pc.pick_flat(leaf, 777, 5, n)), (L, name)
        assert (q > 0).all() and np.array_equal(q, leaf[idx]) and np.array_equal(path[:, -1], idx)
        if name == 'sparse' and L >= 63:
            edge = L // 5
            assert not leaf[:edge].any() and not leaf[L - edge:].any() and (leaf == 0).mean() > 0.9
    zero = np.zeros(L, np.uint32)
    idx, q, _ = pc.pick(zero, pc.rebuild(zero), 1, 0, 8)
    assert (idx == -1).all() and not q.any() and (pc.pick_flat(zero, 1, 0, 8) == -1).all()


def test_every_node_is_the_sum_of_its_children():
    L = 4097
    leaf = pc.random_leaves(L)
    node, lay = pc.rebuild(leaf), pc.layout(L)
    assert lay['levels'] == 2 and int(node[lay['offset'][1]]) == sum(int(x) for x in leaf[:4096]) and int(node[lay['offset'][1] + 1]) == int(leaf[4096])
    assert int(node[0]) == sum(int(x) for x in leaf[:64]) and int(node[64]) == int(leaf[4096])
    big = np.full(1 << 23, pc.QMAX_WORD, np.uint32)                     # (sums above 2^32 stay exact: 2^17, 2^11 and 32 nodes)
    assert pc.layout(1 << 23)['count'] == [1 << 17, 1 << 11, 32] and int(pc.rebuild(big)[-1]) == (1 << 18) * pc.QMAX_WORD


def test_the_set_takes_the_maximum_and_skips_rows_outside():
    leaf = np.array([5, 0, 7, 9], np.uint32)
    got = pc.set_max(leaf, [0, 0, 2, -1, 4, 3, 3], [3, 2, 0, 99, 99, 1, 8])
    assert got.tolist() == [3, 0, 0, 8] and leaf.tolist() == [5, 0, 7, 9]


def test_quantisation_of_the_checker():
    q, _ = pc.quantise(np.array([0.0, 1.0, 0.5, 1e-9, 70000.0, np.nan, np.inf, 3e38], np.float32), 1.0, 0.0)
    assert q.tolist() == [1, 65536, 32768, 1, pc.QMAX_WORD, pc.QMAX_WORD, pc.QMAX_WORD, pc.QMAX_WORD]
    q, _ = pc.quantise(np.array([0.25, np.nan], np.float32), 0.5, 0.0)
    assert q.tolist() == [32768, pc.QMAX_WORD]
    q, _ = pc.quantise(np.array([0.0, 123.0], np.float32), 0.0, 0.0)
    assert q.tolist() == [65536, 65536]                                      # pow(x, 0) = 1, pow(0, 0) included
    w = pc.weights([4, 2, 8, 2, 1], [1, 1, 1, 1, 0], 1.0)
    assert w.tolist() == [0.5, 1.0, 0.25, 1.0, 0.0] and pc.weights([4, 2], [1, 1], 0.0).tolist() == [1.0, 1.0]


# ---------------------------------------------------------------- the ABI mirror
NEW_ENTRIES = ('f110_priority_node_words', 'f110_ptree_rebuild', 'f110_ptree_set', 'f110_ptree_pick', 'f110_priority_install', 'f110_priority_bind',
               'f110_priority_reset', 'f110_priority_sample', 'f110_priority_update', 'f110_priority_set', 'f110_sac_critic_loss_weighted')


def test_the_abi_mirror_covers_the_new_entries(lib):
    from red_gym_amd import _lib
    defines, structs, protos = abi_header.read(host_build.ROOT + '/include/f110_hip.h')
    assert all(name in protos and name in _lib.SYMBOLS for name in NEW_ENTRIES)
    mine = {k: _lib.SYMBOLS[k] for k in NEW_ENTRIES}
    assert abi_header.diff_prototypes({k: protos[k] for k in NEW_ENTRIES}, mine, {k: v for k, v in _lib.RESTYPES.items() if k in mine}, _lib.STRUCTS) == []
    assert protos['f110_priority_node_words'][0] == 'int64' and len(protos['f110_priority_sample'][1]) == 18
    # (the check can fail: an argument of another width is reported)
    drift = dict(mine, f110_ptree_set=mine['f110_ptree_set'][:5] + [C.c_int64] + mine['f110_ptree_set'][6:])
    assert abi_header.diff_prototypes({k: protos[k] for k in NEW_ENTRIES}, drift, {'f110_priority_node_words': C.c_int64}, _lib.STRUCTS)[0].startswith('f110_ptree_set: argument 5')
    for k in ('F110_PRIORITY_SHIFT', 'F110_PRIORITY_MAX_LEAVES', 'F110_PRIORITY_STATE_BYTES'):
        assert defines[k] == getattr(_lib, k)
    for name in NEW_ENTRIES:
        assert list(getattr(lib, name).argtypes) == list(_lib.SYMBOLS[name])


def test_mirrored_structs_against_the_compiler(tmp_path):
    from red_gym_amd import _lib
    assert set(_lib.PRIORITY_STRUCTS) == {'f110_priority_config', 'f110_priority_state', 'f110_priority_buffers'}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "f110_hip.h"', 'int main(void)', '{']
    for name, cls in sorted(_lib.PRIORITY_STRUCTS.items()):
        lines.append('    printf("%s %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, f, name, f) for f, _ in cls._fields_]
    got = dict(line.split() for line in host_build.run_c(tmp_path, 'layout', '\n'.join(lines + ['    return 0;', '}', ''])).splitlines())
    text = re.sub(r'/\*.*?\*/', ' ', open(host_build.ROOT + '/include/f110_hip.h').read(), flags=re.S)
    for name, cls in _lib.PRIORITY_STRUCTS.items():
        assert int(got[name]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(got['%s.%s' % (name, f)]) == getattr(cls, f).offset, (name, f)
        body = re.search(r'typedef struct %s\s*\{(.*?)\}\s*%s\s*;' % (name, name), text, flags=re.S).group(1)
        declared = [re.sub(r'[\s*]|\[\d+\]', '', f) for decl in re.findall(r'\w+\s+([^;]+);', body) for f in decl.split(',')]
        assert declared == [f for f, _ in cls._fields_], (name, declared)
    assert C.sizeof(_lib.PriorityState) == _lib.F110_PRIORITY_STATE_BYTES == pc.STATE_BYTES


def test_library_refuses_before_any_launch(lib):
    from red_gym_amd import _lib
    A = 4096
    for L in LAYOUT_L:
        assert lib.f110_priority_node_words(L) == pc.layout(L)['words']
    assert lib.f110_priority_node_words(0) == -1 and lib.f110_priority_node_words(pc.MAX_LEAVES + 1) == -1
    cases = [(lambda: lib.f110_ptree_rebuild(None, A, 100, None), 'null leaf'), (lambda: lib.f110_ptree_rebuild(A, None, 100, None), 'null node'),
             (lambda: lib.f110_ptree_rebuild(A, A, 0, None), 'L=0'), (lambda: lib.f110_ptree_set(A, A, 100, None, A, 4, None), 'null idx'),
             (lambda: lib.f110_ptree_set(A, A, 100, A, None, 4, None), 'null q'), (lambda: lib.f110_ptree_set(A, A, 100, A, A, -1, None), 'n=-1'),
             (lambda: lib.f110_ptree_pick(A, A, 100, 1, 0, 4, None, A, None), 'null idx_out'), (lambda: lib.f110_ptree_pick(A, A, 100, 1, 0, 4, A, None, None), 'null q_out'),
             (lambda: lib.f110_ptree_pick(A, A, 100, 1, 0, -2, A, A, None), 'n=-2'), (lambda: lib.f110_ptree_pick(A + 2, A, 100, 1, 0, 4, A, A, None), 'not 4-byte'),
             (lambda: lib.f110_priority_install(None, None), 'null handle'), (lambda: lib.f110_priority_bind(None, None), 'null argument'),
             (lambda: lib.f110_priority_reset(None, None), 'null handle'), (lambda: lib.f110_priority_update(None, A, A, A, 4, None, None), 'null handle'),
             (lambda: lib.f110_priority_set(None, A, A, 4, None), 'null handle'),
             (lambda: lib.f110_priority_sample(None, 0, A, 4, 1, 0.99, A, A, A, A, A, A, A, A, A, A, A, None), 'null handle'),
             (lambda: lib.f110_sac_critic_loss_weighted(A, A, A, None, 4, A, None, None, None, None), 'null w'),
             (lambda: lib.f110_sac_critic_loss_weighted(A, A, A, A, 0, A, None, None, None, None), 'n=0')]
    for call, word in cases:
        assert call() == _lib.E_INVALID and word.encode() in lib.f110_last_error(), (word, lib.f110_last_error())
    assert lib.f110_ptree_set(A, A, 100, A, A, 0, None) == 0 and lib.f110_ptree_pick(A, A, 100, 1, 0, 0, A, A, None) == 0     # n = 0: nothing to do
    assert lib.f110_ptree_rebuild(A, None, 64, None) == 0                                                                      # no node: nothing to build


def test_options_and_fresh_state():
    from red_gym_amd import priority
    opt = priority.make_options(True)
    assert opt == dict(exponent=0.6, eps=1e-6, beta=0.4, beta_end=1.0, beta_updates=100000) and priority.make_options(dict(beta=0.5))['beta'] == 0.5
    for bad in (dict(alpha=0.6), 1, 'on'):
        with pytest.raises(TypeError):
            priority.make_options(bad)
    for bad in (dict(beta=-0.1), dict(beta=0.9, beta_end=0.5), dict(beta_updates=0), dict(beta_updates=2.5), dict(eps=float('nan')), dict(exponent=True)):
        with pytest.raises(ValueError):
            priority.make_options(bad)
    raw = priority.fresh_state_bytes(0.4, 6e-6, 1.0)
    s = pc.state_words(np.frombuffer(raw, np.int64))
    assert len(raw) == 64 and s == dict(qmax=pc.ONE, reserved0=0, beta=0.4, beta_step=6e-6, beta_end=1.0, reserved=[0, 0, 0, 0]) and priority.ONE == 1 << 16
