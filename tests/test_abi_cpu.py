"""No-GPU checks of the shipped library: it builds, loads and exports every symbol that include/f110_hip.h declares; the ctypes
mirror in red_gym_amd/_lib.py agrees with that header as a whole -- every prototype's return and argument types, every struct's
fields, sizes and offsets (the latter by the C compiler), every constant -- and each of those comparisons reports a drift planted
in a copy of the table; and the host-only entry point (exact EDT) reproduces scipy's distance transform on every bundled map."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_header
import host_build
from red_gym_amd import _lib, build
from red_gym_amd.maps import load_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _lib.load()


@pytest.fixture(scope='module')
def header():
    return abi_header.read(os.path.join(ROOT, 'include', 'f110_hip.h'))


@pytest.fixture(scope='module')
def compiled_layout(header, tmp_path_factory):
    """sizeof of every struct of the header and offsetof of every field, as strict C99 sees them."""
    return host_build.run_c(tmp_path_factory.mktemp('abi'), 'layout', abi_header.layout_program(header[1]))


def test_header_symbols_all_exported(lib, header):
    declared = set(header[2])
    assert len(declared) > 100 and declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:       # each resolves, and load() gave it the table's types
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(_lib.SYMBOLS[name]) and fn.restype is _lib.RESTYPES.get(name, C.c_int), name


def test_prototypes_match_header(header):
    assert abi_header.diff_prototypes(header[2], _lib.SYMBOLS, _lib.RESTYPES, _lib.STRUCTS) == []


def test_struct_layouts_match_header(header, compiled_layout):
    assert len(_lib.STRUCTS) == 22
    assert abi_header.diff_structs(header[1], _lib.STRUCTS) == []
    assert abi_header.diff_layout(compiled_layout, _lib.STRUCTS, {'f110_adam_state': _lib.F110_ADAM_STATE_BYTES}) == []
    # the *_FIELDS lists (Engine._alloc, episodes.pointers, Consumer._bind walk them) name the pointer fields of a struct each
    lists = {k: v for k, v in vars(_lib).items() if k.endswith('_FIELDS')}
    pointers = [[f for f, t, _ in fields if t.endswith('*')] for fields in header[1].values()]
    assert len(lists) == 9 and all(v in pointers for v in lists.values()), lists


def test_constants_match_header(header):
    mirrored = [k for k in vars(_lib) if k.startswith(('F110_', 'E_')) and isinstance(getattr(_lib, k), int)]
    assert len(mirrored) >= 20 and 'F110_EPISODES_BLOCK' in mirrored and 'E_UNBOUND' in mirrored
    assert abi_header.diff_constants(header[0], vars(_lib)) == []


def _drifted(cls, change):
    """A mirrored struct with other fields: change(list of (name, ctype)) -> list."""
    return type(cls.__name__, (C.Structure,), {'_fields_': change(list(cls._fields_))})


# name: (table, key, the drifted entry, what must be reported, by which comparisons: p prototypes, s structs, l layout, c constants)
_VP = C.c_void_p
DRIFTS = {
    'int32_for_int64': ('symbols', 'f110_noise_ensure', [_VP, C.c_int32, _VP], 'f110_noise_ensure: argument 1', 'p'),
    'int64_for_int32': ('symbols', 'f110_pack_env', [_VP, C.c_int64, _VP, _VP], 'f110_pack_env: argument 1', 'p'),
    'wrong_struct_pointer': ('symbols', 'f110_bind', [_VP, C.POINTER(_lib.ProgressBuffers)], 'f110_bind: argument 1', 'p'),
    'wrong_scalar_pointer': ('symbols', 'f110_launch_epoch', [_VP, C.POINTER(C.c_int32)], 'f110_launch_epoch: argument 1', 'p'),
    'wrong_restype': ('restypes', 'f110_dense_workspace', C.c_int, 'f110_dense_workspace: returns', 'p'),
    'fields_exchanged': ('structs', 'f110_config', _drifted(_lib.Config, lambda f: [f[1], f[0]] + f[2:]), 'f110_config: fields', 'sl'),
    'fields_of_one_width_exchanged': ('structs', 'f110_shaping_config', _drifted(_lib.ShapingConfig, lambda f: f[:2] + [f[3], f[2]] + f[4:]),
                                      'f110_shaping_config: fields', 'sl'),
    'field_dropped': ('structs', 'f110_episodes_buffers', _drifted(_lib.EpisodesBuffers, lambda f: f[:-1]), 'f110_episodes_buffers: fields', 'sl'),
    'array_off_by_one': ('structs', 'f110_pathfollow_config', _drifted(_lib.PathFollowConfig, lambda f: [(n, C.c_double * 3 if n == 'r' else c) for n, c in f]),
                         'f110_pathfollow_config.r:', 'sl'),
    # (the last field, before the tail padding: no size and no offset moves, only the field comparison can see it)
    'field_narrowed': ('structs', 'f110_adam_tensor', _drifted(_lib.AdamTensor, lambda f: f[:-1] + [('n', C.c_int32)]), 'f110_adam_tensor.n:', 's'),
    'constant_off_by_one': ('constants', 'F110_EPISODES_BLOCK', _lib.F110_EPISODES_BLOCK + 1, 'F110_EPISODES_BLOCK:', 'c'),
    'error_code': ('constants', 'E_INDEX', _lib.E_NOMAP, 'F110_E_INDEX:', 'c'),
    'constant_unknown_to_header': ('constants', 'F110_NO_SUCH', 1, 'F110_NO_SUCH:', 'c'),
    'state_bytes': ('sizes', 'f110_adam_state', _lib.F110_ADAM_STATE_BYTES + 8, 'f110_adam_state:', 'l'),
}


@pytest.mark.parametrize('name', sorted(DRIFTS))
def test_the_check_can_fail(header, compiled_layout, name):
    """Each kind of drift, planted in a copy of the tables, is reported under its symbol, field or constant by the comparisons that
    can see it, and nothing else is reported."""
    table, key, entry, report, where = DRIFTS[name]
    defines, structs, protos = header
    t = dict(symbols=dict(_lib.SYMBOLS), restypes=dict(_lib.RESTYPES), structs=dict(_lib.STRUCTS), constants=dict(vars(_lib)),
             sizes={'f110_adam_state': _lib.F110_ADAM_STATE_BYTES})
    assert t[table].get(key) != entry
    t[table][key] = entry
    # (SYMBOLS points at the product's classes, so the prototypes resolve them through the product's STRUCTS)
    found = {'p': abi_header.diff_prototypes(protos, t['symbols'], t['restypes'], _lib.STRUCTS), 's': abi_header.diff_structs(structs, t['structs']),
             'l': abi_header.diff_layout(compiled_layout, t['structs'], t['sizes']), 'c': abi_header.diff_constants(defines, t['constants'])}
    about = report.split(':')[0].split('.')[0]
    for kind, diffs in found.items():
        assert bool(diffs) == (kind in where) and all(d.startswith(about) for d in diffs), (kind, diffs)
    assert any(d.startswith(report) for diffs in found.values() for d in diffs), found


def test_error_reporting_without_gpu(lib):
    # argument validation happens before any HIP call
    rc = lib.f110_create(None, None)
    assert rc == _lib.E_INVALID and b'null' in lib.f110_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)
    out = np.zeros((4, 4), dtype=np.uint32)
    ones = np.ones((4, 4), dtype=np.uint8)
    rc = lib.f110_edt_squared(ones.ctypes.data_as(C.c_void_p), 4, 4, out.ctypes.data_as(C.c_void_p))
    assert rc == _lib.E_INVALID  # no occupied cell


@pytest.mark.parametrize('rel', ['example_map.yaml', 'maps/berlin.yaml', 'maps/skirk.yaml', 'maps/vegas.yaml'])
def test_exact_edt_equals_scipy(lib, assets, rel):
    from scipy.ndimage import distance_transform_edt as edt
    from red_gym_amd.engine import edt_squared
    m = load_map(os.path.join(assets, rel), '.png')
    d2 = edt_squared(m.free)
    ref = m.resolution * edt(m.free.astype(np.float64) * 255.)  # laser_models.py:52,425
    assert np.array_equal(m.resolution * np.sqrt(d2.astype(np.float64)), ref)


def test_exact_edt_small_cases(lib):
    from scipy.ndimage import distance_transform_edt as edt
    from red_gym_amd.engine import edt_squared
    rng = np.random.default_rng(5)
    for shape in [(1, 1), (1, 7), (9, 1), (5, 8), (33, 17), (64, 64)]:
        for dens in (0.02, 0.3, 0.9):
            free = (rng.uniform(size=shape) > dens).astype(np.uint8)
            free.flat[rng.integers(free.size)] = 0
            d2 = edt_squared(free)
            assert np.array_equal(np.sqrt(d2.astype(np.float64)), edt(free))


def test_map_loader_matches_oracle_loader(assets):
    import oracle
    for rel in ['example_map.yaml', 'maps/skirk.yaml']:
        m = load_map(os.path.join(assets, rel), '.png')
        o = oracle.load_map(os.path.join(assets, rel), '.png')
        assert (m.height, m.width, m.resolution) == (o['height'], o['width'], o['resolution'])
        assert (m.orig_x, m.orig_y, m.orig_c, m.orig_s) == (o['orig_x'], o['orig_y'], o['orig_c'], o['orig_s'])
        assert np.array_equal(m.free * 255., o['img'])


def test_product_never_imports_oracle():
    """The shipped package, its drop-in shims and the examples must not reference oracle/ (judge rule: no CPU
    fallback, the checker is test infrastructure); bench.py may, in its cpu_baseline leg only."""
    for top in ('red_gym_amd', 'f110_gym', 'weap_util', 'examples', 'include'):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(('.py', '.h', '.hip', '.cpp')):
                    src = open(os.path.join(dirpath, f)).read()
                    assert 'import oracle' not in src and 'from oracle' not in src, os.path.join(dirpath, f)
                    assert 'f110_oracle' not in src and 'oracle/_build' not in src, os.path.join(dirpath, f)
    bench = open(os.path.join(ROOT, 'bench.py')).read()
    leg = bench[bench.index('def cpu_baseline('):bench.index('class Ranks(')]
    rest = bench.replace(leg, '')
    assert 'import oracle' in leg and 'import oracle' not in rest and 'from oracle' not in rest


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No fallback: without libf110_hip.so the import path raises and names the build command."""
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'nope' / 'libf110_hip.so'))
    with pytest.raises(ImportError, match='no CPU fallback'):
        _lib.load()
