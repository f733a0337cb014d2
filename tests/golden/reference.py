"""Everything the fixture generators know about the reference: where it lies, the stand-in modules its imports need,
its loaders, the two host guards and the helpers every generator shares.  Used ONLY through make_golden.py to produce
the .npz fixtures in this directory; nothing here is imported by bench.py or the product, and the reference does not
exist where the GPU tests run.  Nothing is loaded at import time.

The reference's kernels are plain Python decorated with numba.njit; numba is not installed where the fixtures are
generated, so an identity `njit` stand-in is registered before import (same source, same IEEE-754 double operations,
see SURVEY.md section 8c).  gym, pyglet, cv2, cvxpy and shapely are absent too and get minimal stand-ins; the recorded
functions call none of them.  The package __init__ (which imports `gym`) is bypassed by pre-seeding sys.modules with
namespace modules whose __path__ points at the reference.

Host guards.  Some recorded functions form a 2-element dot product with np.dot, which NumPy hands to the BLAS, and what
a BLAS does with it is the host's business: OpenBLAS's SkylakeX kernel returns fma(x1, y1, x0 * y0), its Haswell and
older kernels the two rounded products and their sum.  Those fixtures record the reference under IEEE arithmetic without
contraction, so make_golden.py puts BLAS_PIN into the environment of their interpreters -- it must
be there before NumPy is first imported -- and their generators call require_unfused_dot().
"""
import importlib
import importlib.util
import os
import runpy
import sys
import types
import warnings

import numpy as np

ROOT_ENV = 'F110_REFERENCE'             # overrides DEFAULT_ROOT; make_golden.py --reference sets it
DEFAULT_ROOT = '/root/reference'
BLAS_PIN = ('OPENBLAS_CORETYPE', 'Haswell')

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (os.path.dirname(TESTS), TESTS, HERE):   # the generators import tests/*_cases.py and the oracle package
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = HERE          # where save() writes (make_golden.py --out)
FRESH = set()       # the files the running make_golden.py call has already written to OUT

PARAMS = {'mu': 1.0489, 'C_Sf': 4.718, 'C_Sr': 5.4562, 'lf': 0.15875, 'lr': 0.17145, 'h': 0.074,
          'm': 3.74, 'I': 0.04712, 's_min': -0.4189, 's_max': 0.4189, 'sv_min': -3.2, 'sv_max': 3.2,
          'v_switch': 7.319, 'a_max': 9.51, 'v_min': -5.0, 'v_max': 20.0, 'width': 0.31, 'length': 0.58}


def path(*parts):
    """A path below the reference's root."""
    return os.path.join(os.environ.get(ROOT_ENV, DEFAULT_ROOT), *parts)


# ---------------------------------------------------------------------------------------------- stand-ins
def _identity_njit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda f: f


def _module(name, **attrs):
    """sys.modules[name], created empty if absent (a generator's recording stand-in stays), hung on its parent."""
    mod = sys.modules.setdefault(name, types.ModuleType(name))
    for k, v in attrs.items():
        if not hasattr(mod, k):
            setattr(mod, k, v)
    parent, _, leaf = name.rpartition('.')
    if parent:
        setattr(sys.modules[parent], leaf, mod)
    return mod


def stand_ins():
    """Registers the stand-ins for the third-party packages the reference imports and this image lacks."""
    _module('numba', njit=_identity_njit)
    _module('gym', Env=type('Env', (object,), {}))
    for name in ('gym.error', 'gym.spaces', 'gym.utils', 'gym.utils.seeding'):
        _module(name)
    _module('pyglet', options={})
    _module('pyglet.gl', GL_POINTS=0, GL_LINES=1)
    for name in ('cv2', 'cvxpy', 'shapely', 'shapely.geometry'):
        _module(name)


# ---------------------------------------------------------------------------------------------- loaders
def _load_file(name, *parts):
    stand_ins()
    spec = importlib.util.spec_from_file_location(name, path(*parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_env(package='gym/f110_gym'):
    """(laser_models, dynamic_models, collision_models, base_classes, f110_env) of a package copy: the current one,
    or the older copy 'f1tenth_gym/gym/f110_gym' (fov 4.7 default)."""
    stand_ins()
    pkg = types.ModuleType('f110_gym')
    pkg.__path__ = [path(package)]
    sub = types.ModuleType('f110_gym.envs')
    sub.__path__ = [path(package, 'envs')]
    sys.modules['f110_gym'] = pkg
    sys.modules['f110_gym.envs'] = sub
    warnings.filterwarnings('ignore', message='Chosen integrator is RK4')
    return tuple(importlib.import_module('f110_gym.envs.' + m)
                 for m in ('laser_models', 'dynamic_models', 'collision_models', 'base_classes', 'f110_env'))


def load_sal():
    """src/SAL.py by file path; its main does not run."""
    return _load_file('ref_sal', 'src', 'SAL.py')


def load_planner():
    """(module, config) of examples/waypoint_follow.py and its config_example_map.yaml, paths made absolute."""
    from argparse import Namespace
    import yaml
    mod = _load_file('ref_waypoint_follow', 'examples', 'waypoint_follow.py')
    with open(path('examples', 'config_example_map.yaml')) as f:
        conf = Namespace(**yaml.safe_load(f))
    conf.wpt_path = path('examples', 'example_waypoints.csv')
    conf.map_path = path('examples', 'example_map')
    return mod, conf


def raceline():
    return np.loadtxt(path('examples', 'example_waypoints.csv'), delimiter=';', skiprows=3)


def run_path(rel, **kw):
    """runpy.run_path of a script of the reference (g10-g12 execute three) with the stand-ins in place."""
    stand_ins()
    return runpy.run_path(path(rel), **kw)


# ---------------------------------------------------------------------------------------------- host guards
def require_unfused_dot():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-3, 3, (4096, 2)), rng.uniform(-3, 3, (4096, 2))
    if not all(np.dot(a[k], b[k]) == a[k, 0] * b[k, 0] + a[k, 1] * b[k, 1] for k in range(4096)):
        raise SystemExit('np.dot fuses its multiply-add on this host (BLAS kernel): the fixture would record the host, not the reference')


# ---------------------------------------------------------------------------------------------- helpers
def fixture(name):
    """Where a generator reads the fixture `name` from: OUT if this make_golden.py call wrote it there, else the committed file."""
    return os.path.join(OUT if name in FRESH else HERE, name)


def save(name, **arrays):
    """Writes OUT/name; returns its size in bytes."""
    out = os.path.join(OUT, name)
    np.savez_compressed(out, **arrays)
    size = os.path.getsize(out)
    print('wrote', name, '%.1f KB' % (size / 1024), flush=True)
    return size


def within(name, v, ref, mag, terms):
    """Asserts |v - ref| <= gamma(terms) * mag elementwise: a recorded fp32 array against the fp64 sum of `terms` terms
    and the sum of their magnitudes (g22, g23)."""
    import bitconv_cases as bc
    err = np.abs(np.asarray(v, np.float64) - ref)
    bound = bc.gamma(terms) * mag
    print('%-18s T = %6d: worst error / bound %.6f, worst error %.3f u * mag' % (
        name, terms, float((err / np.maximum(bound, 1e-300)).max()), float((err / np.maximum(bc.U * mag, 1e-300)).max())))
    assert (err <= bound).all(), name


class StubBuffer:
    """A replay buffer whose sample() returns the prepared arrays (g21, g24)."""

    def __init__(self, arrays):
        self.arrays = arrays

    def __len__(self):
        return len(self.arrays[0])

    def sample(self, batch_size):
        assert batch_size == len(self)
        return self.arrays
