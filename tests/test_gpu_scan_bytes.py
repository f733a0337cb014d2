"""Byte cell codes of the compact scan form of 256 slots (csrc/f110_scan.h: scan_kernel<.., 256, true, true>; f110_map.h:
cell_elem_b): the march on the byte table in 16-column strips against the same form on its u16 table and against the classic
form, `==` on everything a caller sees.  F110_SCAN_FORM and F110_SCAN_CODES are read once per process, so each setting rolls
the cases of scan_bytes_cases.py out in a child process of its own (the three run side by side).  Run against the
bounds-checked build (F110_LIB, tests/test_gpu_bounds.py) the same tests hold its error word clean -- every look-up's offset
inside the byte table: the children inherit the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_bytes_cases as cases

pytestmark = pytest.mark.gpu

# setting -> (F110_SCAN_FORM, F110_SCAN_CODES, the form it must launch, whether it stages rows, whether it reads bytes)
SETTINGS = {'byte': ('compact256', 'byte', 256, 1, 1), 'word': ('compact256', 'word', 256, 1, 0), 'classic': ('classic', None, 0, 0, 0)}
KEYS = ['sums', 'col', 'done', 'lookups', 'rows'] + ['scans%d' % k for k in cases.base.KEEP]


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """setting -> the arrays of its child."""
    d = tmp_path_factory.mktemp('scan_bytes')
    env = {k: v for k, v in os.environ.items() if k not in ('F110_SCAN_FORM', 'F110_SCAN_ROWS', 'F110_SCAN_CODES')}
    procs, logs = {}, {}
    try:
        for name, (form, codes, _, _, _) in SETTINGS.items():
            e = dict(env, F110_SCAN_FORM=form)
            if codes:
                e['F110_SCAN_CODES'] = codes
            logs[name] = open(str(d / (name + '.log')), 'w+')      # (a file, not a pipe: a talkative child never blocks on it)
            procs[name] = subprocess.Popen([sys.executable, os.path.join(cases.base.TESTS, 'scan_bytes_cases.py'), str(d / (name + '.npz'))],
                                           env=e, stdout=logs[name], stderr=subprocess.STDOUT)
        out = {}
        for name, p in procs.items():
            rc = p.wait(timeout=600)
            logs[name].seek(0)
            assert rc == 0, (name, logs[name].read()[-2000:])
            out[name] = np.load(str(d / (name + '.npz')))
        return out
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
        for lg in logs.values():
            lg.close()


def test_every_child_ran_its_setting(runs):
    for name, (_, _, form, lds, byte) in SETTINGS.items():
        assert int(runs[name]['rows_lds']) == lds and int(runs[name]['codes_byte']) == byte, name
        for case in cases.CASES:
            assert int(runs[name][case + '/form']) == form, (name, case)


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_byte_codes_equal_word_codes_and_the_classic_form(runs, name):
    """Scans (fp32 bits of the kept steps, the sum of bit patterns of every car at every step), collisions, the iTTC flag, done,
    the look-up counts and the noise rows over 40 steps with autoreset; no device error (the bounds build's checks included)."""
    ref = runs['classic']
    B, nb, kind = cases.CASES[name]
    for s in SETTINGS:
        assert int(runs[s][name + '/err']) == 0, (s, hex(int(runs[s][name + '/err'])))
    lk = ref[name + '/lookups'][0].astype(np.int64)
    if kind in ('widths', 'far_car'):
        # the off-map rays keep marching: well over the one look-up per beam of a ray that ends at once
        assert lk.min() > 2 * nb
        sc = ref[name + '/scans0']
        assert np.isfinite(sc).all() and (sc > 0).all()
    if kind == 'far_car':
        # a car that far off reads nothing but the border: every beam marches dt[-1, -1] at a time to max_range, the same count
        far = lk[4:20]
        assert len(np.unique(far)) == 1 and far[0] % nb == 0
    if kind != 'd0':
        assert ref[name + '/lookups'][-1].min() > 0
    for s in ('byte', 'word'):
        g = runs[s]
        for key in KEYS:
            a, b = ref['%s/%s' % (name, key)], g['%s/%s' % (name, key)]
            assert a.dtype == b.dtype and a.shape == b.shape, (s, key)
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (s, key)
