"""The row buffer of the compact scan form (csrc/f110_scan.h: scan_kernel<.., 256, true>; f110_scan_plan.h: scan_rowbuf_plan):
fp32 rows staged in LDS and written out by chunk, against the same form with direct stores and against the classic form, `==`
on everything a caller sees.  F110_SCAN_FORM and F110_SCAN_ROWS are read once per process, so each setting rolls the cases of
scan_rowbuf_cases.py out in a child process of its own (the three run side by side).  Run against the bounds-checked build
(F110_LIB, tests/test_gpu_bounds.py) the same tests hold its error word clean -- the slot and the LDS offset of every staged
beam and the beam of every store of the write-out, the last car's included: the children inherit the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_rowbuf_cases as cases

pytestmark = pytest.mark.gpu

# setting -> (F110_SCAN_FORM, F110_SCAN_ROWS, the form it must launch, whether it stages rows)
SETTINGS = {'lds': ('compact256', 'lds', 256, 1), 'direct': ('compact256', 'direct', 256, 0), 'classic': ('classic', None, 0, 0)}
KEYS = ['sums', 'col', 'done', 'lookups', 'rows'] + ['scans%d' % k for k in cases.base.KEEP]


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """setting -> the arrays of its child."""
    d = tmp_path_factory.mktemp('scan_rowbuf')
    env = {k: v for k, v in os.environ.items() if k not in ('F110_SCAN_FORM', 'F110_SCAN_ROWS')}
    procs, logs = {}, {}
    try:
        for name, (form, rows, _, _) in SETTINGS.items():
            e = dict(env, F110_SCAN_FORM=form)
            if rows:
                e['F110_SCAN_ROWS'] = rows
            logs[name] = open(str(d / (name + '.log')), 'w+')      # (a file, not a pipe: a talkative child never blocks on it)
            procs[name] = subprocess.Popen([sys.executable, os.path.join(cases.base.TESTS, 'scan_rowbuf_cases.py'), str(d / (name + '.npz'))],
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
    for name, (_, _, form, lds) in SETTINGS.items():
        assert int(runs[name]['rows_lds']) == lds, name
        for case in cases.CASES:
            assert int(runs[name][case + '/form']) == form, (name, case)


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_staged_rows_equal_direct_stores_and_the_classic_form(runs, name):
    """Scans (fp32 bits of the kept steps, the sum of bit patterns of every car at every step), collisions, the iTTC flag, done,
    the look-up counts and the noise rows over 40 steps with autoreset; no device error (the bounds build's checks included)."""
    ref = runs['classic']
    B, nb, kind = cases.CASES[name]
    for s in SETTINGS:
        assert int(runs[s][name + '/err']) == 0, (s, hex(int(runs[s][name + '/err'])))
    if kind == 'masked_resets':
        assert len(np.unique(ref[name + '/rows'])) > 1            # envs on different rows of the shared table
    if kind == 'd0':
        # the cars on an occupied cell and off the map read the table once per beam and never march; the others do
        lk = ref[name + '/lookups'][0].astype(np.int64)
        still = np.zeros(B, dtype=bool)
        still[cases.D0_OCCUPIED] = still[cases.D0_OFF_MAP] = True
        assert len(np.unique(lk[still])) == 1 and lk[still][0] % nb == 0 and lk[still][0] > 0
        moving = ~still
        moving[cases.D0_NAN] = False
        assert lk[moving].min() > lk[still][0]
    else:
        assert ref[name + '/lookups'][-1].min() > 0
    for s in ('lds', 'direct'):
        g = runs[s]
        for key in KEYS:
            a, b = ref['%s/%s' % (name, key)], g['%s/%s' % (name, key)]
            assert a.dtype == b.dtype and a.shape == b.shape, (s, key)
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (s, key)
