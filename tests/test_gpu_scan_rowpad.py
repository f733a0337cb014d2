"""The march without a row clamp on the row-padded byte cell table (csrc/f110_scan.h: march_ident_pow2_fast<true>, MapView::
init_bytes; f110_map.h: cell_elem_bp): the compact form of 256 slots on its byte table against the same form on its u16 table
and against the classic form, `==` on everything a caller sees.  F110_SCAN_FORM and F110_SCAN_CODES are read once per process, so
each setting rolls the cases of scan_rowpad_cases.py out in a child process of its own (the three run side by side).  Run against
the bounds-checked build (F110_LIB, tests/test_gpu_bounds.py) the same tests hold its error word clean -- every look-up's offset
inside the padded table: the children inherit the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_rowpad_cases as cases

pytestmark = pytest.mark.gpu

# setting -> (F110_SCAN_FORM, F110_SCAN_CODES, the form it must launch, whether it stages rows, whether it reads bytes)
SETTINGS = {'byte': ('compact256', 'byte', 256, 1, 1), 'word': ('compact256', 'word', 256, 1, 0), 'classic': ('classic', None, 0, 0, 0)}
KEYS = ('scans', 'sums', 'col', 'ittc', 'done', 'lookups', 'rows')


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """setting -> the arrays of its child."""
    d = tmp_path_factory.mktemp('scan_rowpad')
    env = {k: v for k, v in os.environ.items() if k not in ('F110_SCAN_FORM', 'F110_SCAN_ROWS', 'F110_SCAN_CODES')}
    procs, logs = {}, {}
    try:
        for name, (form, codes, _, _, _) in SETTINGS.items():
            e = dict(env, F110_SCAN_FORM=form)
            if codes:
                e['F110_SCAN_CODES'] = codes
            logs[name] = open(str(d / (name + '.log')), 'w+')      # (a file, not a pipe: a talkative child never blocks on it)
            procs[name] = subprocess.Popen([sys.executable, os.path.join(cases.TESTS, 'scan_rowpad_cases.py'), str(d / (name + '.npz'))],
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
    """... on a table with the padding rows of its max_range (every child builds it; only 'byte' reads it), and without that
    table on word codes whatever it was asked for."""
    for name, (_, _, form, lds, byte) in SETTINGS.items():
        for case, (mr, _, _, _, _) in cases.CASES.items():
            g = runs[name]
            P = cases.PAD_ROWS[mr]
            assert (int(g[case + '/form']), int(g[case + '/rows_lds']), int(g[case + '/codes_byte'])) == (form, lds, byte if P >= 0 else 0), (name, case)
            assert int(g[case + '/pad_rows']) == P, (name, case)


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_byte_codes_without_row_clamp_equal_word_codes_and_the_classic_form(runs, name):
    """Scans (fp32 bits of every car at every step, and their sums of bit patterns), collisions, the iTTC flag, done, the look-up
    counts and the noise rows; no device error (the bounds build's checks included)."""
    ref = runs['classic']
    mr, H, W, kind, pk = cases.CASES[name]
    nb = cases.BEAMS
    for s in SETTINGS:
        assert int(runs[s][name + '/err']) == 0, (s, hex(int(runs[s][name + '/err'])))
    lk = ref[name + '/lookups'][1].astype(np.int64) - ref[name + '/lookups'][0].astype(np.int64)   # of one step (the counters add up)
    sc = ref[name + '/scans'][0]
    assert np.isfinite(sc).all()
    if pk == 'edge' and kind == 'free':
        # off the map the rays keep marching, dt[-1, -1] at a time, through the padding rows: well over the one look-up per beam
        # of a ray that ends at once, and the beam straight out reads max_range (noise: 0.01 m standard deviation)
        for car in (cases.OUT_DOWN, cases.OUT_UP, cases.ROW_M1, cases.ROW_H, cases.ROW_M2, cases.ROW_H1) + cases.FAR_X + cases.FAR_Y:
            assert lk[car] > 2 * nb, car
        for car in (cases.OUT_DOWN, cases.OUT_UP):
            assert abs(float(sc[car, nb // 2]) - mr) < 0.1, car
        # a car that far off reads nothing but the border: every beam the same count
        far = lk[list(cases.FAR_X + cases.FAR_Y)]
        assert len(np.unique(far)) == 1 and far[0] % nb == 0
    if pk == 'edge' and kind == 'zero':
        # dt[-1, -1] = 0: the first look-up off the map ends the ray -- the cars that stand off the map make one per beam
        for car in (cases.ROW_M1, cases.ROW_H, cases.ROW_M2, cases.ROW_H1) + cases.FAR_X + cases.FAR_Y:
            assert lk[car] == nb, car
    if pk == 'field':
        # car 0 stands behind the 256-slot marker, facing up: the far step of ~60 cells takes its middle beam out of the map
        assert float(sc[0, nb // 2]) > (cases.FIELD - 1) * cases.RES and lk[0] > nb
    for s in ('byte', 'word'):
        g = runs[s]
        for key in KEYS:
            a, b = ref['%s/%s' % (name, key)], g['%s/%s' % (name, key)]
            assert a.dtype == b.dtype and a.shape == b.shape, (s, key)
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (s, key)
