"""The compact forms of the step's scan (one-wave workgroups, LDS images of 256 / 512 LUT slots, their own cell tables:
csrc/f110_scan.h, f110_scan_plan.h) against the classic form, `==` on everything a caller sees.  F110_SCAN_FORM is read once
per process, so each form rolls the cases of scan_compact_cases.py out in a child process of its own (the three run side by
side).  Run against the bounds-checked build (F110_LIB, tests/test_gpu_bounds.py) the same tests hold its error word clean:
the children inherit the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_compact_cases as cases

pytestmark = pytest.mark.gpu

FORMS = {'classic': 0, 'compact256': 256, 'compact512': 512}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """form -> the arrays of its child; 'rule': F110_SCAN_FORM unset, the cases of cases.RULE_CASES."""
    d = tmp_path_factory.mktemp('scan_compact')
    env = {k: v for k, v in os.environ.items() if k != 'F110_SCAN_FORM'}
    jobs = [(f, dict(env, F110_SCAN_FORM=f), []) for f in FORMS] + [('rule', env, [','.join(cases.RULE_CASES)])]
    procs, logs = {}, {}
    try:
        for f, e, extra in jobs:
            logs[f] = open(str(d / (f + '.log')), 'w+')      # (a file, not a pipe: a talkative child never blocks on it)
            procs[f] = subprocess.Popen([sys.executable, os.path.join(cases.TESTS, 'scan_compact_cases.py'), str(d / (f + '.npz'))] + extra,
                                        env=e, stdout=logs[f], stderr=subprocess.STDOUT)
        out = {}
        for f, p in procs.items():
            rc = p.wait(timeout=600)
            logs[f].seek(0)
            assert rc == 0, (f, logs[f].read()[-2000:])
            out[f] = np.load(str(d / (f + '.npz')))
        return out
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
        for lg in logs.values():
            lg.close()


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_compact_equals_classic(runs, name):
    """Scans (fp32 bits), collisions, the iTTC flag, done and the look-up counts over 40 steps with autoreset; every child
    really ran its form, and no device error (the bounds build's index checks included)."""
    ref = runs['classic']
    assert int(ref[name + '/form']) == 0 and int(ref[name + '/err']) == 0
    B, nb, kind = cases.CASES[name]
    if kind == 'masked_resets':
        assert len(np.unique(ref[name + '/rows'])) > 1            # envs on different rows of the shared table
    if kind == 'noise_per_env':                                   # every env its own generator: no two cars see the same noise
        first = ref[name + '/scans0']
        assert len({first[i].tobytes() for i in range(len(first))}) == len(first)
    for f in ('compact256', 'compact512'):
        g = runs[f]
        assert int(g[name + '/form']) == FORMS[f], f
        assert int(g[name + '/err']) == 0, (f, hex(int(g[name + '/err'])))
        for key in ['sums', 'col', 'done', 'lookups', 'rows'] + ['scans%d' % k for k in cases.KEEP]:
            a, b = ref['%s/%s' % (name, key)], g['%s/%s' % (name, key)]
            assert a.dtype == b.dtype and a.shape == b.shape, (f, key)
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (f, key)
    assert ref[name + '/lookups'][-1].min() > 0


def test_rank_boundary_map_against_the_oracle(runs):
    """The synthetic map's cells carry the ranks S - 3 .. S for S = 256 and 512 (S - 2 is the first behind the marker of S) and
    one escape cell; the cars' rays cross every one of them at their first step already, and every form gives the oracle's scan."""
    import oracle
    d2, dt, esc = cases.boundary_map()
    assert np.array_equal(np.unique(d2)[:600], np.arange(600))    # a cell's rank is its value
    B, nb, _ = cases.CASES['boundary']
    poses = cases.boundary_poses(B)
    sc = oracle.Scanner(nb, 2 * np.pi)
    H, W = dt.shape
    sc.set_map_dict({'height': H, 'width': W, 'resolution': cases.RES, 'orig_x': 0.0, 'orig_y': 0.0, 'orig_c': 1.0, 'orig_s': 0.0,
                     'dt': np.ascontiguousarray(dt)})
    # the first look-up of every beam past the car's own cell: which cells it lands on
    ang = poses[:, 0, 2, None] - np.pi + np.arange(nb) * (2 * np.pi / (nb - 1))
    ci, ri = np.floor(poses[:, 0, 0] / cases.RES).astype(int), np.floor(poses[:, 0, 1] / cases.RES).astype(int)
    d0 = dt[ri, ci][:, None]
    x1, y1 = poses[:, 0, 0, None] + d0 * np.cos(ang), poses[:, 0, 1, None] + d0 * np.sin(ang)
    c1, r1 = np.floor(x1 / cases.RES).astype(int), np.floor(y1 / cases.RES).astype(int)
    ok = (c1 >= 0) & (c1 < W) & (r1 >= 0) & (r1 < H)
    hit = set(d2[r1[ok], c1[ok]].tolist())
    assert {253, 254, 255, 256, 509, 510, 511, 512} <= hit
    assert (ri[0], ci[0]) == esc                                  # car 0 stands on the escape cell: its beams' first look-up
    # the oracle's envs: zero actions, so every step scans the spawn pose with the next noise row
    noise = oracle.noise_table(12345, cases.T + 4, nb)
    envs = [oracle.Env(sc, 1, noise=noise) for _ in range(B)]
    for b in range(B):
        envs[b].reset(poses[b])
    want = {}
    for k in range(cases.T):
        obs = [envs[b].step(np.zeros((1, 2))) for b in range(B)]
        if k in cases.KEEP:
            want[k] = np.stack([o['scans'][0] for o in obs]).astype(np.float32)
    for f in FORMS:
        for k in cases.KEEP:
            assert np.array_equal(runs[f]['boundary/scans%d' % k], want[k]), (f, k)


def test_the_rule_routes_example_map_and_not_a_wide_road(runs):
    """F110_SCAN_FORM unset, 32 768 x 1.  On example_map the scan is classic and the shares unknown until the first reset of all
    envs has learnt them; then the form is 256, the launch epoch has moved, and everything `==` the classic child.  Berlin's mask
    re-installed at 0.0625 m (a road of more than 2 x 25 cells) learns shares over the cap and stays classic."""
    g, ref = runs['rule'], runs['classic']
    n = 'cars32768'
    assert int(g[n + '/form_before']) == 0 and g[n + '/shares_before'][2:].tolist() == [-1.0, -1.0]
    assert int(g[n + '/form']) == 256 and int(g[n + '/epoch_moved']) == 1 and int(g[n + '/err']) == 0
    whole, reach = g[n + '/shares'][:2], g[n + '/shares'][2:]
    assert (whole > 0.8).all()                 # most free cells of the map lie behind both markers: open ground ...
    assert (reach >= 0).all() and (reach < 0.001).all()           # ... which next to none of the cars can reach
    assert int(ref[n + '/form']) == 0
    for key in ['sums', 'col', 'done', 'lookups', 'rows'] + ['scans%d' % k for k in cases.KEEP]:
        a, b = ref['%s/%s' % (n, key)], g['%s/%s' % (n, key)]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), key
    assert int(g['wide/form_before']) == 0 and int(g['wide/form']) == 0 and int(g['wide/err']) == 0
    reach = g['wide/shares'][2:]
    assert int(g['wide/epoch_moved']) == 1 and (reach > 0.02).all() and reach[0] > 0.2      # learnt, and over the cap of 0.004
