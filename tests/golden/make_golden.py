"""The one way to generate the golden fixtures of this directory, by RUNNING THE REFERENCE (reference.py knows where it
lies and how it loads) where it is present:

    python tests/golden/make_golden.py [--reference DIR] [--out DIR] [--check] [names...]

`names` are rows of TABLE (default: all).  Each row runs in a fresh interpreter -- the reference keeps its scanner in
class statics -- in the table's order, which respects "reads".  --out writes there instead of into this directory; a row
then reads an input fixture from DIR if this call wrote it there, else the committed file.  --check generates into a
temporary directory and compares with the committed files array by array (key set, dtype, shape, bytes), one line per
file, exit status 1 on any difference.

Outputs are data only (inputs + recorded outputs, np.savez_compressed).  The reference itself never travels; tests load
the .npz files.  legacy_scan.npz and lidar_datasets/ are the reference's own data, kept unchanged: no row writes them.
"""
import argparse
import collections
import importlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

import reference

Row = collections.namedtuple('Row', 'name module function args writes reads pin host_dependent note')


def row(name, module, function, writes, reads=(), args=(), pin=False, host_dependent=(), note=''):
    """writes / reads: .npz files (reads: what the generator np.loads); pin: reference.BLAS_PIN in the interpreter's
    environment (the generators from g15 on have always run under it; g1-g14 never have, and g8's recorded actions
    change under it on a host whose BLAS fuses, so they still do not); host_dependent: arrays that --check reports
    instead of comparing."""
    return Row(name, module, function, tuple(args), tuple(writes), tuple(reads), pin, tuple(host_dependent), note)


G20_NOTE = """Does not reproduce across hosts: h, mean, log_std, action and log_prob are fp32 sums of the reference Actor's CPU
convolutions and linears and follow the host's CPU kernel selection (largest differences seen against the committed file:
1.2e-5 in h, 5.6e-4 in log_prob); eps, seed, the weights, the scales and keys reproduce.  The committed file matched none
of: the defaults, ONEDNN_MAX_CPU_ISA=AVX2 / SSE41 / AVX512_CORE, ATEN_CPU_CAPABILITY=avx2 / default / avx512, oneDNN off,
MKL_CBWR=COMPATIBLE / AVX2 / AVX512, MKL_ENABLE_INSTRUCTIONS=AVX2 / SSE4_2, OPENBLAS_CORETYPE=SkylakeX, with one thread
throughout.  Sound for its use all the same: h is stored as an INPUT, and tests/test_policyhead_cpu.py's g20 pin passes
on a regenerated file as on the committed one.  Do not overwrite the committed file without a reason to."""

TABLE = [
    row('g1', 'make_golden_core', 'g1_scan', ['g1_scan.npz']),
    row('g2', 'make_golden_core', 'g2_noise', ['g2_noise.npz']),
    row('g3', 'make_golden_core', 'g3_dynamics', ['g3_dynamics.npz']),
    row('g4', 'make_golden_core', 'g4_gjk', ['g4_gjk.npz']),
    row('g5', 'make_golden_core', 'g5_ttc', ['g5_ttc.npz']),
    row('g6', 'make_golden_core', 'g6_raycast', ['g6_raycast.npz']),
    row('g7', 'make_golden_core', 'g7_sim', ['g7_sim.npz']),
    row('g8', 'make_golden_core', 'g8_env', ['g8_env.npz'], note='about a minute'),
    row('g9', 'make_golden_reference_pins', 'g9_env2', ['g9_env2.npz'], note='about two minutes'),
    row('g10', 'make_golden_reference_pins', 'g10_bitmap_calls', ['g10_bitmap_calls.npz'], reads=['g1_scan.npz', 'g8_env.npz']),
    row('g11', 'make_golden_reference_pins', 'g11_centerline', ['g11_centerline.npz']),
    row('g12', 'make_golden_reference_pins', 'g12_pointgrid', ['g12_pointgrid.npz'], note='runs on the older package copy'),
    row('g13', 'make_golden_raycast_edges', 'g13_raycast_edges', ['g13_raycast_edges.npz']),
] + [
    row('g14_' + c, 'make_golden_configs', 'record', ['g14_%s.npz' % f for f in files], args=[c])
    for c, files in (('A', 'A'), ('B', 'B'), ('C', 'C'), ('D', 'D'), ('E', 'E'), ('F', 'F'), ('G', 'G'), ('H', ('H_shared', 'H_own')))
] + [
    row('g15', 'make_golden_progress', 'g15_nearest', ['g15_nearest.npz'], reads=['g8_env.npz'], pin=True),
    row('g16', 'make_golden_shaping', 'g16_shaping', ['g16_shaping.npz'], reads=['g8_env.npz', 'g10_bitmap_calls.npz'], pin=True,
        note='asserts that the file is smaller than g6_raycast.npz'),
    row('g17', 'make_golden_paths', 'g17_paths', ['g17_paths.npz'], pin=True, note='asserts that the file is smaller than half of g6_raycast.npz'),
    row('g18', 'make_golden_replay', 'g18_replay', ['g18_replay.npz'], pin=True),
    row('g19', 'make_golden_path_configs', 'g19_path_configs', ['g19_path_configs.npz'], pin=True,
        note='asserts that the file is smaller than g17_paths.npz'),
    row('g20', 'make_golden_head', 'g20_head', ['g20_head.npz'], pin=True,
        host_dependent=['h', 'mean', 'log_std', 'action', 'log_prob'], note=G20_NOTE),
    row('g21', 'make_golden_critic', 'g21_critic', ['g21_critic.npz'], pin=True),
    row('g22', 'make_golden_trunk', 'g22_trunk', ['g22_trunk.npz', 'g22_trunk_unit.npz'], pin=True),
    row('g23', 'make_golden_dense', 'g23_dense', ['g23_dense.npz'], reads=['g22_trunk.npz', 'g22_trunk_unit.npz'], pin=True),
    row('g24', 'make_golden_update', 'g24_update', ['g24_update.npz'], pin=True),
]
ROWS = {r.name: r for r in TABLE}


def resolve(r):
    """The row's generator; importing its module loads nothing of the reference."""
    return getattr(importlib.import_module(r.module), r.function)


def generate(names, root, out):
    """Runs the rows `names` in the table's order, each in an interpreter of its own."""
    fresh = []
    for r in TABLE:
        if r.name not in names:
            continue
        env = dict(os.environ, **{reference.ROOT_ENV: root})
        if r.pin:
            env.setdefault(*reference.BLAS_PIN)
        t = time.time()
        print('==', r.name, flush=True)
        subprocess.run([sys.executable, os.path.abspath(__file__), '--out', out, '--child', r.name] + fresh, env=env, check=True)
        print('   %.1fs' % (time.time() - t), flush=True)
        fresh += r.writes


def differences(r, name, out):
    """(diffs, notes) of the committed file `name` against the one in `out`: what differs, [] if nothing does, and, for the
    row's host-dependent arrays, which are compared in dtype and shape only, each one's largest absolute difference."""
    a, b = np.load(os.path.join(reference.HERE, name)), np.load(os.path.join(out, name))
    diffs, notes = [], []
    if sorted(a.files) != sorted(b.files):
        diffs.append('keys %s' % sorted(set(a.files) ^ set(b.files)))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            diffs.append('%s: %s %s -> %s %s' % (k, x.dtype, x.shape, y.dtype, y.shape))
        elif k in r.host_dependent:
            notes.append('%s %.2g' % (k, np.abs(x.astype(np.float64) - y).max()))
        elif x.tobytes() != y.tobytes():
            diffs.append('%s: bytes' % k)
    return diffs, notes


def check(names, root):
    bad = 0
    with tempfile.TemporaryDirectory() as out:
        generate(names, root, out)
        for r in TABLE:
            for name in r.writes if r.name in names else ():
                diffs, notes = differences(r, name, out)
                line = 'DIFFERENT: ' + '; '.join(diffs) if diffs else 'same'
                if notes:
                    line += ', but for the host-dependent arrays (see the row\'s note), largest |difference|: ' + ', '.join(notes)
                print('%-24s %s' % (name, line))
                bad += bool(diffs)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', metavar='DIR', default=reference.path(), help='the reference\'s root (default: $%s, else %s)'
                    % (reference.ROOT_ENV, reference.DEFAULT_ROOT))
    ap.add_argument('--out', metavar='DIR', default=reference.HERE)
    ap.add_argument('--check', action='store_true')
    ap.add_argument('--child', metavar='ROW', help=argparse.SUPPRESS)   # internal: run ROW here; names = the files written so far
    ap.add_argument('names', nargs='*')
    args = ap.parse_args()
    if args.child:
        reference.OUT, reference.FRESH = args.out, set(args.names)
        r = ROWS[args.child]
        return resolve(r)(*r.args)
    unknown = [n for n in args.names if n not in ROWS]
    if unknown:
        ap.error('no such row: %s (rows: %s)' % (' '.join(unknown), ' '.join(ROWS)))
    names = args.names or list(ROWS)
    if args.check:
        return check(names, args.reference)
    os.makedirs(args.out, exist_ok=True)
    generate(names, args.reference, args.out)


if __name__ == '__main__':
    sys.exit(main())
