"""The recorded reference runs of tests/golden/g14_<case>.npz (make_golden.py g14_<case>), for replay through the oracle
(test_oracle_configs.py) and through the C ABI (test_gpu_configs.py).  A plain module, not a conftest.

load_case(golden, name) -> Case(kwargs, poses, actions, expected) plus what a replay needs around them:
    kwargs    the reference constructor's keywords (map as a bare name, integrator as 'RK4' / 'Euler')
    poses     the poses of every reset, in order
    actions   [R, A, 2] the action of every step record (zeros at reset records)
    expected  the arrays the reference produced, one row per record (a record = one reset or one step)
    case.ops()  every operation in order: ('update_params', params, index), ('update_map', name), ('reset', r, poses),
                ('step', r, action) with r the record the operation produces
compare(...) holds every assertion; both test files call it for every record, agent and beam.
"""
import collections
import json
import os

import numpy as np

NB = 1080
NAMES = ['A', 'B', 'C', 'D', 'E', 'F', 'G', 'H_shared', 'H_own']
RESET, STEP = 0, 1
PER_RECORD = ('state', 'scan_pose', 'collisions', 'collision_idx', 'toggles', 'lap_counts', 'lap_times',
              'checkpoint_done', 'done', 'current_time')


class Case(collections.namedtuple('Case', 'kwargs poses actions expected')):
    def ops(self):
        calls = collections.defaultdict(list)
        for c in self.expected['calls']:
            calls[c['before']].append(c)
        kind, arg = self.expected['op_kind'], self.expected['op_arg']
        for r in range(len(kind)):
            for c in calls[r]:
                if c['call'] == 'update_params':
                    yield ('update_params', c['params'], c['index'])
                else:
                    yield ('update_map', c['map'])
            if kind[r] == RESET:
                yield ('reset', r, arg[r].copy())
            else:
                yield ('step', r, arg[r, :, :2].copy())

    @property
    def records(self):
        return len(self.expected['op_kind'])

    @property
    def noise_rows(self):
        """The noise row every record's scans carry: 0 at a reset (its zero-action step), then counting up."""
        rows, n = [], 0
        for k in self.expected['op_kind']:
            n = 0 if k == RESET else n + 1
            rows.append(n)
        return np.array(rows)

    def ctor(self):
        """kwargs without the bookkeeping entry of case H (whose params fixed the class statics)."""
        return {k: v for k, v in self.kwargs.items() if k != 'statics_params'}

    @property
    def table_params(self):
        return self.kwargs.get('statics_params', self.kwargs['params'])


def load_case(golden, name):
    g = golden('g14_%s.npz' % name)
    exp = {k: g[k] for k in g.files}
    kw = json.loads(str(exp.pop('kwargs')))
    exp['calls'] = json.loads(str(exp['calls']))
    A = kw['num_agents']
    exp['opp_mod'] = np.unpackbits(exp['opp_mod'], axis=-1)[..., :NB].astype(bool)
    assert exp['scans'].shape == (len(exp['scan_records']), A, NB) == exp['opp_mod'].shape
    kind, arg = exp['op_kind'], exp['op_arg']
    poses = [arg[r].copy() for r in range(len(kind)) if kind[r] == RESET]
    actions = np.where((kind == STEP)[:, None, None], arg[:, :, :2], 0.0)
    return Case(kw, poses, actions, exp)


def map_yaml(assets, name):
    return os.path.join(assets, 'example_map.yaml') if name == 'example_map' else os.path.join(assets, 'maps', name + '.yaml')


def map_arg(assets, name):
    """The `map` keyword: packaged names as they are, example_map as a path without extension (f110_env.py:106-118)."""
    return os.path.join(assets, 'example_map') if name == 'example_map' else name


def compare(case, r, got, state_tol, scan_tol, exact_unmodified, tag=''):
    """One record of a replay against the reference.  got: dict with the PER_RECORD keys (scan_pose optional) and, at a
    sampled record, 'scans' [A, nb] fp64 and 'opp_mod' [A, nb] bool (beams whose value differs from the map scan plus
    noise at the scan pose).  Flags, indices, counters, toggles, done, lap_times and current_time ==; state within
    state_tol; scans within scan_tol, and == on beams no opponent modified when exact_unmodified."""
    e = case.expected
    where = '%s record %d' % (tag, r)
    for k in ('collisions', 'collision_idx', 'toggles', 'lap_counts', 'checkpoint_done'):
        assert np.array_equal(np.asarray(got[k], dtype=np.float64), e[k][r].astype(np.float64)), (where, k, got[k], e[k][r])
    assert bool(got['done']) == bool(e['done'][r]), (where, 'done')
    assert np.array_equal(np.asarray(got['lap_times'], dtype=np.float64), e['lap_times'][r]), (where, 'lap_times', got['lap_times'], e['lap_times'][r])
    assert float(got['current_time']) == e['current_time'][r], (where, 'current_time', got['current_time'], e['current_time'][r])
    d = np.abs(np.asarray(got['state']) - e['state'][r]).max()
    assert d <= state_tol, (where, 'state', d)
    if 'scan_pose' in got:
        d = np.abs(np.asarray(got['scan_pose']) - e['scan_pose'][r]).max()
        assert d <= state_tol, (where, 'scan_pose', d)
    s = np.nonzero(e['scan_records'] == r)[0]
    if len(s) == 0:
        return False
    want, mod = e['scans'][s[0]], e['opp_mod'][s[0]]
    assert 'scans' in got, (where, 'sampled record without scans')
    sc = np.asarray(got['scans'])
    d = np.abs(sc - want).max()
    assert d <= scan_tol, (where, 'scans', d)
    if exact_unmodified:
        assert np.array_equal(sc[~mod], want[~mod]), (where, 'unmodified beams', np.abs(sc - want)[~mod].max())
    assert np.array_equal(np.asarray(got['opp_mod']), mod), (where, 'opponent-modified beams',
                                                             np.argwhere(np.asarray(got['opp_mod']) != mod)[:5])
    return True


class OracleReplay(object):
    """One oracle.Env driven by a case's operations.  The beam tables come from the params that fixed the reference's
    class statics (case H: another env's)."""

    def __init__(self, assets, case):
        import oracle
        self.oracle, self.assets, self.case = oracle, assets, case
        kw = case.kwargs
        self.scanner = oracle.Scanner(NB, kw['fov'], params=case.table_params)
        self.scanner.set_map(map_yaml(assets, kw['map']), '.png')
        self.noise = oracle.noise_table(kw['seed'], int(case.noise_rows.max()) + 2)
        self.env = oracle.Env(self.scanner, kw['num_agents'], params=kw['params'], time_step=kw['timestep'],
                              integrator=getattr(oracle, kw['integrator'].upper()), ego_idx=kw['ego_idx'], noise=self.noise)
        self.map_scanner = self.scanner   # follows update_map, for the map scan of the opponent-modified test

    def apply(self, op):
        """Returns the record's observation for 'reset' / 'step', None for the update calls."""
        if op[0] == 'update_params':
            self.env.update_params(op[1], op[2])
        elif op[0] == 'update_map':
            self.env.update_map(map_yaml(self.assets, op[1]), '.png')
            self.map_scanner = self.oracle.Scanner(NB, self.case.kwargs['fov'])
            self.map_scanner.set_map(map_yaml(self.assets, op[1]), '.png')
        elif op[0] == 'reset':
            return self._got(op[1], self.env.reset(op[2]))
        else:
            return self._got(op[1], self.env.step(op[2]))

    def _got(self, r, o):
        got = {k: o[k] for k in ('state', 'collisions', 'collision_idx', 'toggles', 'lap_counts', 'lap_times', 'done',
                                 'current_time', 'scans')}
        got['scan_pose'] = o['scan_poses']
        got['checkpoint_done'] = o['toggles'] >= 4
        got['opp_mod'] = o['scans'] != self.map_scan(o['scan_poses'], r)
        return got

    def map_scan(self, scan_poses, r):
        """What every car's scan is before check_ttc / ray_cast_agents: the map scan at its pose plus its noise row."""
        return self.map_scanner.scan_batch(scan_poses) + self.noise[self.case.noise_rows[r]]
