"""The oracle's composed path (oracle.Env: Simulator.step, F110Env.step / reset / _check_done, update_params, update_map)
against runs of the REFERENCE at off-default configurations: g14, tests/golden/make_golden.py g14_A ... g14_H.

Every record, agent and beam is compared (tests/config_cases.py: compare): every boolean, index, counter, toggle and
`done` ==; lap_times and current_time ==; state <= 1e-12; scans == where no opponent modified the beam and <= 1e-12 where
one did; the set of opponent-modified beams ==.
"""
import numpy as np
import pytest

from config_cases import NAMES, NB, OracleReplay, compare, load_case


def _replay(golden, assets, name):
    case = load_case(golden, name)
    rp = OracleReplay(assets, case)
    seen, sampled = 0, 0
    for op in case.ops():
        got = rp.apply(op)
        if got is None:
            continue
        sampled += bool(compare(case, op[1], got, 1e-12, 1e-12, True, name))
        seen += 1
    assert seen == case.records and sampled == len(case.expected['scan_records'])
    return case


def test_case_A_three_cars_ego_in_the_middle(golden, assets):
    case = _replay(golden, assets, 'A')
    e = case.expected
    assert case.kwargs['ego_idx'] == 1 and ((e['collisions'][:, 2] == 1) & ~e['done']).any() and e['done'][-1]


def test_case_B_pile_up(golden, assets):
    case = _replay(golden, assets, 'B')
    e = case.expected
    assert (e['collisions'][:, :3].sum(axis=1) == 3).any() and (e['collision_idx'][:, 3] == -1).all()


def test_case_C_euler_on_a_5cm_map(golden, assets):
    case = _replay(golden, assets, 'C')
    assert case.kwargs['integrator'] == 'Euler' and case.kwargs['map'] == 'skirk' and case.expected['done'][-1]


def test_case_D_laps_with_three_cars(golden, assets):
    case = _replay(golden, assets, 'D')
    e = case.expected
    assert len(set(e['lap_times'][-1].tolist())) == 3 and not e['collisions'].any() and e['done'][-1]


def test_case_E_update_params(golden, assets):
    case = _replay(golden, assets, 'E')
    assert [c['index'] for c in case.expected['calls']] == [1, -1]


def test_case_F_resets(golden, assets):
    case = _replay(golden, assets, 'F')
    assert len(case.poses) == 3


def test_case_G_update_map(golden, assets):
    case = _replay(golden, assets, 'G')
    assert [c['map'] for c in case.expected['calls']] == ['berlin', 'example_map']


@pytest.mark.parametrize('which', ['H_shared', 'H_own'])
def test_case_H_class_statics(golden, assets, which):
    case = _replay(golden, assets, which)
    other = load_case(golden, 'H_own' if which == 'H_shared' else 'H_shared')
    assert case.records != other.records   # the wall hit comes at another step with the other car's outline
    assert np.array_equal(case.expected['op_arg'][:10], other.expected['op_arg'][:10])


def test_cases_cover_the_configurations(golden):
    """What the fixtures are for: agents 3 and 4, ego_idx 1, 2 and 3, Euler, timesteps 0.005 and 0.02, 0.05 m maps, fov 4.7,
    another seed, non-default vehicles."""
    kws = [load_case(golden, n).kwargs for n in NAMES]
    assert {k['num_agents'] for k in kws} >= {1, 2, 3, 4} and {k['ego_idx'] for k in kws} >= {0, 1, 2, 3}
    assert {k['timestep'] for k in kws} >= {0.005, 0.01, 0.02} and {k['integrator'] for k in kws} == {'RK4', 'Euler'}
    assert {k['map'] for k in kws} >= {'example_map', 'berlin', 'skirk'} and {k['seed'] for k in kws} == {12345, 777}
    assert any(k['fov'] == 4.7 for k in kws) and NB == 1080
