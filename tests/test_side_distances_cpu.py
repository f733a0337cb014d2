"""Side distances per vehicle, the part that needs no device: the premise of tests/test_gpu_side_distances.py (the two
readings of "num_envs reference envs" -- one process's class statics / independently constructed envs -- really give
different collision histories in the scenario used there), the tables Engine builds for a slot against the oracle's, and
the ABI declarations."""
import os

import numpy as np

import oracle
from side_distance_cases import VEHICLES, WALL_ENVS, Scanners, batch, differs, oracle_history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_tables_of_every_test_vehicle_are_the_oracles():
    """Engine builds a slot's table with engine.beam_tables (NumPy, the reference's operands); the oracle's Scanner builds
    its own in C.  For the vehicles of these tests the two are the same bits, so `==` on collisions is a fair demand."""
    from red_gym_amd.engine import beam_tables
    for p in VEHICLES:
        side = beam_tables(1080, 2 * np.pi, p)[2]
        sc = oracle.Scanner(1080, 2 * np.pi, params=p)
        assert np.array_equal(side, sc.side_distances)
    big, small = (beam_tables(1080, 2 * np.pi, p)[2] for p in VEHICLES[1:])
    dflt = beam_tables(1080, 2 * np.pi, VEHICLES[0])[2]
    assert (big > dflt).all() and (small < dflt).all()


def test_own_scanner_and_shared_scanner_histories_differ(assets):
    """The scenario of the GPU step-path test can fail: for at least one env of EACH non-default vehicle, an oracle env on
    its own scanner and one on env 0's scanner disagree in `collisions` or `done` at some step (the larger car's wall hit
    comes earlier with its own outline, the smaller car's later); envs on the default vehicle never disagree."""
    for A in (1, 2):
        B, T = 12, 90
        env_par, poses, acts = batch(B, A)
        scs = Scanners(assets)
        noise = oracle.noise_table(12345, T + 4)
        own = oracle_history(lambda e: scs.of(env_par[e]), env_par, poses, acts, T, A, noise)
        shared = oracle_history(lambda e: scs.of(env_par[0]), env_par, poses, acts, T, A, noise)
        first = {e: differs(own[e], shared[e]) for e in range(B)}
        print('A=%d first differing step per env: %s' % (A, first))
        for v in (1, 2):
            assert any(first[e] is not None for e in range(B) if e % 3 == v), (A, v, first)
        assert all(first[e] is None for e in range(B) if e % 3 == 0)
        wall = range(B)[WALL_ENVS]
        assert sum(int(own[e]['done'].any()) for e in wall) >= 4     # the steered envs do hit the wall and reset
        # the larger car is stopped EARLIER by its own table than by the default car's
        e_big = next(e for e in wall if e % 3 == 1 and first[e] is not None)
        assert own[e_big]['collisions'][first[e_big]].any() and not shared[e_big]['collisions'][first[e_big]].any()


def test_header_binding_and_docs_name_the_new_entry_points():
    from red_gym_amd import _lib
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()        # (the header against the binding: tests/test_abi_cpu.py)
    for name, nargs in (('f110_set_side_distance_slots', 3), ('f110_check_ttc_slots', 7)):
        assert len(_lib.SYMBOLS[name]) == nargs and name in integ

