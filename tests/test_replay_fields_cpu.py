"""The field table of a replay batch (red_gym_amd.replay.sample_fields) without a device: the exact key set, shapes and dtypes for n = 5
transitions of 2 action values at nstep 1 and 3, with and without priorities, at stack 1 and 3 -- written out here, not computed from the
function: the names are what sample_out allocates, what the sampling entries return beside 'frames', and what SACAgent reads."""
import pytest

N, ACTION_DIM, STACK = 5, 2, 3

BASE = {'indices': ((5,), 'int64'), 's_idx': ((5,), 'int64'), 'ns_idx': ((5,), 'int64'), 'a': ((5, 2), 'float32'), 'r': ((5,), 'float64'),
        'd': ((5,), 'uint8'), 'ok': ((5,), 'uint8')}
WALK = {'discount': ((5,), 'float64'), 'span': ((5,), 'int32')}                  # nstep > 1, and always from the priority draw
PRIO = {'prio': ((5,), 'int32'), 'weight': ((5,), 'float32')}                    # the priority draw only
STACKS = {'pair': ((2, 5), 'int64'), 'stacks': ((2, 5, 3), 'int64'), 's_stack': ((5, 3), 'int64'), 'ns_stack': ((5, 3), 'int64'),
          'depth': ((2, 5), 'int32')}                                            # stack > 1; s_idx and ns_idx stay [5]

# (nstep, priorities, stack) -> the table
TABLE = {
    (1, False, 1): {**BASE},
    (3, False, 1): {**BASE, **WALK},
    (1, True, 1): {**BASE, **WALK, **PRIO},
    (3, True, 1): {**BASE, **WALK, **PRIO},
    (1, False, 3): {**BASE, **STACKS},
    (3, False, 3): {**BASE, **WALK, **STACKS},
    (1, True, 3): {**BASE, **WALK, **PRIO, **STACKS},
    (3, True, 3): {**BASE, **WALK, **PRIO, **STACKS},
}
COMBOS = sorted(TABLE)


def test_the_table_has_the_sizes_it_names():
    assert len(TABLE) == 8 and [len(TABLE[c]) for c in COMBOS] == [7, 12, 11, 16, 9, 14, 11, 16]


@pytest.mark.parametrize('nstep,priorities,stack', COMBOS)
def test_sample_fields_is_the_table(nstep, priorities, stack):
    import torch
    from red_gym_amd.replay import sample_fields
    got = sample_fields(N, ACTION_DIM, nstep, priorities, stack)
    want = {k: (shape, getattr(torch, dt)) for k, (shape, dt) in TABLE[(nstep, priorities, stack)].items()}
    assert sorted(got) == sorted(want)
    for k in want:
        assert (tuple(got[k][0]), got[k][1]) == want[k], k
    # the defaults are the plain one-step batch, and a second call returns a table of its own
    assert sample_fields(N, ACTION_DIM) == sample_fields(N, ACTION_DIM, 1, False, 1) and sample_fields(N, ACTION_DIM) is not sample_fields(N, ACTION_DIM)
