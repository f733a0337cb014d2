"""Generates g18_replay.npz: the reference's OWN ReplayBuffer (src/SAL.py:447-463) pushed 0 .. 3 * capacity times for the
capacities of tests/replay_cases.py: len() and the ids of the pushes that survive, in the deque's order.

Run through make_golden.py, with g16's loader of src/SAL.py (reference.load_sal(): by file path, with empty stand-in modules
for cv2, cvxpy, gym and pyglet).  The fixture holds recorded results only.
"""
import numpy as np

import reference
import replay_cases as rc


def g18_replay():
    sal = reference.load_sal()
    capacity, pushes, length, ids, offsets = [], [], [], [], [0]
    for cap in rc.FIFO_CAPACITIES:
        for n in range(3 * cap + 1):
            buf = sal.ReplayBuffer(capacity=cap)
            for i in range(n):
                buf.push(np.full((1,), i), np.zeros(1), float(i), np.full((1,), i + 1), False)
            kept = [int(t[2]) for t in buf.buffer]
            assert [int(t[0][0]) for t in buf.buffer] == kept
            capacity.append(cap); pushes.append(n); length.append(len(buf)); ids.extend(kept); offsets.append(len(ids))
    reference.save('g18_replay.npz', capacity=np.array(capacity, np.int32), pushes=np.array(pushes, np.int32), length=np.array(length, np.int32),
                   ids=np.array(ids, np.int32), offsets=np.array(offsets, np.int32))
    print('  %d cases' % len(capacity))
