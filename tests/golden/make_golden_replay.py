"""Generates g18_replay.npz: the reference's OWN ReplayBuffer (src/SAL.py:447-463) pushed 0 .. 3 * capacity times for the
capacities of tests/replay_cases.py: len() and the ids of the pushes that survive, in the deque's order.

Dev-container only, like make_golden_shaping.py, whose loader of src/SAL.py (by file path, with empty stand-in modules for cv2,
cvxpy, gym and pyglet) it uses.  The fixture holds recorded results only.

    python tests/golden/make_golden_replay.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import replay_cases as rc  # noqa: E402
from make_golden_shaping import load_reference_sal  # noqa: E402


def main():
    sal = load_reference_sal()
    capacity, pushes, length, ids, offsets = [], [], [], [], [0]
    for cap in rc.FIFO_CAPACITIES:
        for n in range(3 * cap + 1):
            buf = sal.ReplayBuffer(capacity=cap)
            for i in range(n):
                buf.push(np.full((1,), i), np.zeros(1), float(i), np.full((1,), i + 1), False)
            kept = [int(t[2]) for t in buf.buffer]
            assert [int(t[0][0]) for t in buf.buffer] == kept
            capacity.append(cap); pushes.append(n); length.append(len(buf)); ids.extend(kept); offsets.append(len(ids))
    out = os.path.join(HERE, 'g18_replay.npz')
    np.savez_compressed(out, capacity=np.array(capacity, np.int32), pushes=np.array(pushes, np.int32), length=np.array(length, np.int32),
                        ids=np.array(ids, np.int32), offsets=np.array(offsets, np.int32))
    print('wrote %s: %d cases, %d bytes' % (out, len(capacity), os.path.getsize(out)))


if __name__ == '__main__':
    main()
