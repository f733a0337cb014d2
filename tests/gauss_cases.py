"""The checker of the policy's Gaussian draws (csrc/f110_gauss.h) and its table of cases.  The checker is NumPy itself: element
(row r, column j) of call t of stream s under seed is the first standard_normal() of Generator(Philox(key=[seed, s], counter=[0, j, r,
t])), rounded once to fp32 -- the contract of include/f110_hip.h -- so nothing is recorded and every comparison is `==` on bits.
words_used reads, from the bit generator's state behind the draw, how many raw words the element took: the elements that took more
than one (a wedge test, a rejected trial, the tail) and those that crossed into the second Philox block are what a test must have met
before its `==` means anything, and require() asserts that from the reference alone."""
import functools

import numpy as np

TAIL = 3.6541528853610088           # ziggurat_nor_r: |x| beyond it came from the tail
# seed, stream, t: rows 0 .. 4095, A = 16 each
BASE = [(2025, 0, 0), (2025, 1, 0), (2025, 2, 2 ** 40 + 3)]
BASE_ROWS, BASE_A = 4096, 16
# what a case must hold before a test may rest on it: elements of more than one word, of five words or more, tail draws
MIN_MULTI, MIN_SECOND_BLOCK, MIN_TAIL = 500, 2, 5
# (n, A) where the walk can go wrong: one element, one row, one short of and one past a wave, A no power of two, more than one
# workgroup with a last group of stores that is not whole
SHAPES = [(1, 1), (1, 16), (63, 16), (65, 17), (4097, 3)]
GS_THREADS, GS_MAX_BLOCKS = 256, 2048       # csrc/f110_gauss_plan.h: beyond their product the lanes stride


def _u64(values):
    return np.array([int(v) % 2 ** 64 for v in values], dtype=np.uint64)


def one(seed, stream, t, r, j):
    """(the fp64 normal, raw words taken) of one element."""
    bg = np.random.Philox(key=_u64([seed, stream]), counter=_u64([0, j, r, t]))
    x = np.random.Generator(bg).standard_normal()
    st = bg.state
    return x, (int(st['state']['counter'][0]) - 1) * 4 + int(st['buffer_pos'])


@functools.lru_cache(maxsize=None)
def _table(seed, stream, t, rows, A):
    x, w = np.empty((len(rows), A), np.float64), np.empty((len(rows), A), np.int64)
    for i, r in enumerate(rows):
        for j in range(A):
            x[i, j], w[i, j] = one(seed, stream, t, r, j)
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def _rows(rows):
    return tuple(range(rows)) if isinstance(rows, (int, np.integer)) else tuple(int(r) % 2 ** 64 for r in rows)


def draws64(seed, stream, t, rows, A):
    return _table(int(seed), int(stream), int(t), _rows(rows), int(A))[0]


def draws(seed, stream, t, rows, A):
    """The fp32 [len(rows), A] array of the contract; rows: the row ids, or a count n for 0 .. n-1.  Read-only and shared."""
    out = draws64(seed, stream, t, rows, A).astype(np.float32)
    out.setflags(write=False)
    return out


def words_used(seed, stream, t, rows, A):
    """Each element's raw-word count: (counter[0] - 1) * 4 + buffer_pos of its bit generator behind the draw."""
    return _table(int(seed), int(stream), int(t), _rows(rows), int(A))[1]


def census(seed, stream, t, rows=BASE_ROWS, A=BASE_A):
    """(elements of more than one word, elements of five words or more, tail draws)."""
    w, x = words_used(seed, stream, t, rows, A), draws64(seed, stream, t, rows, A)
    return int((w > 1).sum()), int((w >= 5).sum()), int((np.abs(x) > TAIL).sum())


def require(seed, stream, t, rows=BASE_ROWS, A=BASE_A):
    """The three minimums, from the reference alone: a case of easy draws only proves nothing."""
    multi, second, tail = census(seed, stream, t, rows, A)
    assert multi >= MIN_MULTI and second >= MIN_SECOND_BLOCK and tail >= MIN_TAIL, (seed, stream, t, multi, second, tail)
