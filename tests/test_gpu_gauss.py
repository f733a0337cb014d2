"""The policy's Gaussian draws on the GPU (csrc/f110_gauss.h) against NumPy itself (tests/gauss_cases.py), compared as raw bit
patterns with no tolerance: f110_gauss_fill_at through the raw ABI on guarded buffers at the three base cases -- each first shown, from
the reference alone, to hold hundreds of multi-word elements, elements that cross into the second Philox block and tail draws -- and
at the shapes where the walk can go wrong, the grid-stride pass included; row ids; the device's call counters, their advance and a
loaded state; a captured fill replayed; repeatability.  A difference is reported with its element and the raw words NumPy took for it."""
import ctypes as C

import numpy as np
import pytest

import gauss_cases as gc
import gpu_checks as gk

pytestmark = pytest.mark.gpu

NAN = float('nan')
WORD_FILL = -7                                  # of the int64 margins around the 64-byte state


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _fill_at(seed, stream, t, n, A, rows=None, off=0):
    """f110_gauss_fill_at into a NaN-filled guarded buffer `off` floats past a 16-byte boundary -> the [n, A] host array; the margins
    must be as they were and every element written."""
    import torch
    from red_gym_amd import _lib
    out = gk.Guarded(n * A, off=off, fill=NAN)
    r = None if rows is None else gk.to_device(np.array([int(v) % 2 ** 64 for v in rows], np.uint64).view(np.int64))
    _lib.check(_lib.load().f110_gauss_fill_at(int(seed) % 2 ** 64, stream, int(t) % 2 ** 64, n, A, _lib.ptr(r), out.ptr, _stream()))
    torch.cuda.synchronize()
    got = out.read().reshape(n, A)
    assert not np.isnan(got).any(), 'an element was not written'
    return got


def _same(got, want, case, rows=None):
    """`==` on bits; the first difference is named with its element and what the reference did there."""
    got, want = gk.to_host(got) if hasattr(got, 'detach') else np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype)
    bad = np.argwhere(gk.bits(got) != gk.bits(want))
    if len(bad):
        i, j = (int(v) for v in bad[0])
        r = i if rows is None else int(rows[i])
        x, words = gc.one(case[0], case[1], case[2], r, j)
        raise AssertionError('%d of %d elements differ from NumPy; first: case (seed, stream, t) = %s row %d column %d: got %r, NumPy %r '
                             '(fp64 %r, %d raw words)' % (len(bad), got.size, case, r, j, float(got[i, j]), float(want[i, j]), x, words))


@pytest.mark.parametrize('case', gc.BASE)
def test_base_cases_equal_numpy(case):
    gc.require(*case)
    _same(_fill_at(*case, gc.BASE_ROWS, gc.BASE_A), gc.draws(*case, gc.BASE_ROWS, gc.BASE_A), case)


@pytest.mark.parametrize('n,A', gc.SHAPES)
def test_shapes_equal_numpy(n, A):
    """Aligned (16-byte stores, a last group that is not whole at 65 x 17 and 4097 x 3) and 4, 8 and 12 bytes past a boundary (single
    stores).  The elements are those of the first base case where the shape lies inside it."""
    case = gc.BASE[0]
    gc.require(*case)
    want = gc.draws(*case, gc.BASE_ROWS, gc.BASE_A)[:n, :A] if A <= gc.BASE_A and n <= gc.BASE_ROWS else gc.draws(*case, n, A)
    for off in (0, 1, 2, 3):
        _same(_fill_at(*case, n, A, off=off), want, case)


def test_out_four_but_not_sixteen_byte_aligned():
    case = gc.BASE[1]
    gc.require(*case)
    _same(_fill_at(*case, gc.BASE_ROWS, gc.BASE_A, off=1), gc.draws(*case, gc.BASE_ROWS, gc.BASE_A), case)


def test_grid_stride_pass():
    """n * A above GS_MAX_BLOCKS * GS_THREADS: the lanes walk twice.  NumPy checks the rows either side of the seam, the first and
    the last (0.1 s of it); every element is also `==` what fills of explicit row ids that fit one pass give -- a path the base cases
    and the row tests pin on NumPy."""
    per_pass = gc.GS_THREADS * gc.GS_MAX_BLOCKS // 16
    n, case = per_pass + 300, gc.BASE[0]
    gc.require(*case)
    got = _fill_at(*case, n, 16)
    picked = list(range(64)) + list(range(per_pass - 64, n))
    _same(got[picked], gc.draws(*case, picked, 16), case, picked)
    half = n // 2
    for lo, hi in ((0, half), (half, n)):
        assert (hi - lo) * 16 <= gc.GS_THREADS * gc.GS_MAX_BLOCKS
        assert gk.same(_fill_at(*case, hi - lo, 16, rows=range(lo, hi)), got[lo:hi]), (lo, hi)


def test_row_ids():
    case = gc.BASE[0]
    gc.require(*case)
    full = gc.draws(*case, gc.BASE_ROWS, gc.BASE_A)
    rows = np.random.default_rng(3).permutation(gc.BASE_ROWS)[:100]
    assert (rows >= 5).sum() > 0 and len(set(rows.tolist())) == 100
    _same(_fill_at(*case, 100, gc.BASE_A, rows=rows), full[rows], case, rows)
    for off in (0, 2):
        far = [2 ** 33 + 5, 2 ** 62, 2 ** 64 - 1, 0, 2 ** 63]
        _same(_fill_at(*case, len(far), gc.BASE_A, rows=far, off=off), gc.draws(*case, far, gc.BASE_A), case, far)
    # a row drawn alone is the row drawn among 4 096
    _same(_fill_at(*case, 1, gc.BASE_A, rows=[4095]), full[4095:], case, [4095])


def test_counters_on_the_device():
    """fill reads t on the device and the advance behind it adds one to that stream's counter alone; the state's margins stay."""
    import torch
    from red_gym_amd import _lib
    from red_gym_amd.gauss import fresh_state_words
    lib, t0, stream, n, A = _lib.load(), 2 ** 40 + 1, 2, 65, 16
    st = gk.Guarded(8, dtype=torch.int64, fill=WORD_FILL, values=np.array(fresh_state_words(2025, (11, 12, t0, 14)), np.int64))
    got = []
    for advance in (1, 1, 0, 0):
        out = gk.Guarded(n * A, fill=NAN)
        _lib.check(lib.f110_gauss_fill(st.ptr, stream, n, A, None, out.ptr, advance, _stream()))
        torch.cuda.synchronize()
        got.append((out.read().reshape(n, A), st.read().tolist()))
    for k, (t, calls) in enumerate(((t0, t0 + 1), (t0 + 1, t0 + 2), (t0 + 2, t0 + 2), (t0 + 2, t0 + 2))):
        _same(got[k][0], gc.draws(2025, stream, t, n, A), (2025, stream, t))
        assert got[k][1] == [2025, 11, 12, calls, 14, 0, 0, 0], (k, got[k][1])


def test_source_advances_loads_and_draws_the_third_base_case():
    import torch
    from red_gym_amd.gauss import GaussianSource
    src = GaussianSource(2025)
    assert src.state.dtype == torch.int64 and tuple(src.state.shape) == (8,) and src.calls() == [0, 0, 0, 0]
    a, b = src.normal(64, 16, stream=1), src.normal(64, 16, stream=1)
    c = src.normal(64, 16, stream=1, advance=False)
    assert src.calls() == [0, 2, 0, 0]
    for t, got in enumerate((a, b, c)):
        _same(got, gc.draws(2025, 1, t, 64, 16), (2025, 1, t))
    _same(src.normal_at(1, 1, 64, 16), gc.draws(2025, 1, 1, 64, 16), (2025, 1, 1))
    assert src.calls() == [0, 2, 0, 0] and src.state_dict() == dict(seed=2025, calls=[0, 2, 0, 0])
    case = gc.BASE[2]
    gc.require(*case)
    ptr = src.state.data_ptr()
    src.load_state_dict(dict(seed=case[0], calls=[7, 8, case[2], 2 ** 64 - 1]))
    assert src.state.data_ptr() == ptr
    out = torch.full((gc.BASE_ROWS, gc.BASE_A), NAN, dtype=torch.float32, device='cuda')
    assert src.normal(gc.BASE_ROWS, gc.BASE_A, stream=2, out=out) is out
    _same(out, gc.draws(*case, gc.BASE_ROWS, gc.BASE_A), case)
    assert src.calls() == [7, 8, case[2] + 1, 2 ** 64 - 1]
    src.normal(1, 1, stream=3)                                          # the counter wraps like any 64-bit counter
    assert src.calls() == [7, 8, case[2] + 1, 0]
    # another seed gives other draws, by value and by state
    other = GaussianSource(2026)
    assert not gk.same(other.normal(64, 16, stream=1), a) and gk.same(other.normal_at(1, 0, 64, 16), gc.draws(2026, 1, 0, 64, 16))
    for bad in (dict(n=0, A=16), dict(n=4, A=33), dict(n=4, A=16, stream=4), dict(n=4, A=16, out=torch.zeros((4, 16), device='cuda', dtype=torch.float64)),
                dict(n=4, A=16, rows=torch.zeros(3, dtype=torch.int64, device='cuda'))):
        with pytest.raises(ValueError):
            src.normal(**bad)


def test_captured_fill_replays_with_a_fresh_t():
    import torch
    from red_gym_amd.gauss import GaussianSource
    src, t0, n, A = GaussianSource(2025), 5, 63, 16
    src.load_state_dict(dict(seed=2025, calls=[t0, 0, 0, 0]))
    rows = gk.to_device(np.arange(100, 100 + n, dtype=np.int64))
    out = torch.full((n, A), NAN, dtype=torch.float32, device='cuda')
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        src.normal(n, A, stream=0, rows=rows, out=out)
    cur.wait_stream(side)
    assert src.calls() == [t0, 0, 0, 0] and bool(torch.isnan(out).all())  # a capture executes nothing
    for k in range(3):
        g.replay()
        _same(out, gc.draws(2025, 0, t0 + k, range(100, 100 + n), A), (2025, 0, t0 + k), list(range(100, 100 + n)))
    assert src.calls() == [t0 + 3, 0, 0, 0]


def test_the_same_call_twice_is_bitwise_equal():
    case = (77, 3, 2 ** 63 + 9)
    a, b = _fill_at(*case, 4097, 16), _fill_at(*case, 4097, 16)
    assert gk.same(a, b)
    assert abs(float(a.mean())) < 0.02 and abs(float(a.std()) - 1.0) < 0.02       # 65 552 standard normals
