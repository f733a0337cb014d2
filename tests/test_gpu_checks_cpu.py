"""tests/gpu_checks.py on the CPU: the one guard check and the one bit comparison that the GPU tests of every kernel family trust."""
import numpy as np
import pytest

import gpu_checks as gk

NAN = float('nan')


@pytest.mark.parametrize('fill', [-7.0, NAN], ids=['-7', 'nan'])
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('off', range(4))
def test_guards_either_side(off, dtype, fill):
    """Untouched, read() passes; a store to the last element of the leading guard or the first of the trailing one makes it raise and
    says which side; a store inside the body does neither and ends untouched()."""
    import torch

    def fresh():
        return gk.Guarded(10, off=off, dtype=getattr(torch, dtype), fill=fill, device='cpu')

    g = fresh()
    assert g.data.shape == (10,) and g.whole.shape == (2 * gk.GUARD + off + 10,) and g.ptr == g.whole.data_ptr() + (gk.GUARD + off) * g.whole.element_size()
    assert g.read().shape == (10,) and g.read().dtype == np.dtype(dtype) and g.untouched()
    for at, side in ((gk.GUARD + off - 1, 'in front'), (gk.GUARD + off + 10, 'behind')):
        g = fresh()
        g.whole[at] = 1.0
        with pytest.raises(AssertionError, match=side):
            g.read()
        assert g.untouched()
    for at in (0, 9):
        g = fresh()
        g.data[at] = 1.0
        assert g.read()[at] == 1.0 and not g.untouched()
    if not np.isnan(fill):                                                       # NaN in a guard of numbers is a write too
        g = fresh()
        g.whole[0] = NAN
        with pytest.raises(AssertionError):
            g.read()


def test_values_and_the_gaps_between_rows():
    import torch
    values = np.arange(15, dtype=np.float32).reshape(3, 5)
    values.setflags(write=False)
    for fill in (-7.0, NAN):
        def fresh():
            return gk.Guarded.matrix(3, 5, 8, off=1, values=values, fill=fill, device='cpu')
        m = fresh()
        assert m.count == 21 and m.data.data_ptr() % 16 == 4 and tuple(m.view.shape) == (3, 5) and m.view.stride() == (8, 1)
        assert np.array_equal(m.read(3, 5, 8), values) and np.array_equal(m.read(), values)
        m.view[1, 4] = 99.0                                                      # the last column of a row: inside
        assert m.read(3, 5, 8)[1, 4] == 99.0
        m = fresh()
        m.data[1 * 8 + 5] = 99.0                                                 # row 1, column 5: the first element of a gap
        for args in ((3, 5, 8), ()):
            with pytest.raises(AssertionError, match='between the rows'):
                m.read(*args)
    flat = gk.Guarded(4, values=[1.0, 2.0, 3.0, 4.0], dtype=torch.float64, fill=7.0, device='cpu')
    assert flat.read().tolist() == [1.0, 2.0, 3.0, 4.0] and not flat.untouched()


def test_bits_differing_and_same():
    import torch
    zeros = np.array([0.0, -0.0], np.float32)
    assert gk.bits(zeros).dtype == np.uint32 and gk.bits(zeros.astype(np.float64)).dtype == np.uint64
    assert gk.bits(torch.as_tensor(zeros)).tolist() == [0, 0x80000000]
    assert gk.differing(zeros, zeros[::-1]) == 2 and not gk.same(zeros, zeros[::-1]) and gk.same(zeros, zeros.copy())
    nans = np.array([0x7fc00000, 0x7fc00001], np.uint32).view(np.float32)
    assert gk.same(nans, nans.copy()) and gk.differing(nans, nans[::-1]) == 2
    # an fp64 pair that agrees once rounded to fp32 differs at its own width; `want` is cast to got's dtype, never the reverse
    a, b = np.array([1.0]), np.array([1.0 + 2.0 ** -40])
    assert a.astype(np.float32) == b.astype(np.float32) and gk.differing(a, b) == 1 and not gk.same(torch.as_tensor(a), b)
    assert gk.same(a.astype(np.float32), b) and gk.same(torch.as_tensor(a), a.astype(np.float32))
    with pytest.raises(AssertionError):
        gk.differing(np.zeros(3, np.float32), np.zeros((3, 1), np.float32))
    assert not gk.same(np.zeros(3, np.float32), np.zeros((3, 1), np.float32))
    with pytest.raises(AssertionError):
        gk.bits(np.zeros(3, np.int32))


def test_equal_wants_dtype_shape_and_every_bit():
    zeros, nans = np.array([0.0, -0.0]), np.array([np.nan, 1.0])
    assert gk.equal(zeros, zeros.copy()) and not gk.equal(zeros, zeros[::-1]) and gk.equal(nans, nans.copy())
    assert not gk.equal(zeros, zeros.astype(np.float32)) and not gk.equal(zeros.astype(np.float32), zeros)     # (no cast either way)
    ints = np.array([1, 2, 3], np.int32)
    assert gk.equal(ints, ints.copy()) and not gk.equal(ints, ints.astype(np.int64)) and not gk.equal(ints, np.array([1, 2, 4], np.int32))
    assert not gk.equal(ints, ints.reshape(3, 1)) and not gk.equal(ints, ints.astype(np.float64))
    assert gk.equal(np.array([True, False]), np.array([True, False])) and not gk.equal(np.array([1, 0], np.uint8), np.array([True, False]))


def test_to_device_copies():
    assert gk.to_device(None) is None
    a = np.arange(4, dtype=np.float32)
    a.setflags(write=False)
    t = gk.to_device(a, device='cpu')
    t += 1.0
    assert a.tolist() == [0.0, 1.0, 2.0, 3.0] and gk.to_host(t).tolist() == [1.0, 2.0, 3.0, 4.0]
    import torch
    assert gk.to_device(a, torch.float64, device='cpu').dtype == torch.float64
