"""What the GPU tests of the kernel families share: host <-> device copies, comparison as raw bit patterns at the array's own width,
and output buffers between guards for the raw-ABI tests.  torch is imported inside functions only, so collection needs no device."""
import numpy as np

GUARD = 64


def to_host(t):
    return t.detach().cpu().numpy()


def to_device(a, dtype=None, device='cuda'):
    """A tensor that holds a copy of `a` (the checkers' cached inputs are read-only and never back a tensor); None stays None."""
    import torch
    if a is None:
        return None
    t = torch.as_tensor(np.array(a), device=device)
    return t if dtype is None else t.to(dtype)


def packed(imgs):
    """uint8 images as the int64 words of bit-packed frames, on the device."""
    import replay_cases as rc
    return to_device(rc.pack(imgs).view(np.int64))


def _host(a):
    return to_host(a) if hasattr(a, 'detach') else np.asarray(a)


def bits(a):
    """The raw patterns of a host array or a device tensor: uint32 for fp32, uint64 for fp64."""
    a = np.ascontiguousarray(_host(a))
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def differing(got, want):
    """The number of elements of `got` whose patterns are not those of `want` cast to got's dtype."""
    got = _host(got)
    want = np.asarray(_host(want), got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((bits(got) != bits(want)).sum())


def same(got, want):
    return _host(got).shape == _host(want).shape and differing(got, want) == 0


def equal(got, want):
    """`==` at the array's own width: the same dtype and shape, bit patterns for floats, values for the integers."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return same(got, want) if got.dtype.kind == 'f' else bool((got == want).all())


class Guarded:
    """count elements of `dtype` (fp32 unless given) with GUARD elements of `fill` either side, the first `off` elements past a
    16-byte boundary; through matrix() a [rows, cols] view whose rows lie ld apart, with `fill` between the rows.  `fill` may be
    NaN."""

    def __init__(self, count, off=0, dtype=None, fill=-7.0, values=None, device='cuda'):
        import torch
        self.count, self.fill, self.off, self.shape = count, fill, off, None
        self.whole = torch.full((GUARD + off + count + GUARD,), fill, dtype=torch.float32 if dtype is None else dtype, device=device)
        self.data = self.whole[GUARD + off:GUARD + off + count]
        assert self.whole.data_ptr() % 16 == 0 and self.data.data_ptr() % 16 == (self.whole.element_size() * off) % 16
        if values is not None:
            self.data.copy_(to_device(values, device=device).reshape(-1))

    @classmethod
    def matrix(cls, rows, cols, ld, off=0, values=None, **kw):
        m = cls((rows - 1) * ld + cols, off, **kw)
        m.shape = (rows, cols, ld)
        m.view = m.data.as_strided((rows, cols), (ld, 1))
        if values is not None:
            m.view.copy_(to_device(values, device=m.whole.device))
        return m

    ptr = property(lambda self: self.data.data_ptr())

    def _holds_fill(self, a):
        return bool((np.isnan(a) if np.isnan(self.fill) else a == np.asarray(self.fill, a.dtype)).all())

    def read(self, rows=None, cols=None, ld=None):
        """A host copy of the body, or of the [rows, cols] view (a matrix()'s own unless given); both guards, and the elements
        between the rows, must still hold `fill`."""
        w = to_host(self.whole)
        lo, hi = GUARD + self.off, GUARD + self.off + self.count
        assert self._holds_fill(w[:lo]), 'the guard in front of the buffer was written'
        assert self._holds_fill(w[hi:]), 'the guard behind the buffer was written'
        if rows is None and self.shape is None:
            return w[lo:hi].copy()
        rows, cols, ld = self.shape if rows is None else (rows, cols, ld)
        padded = np.full(rows * ld, self.fill, w.dtype)
        padded[:self.count] = w[lo:hi]
        padded = padded.reshape(rows, ld)
        assert self._holds_fill(padded[:, cols:]), 'the elements between the rows were written'
        return padded[:, :cols].copy()

    def untouched(self):
        """The whole body still holds `fill`: an output passed as NULL is not written."""
        return self._holds_fill(to_host(self.data))
