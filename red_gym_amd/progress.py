"""Host side of the progress tracker (csrc/f110_progress.h): the per-raceline tables the kernel looks up.

They are computed here with NumPy and uploaded (tables come from the host), so the device never takes
the sqrt of a segment or an atan2 and the tests can demand `==` of a NumPy checker for every output."""
import numpy as np


def raceline_xy(raceline):
    """Columns 0, 1 = (x, y) of a raceline given as an [M, >= 2] array (or tensor), as a contiguous fp64 [M, 2] array."""
    if hasattr(raceline, 'detach'):
        raceline = raceline.detach().cpu().numpy()
    a = np.asarray(raceline, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError('a raceline is an [M, >= 2] array (columns 0, 1 = x, y), got shape %s' % (a.shape,))
    return np.ascontiguousarray(a[:, :2])


def raceline_tables(xy):
    """(len [M-1], cum [M], psi [M-1], L) of the polyline xy [M, 2]: segment lengths, arc length at every point, segment
    headings and the lap length = arc length of the open polyline plus the gap from its last point back to its first
    (0 for a file whose last row repeats the first).  The segments are those nearest_point_on_trajectory searches
    (examples/waypoint_follow.py:16-47): the closing one is not among them."""
    xy = raceline_xy(xy)
    if xy.shape[0] < 2:
        raise ValueError('a raceline has at least 2 points, got %d' % xy.shape[0])
    dx = xy[1:, 0] - xy[:-1, 0]
    dy = xy[1:, 1] - xy[:-1, 1]
    length = np.sqrt(dx * dx + dy * dy)
    cum = np.concatenate([[0.], np.cumsum(length)])
    psi = np.arctan2(dy, dx)
    ex, ey = xy[0, 0] - xy[-1, 0], xy[0, 1] - xy[-1, 1]
    gap = np.sqrt(ex * ex + ey * ey)
    return length, cum, psi, float(cum[-1] + gap)


class PackedRacelines(object):
    """K racelines in the layout f110_progress_install takes: xy [total, 2] back to back, offsets [K + 1], len / cum / psi
    [total] (raceline k's at offsets[k]; a raceline's last len / psi entry is unused and 0), lap_length [K]."""

    def __init__(self, racelines):
        lines = [raceline_xy(r) for r in racelines]
        if not lines:
            raise ValueError('at least one raceline')
        self.K = len(lines)
        self.offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([a.shape[0] for a in lines])]), dtype=np.int32)
        self.xy = np.ascontiguousarray(np.concatenate(lines, axis=0))
        total = self.xy.shape[0]
        self.len, self.cum, self.psi = np.zeros(total), np.zeros(total), np.zeros(total)
        self.lap_length = np.zeros(self.K)
        for k, a in enumerate(lines):
            length, cum, psi, L = raceline_tables(a)
            o, m = int(self.offsets[k]), a.shape[0]
            self.len[o:o + m - 1], self.cum[o:o + m], self.psi[o:o + m - 1] = length, cum, psi
            self.lap_length[k] = L
