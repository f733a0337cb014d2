"""Host side of the progress tracker (csrc/f110_progress.h): the per-raceline tables the kernel looks up.

They are computed here with NumPy and uploaded (tables come from the host), so the device never takes
the sqrt of a segment or an atan2 and the tests can demand `==` of a NumPy checker for every output.  ProgressTracker is the Engine's side of it."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .consumer import Consumer


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


class ProgressTracker(Consumer):
    """The progress tracker of one Engine (f110_progress_install / _bind / _update).  The outputs live in `buf` (tensors [B, A]:
    s, d, heading_error, delta, progress, s_prev, seg, seen -- and lap_length [B], every env's lap length, which the host fills at
    an install and no kernel reads), allocated and bound by the first install and kept from then on; `lap_length` is that tensor."""
    NAME = 'progress'
    INFO = {'frenet_s': 's', 'frenet_d': 'd', 'heading_error': 'heading_error', 'progress': 'progress', 'progress_delta': 'delta',
            'lap_length': 'lap_length'}
    STATE = {'progress': 'progress', 's_prev': 's_prev', 'seen': 'seen'}
    DTYPES = {'s': torch.float64, 'd': torch.float64, 'heading_error': torch.float64, 'delta': torch.float64,
              'progress': torch.float64, 's_prev': torch.float64, 'seg': torch.int32, 'seen': torch.uint8}
    lap_length = None

    def install(self, racelines, raceline_of_env=None, grid=True):
        """`racelines` one [M, >= 2] array (columns 0, 1 = x, y) or a sequence of K of them, `raceline_of_env` int array
        [num_envs] (None: every env on raceline 0).  The tables are computed here with NumPy and the handle keeps its own
        device copy of everything; an install starts every car anew.  grid=False searches every segment even for a single
        raceline (the results are the same).  ValueError for what the library refuses: a zero-length segment, fewer than 2
        points, non-finite coordinates, a raceline index outside 0..K-1."""
        eng = self.eng
        if torch.is_tensor(racelines) or (isinstance(racelines, np.ndarray) and racelines.ndim == 2):
            racelines = [racelines]
        pk = PackedRacelines(racelines)
        assign = None
        if raceline_of_env is not None:
            assign = np.ascontiguousarray(raceline_of_env, dtype=np.int32)
            if assign.shape != (eng.B,):
                raise ValueError('raceline_of_env must have one entry per env (%d), got shape %s' % (eng.B, assign.shape))
        xy, offsets, *tables = [a.ctypes.data_as(C.c_void_p) if a is not None else None
                                for a in (pk.xy, pk.offsets, pk.len, pk.cum, pk.psi, pk.lap_length, assign)]
        _lib.check(eng.lib.f110_progress_install(eng._h, xy, offsets, pk.K, *tables, int(bool(grid))))
        if self.buf is None:
            buf = {k: torch.zeros((eng.B, eng.A), dtype=dt, device=eng.device) for k, dt in self.DTYPES.items()}
            buf['lap_length'] = torch.zeros((eng.B,), dtype=torch.float64, device=eng.device)
            self._bind(buf, _lib.ProgressBuffers)
            self.lap_length = buf['lap_length']
        else:
            self.restart()
        lap = pk.lap_length[assign] if assign is not None else np.full(eng.B, pk.lap_length[0])
        self.lap_length.copy_(torch.as_tensor(lap))
        self.on = True

    def remove(self):
        """No launch, no info key, no state_dict key remains; the buffers stay for the next install."""
        if self.on:
            _lib.check(self.eng.lib.f110_progress_install(self.eng._h, None, None, 0, None, None, None, None, None, 0))
        self.on = False

    def restart(self):
        """Every car's progress starts anew with the next update."""
        self.buf['seen'].zero_()
