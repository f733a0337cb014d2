"""Host side of the path follower (csrc/f110_pathfollow.h): the action side of the reference's RL consumer, SACF110Env.step
(src/SAL.py).  The policy's 16 numbers become a path of 8 points (compute_vectors_with_angle_clamp :585-608,
_calculate_global_path :157-181), the path becomes an acceleration (MPC_controller :615-739: not-a-knot splines, reference
states and the first QP, the only one whose result the reference uses) and a (steer, speed) pair (MPC_converter :741-764);
behind every step the waypoint index follows the pose (_update_path_index :252-259).  DEFAULTS are SAL's numbers (car_length
:56, vector_length :57, DIST_THRESHOLD :36, MPC_PARAMS :37-45, max_steer :210).

Two things of the reference are dead or broken and are decided here: `pending_action` is never set and is left out; the path
has 8 points but a new one is only decoded at `sub_index >= 16`, so the reference raises IndexError once the index reaches
8 -- `replan_at` (1..8, default 8 = the number of points) decodes the new path, from the raw action of that step, where the
reference would raise.  There is no CPU path: everything is computed by libf110_hip.so's pathfollow kernels."""
import ctypes as C

import torch

from . import _lib
from .consumer import Consumer

DEFAULTS = dict(agent=0, car_length=0.3, vector_length=0.5, max_diff_deg=10.0, dist_threshold=0.2, replan_at=8,
                desired_velocity=2.0, timestep=0.1, horizon=5, q=(1.0, 1.0, 0.1, 0.1), r=(0.1, 0.1), p=(10.0, 10.0, 1.0, 1.0),
                max_steer=0.4189)
POINTS = 8


def make_config(**cfg):
    """An f110_pathfollow_config from keyword options; the missing ones take DEFAULTS (SAL's numbers).  q, r, p are the
    diagonals of state_cost, input_cost and terminal_cost, in the state's order (x, y, vx, vy) and the input's (ax, ay)."""
    unknown = set(cfg) - set(DEFAULTS)
    if unknown:
        raise TypeError('unknown pathfollow option(s): %s' % ', '.join(sorted(unknown)))
    c = _lib.PathFollowConfig()
    for k, d in DEFAULTS.items():
        v = cfg.get(k, d)
        if isinstance(d, tuple):
            v = tuple(float(x) for x in v)
            if len(v) != len(d):
                raise ValueError('%s takes %d weights, got %d' % (k, len(d), len(v)))
            setattr(c, k, (C.c_double * len(d))(*v))
        else:
            setattr(c, k, int(v) if isinstance(d, int) else float(v))
    return c


def validate(num_agents=1, **cfg):
    """f110_pathfollow_validate (host only, no device): ValueError for what an install would refuse."""
    _lib.check(_lib.load().f110_pathfollow_validate(C.byref(make_config(**cfg)), int(num_agents)))


def _f64(t, dev, shape, what):
    t = torch.as_tensor(t).to(device=dev, dtype=torch.float64).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError('%s must have shape %s, got %s' % (what, shape, tuple(t.shape)))
    return t


def decode_paths(raw_actions, poses, **cfg):
    """compute_vectors_with_angle_clamp + _calculate_global_path for n independent cases (f110_pathfollow_decode): raw_actions
    [n, 16] and poses [n, 3] = (x, y, yaw), device tensors -> paths [n, 8, 2] fp64."""
    lib, c = _lib.load(), make_config(**cfg)
    dev, n = raw_actions.device, raw_actions.shape[0]
    raw, poses = _f64(raw_actions, dev, (n, 2 * POINTS), 'raw_actions'), _f64(poses, dev, (n, 3), 'poses')
    paths = torch.empty((n, POINTS, 2), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.f110_pathfollow_decode(C.byref(c), raw.data_ptr(), poses.data_ptr(), n, paths.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()   # the contiguous copies above may be temporaries
    return paths


def mpc_controls(paths, vels, **cfg):
    """MPC_controller's first control and MPC_converter for n independent cases (f110_pathfollow_mpc): paths [n, 8, 2] and
    vels [n, 2] = (vx, vy), device tensors.  Returns a dict of device tensors: dists [n, 8], ref_traj [n, horizon + 1, 4],
    accel [n, 2], actions [n, 2] = (steer, speed), all fp64, qp_steps [n, 2] int32 (steps of the two active-set walks) and
    errors (a Python int: F110_DEVERR_QP_LIMIT if a walk reached its step limit)."""
    lib, c = _lib.load(), make_config(**cfg)
    dev, n = paths.device, paths.shape[0]
    paths, vels = _f64(paths, dev, (n, POINTS, 2), 'paths'), _f64(vels, dev, (n, 2), 'vels')
    out = {'dists': torch.empty((n, POINTS), dtype=torch.float64, device=dev),
           'ref_traj': torch.empty((n, c.horizon + 1, 4), dtype=torch.float64, device=dev),
           'accel': torch.empty((n, 2), dtype=torch.float64, device=dev),
           'actions': torch.empty((n, 2), dtype=torch.float64, device=dev),
           'qp_steps': torch.zeros((n, 2), dtype=torch.int32, device=dev)}
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.f110_pathfollow_mpc(C.byref(c), paths.data_ptr(), vels.data_ptr(), n, out['dists'].data_ptr(),
                                           out['ref_traj'].data_ptr(), out['accel'].data_ptr(), out['actions'].data_ptr(),
                                           out['qp_steps'].data_ptr(), err.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    out['errors'] = int(err.item())
    return out


def advance_index(paths, index, xy, **cfg):
    """_update_path_index for n independent cases (f110_pathfollow_advance): paths [n, 8, 2], index [n] and xy [n, 2], device
    tensors -> the new index [n] int32."""
    lib, c = _lib.load(), make_config(**cfg)
    dev, n = paths.device, paths.shape[0]
    paths, xy = _f64(paths, dev, (n, POINTS, 2), 'paths'), _f64(xy, dev, (n, 2), 'xy')
    index = torch.as_tensor(index).to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.f110_pathfollow_advance(C.byref(c), paths.data_ptr(), index.data_ptr(), xy.data_ptr(), n, out.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()
    return out


class PathFollower(Consumer):
    """The path follower of one Engine (f110_pathfollow_install / _bind / _act / _update).  The buffers live in `buf`:
    path_points [B, 8, 2] fp64, path_index [B] int32 (< 0: no path), path_replanned [B] uint8, mpc_accel [B, 2] fp64 and
    t_seen [B]; they are allocated and bound by the first install.  `cfg` is the f110_pathfollow_config installed."""
    NAME = 'pathfollow'
    INFO = {'path_points': 'path_points', 'path_index': 'path_index', 'path_replanned': 'path_replanned', 'mpc_accel': 'mpc_accel'}
    STATE = {'path_points': 'path_points', 'path_index': 'path_index', 'path_t_seen': 't_seen'}
    cfg = None

    def install(self, **cfg):
        """`cfg`: options of DEFAULTS (missing ones take SAL's numbers).  An install drops every env's path (restart()).
        TypeError for an unknown option, ValueError for what the library refuses."""
        eng = self.eng
        c = make_config(**cfg)
        _lib.check(eng.lib.f110_pathfollow_install(eng._h, C.byref(c)))
        if self.buf is None:
            with torch.cuda.device(eng.device):
                z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=eng.device)  # noqa: E731
                self._bind({'path_points': z((eng.B, POINTS, 2), torch.float64), 'path_index': z((eng.B,), torch.int32),
                            'path_replanned': z((eng.B,), torch.uint8), 'mpc_accel': z((eng.B, 2), torch.float64),
                            't_seen': z((eng.B,), torch.float64)}, _lib.PathFollowBuffers)
        self.cfg, self.on = c, True
        self.restart()

    def remove(self):
        """No launch, no info key, no state_dict key remains; the buffers stay for the next install."""
        if self.on:
            _lib.check(self.eng.lib.f110_pathfollow_install(self.eng._h, None))
        self.cfg, self.on = None, False

    def act(self, raw_actions, out):
        """The act kernel on the current stream: raw_actions [B, 16] fp64 on the device, contiguous; out [B, A, 2] (or its
        [B * A, 2] view), of which car `agent`'s (steer, speed) pairs are written.  No allocation, no synchronisation."""
        if raw_actions.dtype != torch.float64 or not raw_actions.is_contiguous() or tuple(raw_actions.shape) != (self.eng.B, 2 * POINTS) \
                or raw_actions.device != self.eng.device:
            raise ValueError('raw_actions must be a contiguous fp64 tensor [%d, %d] on %s' % (self.eng.B, 2 * POINTS, self.eng.device))
        if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != self.eng.B * self.eng.A * 2 or out.device != self.eng.device:
            raise ValueError('out must be a contiguous fp64 tensor [%d, %d, 2] on %s' % (self.eng.B, self.eng.A, self.eng.device))
        with torch.cuda.device(self.eng.device):
            _lib.check(self.eng.lib.f110_pathfollow_act(self.eng._h, raw_actions.data_ptr(), out.data_ptr(), self.eng._stream()))
        return out

    def restart(self):
        """Every env decodes a new path at its next act."""
        self.buf['path_index'].fill_(-1)
        self.buf['t_seen'].fill_(-1.0)
        self.buf['path_replanned'].zero_()
