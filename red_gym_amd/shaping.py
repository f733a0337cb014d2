"""Host side of the reward shaper (csrc/f110_shaping.h): the options with the numbers of the reference's RL consumer
(src/SAL.py: map_origin and map_scale :66-67, the clip of _world_to_pixel :142, detect_collison's neighborhood_check :766,
centerline_reward's max_lane_halfwidth :921, the weights of _calculate_rewards :231-244) and the function-level wrapper of
the kernel, and RewardShaper, the Engine's side of it.  There is no CPU path: the terms are computed by libf110_hip.so's
shaping_kernel."""
import ctypes as C

import torch

from . import _lib
from .consumer import Consumer
from .lidar import LidarBitmap

DEFAULTS = dict(rows=256, cols=256, agent=0, neighborhood=1, clip_max=255, scale=10.0, origin_x=128.0, origin_y=128.0,
                max_lane_halfwidth=50.0, w_collision=-100.0, w_progress=10.0, w_centering=2.0)


def make_config(**cfg):
    """An f110_shaping_config from keyword options; the missing ones take DEFAULTS (SAL's numbers)."""
    unknown = set(cfg) - set(DEFAULTS)
    if unknown:
        raise TypeError('unknown shaping option(s): %s' % ', '.join(sorted(unknown)))
    c = _lib.ShapingConfig()
    for k, v in DEFAULTS.items():
        v = cfg.get(k, v)
        setattr(c, k, int(v) if isinstance(DEFAULTS[k], int) else float(v))
    return c


def validate(num_agents=1, **cfg):
    """f110_shaping_validate (host only, no device): ValueError for what an install would refuse."""
    _lib.check(_lib.load().f110_shaping_validate(C.byref(make_config(**cfg)), int(num_agents)))


def reward_terms(bitmaps, xy, prev_xy, **cfg):
    """SACF110Env._calculate_rewards for n independent cases (f110_shaping_terms, no episode logic): bitmaps [n, rows, cols]
    uint8, xy and prev_xy [n, 2] fp64, device tensors.  Returns a dict of device tensors [n]: collision_term,
    progress_term, centering_term, total (fp64) and collided (uint8).  rows / cols default to the bitmaps' shape."""
    lib = _lib.load()
    n, rows, cols = bitmaps.shape
    cfg = dict(cfg, rows=cfg.get('rows', rows), cols=cfg.get('cols', cols))
    c = make_config(**cfg)
    if (c.rows, c.cols) != (rows, cols):
        raise ValueError('bitmaps of %d x %d pixels, config says %d x %d' % (rows, cols, c.rows, c.cols))
    dev = bitmaps.device
    bitmaps = bitmaps.to(torch.uint8).contiguous()
    xy = xy.to(device=dev, dtype=torch.float64).contiguous()
    prev_xy = prev_xy.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(xy.shape) != (n, 2) or tuple(prev_xy.shape) != (n, 2):
        raise ValueError('xy and prev_xy must have shape (%d, 2)' % n)
    out = {k: torch.empty((n,), dtype=torch.float64, device=dev) for k in ('collision_term', 'progress_term', 'centering_term', 'total')}
    out['collided'] = torch.empty((n,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.f110_shaping_terms(C.byref(c), bitmaps.data_ptr(), xy.data_ptr(), prev_xy.data_ptr(), n,
                                          out['collision_term'].data_ptr(), out['progress_term'].data_ptr(),
                                          out['centering_term'].data_ptr(), out['total'].data_ptr(),
                                          out['collided'].data_ptr(), stream))
        torch.cuda.current_stream(dev).synchronize()   # the contiguous copies above may be temporaries
    return out


class RewardShaper(Consumer):
    """The reward shaper of one Engine (f110_shaping_install / _bind / _update) and the renderer of the bitmap it reads.  The
    buffers live in `buf`: bitmap [B, rows, cols] uint8, collision_term, progress_term, centering_term, total [B] fp64,
    collided [B] uint8 and the state prev_xy [B, 2], t_seen [B]; they are allocated and bound by the first install and again
    only when rows / cols change.  `cfg` is the f110_shaping_config installed."""
    NAME = 'shaping'
    INFO = {'reward_collision': 'collision_term', 'reward_progress': 'progress_term', 'reward_centering': 'centering_term',
            'bitmap_collided': 'collided', 'lidar_bitmap': 'bitmap'}
    STATE = {'prev_xy': 'prev_xy', 't_seen': 't_seen', 'lidar_bitmap': 'bitmap'}
    DTYPES = {'collision_term': torch.float64, 'progress_term': torch.float64, 'centering_term': torch.float64,
              'total': torch.float64, 'collided': torch.uint8, 't_seen': torch.float64}
    cfg, _to_img = None, None

    def install(self, **cfg):
        """`cfg`: options of DEFAULTS (missing ones take SAL's numbers).  An install starts the shaper anew (restart()).
        TypeError for an unknown option, ValueError for what the library refuses."""
        eng = self.eng
        c = make_config(**cfg)
        _lib.check(eng.lib.f110_shaping_install(eng._h, C.byref(c)))
        with torch.cuda.device(eng.device):
            if self.buf is None or tuple(self.buf['bitmap'].shape[1:]) != (c.rows, c.cols):
                buf = {k: torch.zeros((eng.B,), dtype=dt, device=eng.device) for k, dt in self.DTYPES.items()}
                buf['prev_xy'] = torch.zeros((eng.B, 2), dtype=torch.float64, device=eng.device)
                buf['bitmap'] = torch.zeros((eng.B, c.rows, c.cols), dtype=torch.uint8, device=eng.device)
                self._bind(buf, _lib.ShapingBuffers)
                self.reward = buf['total']
        self.close()
        self._to_img = LidarBitmap(eng.num_beams, bg_color='black', draw_mode='FILL', output_image_dims=(c.rows, c.cols),
                                   device=eng.device_index)
        self.cfg, self.on = c, True
        self.restart()

    def remove(self):
        """No launch, no info key, no state_dict key remains; the buffers stay for the next install of the same image size."""
        if self.on:
            _lib.check(self.eng.lib.f110_shaping_install(self.eng._h, None))
        self.cfg, self.on = None, False
        self.close()

    def update(self):
        """What follows every step.  The kernel reads the bitmap while it still holds the PREVIOUS step's image; only then is
        the new scan rendered into the same buffer."""
        self.kernel()
        self.render()

    def render(self):
        """Draws the current scan of car `agent` into the bitmap: lidar_to_bitmap(scan, output_image_dims=(rows, cols),
        bg_color='black', draw_mode='FILL') (SAL.py:76-77)."""
        self._to_img(self.eng.t['scans'][:, self.cfg.agent], out=self.buf['bitmap'])

    def restart(self):
        """The next update takes its previous position from its own pose (it pays no progress) and reads the image of the
        scans as they stand."""
        self.buf['t_seen'].fill_(-1.0)
        self.render()

    def close(self):
        if self._to_img is not None:
            self._to_img.close()
            self._to_img = None
