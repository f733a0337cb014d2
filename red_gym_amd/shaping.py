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
from .replay import pack_bitmaps, unpack_bitmaps, words

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


IMAGES = ('bytes', 'bits')


def image_form(image):
    """True for image='bits', False for 'bytes' (how the shaper holds its bitmap); ValueError for anything else."""
    if image not in IMAGES:
        raise ValueError("image must be 'bytes' or 'bits', not %r" % (image,))
    return image == 'bits'


def validate(num_agents=1, image='bytes', **cfg):
    """f110_shaping_validate (host only, no device): ValueError for what an install would refuse."""
    image_form(image)
    _lib.check(_lib.load().f110_shaping_validate(C.byref(make_config(**cfg)), int(num_agents)))


def reward_terms(bitmaps, xy, prev_xy, **cfg):
    """SACF110Env._calculate_rewards for n independent cases (f110_shaping_terms, no episode logic): bitmaps [n, rows, cols]
    uint8, xy and prev_xy [n, 2] fp64, device tensors.  Returns a dict of device tensors [n]: collision_term,
    progress_term, centering_term, total (fp64) and collided (uint8).  rows / cols default to the bitmaps' shape."""
    n, rows, cols = bitmaps.shape
    return _terms(_lib.load().f110_shaping_terms, bitmaps.to(torch.uint8).contiguous(), rows, cols, xy, prev_xy, cfg)


def reward_terms_bits(packed, xy, prev_xy, **cfg):
    """The same from images held as bits (f110_shaping_terms_bits): packed [n, rows, ceil(cols / 64)] int64 in the replay ring's
    format, as LidarBitmap.bits and replay.pack_bitmaps return it.  `cols` must be given (the words do not tell it); rows
    defaults to the shape."""
    n, rows, w = packed.shape
    if 'cols' not in cfg:
        raise ValueError('reward_terms_bits: cols must be given')
    cols = cfg['cols']
    if w != words(cols):
        raise ValueError('%d words per row do not hold %d pixels' % (w, cols))
    return _terms(_lib.load().f110_shaping_terms_bits, packed.to(torch.int64).contiguous(), rows, int(cols), xy, prev_xy, cfg)


def _terms(entry, images, rows, cols, xy, prev_xy, cfg):
    n = images.shape[0]
    cfg = dict(cfg, rows=cfg.get('rows', rows), cols=cfg.get('cols', cols))
    c = make_config(**cfg)
    if (c.rows, c.cols) != (rows, cols):
        raise ValueError('bitmaps of %d x %d pixels, config says %d x %d' % (rows, cols, c.rows, c.cols))
    dev = images.device
    xy = xy.to(device=dev, dtype=torch.float64).contiguous()
    prev_xy = prev_xy.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(xy.shape) != (n, 2) or tuple(prev_xy.shape) != (n, 2):
        raise ValueError('xy and prev_xy must have shape (%d, 2)' % n)
    out = {k: torch.empty((n,), dtype=torch.float64, device=dev) for k in ('collision_term', 'progress_term', 'centering_term', 'total')}
    out['collided'] = torch.empty((n,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(entry(C.byref(c), images.data_ptr(), xy.data_ptr(), prev_xy.data_ptr(), n,
                         out['collision_term'].data_ptr(), out['progress_term'].data_ptr(),
                         out['centering_term'].data_ptr(), out['total'].data_ptr(),
                         out['collided'].data_ptr(), stream))
        torch.cuda.current_stream(dev).synchronize()   # the contiguous copies above may be temporaries
    return out


class RewardShaper(Consumer):
    """The reward shaper of one Engine (f110_shaping_install / _bind / _update) and the renderer of the bitmap it reads.  The
    buffers live in `buf`: bitmap [B, rows, cols] uint8 -- or, installed with image='bits', [B, rows, ceil(cols / 64)] int64,
    one bit per pixel in the replay ring's format -- collision_term, progress_term, centering_term, total [B] fp64,
    collided [B] uint8 and the state prev_xy [B, 2], t_seen [B]; they are allocated and bound by the first install and again
    only when rows / cols or the image form change.  `cfg` is the f110_shaping_config installed, `bits` the image form."""
    NAME = 'shaping'
    INFO = {'reward_collision': 'collision_term', 'reward_progress': 'progress_term', 'reward_centering': 'centering_term',
            'bitmap_collided': 'collided', 'lidar_bitmap': 'bitmap'}
    STATE = {'prev_xy': 'prev_xy', 't_seen': 't_seen', 'lidar_bitmap': 'bitmap'}
    IMAGE_KEYS = ('lidar_bitmap', 'lidar_bitmap_bits')   # the key of the bitmap in `info` and state_dict(): bytes, bits
    DTYPES = {'collision_term': torch.float64, 'progress_term': torch.float64, 'centering_term': torch.float64,
              'total': torch.float64, 'collided': torch.uint8, 't_seen': torch.float64}
    cfg, bits, _to_img = None, False, None

    def install(self, image='bytes', **cfg):
        """`cfg`: options of DEFAULTS (missing ones take SAL's numbers); `image`: 'bytes' or 'bits', how the bitmap is held --
        it is no field of the config: it selects the buffer, its binding, the renderer's call and the bitmap's key
        (IMAGE_KEYS).  An install starts the shaper anew (restart()).  TypeError for an unknown option, ValueError for what the
        library refuses."""
        bits = image_form(image)
        eng = self.eng
        c = make_config(**cfg)
        _lib.check(eng.lib.f110_shaping_install(eng._h, C.byref(c)))
        shape = (eng.B, c.rows, words(c.cols)) if bits else (eng.B, c.rows, c.cols)
        with torch.cuda.device(eng.device):
            if self.buf is None or tuple(self.buf['bitmap'].shape) != shape or bits != self.bits:
                buf = {k: torch.zeros((eng.B,), dtype=dt, device=eng.device) for k, dt in self.DTYPES.items()}
                buf['prev_xy'] = torch.zeros((eng.B, 2), dtype=torch.float64, device=eng.device)
                buf['bitmap'] = torch.zeros(shape, dtype=torch.int64 if bits else torch.uint8, device=eng.device)
                self.bits = bits
                key = self.IMAGE_KEYS[bits]
                self.INFO = {k: v for k, v in type(self).INFO.items() if v != 'bitmap'}
                self.STATE = {k: v for k, v in type(self).STATE.items() if v != 'bitmap'}
                self.INFO[key] = self.STATE[key] = 'bitmap'
                self._bind(buf, _lib.ShapingBuffers, {'bitmap': None if bits else 'bitmap', 'bitmap_bits': 'bitmap' if bits else None})
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
        draw = self._to_img.bits if self.bits else self._to_img
        draw(self.eng.t['scans'][:, self.cfg.agent], out=self.buf['bitmap'])

    def restart(self):
        """The next update takes its previous position from its own pose (it pays no progress) and reads the image of the
        scans as they stand."""
        self.buf['t_seen'].fill_(-1.0)
        self.render()

    def state_keys(self):
        return set(self.STATE) | set(self.IMAGE_KEYS)

    def load(self, sd):
        """A checkpoint that holds the bitmap in the other form is converted (f110_replay_pack / f110_replay_unpack)."""
        mine, other = self.IMAGE_KEYS[self.bits], self.IMAGE_KEYS[not self.bits]
        if mine not in sd and other in sd and sd[other].dim() == 3:
            img = sd[other].to(self.eng.device)
            if self.bits:
                sd = dict(sd, **{mine: pack_bitmaps(img)})
            elif img.shape[2] == words(self.cfg.cols):
                sd = dict(sd, **{mine: unpack_bitmaps(img, self.cfg.cols)})
        Consumer.load(self, sd)

    def close(self):
        if self._to_img is not None:
            self._to_img.close()
            self._to_img = None
