"""CHECKER, images and pose sets for the reward shaper (csrc/f110_shaping.h) -- test infrastructure, never imported by the
product.  The checker restates the semantics of include/f110_hip.h ("Reward shaping") in Python scalars; it is pinned on the
reference's own SACF110Env._calculate_rewards by tests/golden/g16_shaping.npz (test_shaping_cpu.py), and the GPU tests demand
`==` of it for every output of the kernel."""
import math

import numpy as np

DEFAULTS = dict(rows=256, cols=256, agent=0, neighborhood=1, clip_max=255, scale=10.0, origin_x=128.0, origin_y=128.0,
                max_lane_halfwidth=50.0, w_collision=-100.0, w_progress=10.0, w_centering=2.0)
TERMS = ('collision_term', 'progress_term', 'centering_term', 'total')


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def world_to_pixel(v, origin, scale, clip_max):
    """clip(trunc(origin + v * scale), 0, clip_max) for every finite v (Python's int is unbounded; a product that
    overflowed to +-inf clips like any other value beyond the interval)."""
    p = origin + float(v) * scale
    if math.isinf(p):
        return clip_max if p > 0 else 0
    return min(max(int(p), 0), clip_max)


def collided(img, px, py, n):
    rows, cols = img.shape
    for dy in range(-n, n + 1):
        for dx in range(-n, n + 1):
            if dx == 0 and dy == 0:
                continue
            nx, ny = px + dx, py + dy
            if 0 <= nx < cols and 0 <= ny < rows and img[ny, nx] == 255:
                return 1
    return 0


def row_center_distance(img, car_x, car_y):
    """|car_x - midpoint of the run of 255 around car_x in row car_y|, or None (outside the image, the car's pixel is not
    255, or a one-pixel run)."""
    rows, cols = img.shape
    if not (0 <= car_y < rows and 0 <= car_x < cols):
        return None
    left = car_x
    while left >= 0 and img[car_y, left] == 255:
        left -= 1
    left += 1
    right = car_x
    while right < cols and img[car_y, right] == 255:
        right += 1
    right -= 1
    if left >= right:
        return None
    return abs(car_x - (left + right) / 2.0)


def reward_terms(img, x, y, x0, y0, cfg=DEFAULTS):
    """The terms of one env: dict with px, py, collided, dist (NaN where the reference has None) and the four rewards."""
    x, y, x0, y0 = float(x), float(y), float(x0), float(y0)
    nan = float('nan')
    if not (math.isfinite(x) and math.isfinite(y)):
        return dict(px=0, py=0, collided=0, dist=nan, collision_term=nan, progress_term=nan, centering_term=nan, total=nan)
    px = world_to_pixel(x, cfg['origin_x'], cfg['scale'], cfg['clip_max'])
    py = world_to_pixel(y, cfg['origin_y'], cfg['scale'], cfg['clip_max'])
    hit = collided(img, px, py, cfg['neighborhood'])
    collision_term = cfg['w_collision'] if hit else 0.0
    dx, dy = x - x0, y - y0
    s = dx * dx + dy * dy
    progress_term = math.sqrt(s) * cfg['w_progress']
    dist = row_center_distance(img, int(x), int(y))
    if dist is None:
        reward = -1.0
    else:
        reward = max(0.0, 1.0 - dist / cfg['max_lane_halfwidth'])
    centering_term = reward * cfg['w_centering']
    total = ((0.0 + progress_term) + collision_term) + centering_term
    return dict(px=px, py=py, collided=hit, dist=nan if dist is None else dist, collision_term=collision_term,
                progress_term=progress_term, centering_term=centering_term, total=total)


class ShapingChecker(object):
    """The shaper of n envs with its episode logic: update() is one f110_shaping_update."""

    def __init__(self, n, timestep, cfg=DEFAULTS):
        self.n, self.timestep, self.cfg = n, float(timestep), cfg
        self.prev_xy, self.t_seen = np.zeros((n, 2)), np.full(n, -1.0)
        self.out = {k: np.zeros(n) for k in TERMS}
        self.out['collided'] = np.zeros(n, dtype=np.uint8)

    def update(self, imgs, xy, clock):
        """imgs [n, rows, cols]: the image of every env's PREVIOUS scan; xy [n, 2] the new positions; clock [n] the envs'
        current_time.  Returns the outputs (copies)."""
        for e in range(self.n):
            x, y, now = float(xy[e, 0]), float(xy[e, 1]), float(clock[e])
            if now == self.timestep:                     # reset by its last step: nothing is paid (comes first, idempotent)
                for k in TERMS:
                    self.out[k][e] = 0.0
                self.out['collided'][e] = 0
                self.prev_xy[e] = (x, y)
                self.t_seen[e] = now
                continue
            if now == self.t_seen[e]:                    # not stepped since its previous update: untouched
                continue
            x0, y0 = (x, y) if self.t_seen[e] < 0 else self.prev_xy[e]
            r = reward_terms(imgs[e], x, y, x0, y0, self.cfg)
            for k in TERMS:
                self.out[k][e] = r[k]
            self.out['collided'][e] = r['collided']
            if math.isfinite(x) and math.isfinite(y):
                self.prev_xy[e] = (x, y)
            self.t_seen[e] = now
        return {k: v.copy() for k, v in self.out.items()}


def same(a, b):
    """Element-wise equality with NaN == NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == 'f' or b.dtype.kind == 'f':
        return (a == b) | (np.isnan(a) & np.isnan(b))
    return a == b


# ---------------------------------------------------------------------------------------------- images
def hand_images(rows, cols):
    """Hand-built 0 / 255 images for the edges of the run search, [k, rows, cols]; the rows used are 0 .. 9 (every size
    has at least 10): row 0 empty, row 1 full, row 2 a run touching column 0, row 3 a run touching column cols-1, row 4
    one-pixel runs, row 5 a long run with holes, row 6 runs that end exactly on the 64-pixel chunk borders, row 7
    alternating pixels, rows 8-9 full (neighbours for the collision test)."""
    out = []
    a = np.zeros((rows, cols), np.uint8)
    a[1, :] = 255
    a[2, :max(2, cols // 3)] = 255
    a[3, cols - max(2, cols // 4):] = 255
    a[4, ::7] = 255
    a[5, 1:cols - 1] = 255
    a[5, cols // 2] = 0
    a[5, min(cols - 2, 70)] = 0
    for b in range(0, cols, 64):
        a[6, b:min(b + 64, cols)] = 255 if (b // 64) % 2 == 0 else 0
    a[7, ::2] = 255
    a[8:10, :] = 255
    out.append(a)
    b = a.copy()                                           # the same rows further down, and chunk borders off by one
    b[6, :] = 255
    b[6, [c for c in (63, 64, 127, 128, 191, 192, 255, 256) if c < cols]] = 0
    b[10:, :] = 255 if rows > 10 else 0
    out.append(b)
    c = np.full((rows, cols), 255, np.uint8)               # everything filled but the border columns and a diagonal
    c[:, 0] = 0
    c[:, cols - 1] = 0
    for r in range(rows):
        c[r, (r * 5) % cols] = 0
    out.append(c)
    out.append(np.zeros((rows, cols), np.uint8))           # nothing filled
    out.append(np.full((rows, cols), 255, np.uint8))       # everything filled: every row one run from edge to edge
    d = np.zeros((rows, cols), np.uint8)                   # the left two thirds filled, a hole every 11th row
    d[:, :2 * cols // 3] = 255
    d[::11, cols // 5] = 0
    out.append(d)
    return np.stack(out)


def designed_poses(rows, cols, n, seed, cfg=DEFAULTS):
    """n cases (x, y, x0, y0) for an image of rows x cols that reach every branch whatever the image holds: positions
    inside the image in raw metres (centering), around the image centre (where a FILL image is filled), on the first
    rows (the hand-built ones), pixel coordinates just either side of an integer, negative coordinates, |x| large enough
    to clip, 1e300, and positions outside the image."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4))
    for k in range(n):
        kind = k % 12
        if kind == 0:                 # anywhere inside the image, in metres
            x, y = rng.uniform(0, cols), rng.uniform(0, rows)
        elif kind == 1:               # inside the image, far from its centre column: a wide run's reward clamps to 0
            x, y = rng.choice([rng.uniform(0, cols / 5), rng.uniform(4 * cols / 5, cols)]), rng.uniform(0, rows)
        elif kind in (2, 3):          # around the centre of the image: a FILL image is filled there
            x, y = cols / 2 + rng.uniform(-cols / 4, cols / 4), rows / 2 + rng.uniform(-rows / 6, rows / 6)
        elif kind in (5, 6):          # the hand-built rows
            x, y = rng.uniform(-0.9, cols + 0.5), rng.uniform(0, 10)
        elif kind == 7:               # a pixel coordinate one step either side of an integer; metres around zero
            px, py = rng.integers(0, cfg['clip_max'] + 2), rng.integers(0, cfg['clip_max'] + 2)
            x = np.nextafter((px - cfg['origin_x']) / cfg['scale'], rng.choice([-np.inf, np.inf]))
            y = np.nextafter((py - cfg['origin_y']) / cfg['scale'], rng.choice([-np.inf, np.inf]))
        elif kind in (4, 8):          # a track-sized pose: negative coordinates, pixels all over the image
            x, y = rng.uniform(-14, 14), rng.uniform(-14, 14)
        elif kind == 9:               # clipped pixels, outside the image in metres
            x, y = rng.choice([-1e3, 1e3, -40.0, 300.5, 1e300, -1e300]), rng.choice([-77.0, 5.5, 1e300, 1e9, float(rows), -1.0])
        elif kind == 10:              # just either side of the image's edges in metres
            x = rng.choice([-1.0, np.nextafter(-1.0, 0), -0.5, 0.0, cols - 1.0, np.nextafter(float(cols), 0), float(cols)])
            y = rng.choice([-1.0, np.nextafter(-1.0, 0), -0.5, 0.0, rows - 1.0, np.nextafter(float(rows), 0), float(rows)])
        else:                         # integer metres exactly
            x, y = float(rng.integers(0, cols)), float(rng.integers(0, rows))
        step = rng.choice([0.0, 0.02, 0.3, 5.0])
        ang = rng.uniform(0, 2 * np.pi)
        out[k] = (x, y, x - step * np.cos(ang), y - step * np.sin(ang))
    return out


def unpack_images(g, group):
    """Images of one size group of g16 as [k, rows, cols] uint8 of 0 / 255."""
    rows, cols = (int(v) for v in g['shape_' + group])
    bits = np.unpackbits(g['img_' + group], axis=1)[:, :rows * cols]
    return (bits.reshape(-1, rows, cols) * 255).astype(np.uint8)


GROUPS = ('a', 'b', 'c')    # 256 x 256, 75 x 100, 40 x 300
