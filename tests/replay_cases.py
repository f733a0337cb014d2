"""The checker of the replay buffer (csrc/f110_replay.h), NumPy and Python ints only: the packed frame format, the splitmix64
draw, and a mirror of the ring built on collections.deque, which is what the reference's ReplayBuffer (src/SAL.py:447-463) is."""
from collections import deque

import numpy as np

TRIES = 64
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
FIFO_CAPACITIES = (1, 3, 8)


def words(cols):
    return (cols + 63) // 64


def pack(imgs):
    """[n, rows, cols] uint8 -> [n, rows, words] uint64: np.packbits(row == 255, bitorder='little') zero-padded to 8 * words bytes."""
    imgs = np.asarray(imgs)
    n, rows, cols = imgs.shape
    w = words(cols)
    by = np.packbits(imgs == 255, axis=2, bitorder='little')
    out = np.zeros((n, rows, 8 * w), np.uint8)
    out[:, :, :by.shape[2]] = by
    return np.ascontiguousarray(out).view('<u8').reshape(n, rows, w)


def unpack(packed, cols):
    """[n, rows, words] uint64 -> [n, rows, cols] uint8 of 0 / 255."""
    packed = np.ascontiguousarray(np.asarray(packed).astype('<u8'))
    n, rows, w = packed.shape
    bits = np.unpackbits(packed.view(np.uint8).reshape(n, rows, 8 * w), axis=2, bitorder='little')
    return (bits[:, :, :cols] * 255).astype(np.uint8)


def edge_images(rows, cols):
    """All-0, all-255, one pixel at columns 0, 63, 64 and cols - 1 (those the row has), and one of arbitrary bytes with some 255
    (only 255 is a set bit: 254, 128 and 1 are not)."""
    out = [np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)]
    for k, c in enumerate(sorted({min(c, cols - 1) for c in (0, 63, 64, cols - 1)})):
        a = np.zeros((rows, cols), np.uint8)
        a[(k * 7) % rows, c] = 255
        out.append(a)
    rng = np.random.default_rng(rows * 1000 + cols)
    a = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    a[rng.uniform(size=(rows, cols)) < 0.3] = 255
    a.flat[::5] = 254
    out.append(a)
    return np.stack(out)


def random_images(rows, cols, n=7, seed=0):
    """n images of arbitrary bytes, 30 % of the pixels 255; every image holds 254 and 127 where it has the room (neither is a
    set bit)."""
    rng = np.random.default_rng([rows, cols, n, seed])
    a = rng.integers(0, 256, (n, rows, cols)).astype(np.uint8)
    a[rng.uniform(size=a.shape) < 0.3] = 255
    flat = a.reshape(n, -1)
    if flat.shape[1] >= 2:
        flat[:, flat.shape[1] // 2] = 254
        flat[:, flat.shape[1] // 2 - 1] = 127
    return a


# ---------------------------------------------------------------------------------------------- the code paths a size selects
REPLAY_THREADS, REPLAY_ROWS = 256, 16      # csrc/f110_replay.h

# every path of replay_pack_image / replay_unpack_row / the gather grid, see paths() and test_replay_cpu.py
SHAPES = [(3, 64), (75, 64), (5, 128), (75, 320),                                                       # dense
          (17, 16), (33, 48), (16, 96), (224, 224), (20, 272),                                          # aligned
          (84, 84), (1, 17), (15, 15), (10, 65), (12, 255), (9, 257), (31, 260), (7, 513), (40, 1028)]  # bytewise


def paths(rows, cols):
    """What csrc/f110_replay.h does with an image of rows x cols, restated from its arithmetic.  pack: the branch of
    replay_pack_image ('dense': cols a multiple of 64, 'aligned': of 16, 'bytewise': the rest), the passes of its loop over the
    rows * 4 * words 16-bit pieces (a workgroup takes 4 * 256 per pass in the first two branches, 256 in the third) and whether
    the last pass is a partial one; unpack: the form of replay_unpack_row ('vec4': cols a multiple of 4, 4 pixels per lane and
    256 per pass; 'scalar': 64 per pass) and its passes; row_blocks: the gather's and the unpack's grid.y."""
    units = rows * 4 * words(cols)
    if cols % 16 == 0:
        branch, per_pass = ('dense' if cols % 64 == 0 else 'aligned'), 4 * REPLAY_THREADS
    else:
        branch, per_pass = 'bytewise', REPLAY_THREADS
    form, per_row_pass = ('vec4', 4 * 64) if cols % 4 == 0 else ('scalar', 64)
    return dict(pack=branch, pack_passes=-(-units // per_pass), pack_last_partial=units % per_pass != 0, unpack=form,
                unpack_passes=-(-cols // per_row_pass), row_blocks=-(-rows // REPLAY_ROWS))


# the sizes the ring itself is run at (tests/test_gpu_replay.py): every pack branch and both unpack forms with one pass and with
# several, the row counts around a gather block
RING_SHAPES = [(3, 64), (75, 320), (17, 16), (16, 96), (224, 224), (20, 272), (84, 84), (1, 17), (15, 15), (10, 65), (9, 257), (40, 1028)]


def scripted_pushes(rows, cols, B, T, action_dim, timestep):
    """The inputs of 2 T + 3 pushes the test writes itself (B >= 5), a list of dicts: frame [B, rows, cols] uint8 (40 % of the
    pixels 255, the rest arbitrary bytes; another one per env and push), action [B, action_dim] fp32 (arange-distinct over push,
    env and component), reward [B] fp64, done [B] uint8 and clock [B] fp64.  Every clock advances by `timestep` per push, but env
    1 stands still at push 3 (not stepped: invalid) and env 2 reads exactly `timestep` at push 5 (its reset: invalid) after its
    done at push 4; env 4 is done at push 1 and env 0 at push 2 T + 1."""
    rng = np.random.default_rng([rows, cols, B, T, action_dim])
    clock = 0.37 + 0.11 * np.arange(B)
    out = []
    for k in range(2 * T + 3):
        frame = rng.integers(0, 255, (B, rows, cols)).astype(np.uint8)
        frame[rng.uniform(size=frame.shape) < 0.4] = 255
        step = np.full(B, float(timestep))
        if k == 3:
            step[1] = 0.0
        clock = clock + step
        if k == 5:
            clock[2] = float(timestep)
        done = np.zeros(B, np.uint8)
        done[[e for e, at in ((2, 4), (4, 1), (0, 2 * T + 1)) if at == k]] = 1
        action = (np.arange(B * action_dim).reshape(B, action_dim) + 10000.0 * k).astype(np.float32)
        out.append(dict(frame=frame, action=action, reward=rng.normal(size=B) * 10.0 ** rng.integers(-3, 4, B), done=done, clock=clock.copy()))
    return out


def binary(frame):
    """What a stored frame reads back as: 255 where the pixel is 255, 0 elsewhere."""
    return np.where(np.asarray(frame) == 255, 255, 0).astype(np.uint8)


def splitmix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(valid, count, seed, first, n):
    """n draws over `valid` [T, B] after `count` pushes: (indices, ok, candidates tried).  Attempt k of draw j takes z =
    splitmix64(seed + GOLDEN * (1 + j * TRIES + k)), candidate = (z * stored * B) >> 64 -> (age, env), step slot = (count - 1 - age) % T."""
    valid = np.asarray(valid)
    T, B = valid.shape
    stored = min(max(int(count), 0), T)
    total = stored * B
    idx, ok, cands = [], [], []
    for i in range(n):
        j = (first + i) & M64
        pick = -1
        if total > 0:
            for k in range(TRIES):
                z = splitmix64(seed + GOLDEN * (1 + j * TRIES + k))
                cand = (z * total) >> 64
                cands.append(cand)
                age, env = divmod(cand, B)
                slot = (count - 1 - age) % T
                if valid[slot, env]:
                    pick = slot * B + env
                    break
        idx.append(pick)
        ok.append(int(pick >= 0))
    return np.array(idx, np.int64), np.array(ok, np.uint8), cands


# the synthetic input of the draw test on the GPU: the CPU suite shows that every draw on it finds a transition (ok = 1), so the
# redraw hides nothing there
DRAW_CASE = dict(T=5, B=7, count=13, seed=12345, n=256)


def draw_case_valid():
    T, B = DRAW_CASE['T'], DRAW_CASE['B']
    s, e = np.meshgrid(np.arange(T), np.arange(B), indexing='ij')
    return ((s * 7 + e * 3) % 4 != 0).astype(np.uint8)


def fifo(capacity, pushes):
    """deque(maxlen=capacity) after `pushes` appends of 0, 1, 2, ...: (len, the ids that survive, oldest first)."""
    d = deque(maxlen=capacity)
    for i in range(pushes):
        d.append(i)
    return len(d), list(d)


class Mirror(object):
    """The ring as the reference would keep it: a deque(maxlen=T) of pushes, each holding for every env what
    replay_buffer.push(obs, action, reward, next_obs, done) was given -- or nothing where the transition is invalid."""

    def __init__(self, T, B, rows, cols, action_dim, timestep):
        self.T, self.B, self.rows, self.cols, self.ad, self.timestep = T, B, rows, cols, action_dim, timestep
        self.steps = deque(maxlen=T)
        self.count, self.chain_start = 0, 0
        self.prev_frame = None
        self.t_seen = np.full(B, -1.0)

    def break_chain(self):
        self.chain_start = self.count
        self.t_seen[:] = -1.0

    def push(self, frame, action, reward, done, clock):
        """What the step returned for all envs; returns the valid flags [B] the push decides."""
        clock = np.asarray(clock, np.float64)
        valid = (self.count > self.chain_start) & (clock != self.timestep) & (clock != self.t_seen)
        rec = []
        for e in range(self.B):
            if valid[e]:
                rec.append((self.prev_frame[e].copy(), np.asarray(action[e], np.float32).copy(), float(reward[e]), frame[e].copy(), int(bool(done[e]))))
            else:
                rec.append(None)
        self.steps.append((self.count, rec))
        self.prev_frame = np.array(frame, copy=True)
        self.t_seen = clock.copy()
        self.count += 1
        return valid.astype(np.uint8)

    def __len__(self):
        return sum(r is not None for _, rec in self.steps for r in rec)

    def valid_array(self):
        v = np.zeros((self.T, self.B), np.uint8)
        for c, rec in self.steps:
            v[c % self.T] = [r is not None for r in rec]
        return v

    def at(self, indices):
        """(s, a, r, ns, d, ok) for indices = step slot * B + env; zeros and ok = 0 for -1, an invalid or an evicted one."""
        n = len(indices)
        s, ns = np.zeros((n, self.rows, self.cols), np.uint8), np.zeros((n, self.rows, self.cols), np.uint8)
        a, r = np.zeros((n, self.ad), np.float32), np.zeros(n, np.float64)
        d, ok = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        by_slot = {c % self.T: rec for c, rec in self.steps}
        for i, idx in enumerate(indices):
            idx = int(idx)
            if not 0 <= idx < self.T * self.B:
                continue
            slot, env = divmod(idx, self.B)
            t = by_slot.get(slot, [None] * self.B)[env]
            if t is not None:
                s[i], a[i], r[i], ns[i], d[i], ok[i] = t[0], t[1], t[2], t[3], t[4], 1
        return s, a, r, ns, d, ok
