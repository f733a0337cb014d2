"""The checker of the bit convolution (csrc/f110_bitconv.h), NumPy only: the numerics contract of include/f110_hip.h restated tap
by tap in float32 -- acc = 0; taps ky major, kx minor: acc = acc + w[c][ky][kx] where the tap's pixel is set; out = (acc * on) +
bias[c]; out < 0 ? 0 : out with relu -- so that the GPU's output can be compared with `==`, and the gradients in float64."""
import numpy as np

import replay_cases as rc

U = 2.0 ** -24                                 # unit roundoff of fp32

# (rows, cols, kernel, stride, channels): SAL's layer; cols no multiple of 64 with windows across the word boundary at every
# phase and an odd channel count; five words with a tail word and a stride that does not divide; one output; kernel 1 on three words
CASES = [(256, 256, 8, 4, 16), (75, 100, 3, 1, 5), (40, 300, 8, 3, 1), (8, 8, 8, 8, 64), (9, 130, 1, 1, 2)]
ONS = (1.0, 255.0, 1.0 / 255.0)
BACKWARD_CASES = CASES[:3]
BACKWARD_N = (3, 67)                           # 67: a count that no block size divides

# ---------------------------------------------------------------------------------------------- the code paths a shape selects
BC_TX, BC_TY, BC_MAX_K, BC_LWORDS, BC_CHUNK, BC_MAX_PARTIALS = 64, 4, 8, 9, 16, 1024      # csrc/f110_bitconv.h
BC_LROWS = (BC_TY - 1) * BC_MAX_K + BC_MAX_K
FORWARD_GROUP = 1 << 23                        # workgroups of one forward launch at most (bitconv_forward)

# see paths() and test_bitconv_cpu.py.  Forward, packed and uint8 entry, (rows, cols, kernel, stride, channels) on the three
# images of images() and on edge images:
SHAPES = [(33, 520, 8, 8, 17),        # OH 4, OW 65: 32 rows and 8 words staged, the second x-tile is one output on the tail word (word 8)
          (20, 400, 7, 5, 33),        # kernel 7, windows across a word boundary, one partial y-tile, three chunks of channels
          (14, 420, 6, 6, 64),        # kernel 6, stride = kernel with a window at bit 60, 64 channels on two x-tiles
          (30, 150, 5, 2, 16),        # kernel 5, four y-tiles with one row in the last
          (12, 270, 4, 3, 3),         # kernel 4, windows at bits 61 .. 63
          (9, 200, 2, 1, 48),         # kernel 2, a window at bit 63, four x-tiles
          (6, 140, 2, 2, 1),          # kernel 2 that never leaves its word, one channel on two x-tiles
          (5, 129, 1, 1, 15),         # kernel 1 on three x-tiles
          (24, 260, 8, 4, 16),        # SAL's kernel and stride with OW exactly 64 and OH 5
          (7, 70, 3, 3, 20)]          # one tile, partial both ways
# Backward, (rows, cols, kernel, stride, channels, n): the same shapes; n chosen so that a workgroup walks one tile (G < 1024),
# one or two (n tiles = 1600 on G = 1024) and two or three (2200 on 1024); the large n go through an index over five frames, so grad_out is all that grows (5.9 MB at most)
BACKWARD_SHAPES = [(33, 520, 8, 8, 17, 3), (20, 400, 7, 5, 33, 1), (14, 420, 6, 6, 64, 3), (30, 150, 5, 2, 16, 3), (12, 270, 4, 3, 3, 1),
                   (9, 200, 2, 1, 48, 3), (6, 140, 2, 2, 1, 1100), (5, 129, 1, 1, 15, 3), (24, 260, 8, 4, 16, 1), (7, 70, 3, 3, 20, 1600)]
EXACT_FRAMES = 5                               # distinct frames of an exact backward case: three random, an empty, an all-set one
EXACT_ONS = ONS


def paths(rows, cols, kernel, stride, channels, n):
    """What csrc/f110_bitconv.h does with n images of rows x cols, restated from its arithmetic (bitconv_tile, bitconv_mask,
    bitconv_stage, the two host functions).  Per x-tile: nx outputs from image column 64 tx stride, that is word `wbase` bit
    `off`, `nwords` words staged per row; per y-tile: ny rows of outputs on `nrows` image rows.  Returned: oh, ow, tiles_x,
    tiles_y; the largest nrows, nwords, wbase and off over the tiles; straddles: some lane that computes an output has a window
    across a word boundary ((pos & 63) + kernel > 64, the two-word branch of bitconv_mask); partial_x / partial_y: the last tile
    of a row / column of tiles holds fewer than 64 / 4 outputs; last_word: the largest word any tile stages (always inside the
    row's `words`); tail_word: that word is the one the row's last cols % 64 pixels end in; u8_bytes: the uint8 entry thresholds
    a row's end byte by byte (cols no multiple of 16); chunks, rem: ceil(C / 16) workgroups in grid.y of the backward pass and
    the channels of a partly filled last one; G, passes: the partials and the most tiles a workgroup walks, uneven: some walk
    one fewer; group, launches: the images of one forward launch and the launches."""
    oh, ow = out_size(rows, cols, kernel, stride)
    words = rc.words(cols)
    tiles_x, tiles_y = -(-ow // BC_TX), -(-oh // BC_TY)
    nwords = wbase = off = last_word = 0
    straddles = False
    for tx in range(tiles_x):
        nx = min(BC_TX, ow - tx * BC_TX)
        col0 = tx * BC_TX * stride
        wb, of = col0 >> 6, col0 & 63
        nw = (of + (nx - 1) * stride + kernel + 63) >> 6
        pos = of + np.arange(nx) * stride
        straddles = straddles or bool(((pos & 63) + kernel > 64).any())
        nwords, wbase, off, last_word = max(nwords, nw), max(wbase, wb), max(off, of), max(last_word, wb + nw - 1)
    nrows = max((min(BC_TY, oh - ty * BC_TY) - 1) * stride + kernel for ty in range(tiles_y))
    tiles = n * tiles_x * tiles_y
    G = min(tiles, BC_MAX_PARTIALS)
    group = max(1, FORWARD_GROUP // (tiles_x * tiles_y))
    return dict(oh=oh, ow=ow, tiles_x=tiles_x, tiles_y=tiles_y, nrows=nrows, nwords=nwords, wbase=wbase, off=off, straddles=straddles,
                partial_x=ow % BC_TX != 0, partial_y=oh % BC_TY != 0, words=words, last_word=last_word,
                tail_word=cols % 64 != 0 and last_word == words - 1, u8_bytes=cols % 16 != 0,
                chunks=-(-channels // BC_CHUNK), rem=channels % BC_CHUNK, G=G, passes=-(-tiles // G), uneven=tiles % G != 0,
                group=group, launches=-(-n // group))


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k fp32 roundings."""
    return k * U / (1.0 - k * U)


def out_size(rows, cols, kernel, stride):
    return (rows - kernel) // stride + 1, (cols - kernel) // stride + 1


def images(rows, cols):
    """The three images of a forward case: one of replay_cases.random_images, an all-set one, an empty one."""
    return np.stack([rc.random_images(rows, cols, n=1, seed=11)[0], np.full((rows, cols), 255, np.uint8), np.zeros((rows, cols), np.uint8)])


def many_images(rows, cols, n):
    """n images for the backward cases: random ones, the last all-set and the one before it empty (n >= 3)."""
    a = rc.random_images(rows, cols, n=n, seed=5)
    a[-1] = 255
    a[-2] = 0
    return a


def params(kernel, channels, seed=0):
    """weight [C, 1, k, k] and bias [C] in fp32 of mixed sign and magnitude (cancellation makes the order of the taps matter)."""
    rng = np.random.default_rng([kernel, channels, seed])
    w = (rng.normal(size=(channels, 1, kernel, kernel)) * 10.0 ** rng.integers(-2, 2, (channels, 1, kernel, kernel))).astype(np.float32)
    b = rng.normal(size=channels).astype(np.float32)
    return w, b


def taps(bits, kernel, stride):
    """bits [n, rows, cols] bool -> a list over the taps (ky major, kx minor) of [n, OH, OW] bool views: tap (ky, kx) of every window."""
    n, rows, cols = bits.shape
    oh, ow = out_size(rows, cols, kernel, stride)
    return [bits[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride] for ky in range(kernel) for kx in range(kernel)]


def forward(imgs, weight, bias, stride, on, relu):
    """The contract in float32 on uint8 images [n, rows, cols] (a pixel is set iff it == 255) -> [n, C, OH, OW] float32."""
    bits = np.asarray(imgs) == 255
    w = np.asarray(weight, np.float32)
    ch, _, k, _ = w.shape
    sel = taps(bits, k, stride)
    acc = np.zeros((bits.shape[0], ch) + sel[0].shape[1:], np.float32)
    zero = np.float32(0.0)
    for t, s in enumerate(sel):
        wt = w[:, 0, t // k, t % k]
        acc = acc + np.where(s[:, None], wt[None, :, None, None], zero).astype(np.float32)
        assert acc.dtype == np.float32
    b = np.zeros(ch, np.float32) if bias is None else np.asarray(bias, np.float32)
    out = (acc * np.float32(on)).astype(np.float32) + b[None, :, None, None]
    assert out.dtype == np.float32
    if relu:
        out = np.where(out < 0, zero, out).astype(np.float32)
    return out


def gradients(imgs, grad_out, kernel, stride, on):
    """In float64 with `on` as the fp32 the kernel multiplies by: (grad_weight [C, 1, k, k], grad_bias [C], sum |grad_out * bit|
    per weight, sum |grad_out| per channel) -- the last two scale the bounds of an fp32 sum."""
    bits = np.asarray(imgs) == 255
    g = np.asarray(grad_out, np.float64)
    ch = g.shape[1]
    on = float(np.float32(on))
    gw, aw = np.zeros((ch, 1, kernel, kernel)), np.zeros((ch, 1, kernel, kernel))
    for t, s in enumerate(taps(bits, kernel, stride)):
        gs = g * s[:, None]
        gw[:, 0, t // kernel, t % kernel] = on * gs.sum(axis=(0, 2, 3))
        aw[:, 0, t // kernel, t % kernel] = np.abs(gs).sum(axis=(0, 2, 3))
    return gw, g.sum(axis=(0, 2, 3)), aw, np.abs(g).sum(axis=(0, 2, 3))


def grad_bounds(imgs, grad_out, kernel, stride, on):
    """(bound on |grad_weight error|, bound on |grad_bias error|): M = n * OH * OW terms summed in fp32 in any order, gamma_M times
    the sum of magnitudes; one more rounding for the product with `on`."""
    g = np.asarray(grad_out)
    m = g.shape[0] * g.shape[2] * g.shape[3]
    _, _, aw, ab = gradients(imgs, grad_out, kernel, stride, on)
    return gamma(m + 1) * abs(float(np.float32(on))) * aw, gamma(m) * ab


def exact_grad_out(n, channels, oh, ow):
    """grad_out of the exact backward test: integers of [-4, 4] as fp32, every element drawn on its own."""
    return np.random.default_rng([n, channels, oh, ow]).integers(-4, 5, (n, channels, oh, ow)).astype(np.float32)


def exact_index(n, with_index):
    """The frame of each of n samples out of EXACT_FRAMES: without an index sample i reads frame i % EXACT_FRAMES (the test lays
    the frames out so); with one, seeded draws with -1 at every 97th place from the second on and an entry beyond the frames at
    every 193rd from the third on (the large n only: at n = 3 the last sample takes that place); the last two samples read a
    random and the all-set frame (one sample alone: a random one)."""
    if not with_index:
        return np.arange(n, dtype=np.int64) % EXACT_FRAMES
    idx = np.random.default_rng([n, 7]).integers(0, EXACT_FRAMES, n).astype(np.int64)
    idx[1::97] = -1
    idx[2::193] = EXACT_FRAMES + 3
    idx[-1] = EXACT_FRAMES - 1 if n > 1 else 1             # (a lone all-set frame would give every tap of a channel the same sum)
    if n > 3:
        idx[-2] = 0
    return idx


def pick(imgs, index):
    """The images an index reads: imgs[index], an empty one for -1 and for an entry beyond the frames."""
    imgs, index = np.asarray(imgs), np.asarray(index)
    ok = (index >= 0) & (index < imgs.shape[0])
    return np.where(ok[:, None, None], imgs[np.where(ok, index, 0)], np.uint8(0))


def exact_sums(imgs, grad_out, kernel, stride):
    """(sum of grad_out * bit per weight [C, 1, k, k], sum of grad_out per channel [C]) as int64, for a grad_out of integers with
    n OH OW max|grad_out| < 2^24: then every partial sum of fp32 terms, in any order and under any tiling, is an integer below
    2^24 in magnitude and so exact -- the kernels have no freedom left, and the sums here are what they must give."""
    bits = np.asarray(imgs) == 255
    g = np.asarray(grad_out)
    gi = g.astype(np.int64)
    assert (gi == g).all() and g.shape[0] * g.shape[2] * g.shape[3] * max(int(np.abs(gi).max()), 4) < 2 ** 24
    sw = np.zeros((g.shape[1], 1, kernel, kernel), np.int64)
    for t, s in enumerate(taps(bits, kernel, stride)):
        sw[:, 0, t // kernel, t % kernel] = (gi * s[:, None]).sum(axis=(0, 2, 3))
    return sw, gi.sum(axis=(0, 2, 3))


def exact_gradients(sums, on):
    """What the contract leaves of the exact sums: grad_weight = fp32(sum) * fp32(on), one correctly rounded product, and
    grad_bias = the sum."""
    sw, sb = sums
    assert np.abs(sw).max() < 2 ** 24 and np.abs(sb).max() < 2 ** 24
    gw = sw.astype(np.float32) * np.float32(on)
    assert gw.dtype == np.float32
    return gw, sb.astype(np.float32)


def holds_something(sums):
    """The exact comparison can see a lost, swapped or misplaced channel: no channel's sums are all zero, no two neighbouring
    channels have the same, and in every chunk of BC_CHUNK channels beyond the first some channel differs from the one BC_CHUNK
    before it."""
    sw, sb = sums
    ch = sw.shape[0]
    flat = np.concatenate([sw.reshape(ch, -1), sb[:, None]], axis=1)
    assert (flat != 0).any(axis=1).all() and (sw != 0).any()
    assert (flat[1:] != flat[:-1]).any(axis=1).all()
    for c0 in range(BC_CHUNK, ch, BC_CHUNK):
        assert (flat[c0:c0 + BC_CHUNK] != flat[c0 - BC_CHUNK:c0 - BC_CHUNK + min(BC_CHUNK, ch - c0)]).any()
    return True


def bit_patterns(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
