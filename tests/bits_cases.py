"""Scans, image sizes and the NumPy packing for the bits form of the lidar bitmap (f110_bitmap_render_bits, the shaper and the
replay push behind shape_rewards(image='bits')) -- test infrastructure, never imported by the product."""
import numpy as np

MODES = ('FILL', 'POLYGON', 'RAYS')

# (rows, cols): both parities of ceil(cols / 32), cols below one word, rows for half of the kernel's threads (two threads per row
# in FILL's parity pass), the 16-byte store path (cols a multiple of 128) and the per-word one
SIZES = [(256, 256), (75, 100), (40, 300), (9, 257), (10, 65), (15, 15), (1, 17)]


def words(cols):
    return (cols + 63) // 64


def pack(on):
    """[n, rows, cols] bool (pixel holds the draw colour) -> [n, rows, words] uint64: np.packbits(bitorder='little') of every
    row, zero-padded to 8 * words bytes -- tests/replay_cases.pack with the comparison left to the caller."""
    on = np.asarray(on, dtype=bool)
    n, rows, cols = on.shape
    w = words(cols)
    by = np.packbits(on, axis=2, bitorder='little')
    out = np.zeros((n, rows, 8 * w), np.uint8)
    out[:, :, :by.shape[2]] = by
    return np.ascontiguousarray(out).view('<u8').reshape(n, rows, w)


def unpack(packed, cols):
    """[n, rows, words] uint64 -> [n, rows, cols] uint8 of 0 / 255."""
    packed = np.ascontiguousarray(np.asarray(packed).astype('<u8'))
    n, rows, w = packed.shape
    bits = np.unpackbits(packed.view(np.uint8).reshape(n, rows, 8 * w), axis=2, bitorder='little')
    return (bits[:, :, :cols] * 255).astype(np.uint8)


def as_u64(t):
    """An int64 device tensor of packed words as a NumPy uint64 array."""
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)


def scans(n, nb=1080, seed=0, reach=12.0):
    """n scans of nb beams: a corridor with occlusion jumps, an all-noise scan, one that leaves the image everywhere, one that
    stays within a few pixels of the centre, then corridors again.  `reach`: the corridor's size in metres (an image of a few
    pixels wants a small one, so that its polygon has an inside)."""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2 * np.pi, nb)
    out = np.empty((n, nb))
    for i in range(n):
        kind = i % 5
        if kind == 1:
            out[i] = rng.uniform(0, reach, nb)
        elif kind == 2:
            out[i] = rng.uniform(5 * reach, 8 * reach, nb)
        elif kind == 3:
            out[i] = rng.uniform(0, 0.3, nb)
        else:
            base = 0.2 * reach + 0.15 * reach * np.abs(np.sin(th * rng.integers(1, 4) + rng.uniform(0, 6)))
            base = base / np.maximum(np.abs(np.cos(th + rng.uniform(0, 6))), 0.08)
            jumps = rng.random(nb) < 0.01
            base = np.where(np.cumsum(jumps) % 2 == 1, base * rng.uniform(1.5, 4), base)
            out[i] = np.clip(base, 0, 3 * reach) + rng.normal(0, 0.01, nb)
    return out
