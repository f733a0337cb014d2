"""The checker of the fused policy stem (csrc/f110_bitconv2.h), NumPy only: the numerics contract of include/f110_hip.h restated
step by step in float32 -- a1 = the first layer as bitconv_cases.forward; acc = 0; for ci major, ky, kx minor: acc = fma(w2[co][ci]
[ky][kx], a1[ci][s2 oy + ky][s2 ox + kx], acc) with one rounding per step; out = acc + b2[co]; out < 0 ? 0 : out with relu2 -- so that
the GPU's output can be compared with `==`; and the banding arithmetic of the kernel restated, so that every case can be shown to
select what its comment claims."""
import numpy as np

import bitconv_cases as bc
import replay_cases as rc

# csrc/f110_bitconv2.h
BC2_KSTEPS, BC2_ACCS, BC2_LDS_BYTES, BC2_MAX_GRID, BC2_MAX_OW1 = 64, 6, 64 * 1024, 2048, 64

# (rows, cols, k1, s1, C1, k2, s2, C2); what each selects is asserted from paths2() in test_bitconv2_cpu.py
CASES2 = [
    (256, 256, 8, 4, 16, 4, 2, 32),   # SAL: five bands of six rows, K = 256 (four blocks of 16 steps), two N-tiles, six M-tiles per wave, vector stores
    (72, 260, 8, 4, 16, 4, 2, 32),    # OW1 exactly 64, OH1 17 (odd): two bands, the last of one output row; planes of 7 x 31: scalar stores
    (24, 260, 8, 4, 16, 4, 2, 32),    # OW1 64, one band of one output row, two M-tiles on two waves and two idle ones
    (41, 101, 3, 2, 5, 3, 2, 7),      # cols no multiple of 16, a conv1 row and column left over, K = 45 padded to 48, a partial M-tile, kernel 3
    (9, 128, 2, 2, 3, 1, 1, 5),       # k2 = 1, s2 = 1: K = 3 in one step, OW2 = 64, kernel 2
    (40, 300, 7, 5, 4, 4, 4, 20),     # k2 = 4, s2 = 4 (the windows do not overlap), two N-tiles of which one partial, kernel 7
    (30, 200, 6, 6, 9, 2, 1, 64),     # k2 = 2, s2 = 1, C2 = 64: four N-tiles, a wave alone on eight M-tiles (two runs of accumulators), kernel 6
    (30, 120, 5, 2, 16, 3, 1, 33),    # C2 = 33: three N-tiles, two waves reload their weights; K = 144 (three blocks), kernel 5
    (12, 190, 4, 3, 1, 2, 2, 3),      # C1 = 1: K = 4, one step without padding, kernel 4
    (2, 2, 1, 1, 16, 2, 1, 1),        # one output pixel, kernel 1
    (20, 100, 3, 2, 8, 4, 3, 16),     # K = 128 (two blocks), s2 = 3
]
SAL = CASES2[0]
# more work items than workgroups of a launch: a workgroup walks two or three of them (n samples of one band through an index)
LOOP_CASE, LOOP_N = (8, 16, 4, 4, 2, 1, 1, 3), 2 * BC2_MAX_GRID + 5
# (on, relu1, relu2, b1, b2): every `on`, both relus both ways, both biases present and NULL
VARIANTS = ((1.0, True, True, True, True), (255.0, True, False, False, False), (1.0 / 255.0, False, True, True, False), (1.0, False, False, False, True))


def out_size2(rows, cols, k1, s1, k2, s2):
    oh1, ow1 = bc.out_size(rows, cols, k1, s1)
    return (oh1 - k2) // s2 + 1, (ow1 - k2) // s2 + 1


def lds_bytes(k1, s1, c1, k2, s2, br, xw):
    nr1 = (br - 1) * s2 + k2
    return ((nr1 - 1) * s1 + k1) * bc.BC_LWORDS * 8 + BC2_KSTEPS * 4 * 4 + c1 * nr1 * xw * 4


def paths2(rows, cols, k1, s1, c1, k2, s2, c2, n=3):
    """What csrc/f110_bitconv2.h does with n images, restated from its arithmetic (bitconv2_geometry on the host, the kernel's
    split of tiles among waves).  oh1, ow1, oh2, ow2; xw: columns of a1 that conv2 reads, unused_cols / unused_rows: conv1
    columns / rows no window reaches; ktot = C1 k2 k2, ksteps = ceil(ktot / 4), kpad: K is padded, blocks: ceil(ksteps / 16), the
    instantiation of the multiply; br: output rows of a band (the most whose LDS fits BC2_LDS_BYTES), bands, last_rows: rows of
    the last band; lds: bytes of a workgroup; straddles: a window of the first layer crosses a word boundary; u8_bytes: the
    uint8 entry thresholds a row's end byte by byte; NT: N-tiles of 16 channels, partial_n: the last holds fewer; nwn: waves
    side by side in N, mw: waves sharing the M-tiles; reload: a wave owns two N-tiles; MT: M-tiles of a full band, partial_m:
    the band's pixels are no multiple of 16; per: M-tiles of a wave's run, runs: passes of BC2_ACCS accumulators over it,
    ragged: the last pass holds fewer; idle: a wave without M-tiles; vec / scalar: some lane stores four pixels at once / one
    by one (for an `out` aligned to 16 bytes); items, grid, walks: work items, workgroups, and the most items one walks."""
    oh1, ow1 = bc.out_size(rows, cols, k1, s1)
    oh2, ow2 = (oh1 - k2) // s2 + 1, (ow1 - k2) // s2 + 1
    xw = (ow2 - 1) * s2 + k2
    ktot = c1 * k2 * k2
    ksteps = -(-ktot // 4)
    br = 1
    while br < oh2 and lds_bytes(k1, s1, c1, k2, s2, br + 1, xw) <= BC2_LDS_BYTES:
        br += 1
    bands = -(-oh2 // br)
    last_rows = oh2 - (bands - 1) * br
    pos = np.arange(xw) * s1
    NT = -(-c2 // 16)
    nwn = 4 if NT >= 4 else 2 if NT >= 2 else 1
    mw = 4 // nwn
    vec = scalar = idle = ragged = False
    runs = 0
    for band in range(bands):
        nyb = min(br, oh2 - band * br)
        mband = nyb * ow2
        MT = -(-mband // 16)
        per = -(-MT // mw)
        for mg in range(mw):
            mine = min(MT, (mg + 1) * per) - mg * per
            idle = idle or mine <= 0
            if mine > 0:
                runs = max(runs, -(-mine // BC2_ACCS))
                ragged = ragged or mine % BC2_ACCS != 0
        for co in range(c2):
            for m0 in range(0, MT * 16, 4):
                v = m0 + 4 <= mband and ((co * oh2 * ow2 + band * br * ow2 + m0) * 4) % 16 == 0
                vec, scalar = vec or v, scalar or (not v and m0 < mband)
    mband = br * ow2
    items = n * bands
    grid = min(items, BC2_MAX_GRID)
    return dict(oh1=oh1, ow1=ow1, oh2=oh2, ow2=ow2, xw=xw, unused_cols=ow1 - xw, unused_rows=oh1 - ((oh2 - 1) * s2 + k2), ktot=ktot,
                ksteps=ksteps, kpad=ktot % 4 != 0, blocks=-(-ksteps // 16), br=br, bands=bands, last_rows=last_rows,
                lds=lds_bytes(k1, s1, c1, k2, s2, br, xw), straddles=bool(((pos & 63) + k1 > 64).any()), u8_bytes=cols % 16 != 0,
                NT=NT, partial_n=c2 % 16 != 0, nwn=nwn, mw=mw, reload=NT == 3, MT=-(-mband // 16), partial_m=mband % 16 != 0,
                per=-(-(-(-mband // 16)) // mw), runs=runs, ragged=ragged, idle=idle, vec=vec, scalar=scalar, items=items, grid=grid,
                walks=-(-items // grid))


def fma32(a, b, c):
    """fp32 fma(a, b, c), exactly, on arrays: in fp64 the product of two fp32 is exact; its sum with c is rounded to odd (TwoSum
    gives the error of the fp64 addition; where there is one and the sum's last bit is 0, the neighbour towards the error is
    taken), and an odd-rounded fp64 rounds to fp32 as the exact value would."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def accumulate2(a1, w2, s2):
    """The fma chain of layer 2 on a1 [n, C1, OH1, OW1] -> acc [n, C2, OH2, OW2] float32, before bias and relu."""
    a1, w2 = np.asarray(a1, np.float32), np.asarray(w2, np.float32)
    c2, c1, k2, _ = w2.shape
    n, _, oh1, ow1 = a1.shape
    oh2, ow2 = (oh1 - k2) // s2 + 1, (ow1 - k2) // s2 + 1
    acc = np.zeros((n, c2, oh2, ow2), np.float32)
    for ci in range(c1):
        for ky in range(k2):
            for kx in range(k2):
                x = a1[:, ci, ky:ky + (oh2 - 1) * s2 + 1:s2, kx:kx + (ow2 - 1) * s2 + 1:s2]
                acc = fma32(w2[None, :, ci, ky, kx, None, None], x[:, None], acc)
    return acc


def finish2(acc, b2, relu2):
    b = np.zeros(acc.shape[1], np.float32) if b2 is None else np.asarray(b2, np.float32)
    out = acc + b[None, :, None, None]
    assert out.dtype == np.float32
    return np.where(out < 0, np.float32(0.0), out).astype(np.float32) if relu2 else out


def forward2(imgs, w1, b1, s1, on, relu1, w2, b2, s2, relu2):
    """The contract on uint8 images [n, rows, cols] -> [n, C2, OH2, OW2] float32."""
    return finish2(accumulate2(bc.forward(imgs, w1, b1, s1, on, relu1), w2, s2), b2, relu2)


def conv2_fp64(a1, w2, b2, s2):
    """(conv2 of a1 in float64 with bias, before relu; the sum of |w2 a1| per output) for the bounds of an fp32 sum."""
    a1, w2 = np.asarray(a1, np.float64), np.asarray(w2, np.float64)
    c2, c1, k2, _ = w2.shape
    n, _, oh1, ow1 = a1.shape
    oh2, ow2 = (oh1 - k2) // s2 + 1, (ow1 - k2) // s2 + 1
    out, mag = np.zeros((n, c2, oh2, ow2)), np.zeros((n, c2, oh2, ow2))
    for ci in range(c1):
        for ky in range(k2):
            for kx in range(k2):
                t = w2[None, :, ci, ky, kx, None, None] * a1[:, None, ci, ky:ky + (oh2 - 1) * s2 + 1:s2, kx:kx + (ow2 - 1) * s2 + 1:s2]
                out += t
                mag += np.abs(t)
    if b2 is not None:
        out += np.asarray(b2, np.float64)[None, :, None, None]
        mag += np.abs(np.asarray(b2, np.float64))[None, :, None, None]
    return out, mag


def params2(k1, c1, k2, c2, seed=0):
    """(w1, b1, w2, b2) in fp32 of mixed sign and magnitude (bc.params for each layer's draw), so that the order of the sum matters."""
    w1, b1 = bc.params(k1, c1, seed)
    rng = np.random.default_rng([k2, c1, c2, seed, 2])
    w2 = (rng.normal(size=(c2, c1, k2, k2)) * 10.0 ** rng.integers(-2, 2, (c2, c1, k2, k2))).astype(np.float32)
    b2 = rng.normal(size=c2).astype(np.float32)
    return w1, b1, w2, b2


def images2(rows, cols):
    """bc.images; where the arbitrary image of replay_cases sets so few pixels that no window of a small image holds one, a
    seeded image of half set pixels takes its place."""
    imgs = bc.images(rows, cols).copy()
    if (imgs[0] == 255).mean() < 0.05:
        imgs[0] = np.where(np.random.default_rng([rows, cols]).random((rows, cols)) < 0.5, 255, 254).astype(np.uint8)
    return imgs
