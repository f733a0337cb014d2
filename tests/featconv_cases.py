"""The checkers of the dense feature-map convolution (csrc/f110_featconv.h), NumPy only: the numerics contract of include/f110_hip.h
restated step by step in float32 so that the GPU's results can be compared with `==` -- the forward is bitconv2_cases' second layer
(finish2(accumulate2(x, w, s), b, relu)); grad_x is the chain over co major, ky, kx minor of the terms whose output pixel exists;
the per-sample partials of grad_weight are chains over the output pixels oy major, ox minor, those of grad_bias plain adds, and
the reduction adds the samples in ascending order.  fp64 sums with their sum of magnitudes supply the bounds, and the banding
arithmetic of the three kernels is restated so that every case can be shown to select what its comment claims."""
import numpy as np

import bitconv_cases as bc
from bitconv2_cases import accumulate2, conv2_fp64, finish2, fma32

# csrc/f110_featconv.h
FC_CHUNK, FC_ACCS, FC_ZERO_BYTES, FC_LDS_BYTES, FC_MAX_GRID, FCW_TILES = 8, 4, 16, 64 * 1024, 2048, 8

# (Ci, H, W, Co, k, s); what each selects is asserted from paths() in test_featconv_cpu.py
CASES = [
    (32, 30, 30, 32, 3, 1),     # SAL conv3: K = 288 in nine whole chunks, two N-tiles, two bands forward, three in grad_x, 18 N-tiles of partials
    (16, 63, 63, 32, 4, 2),     # SAL conv2: K = 256, stride 2: grad_x over a dilated g, a last row and column of x no window reaches
    (5, 11, 13, 7, 3, 2),       # K = 45 padded, partial M- and N-tiles, a dilated g (its windows reach every row and column of x: the rows
                                # and columns no window reaches are conv2's, one each, and those of (32, 6, 6, 8, 4, 3), two each)
    (3, 4, 64, 5, 1, 1),        # k = 1, W at its limit
    (16, 2, 2, 1, 2, 1),        # one output pixel
    (16, 9, 20, 33, 3, 1),      # three N-tiles
    (8, 8, 40, 64, 2, 1),       # four N-tiles, Co k^2 large
    (4, 16, 60, 20, 4, 4),      # windows that do not overlap
    (32, 6, 6, 8, 4, 3),        # Ci k^2 = 512; two rows and two columns of x no window reaches
    # kernel < stride: between two windows lie input pixels that no window reaches (holes()); grad_x is +0 there
    (3, 9, 11, 5, 1, 2),        # k = 1: every odd row and column is a hole, none is left over at the edge; K = 3 and grad_x's K = 5, one padded chunk each
    (4, 10, 13, 6, 2, 3),       # one row and column in three a hole, and two of each left over at the edge; the partials' K = 16 is one whole N-tile
    (2, 12, 14, 4, 3, 4),       # stride 4; grad_x's K = 36 takes two chunks, the partials two N-tiles; one row and three columns left over
    (5, 8, 9, 3, 1, 4),         # k = 1 under stride 4: three rows in four are holes; three rows left over, no column
]
CONV3, CONV2 = CASES[0], CASES[1]
GAP_CASES = [c for c in CASES if c[4] < c[5]]
# the recordings of the reference's own Actor: the row fed as raw 0 / 255 floats, the row fed as / 255 (tests/golden/make_golden.py g22)
GOLDEN = ('g22_trunk.npz', 'g22_trunk_unit.npz')


def golden_layers(g):
    """(name, input, stride, grad_out) of conv2 and conv3 in a recording: conv3's grad_out is the cotangent in the shape of its output,
    conv2's is conv3's grad_input (neither is stored twice)."""
    return (('conv2', g['a1'], 2, g['conv3_grad_input']), ('conv3', g['conv2_out'], 1, g['cotangent'].reshape(g['conv3_out'].shape)))


# more work items than workgroups of a launch: a workgroup walks two or three samples in all three kernels
LOOP_CASE, LOOP_N = (2, 3, 4, 3, 2, 1), 2 * FC_MAX_GRID + 5
# (relu, bias present)
VARIANTS = ((True, True), (False, False), (True, False), (False, True))


def out_size(h, w, k, s):
    return (h - k) // s + 1, (w - k) // s + 1


def holes(h, w, k, s):
    """(the [h, w] mask of the input pixels no window reaches, the mask of those that lie inside the rectangle the windows span: between
    two windows, not behind the last one)."""
    oh, ow = out_size(h, w, k, s)
    rows = (np.arange(h) % s < k) & (np.arange(h) < (oh - 1) * s + k)
    cols = (np.arange(w) % s < k) & (np.arange(w) < (ow - 1) * s + k)
    unreached = ~(rows[:, None] & cols[None, :])
    inside = (np.arange(h) < (oh - 1) * s + k)[:, None] & (np.arange(w) < (ow - 1) * s + k)[None, :]
    return unreached, unreached & inside


def gemm_lds(ktot, planes, nr, xw):
    """koff for whole chunks of K, the zeros a padding term reads, the planes."""
    return -(-ktot // (4 * FC_CHUNK)) * 4 * FC_CHUNK * 4 + FC_ZERO_BYTES + planes * nr * xw * 4


def gradw_lds(ci, co, k, s, br, ow, xw):
    return FC_ZERO_BYTES + -(-co * br * ow * 4 // 16) * 16 + ci * ((br - 1) * s + k) * xw * 4


def paths(ci, h, w, co, k, s, n=3):
    """What csrc/f110_featconv.h does with n samples, restated from its arithmetic (featconv_*_geometry on the host, the kernels'
    split of tiles among waves).  oh, ow; unused_rows / unused_cols: input rows / columns no window reaches.
    Forward: ktot = Ci k k, chunks of 32 terms, kpad: K is padded; xw: staged columns; br: output rows of a band (the most whose
    LDS fits), bands, last_rows; lds; NT: N-tiles of Co, partial_n; MT: M-tiles of a full band, partial_m; jobs: (N-tile, run of
    FC_ACCS M-tiles) of a full band, ragged: a run holds fewer; idle: a wave without a job; items, grid, walks.
    grad_x (gx_*): ktot = Co k k, chunks, kpad; xw = W + k - 1; br: input rows of a band, bands, last_rows; lds; NT of Ci; dilated.
    Partials (gw_*): ktot = Ci k k, NT its N-tiles, partial_n, groups: workgroups of a sample, idle_waves: waves without a live
    N-tile in the last group; MT: M-tiles of Co (the instantiation); br, bands, last_rows, lds; kpad: a band's pixels are no
    multiple of 4; grid, walks: workgroups in x and the most samples one walks."""
    oh, ow = out_size(h, w, k, s)
    d = dict(oh=oh, ow=ow, unused_rows=h - ((oh - 1) * s + k), unused_cols=w - ((ow - 1) * s + k))
    # forward
    ktot, xw = ci * k * k, (ow - 1) * s + k
    br = 1
    while br < oh and gemm_lds(ktot, ci, br * s + k, xw) <= FC_LDS_BYTES:
        br += 1
    bands = -(-oh // br)
    mband = br * ow
    MT, NT = -(-mband // 16), -(-co // 16)
    runs = -(-MT // FC_ACCS)
    items = n * bands
    grid = min(items, FC_MAX_GRID)
    d.update(ktot=ktot, chunks=-(-ktot // (4 * FC_CHUNK)), kpad=ktot % (4 * FC_CHUNK) != 0, xw=xw, br=br, bands=bands,
             last_rows=oh - (bands - 1) * br, lds=gemm_lds(ktot, ci, (br - 1) * s + k, xw), NT=NT, partial_n=co % 16 != 0, MT=MT,
             partial_m=mband % 16 != 0, jobs=NT * runs, ragged=MT % FC_ACCS != 0, idle=NT * runs < 4, items=items, grid=grid,
             walks=-(-items // grid))
    # grad_x
    gk, gxw = co * k * k, w + k - 1
    gbr = 1
    while gbr < h and gemm_lds(gk, co, gbr + k, gxw) <= FC_LDS_BYTES:
        gbr += 1
    gbands = -(-h // gbr)
    d.update(gx_ktot=gk, gx_chunks=-(-gk // (4 * FC_CHUNK)), gx_kpad=gk % (4 * FC_CHUNK) != 0, gx_xw=gxw, gx_br=gbr, gx_bands=gbands,
             gx_last_rows=h - (gbands - 1) * gbr, gx_lds=gemm_lds(gk, co, gbr + k - 1, gxw), gx_NT=-(-ci // 16), gx_partial_n=ci % 16 != 0,
             gx_partial_m=(gbr * w) % 16 != 0, gx_dilated=s > 1, gx_items=n * gbands)
    # partials
    wbr = 1
    while wbr < oh and gradw_lds(ci, co, k, s, wbr + 1, ow, xw) <= FC_LDS_BYTES:
        wbr += 1
    wbands = -(-oh // wbr)
    wNT = -(-ktot // 16)
    groups = -(-wNT // FCW_TILES)
    last = wNT - (groups - 1) * FCW_TILES
    pix = [min(wbr, oh - b * wbr) * ow for b in range(wbands)]
    d.update(gw_NT=wNT, gw_partial_n=ktot % 16 != 0, gw_groups=groups, gw_idle_waves=4 - -(-last // 2), gw_MT=-(-co // 16),
             gw_partial_m=co % 16 != 0, gw_br=wbr, gw_bands=wbands, gw_last_rows=oh - (wbands - 1) * wbr,
             gw_lds=gradw_lds(ci, co, k, s, wbr, ow, xw), gw_kpad=any(p % 4 for p in pix), gw_grid=min(n, FC_MAX_GRID),
             gw_walks=-(-n // min(n, FC_MAX_GRID)))
    return d


def params(ci, co, k, seed=0):
    """(weight [Co, Ci, k, k], bias [Co]) in fp32 of mixed sign and magnitude (params2's recipe), so that the order of a sum matters."""
    rng = np.random.default_rng([k, ci, co, seed, 3])
    w = (rng.normal(size=(co, ci, k, k)) * 10.0 ** rng.integers(-2, 2, (co, ci, k, k))).astype(np.float32)
    b = rng.normal(size=co).astype(np.float32)
    return w, b


def tensor(shape, seed):
    """An fp32 array of mixed sign and magnitude, a fifth of it exact zeros (as behind a ReLU)."""
    rng = np.random.default_rng([seed, 17] + list(shape))
    a = (rng.normal(size=shape) * 10.0 ** rng.integers(-2, 2, shape)).astype(np.float32)
    a[rng.random(shape) < 0.2] = 0.0
    return a


def forward(x, w, b, s, relu):
    """The contract on x [n, Ci, H, W] -> [n, Co, OH, OW] float32."""
    return finish2(accumulate2(x, w, s), b, relu)


def masked(out, grad_out, relu):
    """g of the backward: grad_out where out > 0 under relu, else grad_out."""
    grad_out = np.asarray(grad_out, np.float32)
    return np.where(np.asarray(out) > 0, grad_out, np.float32(0.0)).astype(np.float32) if relu else grad_out


def grad_x(g, w, s, h, wd):
    """grad_x [n, Ci, H, W]: for co major, ky, kx minor, acc = fma(w[co][ci][ky][kx], g[co][(iy - ky) / s][(ix - kx) / s], acc) over
    the terms whose output pixel exists (the others are skipped; fed as zeros they would leave the never negative-zero acc alone)."""
    g, w = np.asarray(g, np.float32), np.asarray(w, np.float32)
    n, co, oh, ow = g.shape
    ci, k = w.shape[1], w.shape[2]
    acc = np.zeros((n, ci, h, wd), np.float32)
    for c in range(co):
        for ky in range(k):
            for kx in range(k):
                ys, xs = slice(ky, ky + (oh - 1) * s + 1, s), slice(kx, kx + (ow - 1) * s + 1, s)
                acc[:, :, ys, xs] = fma32(w[None, c, :, ky, kx, None, None], g[:, c, None], acc[:, :, ys, xs])
    return acc


def partials(g, x, k, s):
    """(P [n, Co, Ci, k, k], B [n, Co]): per sample, for oy major, ox minor: P = fma(g[co][oy][ox], x[ci][s oy + ky][s ox + kx], P)
    and B = B + g[co][oy][ox], from 0."""
    g, x = np.asarray(g, np.float32), np.asarray(x, np.float32)
    n, co, oh, ow = g.shape
    ci = x.shape[1]
    P, B = np.zeros((n, co, ci, k, k), np.float32), np.zeros((n, co), np.float32)
    for oy in range(oh):
        for ox in range(ow):
            P = fma32(g[:, :, oy, ox, None, None, None], x[:, None, :, s * oy:s * oy + k, s * ox:s * ox + k], P)
            B = B + g[:, :, oy, ox]
    assert B.dtype == np.float32
    return P, B


def reduce(P):
    """((P[0] + P[1]) + P[2]) + ... in float32."""
    acc = np.asarray(P[0], np.float32).copy()
    for i in range(1, len(P)):
        acc = acc + P[i]
    assert acc.dtype == np.float32
    return acc


def forward_fp64(x, w, b, s):
    """(the convolution in float64 with bias, before relu; the sum of |terms|)."""
    return conv2_fp64(x, w, b, s)


def grad_x_fp64(g, w, s, h, wd):
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    n, co, oh, ow = g.shape
    ci, k = w.shape[1], w.shape[2]
    out, mag = np.zeros((n, ci, h, wd)), np.zeros((n, ci, h, wd))
    for c in range(co):
        for ky in range(k):
            for kx in range(k):
                ys, xs = slice(ky, ky + (oh - 1) * s + 1, s), slice(kx, kx + (ow - 1) * s + 1, s)
                t = w[None, c, :, ky, kx, None, None] * g[:, c, None]
                out[:, :, ys, xs] += t
                mag[:, :, ys, xs] += np.abs(t)
    return out, mag


def grad_w_fp64(g, x, k, s):
    """(grad_weight, its sum of |terms|, grad_bias, its sum of |terms|) in float64, summed over samples and pixels."""
    g, x = np.asarray(g, np.float64), np.asarray(x, np.float64)
    n, co, oh, ow = g.shape
    ci = x.shape[1]
    gw, mw = np.zeros((co, ci, k, k)), np.zeros((co, ci, k, k))
    for ky in range(k):
        for kx in range(k):
            xs = x[:, :, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s]
            gw[:, :, ky, kx] = np.einsum('nchw,ndhw->cd', g, xs)
            mw[:, :, ky, kx] = np.einsum('nchw,ndhw->cd', np.abs(g), np.abs(xs))
    return gw, mw, g.sum(axis=(0, 2, 3)), np.abs(g).sum(axis=(0, 2, 3))


def gamma(t):
    return bc.gamma(t)


_cache = {}


def reference(case, n, relu, seed=0):
    """Everything the checkers say about `case` on n samples, computed once per (case, n, relu, seed) and left unchanged: x, w, b,
    grad_out, acc (the forward's chain), out (with bias), g, grad_x, P, B, grad_weight, grad_bias."""
    key = (case, n, relu, seed)
    if key not in _cache:
        ci, h, wd, co, k, s = case
        w, b = params(ci, co, k, seed)
        x = tensor((n, ci, h, wd), seed + 1)
        acc = accumulate2(x, w, s)
        out = finish2(acc, b, relu)
        go = tensor(out.shape, seed + 2)
        g = masked(out, go, relu)
        P, B = partials(g, x, k, s)
        r = dict(x=x, w=w, b=b, grad_out=go, acc=acc, out=out, g=g, grad_x=grad_x(g, w, s, h, wd), P=P, B=B, grad_weight=reduce(P),
                 grad_bias=reduce(B))
        for v in r.values():
            v.setflags(write=False)
        _cache[key] = r
    return _cache[key]
