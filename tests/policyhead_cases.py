"""The checker of the policy head (csrc/f110_policyhead.h), NumPy only: the numerics contract of include/f110_hip.h restated -- the
pre-activations as the fp32 fma chain in k order (bitconv2_cases.fma32, exact), so that the GPU's `pre` can be compared with `==`;
the tail and the analytic gradients in fp64 with bounds worked out from the formulas and the documented accuracy of the math
functions, never from the kernel's output; and the tiling of the kernels restated, so that every shape can be shown to select what
its comment claims."""
import numpy as np

import bitconv2_cases as b2
import bitconv_cases as bc

# csrc/f110_policyhead.h and include/f110_hip.h
PH_ROWS, PH_LDS_BYTES, PH_MAX_GRID, PH_PREFETCH, PH_GH_ROWS, PH_THREADS = 64, 64 * 1024, 512, 64, 16, 256
R = 256                                   # F110_POLICYHEAD_SLICE_ROWS
MAX_K, MAX_A = 4096, 32
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# (n, K, A); what each selects is asserted from paths() in test_policyhead_cpu.py
FORWARD_SHAPES = [
    (1, 1, 1),          # one row, one column, one action: a wave of one live row, 15 idle lanes per quad, K padded from 1 to 64
    (17, 3, 1),         # two waves, the second with one row
    (16, 4, 16),        # a full wave and full N-tiles, one block of 16 columns staged by scalars (K < 16)
    (33, 5, 15),        # A = 15: one idle lane per quad
    (64, 512, 16),      # SAL at the batch of an update: one full tile, one chunk of 512 that fills the LDS, vector staging
    (65, 515, 17),      # A = 17: two N-tiles per half (the second with one live lane), chunks of 256: three, the last of 3 columns
    (3, 4096, 32),      # the limits: 16 chunks of 256, all 64 rows of weights live
    (5, 100, 32),       # two N-tiles per half in one chunk of 128 columns, 28 of them zeros
    (20, 1030, 16),     # one N-tile per half and more than one chunk: chunks of 512, the last of 6 columns
    (32835, 8, 2),      # 514 tiles on 512 workgroups: two walk a second tile, the last tile holds 3 rows
]
# (n, K, A) of the backward cases: n in {1, R - 1, R, R + 1, 2R + 3}
BACKWARD_SHAPES = [
    (1, 70, 3),         # one row: a slice of one; K = 70: two 64-column stage-1 blocks, the second partial
    (R - 1, 5, 1),      # a slice one short
    (R, 512, 16),       # SAL: exactly one slice, two grad_h column blocks of 256
    (R + 1, 300, 32),   # two slices, the second of one row; A = 32: all 64 chains; grad_h's second column block partial
    (2 * R + 3, 33, 17),  # three slices, the last of three rows; 34 of 64 chains
]

# accuracy of the fp64 functions, in ulp.  ROCm's device math library ships no accuracy table of its own; these are the
# OpenCL 3.0 full-profile limits it is written to (OpenCL C specification, section 7.4, "Relative Error as ULPs", double
# precision): exp <= 3 ulp, log <= 3 ulp, tanh <= 5 ulp.  NumPy's own: the 4 ulp are what its release notes
# (1.20-1.22, "maximum ULP error of 4") state for the AVX-512 / SVML loops, and for those alone; where NumPy falls through to the C
# library no NumPy document bounds the error -- glibc's manual ("Known Maximum Errors in Math Functions", x86_64, double) lists
# exp 1, log 1 and tanh 2 ulp, inside the same 4; on another C library ULP_NUMPY is an assumption, not a documented limit.
ULP_EXP, ULP_LOG, ULP_TANH, ULP_NUMPY = 3, 3, 5, 4
U64 = 2.0 ** -53
U32 = bc.U
ULP32_REF = 4                              # the fp32 transcendentals of the recording (torch on the CPU): 4 ulp each, as the issue sets


def paths(n, K, A):
    """What csrc/f110_policyhead.h does with n rows, restated from its arithmetic (policyhead_geometry on the host, the kernels'
    indexing).  T: N-tiles per half; kc: columns of K in LDS at a time; chunks, last_chunk: its columns; pad_cols: columns of zeros
    the last chunk multiplies (to a multiple of PH_PREFETCH); restage: every tile stages its chunks; lds: bytes; vec_stage /
    scalar_stage: some block of 16 columns is loaded as four float4 / element by element (for 16-byte aligned weights); idle_lanes:
    lanes of a quad without an action (per half); live_rows: rows of weights in LDS that are not zeros; tiles, grid, walks: forward
    tiles, workgroups, and the most tiles one walks; last_tile_rows; idle_waves: waves of the last tile without a row;
    partial_wave: a wave with fewer than 16 rows; slices, last_slice_rows: of the two-stage reduction; gh_blocks, gh_last_rows,
    gh_kblocks, gh_partial_k: grad_h's workgroups; gw_kblocks, gw_partial_k: stage 1's column blocks; chains: live accumulators of
    a stage-1 lane."""
    T = -(-A // 16)
    kc = min(PH_LDS_BYTES // (128 * T), -(-K // 64) * 64)
    chunks = -(-K // kc)
    last_chunk = K - (chunks - 1) * kc
    vec = scalar = False
    for j in range(A):
        for kb in range(0, chunks * kc, 16):
            v = kb + 16 <= K and (j * K + kb) % 4 == 0
            vec, scalar = vec or v, scalar or (not v and kb < K)
    tiles = -(-n // PH_ROWS)
    grid = min(tiles, PH_MAX_GRID)
    last_tile_rows = n - (tiles - 1) * PH_ROWS
    slices = -(-n // R)
    return dict(T=T, kc=kc, chunks=chunks, last_chunk=last_chunk, pad_cols=-(-last_chunk // PH_PREFETCH) * PH_PREFETCH - last_chunk,
                restage=chunks > 1, lds=128 * T * kc, vec_stage=vec, scalar_stage=scalar, idle_lanes=16 * T - A, live_rows=2 * A,
                tiles=tiles, grid=grid, walks=-(-tiles // grid), last_tile_rows=last_tile_rows, idle_waves=4 - -(-last_tile_rows // 16),
                partial_wave=n % 16 != 0, slices=slices, last_slice_rows=n - (slices - 1) * R, gh_blocks=-(-n // PH_GH_ROWS),
                gh_last_rows=n - (-(-n // PH_GH_ROWS) - 1) * PH_GH_ROWS, gh_kblocks=-(-K // PH_THREADS), gh_partial_k=K % PH_THREADS != 0,
                gw_kblocks=-(-K // 64), gw_partial_k=K % 64 != 0, chains=2 * A)


def workspace_bytes(n, K, A):
    """What f110_policyhead_backward writes: g_pre [n, 2A] rounded up to 4 floats, then [slices, 2A, K + 1]."""
    return 4 * (-(-(n * 2 * A) // 4) * 4 + paths(n, K, A)['slices'] * 2 * A * (K + 1))


# ---------------------------------------------------------------------------------------------- inputs
def inputs(n, K, A, seed=0, special=True):
    """h [n, K] >= 0 (features behind a relu), w_mean, w_log_std [A, K] of mixed sign and magnitude (the order of the sum matters),
    b_mean, b_log_std [A], eps [n, A], all fp32.  With `special`: row n // 2 of h is zeros, so its pre-activations are the biases, and
    b_log_std cycles through -20, 2 (exactly at the clamps), -25, 3 (beyond them), -19.9, 1.9 and ordinary values; row n // 3 (where it
    is another row) is scaled by 1000 so that tanh saturates."""
    rng = np.random.default_rng([n, K, A, seed])
    h = np.maximum(rng.normal(size=(n, K)), 0.0).astype(np.float32)
    scale = 10.0 ** rng.integers(-2, 1, (2, A, K)) / np.sqrt(K)           # (nn.Linear's default scale at most)
    wm, wl = (rng.normal(size=(2, A, K)) * scale).astype(np.float32)
    bm = rng.normal(size=A).astype(np.float32) * np.float32(0.5)
    bl = (0.1 * rng.normal(size=A) - 1.0).astype(np.float32)
    if special:
        cyc = np.array([-20.0, 2.0, -25.0, 3.0, -19.9, 1.9], np.float32)
        k = np.arange(A)
        bl = np.where(k % 8 < 6, cyc[k % 8 % 6], bl).astype(np.float32)
        h[n // 2] = 0.0
        if n // 3 != n // 2:
            h[n // 3] *= np.float32(1000.0)
    eps = rng.normal(size=(n, A)).astype(np.float32)
    return h, wm, bm, wl, bl, eps


# ---------------------------------------------------------------------------------------------- the contract
def pre_activations(h, wm, bm, wl, bl):
    """[n, 2A] float32: acc = 0; for k ascending: acc = fma(w[j][k], h[b][k], acc); + bias (+ 0.0f for None)."""
    h = np.asarray(h, np.float32)
    w = np.concatenate([np.asarray(wm, np.float32), np.asarray(wl, np.float32)])
    A = w.shape[0] // 2
    acc = np.zeros((h.shape[0], 2 * A), np.float32)
    for k in range(h.shape[1]):
        acc = b2.fma32(w[None, :, k], h[:, k, None], acc)
    b = np.concatenate([np.zeros(A, np.float32) if x is None else np.asarray(x, np.float32) for x in (bm, bl)])
    out = acc + b[None, :]
    assert out.dtype == np.float32
    return out


def tail(pre, eps):
    """The tail in fp64 from fp32 pre [n, 2A] and eps [n, A] or None: dict of ls, std, x, y (the action), terms [n, A] and log_prob
    [n] (None without eps), inside (the clamp's gradient mask)."""
    pre = np.asarray(pre, np.float32).astype(np.float64)
    A = pre.shape[1] // 2
    mean, pl = pre[:, :A], pre[:, A:]
    ls = np.minimum(np.maximum(pl, -20.0), 2.0)
    std = np.exp(ls)
    if eps is None:
        y = np.tanh(mean)
        return dict(mean=mean, ls=ls, std=std, x=mean, y=y, om=1.0 - y * y, terms=None, log_prob=None, inside=(pl >= -20.0) & (pl <= 2.0))
    e = np.asarray(eps, np.float32).astype(np.float64)
    x = mean + std * e
    y = np.tanh(x)
    om = 1.0 - y * y
    terms = ((-(e * e) / 2.0 - ls) - HALF_LOG_2PI) - np.log(om + 1e-6)
    lp = np.zeros(pre.shape[0])
    for j in range(A):
        lp = lp + terms[:, j]
    return dict(mean=mean, ls=ls, std=std, x=x, y=y, om=om, terms=terms, log_prob=lp, inside=(pl >= -20.0) & (pl <= 2.0), eps=e)


def _ulp(v):
    """An upper bound of one ulp of the fp64 magnitude v."""
    return 2.0 * U64 * np.abs(v)


def tail_bounds(pre, eps, out_fp32=False):
    """(bound on |action error| [n, A], bound on |log_prob error| [n] or None) between the device's tail and tail(): first-order
    propagation through the formulas of the two implementations' documented errors, doubled for the second order.
    std: (ULP_EXP + ULP_NUMPY) ulp.  x = mean + std eps: that error times |eps|, the roundings of the product and of the sum on
    either side, and one more for a contracted multiply-add.  y = tanh(x): (1 - y^2) dx + (ULP_TANH + ULP_NUMPY) ulp.
    om = 1 - y y: 2 |y| dy + a rounding of y y and of the difference per side.  log(om + 1e-6): (d om + the sum's roundings) /
    the argument + (ULP_LOG + ULP_NUMPY) ulp.  The three subtractions of a term: a rounding of each partial result per side.  The
    row's sum of A terms in order: gamma_A sum |terms| per side.  A result stored as fp32 may round to the other neighbour: one
    ulp32 more."""
    t = tail(pre, eps)
    y = t['y']
    if eps is None:
        dx = np.zeros_like(y)
    else:
        e = t['eps']
        dstd = (ULP_EXP + ULP_NUMPY) * _ulp(t['std'])
        dx = np.abs(e) * dstd + 2.0 * U64 * (np.abs(t['std'] * e) + np.abs(t['x'])) + U64 * np.abs(t['x'])
    dy = t['om'] * dx + (ULP_TANH + ULP_NUMPY) * _ulp(y)
    act = 2.0 * dy + (2.0 * U32 * np.abs(y) if out_fp32 else 0.0)
    if eps is None:
        return act, None
    dom = 2.0 * np.abs(y) * dy + 2.0 * U64 * (y * y + np.abs(t['om']))
    arg = t['om'] + 1e-6
    lg = np.log(arg)
    dlog = (dom + 2.0 * U64 * arg) / arg + (ULP_LOG + ULP_NUMPY) * _ulp(lg)
    q = e * e / 2.0
    dterm = dlog + 2.0 * U64 * (np.abs(q + t['ls']) + np.abs(q + t['ls'] + HALF_LOG_2PI) + np.abs(t['terms']))
    A = y.shape[1]
    gam = A * U64 / (1.0 - A * U64)
    lp = 2.0 * (dterm.sum(axis=1) + 2.0 * gam * np.abs(t['terms']).sum(axis=1))
    if out_fp32:
        lp = lp + 2.0 * U32 * np.abs(t['log_prob'])
    return act, lp


def g_pre(pre, eps, g_y, g_lp, g_in=None):
    """The analytic gradient with respect to pre, fp64 [n, 2A], and its bound (the error of the device's fp64 value against this
    one, first order, doubled; then one rounding to fp32).  g_x = g_y (1 - y^2) + g_lp 2 y (1 - y^2) / ((1 - y^2) + 1e-6); g_mean =
    g_x; g_ls = (g_x std eps - g_lp) [-20 <= pre_ls <= 2]; with eps None g_ls = 0.  g_in [n, 2A] fp32 or None: the contract's grad_pre, added
    exactly (two roundings of the sum, one per side, join the bound)."""
    t = tail(pre, eps)
    y, om = t['y'], t['om']
    gy = np.asarray(g_y, np.float64)
    glp = np.zeros(y.shape[0]) if g_lp is None else np.asarray(g_lp, np.float64)
    glp = glp[:, None]
    c = 1e-6
    f = 2.0 * y * om / (om + c)
    gx = gy * om + glp * f
    # d g_x / d y = -2 y g_y + g_lp (2 om / (om + c) - 4 y^2 c / (om + c)^2)
    dgdy = np.abs(-2.0 * y * gy) + np.abs(glp) * (np.abs(2.0 * om / (om + c)) + 4.0 * y * y * c / (om + c) ** 2)
    if eps is None:
        dy = (ULP_TANH + ULP_NUMPY) * _ulp(y)
    else:
        e = t['eps']
        dstd = (ULP_EXP + ULP_NUMPY) * _ulp(t['std'])
        dx = np.abs(e) * dstd + 2.0 * U64 * (np.abs(t['std'] * e) + np.abs(t['x'])) + U64 * np.abs(t['x'])
        dy = om * dx + (ULP_TANH + ULP_NUMPY) * _ulp(y)
    # the roundings of the expression itself: y y, 1 - y y, om + c, the products, the quotient and the sum, per side
    dgx = dgdy * dy + 16.0 * U64 * (np.abs(gy * om) + np.abs(glp * f))
    if eps is None:
        gl, dgl = np.zeros_like(gx), np.zeros_like(gx)
    else:
        gl = np.where(t['inside'], gx * t['std'] * e - glp, 0.0)
        dgl = np.where(t['inside'], np.abs(t['std'] * e) * dgx + np.abs(gx * e) * dstd + 8.0 * U64 * (np.abs(gx * t['std'] * e) + np.abs(glp)), 0.0)
    g = np.concatenate([gx, gl], axis=1)
    extra = 0.0
    if g_in is not None:
        g = g + np.asarray(g_in, np.float32).astype(np.float64)
        extra = 2.0 * U64 * np.abs(g)
    bound = 2.0 * np.concatenate([dgx, dgl], axis=1) + extra + U32 * np.abs(g)
    return g, bound


def gradients(h, wm, wl, g, g_bound):
    """From g_pre (fp64 [n, 2A]) and its bound: dict of (value, bound) for grad_h, grad_w [2A, K] and grad_b [2A] in fp64.  The
    bounds: g_pre's own propagated through the sum, plus gamma_m sum |terms| for each fp32 sum of m terms (grad_h: 2A fma steps;
    grad_w: R steps in a slice and the slices' sum; grad_b: plain additions, likewise)."""
    h = np.asarray(h, np.float64)
    w = np.concatenate([np.asarray(wm, np.float64), np.asarray(wl, np.float64)])
    n, J = g.shape
    slices = -(-n // R)
    m = min(n, R) + slices
    gh = g @ w
    gh_b = g_bound @ np.abs(w) + bc.gamma(J) * (np.abs(g) @ np.abs(w))
    gw = g.T @ h
    gw_b = g_bound.T @ np.abs(h) + bc.gamma(m) * (np.abs(g).T @ np.abs(h))
    gb = g.sum(axis=0)
    gb_b = g_bound.sum(axis=0) + bc.gamma(m) * np.abs(g).sum(axis=0)
    return dict(grad_h=(gh, gh_b), grad_w=(gw, gw_b), grad_b=(gb, gb_b))


# ---------------------------------------------------------------------------------------------- the recording of the reference (g20)
GROUPS = ('default', 'mean_x40', 'log_std_x400', 'bias_plus_1.9', 'bias_minus_19.9', 'bias_minus_25')
GROUP_ROWS = 16


def group_weights(g, gi):
    """(w_mean, b_mean, w_log_std, b_log_std) of group gi of g20, remade from the stored default initialisation with the fp32
    operation the generator applied to the reference's own tensors."""
    wm, bm, wl, bl = (np.asarray(g[k], np.float32) for k in ('w_mean', 'b_mean', 'w_log_std', 'b_log_std'))
    wm = wm * np.float32(g['mean_scale'][gi])
    wl = wl * np.float32(g['log_std_scale'][gi])
    bl = bl + np.float32(g['log_std_shift'][gi])
    assert wm.dtype == wl.dtype == bl.dtype == np.float32
    return wm, bm, wl, bl


def reference_bounds(h, wm, bm, wl, bl, eps, pre):
    """First-order fp32 bounds of the recording (the reference's Actor.sample in fp32 on the CPU) against the contract on `pre`:
    (bound on mean and the unclamped log_std [n, 2A], bound on the action [n, A], bound on log_prob [n]).
    pre: gamma_{K + 2} (sum |w| |h| + |b|), either side sums K products and a bias in fp32 in some order.  std: its relative error is
    d ls + ULP32_REF u32.  x_t: d mean + |eps| d std + the two roundings.  y: sup of 1 - tanh^2 over [|x| - dx, |x| + dx] times dx +
    ULP32_REF u32.  The reference's ((x_t - mean) / std)^2 / 2 on the rounded x_t: (x_t - mean) / std = eps + r with |r| <= u32 |x_t|
    / std (+ the error of std), so |eps| r + r^2 / 2, and four roundings of the expression.  log std against ls: d ls + ULP32_REF u32
    (1 + |ls|).  log(1 - y^2 + 1e-6): (2 |y| dy + 3 u32) / (the argument - that) + ULP32_REF u32 |log|, infinite where the argument's
    error reaches it.  The sum of A terms in fp32: gamma_{A + 4} sum |terms|."""
    h64 = np.abs(np.asarray(h, np.float64))
    w = np.abs(np.concatenate([wm, wl]).astype(np.float64))
    b = np.abs(np.concatenate([bm, bl]).astype(np.float64))
    K, A = h64.shape[1], wm.shape[0]
    dpre = bc.gamma(K + 2) * (h64 @ w.T + b[None, :])
    t = tail(pre, eps)
    e, y = t['eps'], t['y']
    dls = np.where(t['inside'], dpre[:, A:], 0.0)          # (a clamped entry is exact unless the error reaches across the bound: see below)
    pl = np.asarray(pre, np.float64)[:, A:]
    near = (~t['inside']) & ((np.abs(pl - 2.0) <= dpre[:, A:]) | (np.abs(pl + 20.0) <= dpre[:, A:]))
    dls = np.where(near, dpre[:, A:], dls)
    dstd = t['std'] * (dls + ULP32_REF * U32)
    dx = dpre[:, :A] + np.abs(e) * dstd + 2.0 * U32 * (np.abs(t['std'] * e) + np.abs(t['x']))
    lo = np.maximum(np.abs(t['x']) - dx, 0.0)
    dy = (1.0 - np.tanh(lo) ** 2) * dx + ULP32_REF * U32 * np.abs(y)
    r = U32 * np.abs(t['x']) / t['std'] + (dls + ULP32_REF * U32) * np.abs(e)
    q = e * e / 2.0
    dquad = np.abs(e) * r + r * r / 2.0 + 4.0 * U32 * q
    dlogstd = dls + ULP32_REF * U32 * (1.0 + np.abs(t['ls']))
    arg = t['om'] + 1e-6
    darg = 2.0 * np.abs(y) * dy + 3.0 * U32
    with np.errstate(divide='ignore', invalid='ignore'):
        dlog = np.where(darg < arg, darg / (arg - darg), np.inf) + ULP32_REF * U32 * np.abs(np.log(arg))
    mags = q + np.abs(t['ls']) + HALF_LOG_2PI + np.abs(np.log(arg))
    dlp = (dquad + dlogstd + dlog).sum(axis=1) + bc.gamma(A + 4) * mags.sum(axis=1)
    return dpre, dy, dlp
