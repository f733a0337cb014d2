"""The checkers of the dense layer (csrc/f110_dense.h), NumPy only: the numerics contract of include/f110_hip.h restated step by step
in float32 so that the GPU's results can be compared with `==` -- the forward cuts K into segments of S terms, runs one fma chain per
segment (bitconv2_cases.fma32) and adds the segments' results in ascending order with plain fp32 adds, then the bias, then the
ReLU; grad_x is one chain over h, grad_weight one chain over the rows, grad_bias plain adds over the rows.  fp64 companions with their
sum of magnitudes supply the bounds, and paths() restates the launch plan (csrc/f110_dense_plan.h) so that every shape of the table
can be shown to select what its comment claims."""
import os

import numpy as np

import bitconv_cases as bc
from bitconv2_cases import fma32
from featconv_cases import tensor

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDEN_ROWS = ('g22_trunk.npz', 'g22_trunk_unit.npz')      # featconv_cases.GOLDEN: the recordings whose conv3_out g23 feeds to fc1

# csrc/f110_dense_plan.h
DN_THREADS, DN_BM, DN_BN, DN_KC, DN_SPLIT_BELOW = 256, 32, 64, 32, 256
DN_LDK, DN_LDM, DN_LDN = DN_KC + 4, DN_BM + 16, DN_BN + 16
DN_LDS_BYTES, DN_MAX_GRID_X, DN_MAX_GRID_Y = 64 * 1024, 1 << 28, 65535
MAX_K, MAX_H, MAX_S, MAX_ROWS = 1 << 20, 4096, 4096, 1 << 24
DEFAULT_SEGMENT = 784


def paths(n, K, H, S):
    """What csrc/f110_dense.h does with n rows, restated from its arithmetic (f110_dense_plan.h on the host, the kernels' indexing).
    segs, last_seg: the segments of K and the terms of the last; kpad: a segment whose terms are no multiple of 4 (a step fed zeros);
    chunks: staged chunks of a full segment, chunk_pad: a chunk with fewer than 8 live steps; mblocks, nblocks: blocks of 32 rows and
    of 64 outputs, partial_m / partial_n: a block beyond the matrix's edge; split: every segment has a workgroup of its own and the
    chains go through the workspace; path: 'split', 'registers' (one workgroup walks several segments) or 'single' (one segment);
    workspace: bytes; gx, gy: the forward's grid; sum_blocks: of the second kernel.  (Whether a row is loaded 16 bytes at a time is
    decided by the addresses and ld, not by the shape: LAYOUTS below.)
    Backward: gx_mblocks x gx_nblocks workgroups of grad_x with gx_chunks chunks of H; gw_mblocks x gw_nblocks of grad_weight with
    gw_chunks chunks of rows; gb_blocks of grad_bias; gx_partial_n: K no multiple of 64, gw_partial_m: H no multiple of 32."""
    segs = -(-K // S)
    last = K - (segs - 1) * S
    mblocks, nblocks = -(-n // DN_BM), -(-H // DN_BN)
    split = segs > 1 and mblocks * nblocks < DN_SPLIT_BELOW
    return dict(segs=segs, last_seg=last, kpad=last % 4 != 0, chunks=-(-S // DN_KC), chunk_pad=S % DN_KC != 0 or last % DN_KC != 0,
                mblocks=mblocks, nblocks=nblocks, partial_m=n % DN_BM != 0, partial_n=H % DN_BN != 0, split=split,
                path='split' if split else 'registers' if segs > 1 else 'single', workspace=4 * segs * n * H if split else 0,
                gx=segs if split else mblocks, gy=mblocks * nblocks if split else nblocks, sum_blocks=-(-(n * H) // DN_THREADS) if split else 0,
                gx_mblocks=mblocks, gx_nblocks=-(-K // DN_BN), gx_chunks=-(-H // DN_KC), gx_partial_n=K % DN_BN != 0,
                gw_mblocks=-(-H // DN_BM), gw_nblocks=-(-K // DN_BN), gw_chunks=-(-n // DN_KC), gw_partial_m=H % DN_BM != 0,
                gb_blocks=-(-H // 64))


def _split_edge(K, H, S):
    """The largest n on the split path for (K, H, S) with more than one segment."""
    return (-(-DN_SPLIT_BELOW // -(-H // DN_BN)) - 1) * DN_BM


EDGE = (12, 512, 8)       # (K, H, S) of the pair either side of the plan's boundary: few terms, since n H is 256 blocks' worth
# (n, K, H, S); what each selects is asserted from paths() in test_dense_cpu.py
SHAPES = [
    (1, 1, 1, 4),               # everything is padding: one term, one row, one output
    (5, 7, 3, 4),               # K no multiple of 4, two segments, a short last one
    (17, 37, 33, 8),            # partial tiles in both directions, five segments, a last one of 5
    (16, 64, 16, 64),           # exact tiles, one segment of two full chunks: the workspace is 0 although n is small
    (33, 1572, 20, 784),        # the default segment, three segments, the last 4 long; two blocks of rows
    (40, 100, 130, 36),         # three blocks of outputs, two of rows; a segment of two chunks, the second 4 long; five chunks of H in grad_x
    (_split_edge(*EDGE),) + EDGE,       # the last n whose segments go through the workspace ...
    (_split_edge(*EDGE) + 1,) + EDGE,   # ... and the first that one workgroup walks, adding in registers
]
SAL = (2, 25088, 512, 784)      # SAL's own fc1, on the critics' view with ld = 25104
# how weight and grad_weight lie in memory: name -> (ld(K), offset of the base from a 16-byte boundary in floats)
LAYOUTS = {
    'dense': (lambda K: K, 0),                          # 16-byte loads where K is a multiple of 4
    'view': (lambda K: K + 3, 1),                       # a column view that starts 4 bytes past a boundary: 4-byte accesses
    'aligned_view': (lambda K: (K + 4) // 4 * 4, 0),    # ld > K a multiple of 4: 16-byte loads, the one across the end of K element by element
}
# (relu, bias present)
VARIANTS = ((True, True), (False, False), (True, False), (False, True))


def other_segment(K, S):
    """Another valid S that cuts K differently, or None where every S gives the one chain (K <= 4)."""
    for s in (4, 8, 16, 4 * (-(-K // 4))):
        if s != S and [min(s, K - i) for i in range(0, K, s)] != [min(S, K - i) for i in range(0, K, S)]:
            return s
    return None


# ---------------------------------------------------------------------------------------------- the contract
def chains(x, w, S):
    """sum [n, H] float32 before the bias: per segment acc = fma(x[r][k], w[h][k], acc) for k ascending from 0; sum = acc_0, then
    sum = sum + acc_j."""
    x, w = np.asarray(x, f32), np.asarray(w, f32)
    n, K = x.shape
    total = None
    for k0 in range(0, K, S):
        acc = np.zeros((n, w.shape[0]), f32)
        for k in range(k0, min(K, k0 + S)):
            acc = fma32(x[:, k, None], w[None, :, k], acc)
        total = acc if total is None else total + acc
    assert total.dtype == f32
    return total


def finish(total, b, relu):
    """out = sum + bias (+ 0.0f for None); out < 0 ? 0 : out under relu."""
    out = total + (f32(0.0) if b is None else np.asarray(b, f32)[None, :])
    assert out.dtype == f32
    return np.where(out < 0, f32(0.0), out) if relu else out


def forward(x, w, b, S, relu):
    return finish(chains(x, w, S), b, relu)


def masked(out, grad_out, relu):
    """g of the backward: grad_out where out > 0 under relu, else grad_out."""
    grad_out = np.asarray(grad_out, f32)
    return np.where(np.asarray(out) > 0, grad_out, f32(0.0)).astype(f32) if relu else grad_out


def grad_x(g, w, cols=None):
    """grad_x [n, K] (or its columns `cols`): acc = 0; for h ascending: acc = fma(g[r][h], w[h][k], acc)."""
    g, w = np.asarray(g, f32), np.asarray(w, f32)
    w = w if cols is None else w[:, cols]
    acc = np.zeros((g.shape[0], w.shape[1]), f32)
    for h in range(w.shape[0]):
        acc = fma32(g[:, h, None], w[None, h, :], acc)
    return acc


def grad_weight(g, x, cols=None):
    """grad_weight [H, K] (or its columns `cols`): acc = 0; for r ascending: acc = fma(g[r][h], x[r][k], acc)."""
    g, x = np.asarray(g, f32), np.asarray(x, f32)
    x = x if cols is None else x[:, cols]
    acc = np.zeros((g.shape[1], x.shape[1]), f32)
    for r in range(g.shape[0]):
        acc = fma32(g[r, :, None], x[r, None, :], acc)
    return acc


def grad_bias(g):
    """grad_bias [H]: acc = 0; for r ascending: acc = acc + g[r][h]."""
    g = np.asarray(g, f32)
    acc = np.zeros(g.shape[1], f32)
    for r in range(g.shape[0]):
        acc = acc + g[r]
    assert acc.dtype == f32
    return acc


# ---------------------------------------------------------------------------------------------- fp64 companions: (value, sum of |terms|)
def forward_fp64(x, w, b):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    b = np.zeros(w.shape[0]) if b is None else np.asarray(b, np.float64)
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def grad_x_fp64(g, w):
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    return g @ w, np.abs(g) @ np.abs(w)


def grad_weight_fp64(g, x):
    g, x = np.asarray(g, np.float64), np.asarray(x, np.float64)
    return g.T @ x, np.abs(g).T @ np.abs(x)


def grad_bias_fp64(g):
    g = np.asarray(g, np.float64)
    return g.sum(0), np.abs(g).sum(0)


def gamma(t):
    return bc.gamma(t)


def forward_roundings(K, S):
    """The most roundings a term of the forward passes through: its segment's chain, the adds of the segments, the bias."""
    return min(K, S) + -(-K // S)


# ---------------------------------------------------------------------------------------------- inputs and the cached reference
def params(K, H, seed=0):
    """(weight [H, K], bias [H]) in fp32 of mixed sign and magnitude, so that the order of a sum matters."""
    return tensor((H, K), seed + 11), np.random.default_rng([K, H, seed, 5]).normal(size=H).astype(f32)


_cache = {}


def reference(shape, seed=0, cols=None, variants=None):
    """Everything the checkers say about `shape` = (n, K, H, S), computed once and left unchanged: x, w, b, grad_out, sum (the forward
    before the bias) and, per variant (relu, bias), out[v], g[v], grad_x[v], grad_weight[v], grad_bias[v] (bias only moves the mask).
    cols: grad_weight on these columns only (a large K); variants: only these of VARIANTS."""
    variants = VARIANTS if variants is None else tuple(variants)
    key = (shape, seed, None if cols is None else tuple(cols), variants)
    if key not in _cache:
        n, K, H, S = shape
        w, b = params(K, H, seed)
        x = tensor((n, K), seed + 1)
        go = tensor((n, H), seed + 2)
        r = dict(x=x, w=w, b=b, grad_out=go, sum=chains(x, w, S), out={}, g={}, grad_x={}, grad_weight={}, grad_bias={})
        done = {}
        for v in variants:
            relu, bias = v
            r['out'][v] = finish(r['sum'], b if bias else None, relu)
            g = masked(r['out'][v], go, relu)
            r['g'][v] = g
            same = [u for u in done if np.array_equal(r['g'][u], g)]
            if same:                                                        # (without relu the bias moves nothing in the backward)
                for name in ('grad_x', 'grad_weight', 'grad_bias'):
                    r[name][v] = r[name][same[0]]
            else:
                r['grad_x'][v], r['grad_weight'][v], r['grad_bias'][v] = grad_x(g, w), grad_weight(g, x, cols), grad_bias(g)
            done[v] = True
        for v in r.values():
            for a in (v.values() if isinstance(v, dict) else (v,)):
                a.setflags(write=False)
        _cache[key] = r
    return _cache[key]


SAL_COLS = np.r_[0:70, 70:25018:61, 25018:25088]       # the columns of grad_weight checked at SAL's shape: both edges and every 61st


# ---------------------------------------------------------------------------------------------- the recording of the reference (g23)
def rebuilt_fc1():
    """fc1 of the reference's Actor under torch.manual_seed(22), without the reference: its four layers in their order."""
    import torch
    torch.manual_seed(22)
    convs = [torch.nn.Conv2d(1, 16, 8, 4), torch.nn.Conv2d(16, 32, 4, 2), torch.nn.Conv2d(32, 32, 3, 1)]
    fc1 = torch.nn.Linear(32 * 28 * 28, 512)
    return convs, fc1.weight.detach().numpy(), fc1.bias.detach().numpy()


def golden_inputs():
    """(g23, the batch of two feature rows, weight, bias); fails where the rebuilt parameters are not the recorded ones."""
    g = np.load(os.path.join(GOLDEN, 'g23_dense.npz'))
    rows = [np.load(os.path.join(GOLDEN, name)) for name in GOLDEN_ROWS]
    convs, w, b = rebuilt_fc1()
    for r in rows:
        assert np.array_equal(convs[1].weight.detach().numpy(), r['conv2_weight']) and np.array_equal(convs[2].weight.detach().numpy(), r['conv3_weight']), \
            'this torch does not rebuild the recorded Actor from its seed'
    assert np.array_equal(w[:, g['cols']], g['weight_cols']) and np.array_equal(b, g['bias']), 'this torch does not rebuild the recorded fc1 from its seed'
    x = np.stack([r['conv3_out'].reshape(-1) for r in rows]).astype(np.float32)
    return g, x, w, b


def golden_check(g, x, w, b, pre, grad_x, grad_w_cols, grad_b, report=print):
    """Every recorded array within 2 gamma(T) sum |terms| of the given results (gamma(T) for either side's own error against fp64)."""
    n, K = x.shape
    gm = masked(g['pre'], g['cotangent'], True)
    for name, got, rec, (ref, mag), t in (('pre', pre, g['pre'], forward_fp64(x, w, b), K + 1),
                                          ('grad_input', grad_x, g['grad_input'], grad_x_fp64(gm, w), w.shape[0]),
                                          ('weight_grad', grad_w_cols, g['weight_grad_cols'], grad_weight_fp64(gm, x[:, g['cols']]), n),
                                          ('bias_grad', grad_b, g['bias_grad'], grad_bias_fp64(gm), n)):
        err = np.abs(np.asarray(got, np.float64) - np.asarray(rec, np.float64))
        own = np.abs(np.asarray(got, np.float64) - ref)
        report('%-12s T = %5d: worst |got - recorded| %.3f u mag, |got - fp64| %.3f u mag' % (
            name, t, float((err / np.maximum(bc.U * mag, 1e-300)).max()), float((own / np.maximum(bc.U * mag, 1e-300)).max())))
        assert (err <= 2.0 * gamma(t) * mag).all(), name
