"""The dense layer of the reference's networks on the GPU (csrc/f110_dense.h): fc1 = nn.Linear(32 * 28 * 28, 512) of Actor and the
feature columns of Critic's nn.Linear(32 * 28 * 28 + 16, 512) (src/SAL.py:400, 432) with their ReLU, forward and backward under a
written numerics contract (include/f110_hip.h): K is cut into segments of `segment` terms, each a k-ordered fmaf chain on the fp32
matrix cores, added in ascending order -- so a row's result depends on the row, the parameters and the segment length alone, at
a batch of 1 as at 65 536 -- and the backward is three fixed-order chains without atomics.  There is no CPU path and no torch
fallback: the kernels of libf110_hip.so do the work."""
import ctypes as C

import torch

from . import _lib

MAX_IN, MAX_OUT, MAX_SEGMENT, MAX_ROWS = 1 << 20, 4096, 4096, 1 << 24
DEFAULT_SEGMENT = 784        # one 28 x 28 plane of conv3's output, 196 MFMA steps: SAL's fc1 is 32 segments


def make_config(in_features, out_features, ld=None, segment=DEFAULT_SEGMENT, relu=False):
    """An f110_dense_config; out-of-range integers are clamped into int32 so that validate() can name them.  ld: the row stride of
    weight and grad_weight in elements (None: in_features, a dense [H, K] array)."""
    c, clamp = _lib.DenseConfig(), _lib.clamp
    c.in_features, c.out_features, c.ld = clamp(in_features), clamp(out_features), clamp(in_features if ld is None else ld)
    c.segment, c.relu, c.reserved = clamp(segment), 1 if relu else 0, 0
    return c


def validate(in_features, out_features, ld=None, segment=DEFAULT_SEGMENT, relu=False):
    """f110_dense_validate (host only, no device): ValueError for in_features outside 1..2^20, out_features outside 1..4096, ld
    below in_features and a segment that is not a multiple of 4 in 4..4096."""
    c = make_config(in_features, out_features, ld, segment, relu)
    _lib.check(_lib.load().f110_dense_validate(C.byref(c)))
    return c


def workspace_bytes(cfg, n):
    """f110_dense_workspace: the bytes the forward needs for n rows -- ceil(K / S) * n * H * 4 where every segment gets a workgroup
    of its own (more than one segment and ceil(n / 32) * ceil(H / 64) < 256), else 0; 0 for an invalid configuration and for n
    outside 1..2^24."""
    return int(_lib.load().f110_dense_workspace(C.byref(cfg), max(min(int(n), 2 ** 63 - 1), -2 ** 63)))


def forward_into(cfg, x, weight_ptr, bias, out):
    """f110_dense_forward on the caller's current stream: x [n, K] -> out [n, H] against the weight at address weight_ptr with the
    row stride cfg.ld.  Allocates the workspace the shape asks for."""
    lib = _lib.load()
    dev, n = x.device, int(x.shape[0])
    nbytes = lib.f110_dense_workspace(C.byref(cfg), n)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _lib.check(lib.f110_dense_forward(C.byref(cfg), x.data_ptr(), n, weight_ptr, _lib.ptr(bias), out.data_ptr(), _lib.ptr(ws), _lib.stream(dev)))
    return out


def backward_into(cfg, x, out, grad_out, weight_ptr, grad_x, grad_weight_ptr, grad_bias):
    """f110_dense_backward on the caller's current stream; grad_x and grad_bias tensors or None, grad_weight_ptr an address (rows
    cfg.ld apart) or None."""
    dev = grad_out.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().f110_dense_backward(C.byref(cfg), _lib.ptr(x), _lib.ptr(out), grad_out.data_ptr(), int(grad_out.shape[0]), weight_ptr,
                                                   _lib.ptr(grad_x), grad_weight_ptr, _lib.ptr(grad_bias), _lib.stream(dev)))


class _LinearFeat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, cfg):
        n = int(x.shape[0])
        out = torch.empty((n, cfg.out_features), dtype=torch.float32, device=x.device)
        if n > 0:
            forward_into(cfg, x, weight.data_ptr(), bias, out)
        ctx.cfg, ctx.n = cfg, n
        ctx.save_for_backward(x, weight, out if cfg.relu else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, out = ctx.saved_tensors
        cfg, n, dev = ctx.cfg, ctx.n, grad_out.device
        g = grad_out.to(torch.float32).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(weight) if need_w else None
        gb = torch.empty((cfg.out_features,), dtype=torch.float32, device=dev) if need_b else None
        if n > 0 and (need_x or need_w or need_b):
            backward_into(cfg, x, out, g, weight.data_ptr(), gx, _lib.ptr(gw), gb)
        elif n == 0:
            gw = None if gw is None else gw.zero_()
            gb = None if gb is None else gb.zero_()
        return gx, gw, gb, None


def linear_feat(x, weight, bias=None, relu=False, segment=DEFAULT_SEGMENT):
    """nn.Linear(K, H) (+ ReLU) on fp32 features, on the fp32 matrix cores (csrc/f110_dense.h).
    x [n, K] fp32 contiguous on a GPU, n <= 2^24; weight [H, K] fp32 and bias [H] fp32 or None on the same device, contiguous;
    K <= 2^20, H <= 4096; segment: the k's per chain, a multiple of 4 in 4..4096.  relu: max(out, 0) fused, and its mask in the
    backward.
    Returns [n, H] fp32 on the caller's current stream, without synchronising: per segment of K acc = fma(x[r][k], w[h][k], acc)
    for k ascending from 0, the segments' results added in ascending order, + bias, relu -- the same bits for a row whatever the
    batch around it.  Differentiable in x, weight and bias; the backward computes only what needs_input_grad asks, in the orders
    of include/f110_hip.h, and gives the same bits every time.
    ValueError for what f110_dense_validate refuses and for a dtype, layout, device or shape mismatch."""
    who = 'linear_feat'
    if not torch.is_tensor(x) or not torch.is_tensor(weight):
        raise ValueError('%s: x and weight must be tensors' % who)
    if not x.is_cuda or weight.device != x.device:
        raise ValueError('%s: x and weight must be on the same GPU' % who)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError('%s: x must be fp32 [n, K], not %s %s' % (who, x.dtype, tuple(x.shape)))
    n, k = int(x.shape[0]), int(x.shape[1])
    if weight.dtype != torch.float32 or weight.dim() != 2 or int(weight.shape[1]) != k:
        raise ValueError('%s: weight must be fp32 [H, %d], not %s %s' % (who, k, weight.dtype, tuple(weight.shape)))
    h = int(weight.shape[0])
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (h,) or bias.device != x.device):
        raise ValueError('%s: bias must be fp32 [%d] on x\'s device' % (who, h))
    if not x.is_contiguous() or not weight.is_contiguous() or (bias is not None and not bias.is_contiguous()):
        raise ValueError('%s: x, weight and bias must be contiguous' % who)
    if n > MAX_ROWS:
        raise ValueError('%s: %d rows (at most %d)' % (who, n, MAX_ROWS))
    cfg = validate(k, h, k, segment, relu)
    return _LinearFeat.apply(x, weight, bias, cfg)


class Dense(torch.nn.Module):
    """nn.Linear(in_features, out_features) (+ ReLU) computed by linear_feat.  Its parameters have the names and shapes of
    nn.Linear's, so state dicts pass between the two in both directions."""

    def __init__(self, in_features, out_features, relu=False, segment=DEFAULT_SEGMENT, bias=True, device=None):
        super().__init__()
        validate(int(in_features), int(out_features), None, int(segment))
        ref = torch.nn.Linear(int(in_features), int(out_features), bias=bias, device=device)   # (for its initialisation)
        self.weight = ref.weight
        self.register_parameter('bias', ref.bias)
        self.relu, self.segment = bool(relu), int(segment)

    @classmethod
    def from_linear(cls, linear, relu=False, segment=DEFAULT_SEGMENT):
        """A Dense that shares the parameters of `linear` (the same tensors: training one trains the other).  ValueError unless
        it is an nn.Linear of sizes the kernels take."""
        if not isinstance(linear, torch.nn.Linear):
            raise ValueError('Dense.from_linear: not an nn.Linear')
        validate(linear.in_features, linear.out_features, None, int(segment))
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.weight = linear.weight
        m.register_parameter('bias', linear.bias)
        m.relu, m.segment = bool(relu), int(segment)
        return m

    def forward(self, x):
        return linear_feat(x, self.weight, self.bias, relu=self.relu, segment=self.segment)

    def extra_repr(self):
        return '%d, %d, relu=%s, segment=%d' % (self.weight.shape[1], self.weight.shape[0], self.relu, self.segment)
