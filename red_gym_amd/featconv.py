"""The dense convolutions of the reference's trunk on the GPU (csrc/f110_featconv.h): conv2 = nn.Conv2d(16, 32, 4, 2) and conv3 =
nn.Conv2d(32, 32, 3, 1) of Actor and Critic (src/SAL.py:398-399, 430-431) with their ReLU, forward and backward under a written
numerics contract (include/f110_hip.h): the forward adds in the order of the fused stem's second layer, the backward is
repeatable bit for bit and uses no atomics.  Trunk puts conv1 (from bits), conv2 and conv3 behind one module whose acting and
learning paths return the same bits.  There is no CPU path and no torch fallback: the kernels of libf110_hip.so do the work."""
import ctypes as C

import torch

from . import _lib
from .bitconv import BitConv2d, _plain_conv, conv_bits, conv_bits2

MAX_KERNEL, MAX_STRIDE, MAX_IN, MAX_OUT, MAX_TERMS, MAX_COLS = 4, 4, 32, 64, 512, 64


def make_config(in_channels, rows, cols, out_channels, kernel, stride=1, relu=False):
    """An f110_featconv_config; out-of-range integers are clamped into int32 so that validate() can name them."""
    c, clamp = _lib.FeatconvConfig(), _lib.clamp
    c.in_channels, c.rows, c.cols, c.out_channels = clamp(in_channels), clamp(rows), clamp(cols), clamp(out_channels)
    c.kernel, c.stride, c.relu, c.reserved = clamp(kernel), clamp(stride), 1 if relu else 0, 0
    return c


def validate(in_channels, rows, cols, out_channels, kernel, stride=1, relu=False):
    """f110_featconv_validate (host only, no device): ValueError for kernel or stride outside 1..4, in_channels outside 1..32,
    out_channels outside 1..64, in_channels * kernel^2 or out_channels * kernel^2 above 512, rows or cols below kernel, cols
    above 64."""
    c = make_config(in_channels, rows, cols, out_channels, kernel, stride, relu)
    _lib.check(_lib.load().f110_featconv_validate(C.byref(c)))
    return c


def workspace_bytes(cfg, n):
    """f110_featconv_workspace: n * out_channels * (in_channels * kernel^2 + 1) * 4; 0 for an invalid configuration, for n < 1 and
    where the count does not fit int64."""
    return int(_lib.load().f110_featconv_workspace(C.byref(cfg), max(min(int(n), 2 ** 63 - 1), -2 ** 63)))


def output_size(rows, cols, kernel, stride):
    return (rows - kernel) // stride + 1, (cols - kernel) // stride + 1


class _ConvFeat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, cfg):
        lib = _lib.load()
        dev, n = x.device, int(x.shape[0])
        oh, ow = output_size(cfg.rows, cfg.cols, cfg.kernel, cfg.stride)
        out = torch.empty((n, cfg.out_channels, oh, ow), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.f110_featconv_forward(C.byref(cfg), x.data_ptr(), n, weight.data_ptr(), _lib.ptr(bias), out.data_ptr(), _lib.stream(dev)))
        ctx.cfg, ctx.n = cfg, n
        ctx.save_for_backward(x, weight, out if cfg.relu else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        x, weight, out = ctx.saved_tensors
        cfg, n, dev = ctx.cfg, ctx.n, grad_out.device
        g = grad_out.to(torch.float32).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(weight) if need_w else None
        gb = torch.empty((cfg.out_channels,), dtype=torch.float32, device=dev) if need_b else None
        ws = None
        if need_w or need_b:
            nbytes = lib.f110_featconv_workspace(C.byref(cfg), n)
            assert nbytes == 4 * n * cfg.out_channels * (cfg.in_channels * cfg.kernel * cfg.kernel + 1)
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        if n > 0 and (need_x or need_w or need_b):
            with torch.cuda.device(dev):
                _lib.check(lib.f110_featconv_backward(C.byref(cfg), x.data_ptr(), _lib.ptr(out), g.data_ptr(), n, weight.data_ptr(), _lib.ptr(gx),
                                                      _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), _lib.stream(dev)))
        elif n == 0:
            gw = None if gw is None else gw.zero_()
            gb = None if gb is None else gb.zero_()
        return gx, gw, gb, None


def conv_feat(x, weight, bias=None, stride=1, relu=False):
    """nn.Conv2d(Ci, Co, k, stride) (+ ReLU) on fp32 feature maps, on the fp32 matrix cores (csrc/f110_featconv.h).
    x [n, Ci, H, W] fp32 contiguous on a GPU; weight [Co, Ci, k, k] fp32 and bias [Co] fp32 or None on the same device, contiguous.
    Square kernel and stride, no padding, dilation or groups; k and stride 1..4, Ci <= 32, Co <= 64, Ci k^2 and Co k^2 <= 512,
    W <= 64.  relu: max(out, 0) fused, and its mask in the backward.
    Returns [n, Co, OH, OW] fp32 on the caller's current stream, without synchronising: acc = fma(w[co][ci][ky][kx], x[ci][s oy +
    ky][s ox + kx], acc) for ci major, ky, kx minor from 0, + bias, relu -- the order of conv_bits2's second layer.  Differentiable
    in x, weight and bias; the backward (grad_x, and grad_weight / grad_bias through per-sample partials added in ascending order)
    computes only what needs_input_grad asks and gives the same bits every time (include/f110_hip.h).
    ValueError for what f110_featconv_validate refuses and for a dtype, layout, device or shape mismatch."""
    who = 'conv_feat'
    if not torch.is_tensor(x) or not torch.is_tensor(weight):
        raise ValueError('%s: x and weight must be tensors' % who)
    if not x.is_cuda or weight.device != x.device:
        raise ValueError('%s: x and weight must be on the same GPU' % who)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError('%s: x must be fp32 [n, Ci, H, W], not %s %s' % (who, x.dtype, tuple(x.shape)))
    ci = int(x.shape[1])
    if weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[1] != ci or weight.shape[2] != weight.shape[3]:
        raise ValueError('%s: weight must be fp32 [Co, %d, k, k], not %s %s' % (who, ci, weight.dtype, tuple(weight.shape)))
    co, k = int(weight.shape[0]), int(weight.shape[2])
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (co,) or bias.device != x.device):
        raise ValueError('%s: bias must be fp32 [%d] on x\'s device' % (who, co))
    if not x.is_contiguous() or not weight.is_contiguous() or (bias is not None and not bias.is_contiguous()):
        raise ValueError('%s: x, weight and bias must be contiguous' % who)
    cfg = validate(ci, int(x.shape[2]), int(x.shape[3]), co, k, stride, relu)
    return _ConvFeat.apply(x, weight, bias, cfg)


class FeatConv2d(torch.nn.Module):
    """nn.Conv2d(in_channels, out_channels, kernel_size, stride) (+ ReLU) computed by conv_feat.  Its parameters have the names and
    shapes of nn.Conv2d's, so state dicts pass between the two in both directions."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, relu=False, bias=True, device=None):
        super().__init__()
        k = int(kernel_size)
        validate(int(in_channels), k, k, int(out_channels), k, int(stride))
        ref = torch.nn.Conv2d(int(in_channels), int(out_channels), k, int(stride), bias=bias, device=device)   # (for its initialisation)
        self.weight = ref.weight
        self.register_parameter('bias', ref.bias)
        self.kernel_size, self.stride, self.relu = k, int(stride), bool(relu)

    @classmethod
    def from_conv(cls, conv, relu=False):
        """A FeatConv2d that shares the parameters of `conv` (the same tensors: training one trains the other).  ValueError
        unless it is an nn.Conv2d with a square kernel and stride, no padding, dilation or groups, of sizes the kernels take."""
        if not isinstance(conv, torch.nn.Conv2d):
            raise ValueError('FeatConv2d.from_conv: not an nn.Conv2d')
        k, s = _plain_conv('FeatConv2d.from_conv', conv, '', conv.in_channels, 'in_channels = %d')
        validate(conv.in_channels, k, k, conv.out_channels, k, s)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.weight = conv.weight
        m.register_parameter('bias', conv.bias)
        m.kernel_size, m.stride, m.relu = k, s, bool(relu)
        return m

    def forward(self, x):
        return conv_feat(x, self.weight, self.bias, stride=self.stride, relu=self.relu)

    def extra_repr(self):
        return '%d, %d, kernel_size=%d, stride=%d, relu=%s' % (self.weight.shape[1], self.weight.shape[0], self.kernel_size, self.stride, self.relu)


class Trunk(torch.nn.Module):
    """relu(conv3(relu(conv2(relu(conv1(frames)))))) flattened: what the reference's Actor and Critic feed fc1 (src/SAL.py:405-408,
    436-439), on two-valued images.  Submodules conv1 (a BitConv2d), conv2 and conv3 (FeatConv2d), so a state dict has the
    reference's keys conv1.weight .. conv3.bias.  on: what a set pixel is worth (1.0 for FloatTensor(state) / 255, 255.0 for the raw
    images of update()); cols: the columns of packed frames.
    forward(frames, index=None) -> [n, Co * OH * OW] takes one of two paths: while torch.is_grad_enabled() and one of the six
    parameters requires grad, conv_bits(relu) -> conv_feat(relu) -> conv_feat(relu), differentiable; otherwise conv_bits2 ->
    conv_feat(relu).  Both add conv2 in the same order, so the two paths return the same bits: the features a policy acts on are
    the features it learns from.
    stack = k > 1: conv1 is nn.Conv2d(k, 16, 8, 4) on stacks of k packed frames and forward takes index [n, k]
    (ReplayBuffer.stack_rows).  The two paths are the same: conv_bits on the stack with gradients, conv_bits2 on the stack (the stacked
    fused stem, f110_bitconv2_forward_stack) without, so acting writes no conv1 activations to memory at any stack.  Both add the
    frames j major, then ky, kx, and conv2 in the same order, so they still return the same bits."""

    def __init__(self, on=1.0, cols=None, device=None, stack=1):
        super().__init__()
        self.conv1 = BitConv2d(16, 8, 4, on=on, relu=True, cols=cols, device=device, in_channels=stack)
        self.conv2 = FeatConv2d(16, 32, 4, 2, relu=True, device=device)
        self.conv3 = FeatConv2d(32, 32, 3, 1, relu=True, device=device)
        self._check()

    def _check(self):
        from .bitconv import validate2
        c1, c2, c3 = self.conv1, self.conv2, self.conv3
        if c2.weight.shape[1] != c1.weight.shape[0]:
            raise ValueError('Trunk: conv2.in_channels = %d but conv1 has %d output channels' % (c2.weight.shape[1], c1.weight.shape[0]))
        if c3.weight.shape[1] != c2.weight.shape[0]:
            raise ValueError('Trunk: conv3.in_channels = %d but conv2 has %d output channels' % (c3.weight.shape[1], c2.weight.shape[0]))
        k1, k2 = c1.kernel_size, c2.kernel_size
        big = k1 + c1.stride * (k2 - 1)                                            # the smallest image with one output of conv2
        validate2(big, big, k1, c1.stride, c1.weight.shape[0], k2, c2.stride, c2.weight.shape[0], c1.on)

    @classmethod
    def from_convs(cls, conv1, conv2, conv3, on=1.0, cols=None, stack=1):
        """A trunk that shares the parameters of an existing network's three nn.Conv2d (the same tensors: training one trains the
        other).  ValueError where BitConv2d.from_conv or FeatConv2d.from_conv raises, for channel counts that do not chain, and
        for a conv2 the fused stem refuses.  stack = k: conv1 must be an nn.Conv2d(k, ...); the trunk then reads stacks of k frames."""
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.conv1 = BitConv2d.from_conv(conv1, on=on, relu=True, cols=cols, in_channels=stack)
        m.conv2 = FeatConv2d.from_conv(conv2, relu=True)
        m.conv3 = FeatConv2d.from_conv(conv3, relu=True)
        m._check()
        return m

    stack = property(lambda self: int(self.conv1.weight.shape[1]))

    def forward(self, frames, index=None):
        c1, c2, c3 = self.conv1, self.conv2, self.conv3
        cols = None if frames.dtype == torch.uint8 else c1.cols
        params = (c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias)
        if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in params):
            a1 = conv_bits(frames, c1.weight, c1.bias, stride=c1.stride, on=c1.on, relu=True, index=index, cols=cols)
            a2 = conv_feat(a1, c2.weight, c2.bias, stride=c2.stride, relu=True)
        else:
            a2 = conv_bits2(frames, c1.weight, c1.bias, c2.weight, c2.bias, stride1=c1.stride, stride2=c2.stride, on=c1.on,
                            relu1=True, relu2=True, index=index, cols=cols)
        return conv_feat(a2, c3.weight, c3.bias, stride=c3.stride, relu=True).flatten(1)
