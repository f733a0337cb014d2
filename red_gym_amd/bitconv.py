"""The first layer of the reference's policy computed from bits (csrc/f110_bitconv.h): Actor and Critic both open with
nn.Conv2d(1, 16, kernel_size=8, stride=4) on the 256 x 256 FILL bitmap (src/SAL.py:397, 429), fed FloatTensor(state) / 255 when
acting (:510) and the raw 0 / 255 floats when learning (:536).  An image of two values needs no fp32 copy: conv_bits reads the
env's uint8 bitmap or the replay ring's packed frames directly, forward and backward; `on` is what a set pixel is worth (1.0 and
255.0 for the two scalings above).  There is no CPU path and no torch fallback: the kernels of libf110_hip.so do the work."""
import ctypes as C
import math

import torch

from . import _lib

MAX_KERNEL, MAX_CHANNELS = 8, 64


def make_config(rows, cols, kernel, stride=1, channels=1, on=1.0, relu=False):
    """An f110_bitconv_config; out-of-range integers are clamped into int32 so that validate() can name them."""
    c = _lib.BitconvConfig()
    clamp = lambda v: max(min(int(v), 2 ** 31 - 1), -2 ** 31)  # noqa: E731
    c.rows, c.cols, c.kernel, c.stride, c.channels = clamp(rows), clamp(cols), clamp(kernel), clamp(stride), clamp(channels)
    c.relu = 1 if relu else 0
    c.on = float(on)
    return c


def validate(rows, cols, kernel, stride=1, channels=1, on=1.0, relu=False):
    """f110_bitconv_validate (host only, no device): ValueError for what the kernels refuse."""
    on = float(on)
    if math.isfinite(on) and abs(on) > 3.4028234663852886e38:
        raise ValueError('bitconv: `on` = %g is not finite in fp32' % on)
    c = make_config(rows, cols, kernel, stride, channels, on, relu)
    _lib.check(_lib.load().f110_bitconv_validate(C.byref(c)))
    return c


def output_size(rows, cols, kernel, stride):
    return (rows - kernel) // stride + 1, (cols - kernel) // stride + 1


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class _ConvBits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frames, weight, bias, index, cfg, n, u8):
        lib = _lib.load()
        dev = frames.device
        oh, ow = output_size(cfg.rows, cfg.cols, cfg.kernel, cfg.stride)
        out = torch.empty((n, cfg.channels, oh, ow), dtype=torch.float32, device=dev)
        w = weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        fn = lib.f110_bitconv_forward_u8 if u8 else lib.f110_bitconv_forward
        with torch.cuda.device(dev):
            _lib.check(fn(C.byref(cfg), frames.data_ptr(), frames.shape[0], None if index is None else index.data_ptr(), n,
                          w.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), _stream(dev)))
        ctx.cfg, ctx.n, ctx.u8, ctx.has_bias = cfg, n, u8, bias is not None
        ctx.save_for_backward(frames, index, out if cfg.relu else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .replay import pack_bitmaps
        lib = _lib.load()
        frames, index, out = ctx.saved_tensors
        cfg, n = ctx.cfg, ctx.n
        dev = grad_out.device
        if out is not None:
            grad_out = grad_out * (out > 0)           # relu: the kernel takes grad_out already masked
        g = grad_out.to(torch.float32).contiguous()
        if ctx.u8:
            frames = pack_bitmaps(frames)             # the backward kernel reads bits (1/8 of the bytes, once per update)
        kk = cfg.kernel * cfg.kernel
        gw = torch.empty((cfg.channels, 1, cfg.kernel, cfg.kernel), dtype=torch.float32, device=dev)
        gb = torch.empty((cfg.channels,), dtype=torch.float32, device=dev) if ctx.has_bias and ctx.needs_input_grad[2] else None
        nbytes = lib.f110_bitconv_workspace(C.byref(cfg), n)
        assert nbytes >= 4 * cfg.channels * (kk + 1)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.f110_bitconv_backward(C.byref(cfg), frames.data_ptr(), frames.shape[0], None if index is None else index.data_ptr(), n,
                                                 g.data_ptr(), gw.data_ptr(), None if gb is None else gb.data_ptr(), ws.data_ptr(), _stream(dev)))
        return None, (gw if ctx.needs_input_grad[1] else None), gb, None, None, None, None


def conv_bits(frames, weight, bias=None, stride=1, on=1.0, relu=False, index=None, cols=None):
    """nn.Conv2d(1, C, kernel, stride) on images of two values, from their bits.
    frames: int64 [m, rows, words] device tensor in the replay ring's format (replay.pack_bitmaps, ReplayBuffer.sample_frames)
    with `cols` given, or uint8 [m, rows, cols] (a pixel is set iff it == 255: info['lidar_bitmap']).
    weight [C, 1, k, k] fp32, bias [C] fp32 or None; on: the value of a set pixel; relu: max(out, 0) fused.
    index: None (sample i = frame i) or int64 [n]: the frame of each sample, -1 (or any entry outside 0 .. m - 1) = a frame of
    zeros; repeats are allowed.
    Returns [n, C, OH, OW] fp32 on the caller's current stream, without synchronising: out = on * sum of the weights under set
    pixels + bias, the taps added in the order ky major, kx minor (csrc/f110_bitconv.h).  Differentiable in weight and bias;
    frames are data.  ValueError for what f110_bitconv_validate refuses and for a dtype / shape mismatch."""
    if not torch.is_tensor(frames) or not torch.is_tensor(weight):
        raise ValueError('conv_bits: frames and weight must be tensors')
    if not frames.is_cuda or weight.device != frames.device:
        raise ValueError('conv_bits: frames and weight must be on the same GPU')
    if frames.dim() != 3:
        raise ValueError('conv_bits: frames must be [m, rows, words] int64 or [m, rows, cols] uint8, not %s' % (tuple(frames.shape),))
    if weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[1] != 1 or weight.shape[2] != weight.shape[3]:
        raise ValueError('conv_bits: weight must be fp32 [C, 1, k, k], not %s %s' % (weight.dtype, tuple(weight.shape)))
    ch, k = int(weight.shape[0]), int(weight.shape[2])
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (ch,) or bias.device != frames.device):
        raise ValueError('conv_bits: bias must be fp32 [%d] on the frames\' device' % ch)
    rows = int(frames.shape[1])
    if frames.dtype == torch.uint8:
        u8 = True
        if cols is not None and int(cols) != frames.shape[2]:
            raise ValueError('conv_bits: cols=%d but the uint8 images have %d columns' % (int(cols), frames.shape[2]))
        cols = int(frames.shape[2])
    elif frames.dtype == torch.int64:
        u8 = False
        if cols is None:
            raise ValueError('conv_bits: packed frames need cols=')
        cols = int(cols)
        if cols < 1 or frames.shape[2] != (cols + 63) // 64:
            raise ValueError('conv_bits: %d words per row do not hold %d pixels' % (frames.shape[2], cols))
    else:
        raise ValueError('conv_bits: frames must be int64 (packed) or uint8, not %s' % frames.dtype)
    cfg = validate(rows, cols, k, stride, ch, on, relu)
    if index is not None:
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1 or index.device != frames.device:
            raise ValueError('conv_bits: index must be an int64 vector on the frames\' device')
        index = index.contiguous()
        n = int(index.shape[0])
    else:
        n = int(frames.shape[0])
    return _ConvBits.apply(frames.contiguous(), weight, bias, index, cfg, n, u8)


class BitConv2d(torch.nn.Module):
    """nn.Conv2d(1, out_channels, kernel_size, stride) on two-valued images, computed by conv_bits.  Its parameters have the
    names and shapes of nn.Conv2d's (weight [C, 1, k, k], bias [C]), so state dicts pass between the two in both directions.
    forward(frames, index=None): frames uint8 [n, rows, cols], or int64 packed [m, rows, words] when `cols` was given."""

    def __init__(self, out_channels, kernel_size, stride=1, bias=True, on=1.0, relu=False, cols=None, device=None):
        super().__init__()
        k = int(kernel_size)
        ref = torch.nn.Conv2d(1, int(out_channels), k, int(stride), bias=bias, device=device)   # (for its initialisation)
        self.weight = ref.weight
        self.register_parameter('bias', ref.bias)
        self.kernel_size, self.stride, self.on, self.relu, self.cols = k, int(stride), float(on), bool(relu), cols
        validate(k, k, k, self.stride, int(out_channels), self.on)

    @classmethod
    def from_conv(cls, conv, on=1.0, relu=False, cols=None):
        """A BitConv2d that shares the parameters of `conv` (the same tensors: training one trains the other).  ValueError
        unless it is an nn.Conv2d(1, C, k, stride) with a square kernel and stride, no padding, dilation or groups."""
        pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)  # noqa: E731
        if not isinstance(conv, torch.nn.Conv2d):
            raise ValueError('BitConv2d.from_conv: not an nn.Conv2d')
        if conv.in_channels != 1:
            raise ValueError('BitConv2d.from_conv: in_channels = %d (a bitmap has one channel)' % conv.in_channels)
        if conv.groups != 1 or pair(conv.dilation) != (1, 1) or isinstance(conv.padding, str) or pair(conv.padding) != (0, 0):
            raise ValueError('BitConv2d.from_conv: padding, dilation and groups are not supported')
        ks, st = pair(conv.kernel_size), pair(conv.stride)
        if ks[0] != ks[1] or st[0] != st[1]:
            raise ValueError('BitConv2d.from_conv: kernel and stride must be square')
        validate(ks[0], ks[0], ks[0], st[0], conv.out_channels, on)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.weight = conv.weight
        m.register_parameter('bias', conv.bias)
        m.kernel_size, m.stride, m.on, m.relu, m.cols = ks[0], st[0], float(on), bool(relu), cols
        return m

    def forward(self, frames, index=None):
        return conv_bits(frames, self.weight, self.bias, stride=self.stride, on=self.on, relu=self.relu, index=index,
                         cols=None if frames.dtype == torch.uint8 else self.cols)

    def extra_repr(self):
        return '1, %d, kernel_size=%d, stride=%d, on=%g, relu=%s' % (self.weight.shape[0], self.kernel_size, self.stride, self.on, self.relu)
