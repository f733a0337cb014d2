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
MAX_STACK = _lib.F110_BITCONV_MAX_STACK                         # input channels of conv_bits: frames of a stack
MAX_KERNEL2, MAX_STEM_CHANNELS, MAX_STEM_WIDTH = 4, 16, 64     # conv_bits2: kernel2, the first layer's channels and output width


def _first_layer(c, rows, cols, kernel, stride, channels, on, relu):
    """The fields the two configs share, into `c`."""
    clamp = _lib.clamp
    c.rows, c.cols, c.kernel, c.stride, c.channels = clamp(rows), clamp(cols), clamp(kernel), clamp(stride), clamp(channels)
    c.relu = 1 if relu else 0
    c.on = float(on)
    return c


def _finite_fp32(on):
    """float(on); ValueError for a finite value that fp32 cannot hold (inf and nan are f110_bitconv_validate's to name)."""
    on = float(on)
    if math.isfinite(on) and abs(on) > 3.4028234663852886e38:
        raise ValueError('bitconv: `on` = %g is not finite in fp32' % on)
    return on


def make_config(rows, cols, kernel, stride=1, channels=1, on=1.0, relu=False):
    """An f110_bitconv_config; out-of-range integers are clamped into int32 so that validate() can name them."""
    return _first_layer(_lib.BitconvConfig(), rows, cols, kernel, stride, channels, on, relu)


def validate(rows, cols, kernel, stride=1, channels=1, on=1.0, relu=False):
    """f110_bitconv_validate (host only, no device): ValueError for what the kernels refuse."""
    c = make_config(rows, cols, kernel, stride, channels, _finite_fp32(on), relu)
    _lib.check(_lib.load().f110_bitconv_validate(C.byref(c)))
    return c


def output_size(rows, cols, kernel, stride):
    return (rows - kernel) // stride + 1, (cols - kernel) // stride + 1


def make_config2(rows, cols, kernel, stride, channels, kernel2, stride2, channels2, on=1.0, relu1=True, relu2=True):
    """An f110_bitconv2_config, clamped like make_config."""
    c = _first_layer(_lib.Bitconv2Config(), rows, cols, kernel, stride, channels, on, relu1)
    c.kernel2, c.stride2, c.channels2 = _lib.clamp(kernel2), _lib.clamp(stride2), _lib.clamp(channels2)
    c.relu2 = 1 if relu2 else 0
    return c


def validate2(rows, cols, kernel, stride, channels, kernel2, stride2, channels2, on=1.0, relu1=True, relu2=True):
    """f110_bitconv2_validate (host only, no device): ValueError for what the fused stem refuses -- everything validate()
    refuses in the first layer, more than 16 first-layer channels, kernel2 outside 1..4, stride2 outside 1..kernel2, channels2
    outside 1..64, a first-layer output smaller than kernel2 or wider than 64."""
    c = make_config2(rows, cols, kernel, stride, channels, kernel2, stride2, channels2, _finite_fp32(on), relu1, relu2)
    _lib.check(_lib.load().f110_bitconv2_validate(C.byref(c)))
    return c


def output_size2(rows, cols, kernel, stride, kernel2, stride2):
    oh, ow = output_size(rows, cols, kernel, stride)
    return (oh - kernel2) // stride2 + 1, (ow - kernel2) // stride2 + 1


class _ConvBits(torch.autograd.Function):
    """conv_bits on checked arguments.  A weight [C, 1, K, K] goes to the one-frame entries (f110_bitconv_forward[_u8] /
    f110_bitconv_backward; index [n] or None), one of k > 1 input channels to f110_bitconv_forward_stack / f110_bitconv_backward_stack
    (packed frames, index [n, k])."""

    @staticmethod
    def forward(ctx, frames, weight, bias, index, cfg, n, u8):
        lib = _lib.load()
        dev = frames.device
        k = int(weight.shape[1])
        oh, ow = output_size(cfg.rows, cfg.cols, cfg.kernel, cfg.stride)
        out = torch.empty((n, cfg.channels, oh, ow), dtype=torch.float32, device=dev)
        w = weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        tail = (n, w.data_ptr(), _lib.ptr(b), out.data_ptr(), _lib.stream(dev))
        with torch.cuda.device(dev):
            if k == 1:
                fn = lib.f110_bitconv_forward_u8 if u8 else lib.f110_bitconv_forward
                _lib.check(fn(C.byref(cfg), frames.data_ptr(), frames.shape[0], _lib.ptr(index), *tail))
            else:
                _lib.check(lib.f110_bitconv_forward_stack(C.byref(cfg), frames.data_ptr(), frames.shape[0], index.data_ptr(), k, *tail))
        ctx.cfg, ctx.n, ctx.u8, ctx.k, ctx.has_bias = cfg, n, u8, k, bias is not None
        ctx.save_for_backward(frames, index, out if cfg.relu else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from .replay import pack_bitmaps
        lib = _lib.load()
        frames, index, out = ctx.saved_tensors
        cfg, n, k = ctx.cfg, ctx.n, ctx.k
        dev = grad_out.device
        if out is not None:
            grad_out = grad_out * (out > 0)           # relu: the kernel takes grad_out already masked
        g = grad_out.to(torch.float32).contiguous()
        if ctx.u8:
            frames = pack_bitmaps(frames)             # the backward kernel reads bits (1/8 of the bytes, once per update)
        gw = torch.empty((cfg.channels, k, cfg.kernel, cfg.kernel), dtype=torch.float32, device=dev)
        gb = torch.empty((cfg.channels,), dtype=torch.float32, device=dev) if ctx.has_bias and ctx.needs_input_grad[2] else None
        if n == 0 and k > 1:                          # (the stacked entry takes n >= 1)
            return None, (gw.zero_() if ctx.needs_input_grad[1] else None), (None if gb is None else gb.zero_()), None, None, None, None
        nbytes = lib.f110_bitconv_workspace(C.byref(cfg), n) if k == 1 else lib.f110_bitconv_workspace_stack(C.byref(cfg), k, n)
        assert nbytes >= 4 * cfg.channels * (cfg.kernel * cfg.kernel + 1) + (8 * k * n if k > 1 else 0) and nbytes % 4 == 0
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        tail = (n, g.data_ptr(), gw.data_ptr(), _lib.ptr(gb), ws.data_ptr(), _lib.stream(dev))
        with torch.cuda.device(dev):
            if k == 1:
                _lib.check(lib.f110_bitconv_backward(C.byref(cfg), frames.data_ptr(), frames.shape[0], _lib.ptr(index), *tail))
            else:
                _lib.check(lib.f110_bitconv_backward_stack(C.byref(cfg), frames.data_ptr(), frames.shape[0], index.data_ptr(), k, *tail))
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
    frames are data.  ValueError for what f110_bitconv_validate refuses and for a dtype / shape mismatch.
    A stack of frames: weight [C, k, K, K] with 1 < k <= MAX_STACK is nn.Conv2d(k, C, K, stride) whose input channel j of sample i is
    frame index[i, j]; index int64 [n, k] is then required (ReplayBuffer.stack_rows gives it) and frames are the packed form.  The
    frames are added j major, then ky, kx; grad_weight[:, j] is bit for bit what the one-frame call gives for index[:, j]."""
    who = 'conv_bits'
    if not torch.is_tensor(frames) or not torch.is_tensor(weight):
        raise ValueError('conv_bits: frames and weight must be tensors')
    if not frames.is_cuda or weight.device != frames.device:
        raise ValueError('conv_bits: frames and weight must be on the same GPU')
    if weight.dtype != torch.float32 or weight.dim() != 4 or weight.shape[1] < 1 or weight.shape[2] != weight.shape[3]:
        raise ValueError('conv_bits: weight must be fp32 [C, 1, k, k], not %s %s' % (weight.dtype, tuple(weight.shape)))
    ch, k, ks = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (ch,) or bias.device != frames.device):
        raise ValueError('conv_bits: bias must be fp32 [%d] on the frames\' device' % ch)
    u8, rows, cols = _stack_frames(who, 'weight', k, frames, index, cols)
    cfg = validate(rows, cols, ks, stride, ch, on, relu)
    index, n = _stack_index(who, k, index, frames)
    return _ConvBits.apply(frames.contiguous(), weight, bias, index, cfg, n, u8)


def _stack_frames(who, what, k, frames, index, cols):
    """(u8, rows, cols) of `frames` for `who` as _frames_kind gives them, after the checks of a first layer of k input channels
    (`what`: its weight's name): beyond one, a stack of at most MAX_STACK packed frames named by an index [n, k]."""
    if k > MAX_STACK:
        raise ValueError('%s: %d input channels (a stack has 1..%d frames)' % (who, k, MAX_STACK))
    if k > 1 and frames.dtype != torch.int64:
        raise ValueError('%s: a stack of frames is read from packed int64 frames (the replay ring\'s), not %s' % (who, frames.dtype))
    kind = _frames_kind(who, frames, cols)
    if k > 1 and (not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 2 or index.shape[1] != k or index.device != frames.device):
        raise ValueError('%s: a %s of %d input channels needs an int64 index [n, %d] on the frames\' device' % (who, what, k, k))
    return kind


def _stack_index(who, k, index, frames):
    """(index, n) for `who` once _stack_frames has passed: the [n, k] index of a stack made contiguous, or what _index_arg gives
    for one frame per sample -- an index [n, 1] is then a stack of one frame: the one-frame entry, the same bits."""
    if k > 1:
        return index.contiguous(), int(index.shape[0])
    if torch.is_tensor(index) and index.dim() == 2 and index.shape[1] == 1:
        index = index[:, 0]
    return _index_arg(who, index, frames)


def _frames_kind(who, frames, cols):
    """(u8, rows, cols) of `frames` for `who`: the checks of both entry points."""
    if frames.dim() != 3:
        raise ValueError('%s: frames must be [m, rows, words] int64 or [m, rows, cols] uint8, not %s' % (who, tuple(frames.shape)))
    rows = int(frames.shape[1])
    if frames.dtype == torch.uint8:
        if cols is not None and int(cols) != frames.shape[2]:
            raise ValueError('%s: cols=%d but the uint8 images have %d columns' % (who, int(cols), frames.shape[2]))
        return True, rows, int(frames.shape[2])
    if frames.dtype == torch.int64:
        if cols is None:
            raise ValueError('%s: packed frames need cols=' % who)
        cols = int(cols)
        if cols < 1 or frames.shape[2] != (cols + 63) // 64:
            raise ValueError('%s: %d words per row do not hold %d pixels' % (who, frames.shape[2], cols))
        return False, rows, cols
    raise ValueError('%s: frames must be int64 (packed) or uint8, not %s' % (who, frames.dtype))


def _index_arg(who, index, frames):
    """(index, n) for `who`: the index made contiguous and its length, or None and the number of frames."""
    if index is None:
        return None, int(frames.shape[0])
    if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1 or index.device != frames.device:
        raise ValueError('%s: index must be an int64 vector on the frames\' device' % who)
    return index.contiguous(), int(index.shape[0])


def conv_bits2(frames, w1, b1, w2, b2, stride1=1, stride2=1, on=1.0, relu1=True, relu2=True, index=None, cols=None):
    """conv2(relu(conv1(frames))) of the reference's Actor / Critic in one kernel (csrc/f110_bitconv2.h), for acting: the first
    layer's activations stay in LDS, only the second layer's output is written.
    frames, index, cols, on: as conv_bits.  w1 [C1, 1, k1, k1] and b1 [C1] or None: the first layer, as conv_bits' weight and
    bias (C1 <= 16, and its output at most 64 wide); w2 [C2, C1, k2, k2] fp32 and b2 [C2] or None on the frames' device (k2 <= 4,
    C2 <= 64); relu1 between the layers, relu2 on the output.
    Inference only: the returned [n, C2, OH2, OW2] fp32 tensor has no grad_fn whatever the parameters require (training goes
    through conv_bits and torch's conv2d: BitConvStem chooses).  Always the fused kernel, on the caller's current stream,
    without synchronising.  Numerics: the first layer exactly as conv_bits, the second acc = fma(w2[co][ci][ky][kx], a1, acc)
    for ci major, ky, kx minor from 0, + b2 -- a function of the bits and the four tensors alone (include/f110_hip.h).
    ValueError for what f110_bitconv2_validate refuses and for a dtype / shape mismatch.
    A stack of frames: w1 [C1, k, k1, k1] with 1 < k <= MAX_STACK selects f110_bitconv2_forward_stack, the same kernel with conv_bits'
    stacked first layer (frames j major, then ky, kx; `on`, b1 and relu1 once, after the last frame): packed int64 frames and an int64
    index [n, k] are then required, as for conv_bits.  The result is bit for bit conv_feat's of conv_bits' stacked output; an index
    [n, 1] with a w1 of one input channel goes to the one-frame entry."""
    who = 'conv_bits2'
    if not torch.is_tensor(frames) or not torch.is_tensor(w1) or not torch.is_tensor(w2):
        raise ValueError('%s: frames, w1 and w2 must be tensors' % who)
    if not frames.is_cuda or w1.device != frames.device or w2.device != frames.device:
        raise ValueError('%s: frames, w1 and w2 must be on the same GPU' % who)
    if w1.dtype != torch.float32 or w1.dim() != 4 or w1.shape[1] < 1 or w1.shape[2] != w1.shape[3]:
        raise ValueError('%s: w1 must be fp32 [C1, 1, k1, k1] or [C1, k, k1, k1], not %s %s' % (who, w1.dtype, tuple(w1.shape)))
    c1, k, k1 = int(w1.shape[0]), int(w1.shape[1]), int(w1.shape[2])
    if w2.dtype != torch.float32 or w2.dim() != 4 or w2.shape[1] != c1 or w2.shape[2] != w2.shape[3]:
        raise ValueError('%s: w2 must be fp32 [C2, %d, k2, k2], not %s %s' % (who, c1, w2.dtype, tuple(w2.shape)))
    c2, k2 = int(w2.shape[0]), int(w2.shape[2])
    for name, b, ch in (('b1', b1, c1), ('b2', b2, c2)):
        if b is not None and (not torch.is_tensor(b) or b.dtype != torch.float32 or tuple(b.shape) != (ch,) or b.device != frames.device):
            raise ValueError('%s: %s must be fp32 [%d] on the frames\' device' % (who, name, ch))
    u8, rows, cols = _stack_frames(who, 'w1', k, frames, index, cols)
    cfg = validate2(rows, cols, k1, stride1, c1, k2, stride2, c2, on, relu1, relu2)
    index, n = _stack_index(who, k, index, frames)
    lib = _lib.load()
    dev = frames.device
    frames = frames.contiguous()
    tensors = [None if t is None else t.detach().contiguous() for t in (w1, b1, w2, b2)]
    oh2, ow2 = output_size2(rows, cols, k1, stride1, k2, stride2)
    out = torch.empty((n, c2, oh2, ow2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if k > 1 and n == 0:
            pass                                      # (the stacked entry takes n >= 1)
        elif k > 1:
            _lib.check(lib.f110_bitconv2_forward_stack(C.byref(cfg), frames.data_ptr(), frames.shape[0], index.data_ptr(), k, n,
                                                       *[_lib.ptr(t) for t in tensors], out.data_ptr(), _lib.stream(dev)))
        else:
            fn = lib.f110_bitconv2_forward_u8 if u8 else lib.f110_bitconv2_forward
            _lib.check(fn(C.byref(cfg), frames.data_ptr(), frames.shape[0], _lib.ptr(index), n, *[_lib.ptr(t) for t in tensors], out.data_ptr(),
                          _lib.stream(dev)))
    return out


def _plain_conv(who, conv, name, in_channels, wrong_in):
    """(kernel, stride) of an nn.Conv2d with `in_channels` inputs, a square kernel and stride, no padding, dilation or groups;
    ValueError from `who` otherwise.  name: what the messages call the layer ('' for the only one); wrong_in: the sentence for
    another in_channels, with one %d for it."""
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)  # noqa: E731
    if not isinstance(conv, torch.nn.Conv2d):
        raise ValueError('%s: %s an nn.Conv2d' % (who, name + ' is not' if name else 'not'))
    if conv.in_channels != in_channels:
        raise ValueError('%s: %s' % (who, wrong_in % conv.in_channels))
    if conv.groups != 1 or pair(conv.dilation) != (1, 1) or isinstance(conv.padding, str) or pair(conv.padding) != (0, 0):
        raise ValueError('%s: padding, dilation and groups are not supported%s' % (who, ' in ' + name if name else ''))
    ks, st = pair(conv.kernel_size), pair(conv.stride)
    if ks[0] != ks[1] or st[0] != st[1]:
        raise ValueError('%s: %skernel and stride must be square' % (who, name + '\'s ' if name else ''))
    return ks[0], st[0]


def _stack_channels(who, in_channels):
    """ValueError from `who` unless in_channels is an int in 1..MAX_STACK."""
    if isinstance(in_channels, bool) or not isinstance(in_channels, int) or not 1 <= in_channels <= MAX_STACK:
        raise ValueError('%s: in_channels %r (an int in 1..%d: the frames of a stack)' % (who, in_channels, MAX_STACK))


class BitConv2d(torch.nn.Module):
    """nn.Conv2d(1, out_channels, kernel_size, stride) on two-valued images, computed by conv_bits.  Its parameters have the
    names and shapes of nn.Conv2d's (weight [C, 1, k, k], bias [C]), so state dicts pass between the two in both directions.
    forward(frames, index=None): frames uint8 [n, rows, cols], or int64 packed [m, rows, words] when `cols` was given.
    in_channels = k > 1: nn.Conv2d(k, ...) on stacks of k packed frames, forward(frames, index [n, k]) (conv_bits)."""

    def __init__(self, out_channels, kernel_size, stride=1, bias=True, on=1.0, relu=False, cols=None, device=None, in_channels=1):
        super().__init__()
        k = int(kernel_size)
        _stack_channels('BitConv2d', in_channels)
        ref = torch.nn.Conv2d(in_channels, int(out_channels), k, int(stride), bias=bias, device=device)   # (for its initialisation)
        self.weight = ref.weight
        self.register_parameter('bias', ref.bias)
        self.kernel_size, self.stride, self.on, self.relu, self.cols = k, int(stride), float(on), bool(relu), cols
        validate(k, k, k, self.stride, int(out_channels), self.on)

    @classmethod
    def from_conv(cls, conv, on=1.0, relu=False, cols=None, in_channels=1):
        """A BitConv2d that shares the parameters of `conv` (the same tensors: training one trains the other).  ValueError
        unless it is an nn.Conv2d(in_channels, C, k, stride) with a square kernel and stride, no padding, dilation or groups;
        in_channels: 1, a bitmap's one channel, or the frames of a stack, 2..MAX_STACK, which the caller names."""
        _stack_channels('BitConv2d.from_conv', in_channels)
        wrong = 'in_channels = %d (a bitmap has one channel)' if in_channels == 1 else 'in_channels = %%d (the stack has %d frames)' % in_channels
        k, s = _plain_conv('BitConv2d.from_conv', conv, '', in_channels, wrong)
        validate(k, k, k, s, conv.out_channels, on)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.weight = conv.weight
        m.register_parameter('bias', conv.bias)
        m.kernel_size, m.stride, m.on, m.relu, m.cols = k, s, float(on), bool(relu), cols
        return m

    def forward(self, frames, index=None):
        return conv_bits(frames, self.weight, self.bias, stride=self.stride, on=self.on, relu=self.relu, index=index,
                         cols=None if frames.dtype == torch.uint8 else self.cols)

    def extra_repr(self):
        return '%d, %d, kernel_size=%d, stride=%d, on=%g, relu=%s' % (self.weight.shape[1], self.weight.shape[0], self.kernel_size, self.stride, self.on,
                                                                       self.relu)


def _plain_conv2(who, conv2, in_channels):
    """(kernel, stride) of an nn.Conv2d(in_channels, C2, k2, stride2) that the stem can run; ValueError otherwise."""
    return _plain_conv(who, conv2, 'conv2', in_channels, 'conv2.in_channels = %%d but conv1 has %d output channels' % in_channels)


class BitConvStem(torch.nn.Module):
    """relu(conv2(relu(conv1(frames)))): the two layers the reference's Actor and Critic open with, on two-valued images.
    Submodules conv1 (a BitConv2d) and conv2 (an nn.Conv2d), so a state dict has the reference's keys conv1.weight, conv1.bias,
    conv2.weight, conv2.bias.  forward(frames, index=None) takes one of two paths: while torch.is_grad_enabled() and one of the
    four parameters requires grad, conv_bits(relu=True) -> F.conv2d -> relu, differentiable as before; otherwise (acting, the
    no_grad block of an update) conv_bits2, the fused kernel, whose result has no grad_fn.  The two paths agree to fp32
    rounding, not bit for bit: torch picks conv2's summation order on the first, the second adds in the order of the contract
    (include/f110_hip.h).
    in_channels = k > 1: conv1 is nn.Conv2d(k, ...) on stacks of k packed frames, forward(frames, index [n, k]); the same two paths,
    conv_bits on the stack with gradients and the stacked fused kernel without."""

    def __init__(self, channels1=16, kernel1=8, stride1=4, channels2=32, kernel2=4, stride2=2, on=1.0, cols=None, device=None, in_channels=1):
        super().__init__()
        self.conv1 = BitConv2d(channels1, kernel1, stride1, on=on, relu=True, cols=cols, device=device, in_channels=in_channels)
        self.conv2 = torch.nn.Conv2d(int(channels1), int(channels2), int(kernel2), int(stride2), device=device)
        self._check()

    def _check(self):
        k2, s2 = _plain_conv2('BitConvStem', self.conv2, self.conv1.weight.shape[0])
        k1 = self.conv1.kernel_size
        big = k1 + self.conv1.stride * (k2 - 1)                                   # the smallest image with one output
        validate2(big, big, k1, self.conv1.stride, self.conv1.weight.shape[0], k2, s2, self.conv2.out_channels, self.conv1.on)

    @classmethod
    def from_convs(cls, conv1, conv2, on=1.0, cols=None, in_channels=1):
        """A stem that shares the parameters of an nn.Conv2d pair (the same tensors: training one trains the other).  ValueError
        where BitConv2d.from_conv raises for conv1, and for a conv2 with padding, dilation, groups, a non-square kernel or stride,
        or in_channels != conv1.out_channels, or sizes the fused kernel refuses.  in_channels = k: conv1 must be an nn.Conv2d(k, ...);
        the stem then reads stacks of k frames."""
        first = BitConv2d.from_conv(conv1, on=on, relu=True, cols=cols, in_channels=in_channels)
        _plain_conv2('BitConvStem.from_convs', conv2, conv1.out_channels)
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.conv1, m.conv2 = first, conv2
        m._check()
        return m

    def forward(self, frames, index=None):
        c1, c2 = self.conv1, self.conv2
        cols = None if frames.dtype == torch.uint8 else c1.cols
        params = (c1.weight, c1.bias, c2.weight, c2.bias)
        if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in params):
            a1 = conv_bits(frames, c1.weight, c1.bias, stride=c1.stride, on=c1.on, relu=True, index=index, cols=cols)
            return torch.relu(torch.nn.functional.conv2d(a1, c2.weight, c2.bias, stride=c2.stride))
        return conv_bits2(frames, c1.weight, c1.bias, c2.weight, c2.bias, stride1=c1.stride, stride2=c2.stride[0], on=c1.on,
                          relu1=True, relu2=True, index=index, cols=cols)
