"""Bit convolution without a GPU: the checker of tests/bitconv_cases.py against the reference's own operator (torch's conv2d in
fp64 on the unpacked image), the library's host-only validate entry, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bitconv_cases as bc
import replay_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('f110_bitconv_validate', 'f110_bitconv_workspace', 'f110_bitconv_forward', 'f110_bitconv_forward_u8',
               'f110_bitconv_backward', 'f110_replay_locate')


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.CASES)
def test_checker_against_conv2d_in_fp64(rows, cols, kernel, stride, channels):
    """|checker - conv2d_fp64(unpacked * on)| <= gamma_k (|on| sum |w[c]| + |b[c]|) per element, k = kernel^2 + 2 roundings
    (kernel^2 additions, the product with `on`, the bias): the bound of a recursive fp32 sum, derived, not tuned."""
    import torch
    import torch.nn.functional as F
    imgs = bc.images(rows, cols)
    w, b = bc.params(kernel, channels)
    unpacked = torch.as_tensor(rc.unpack(rc.pack(imgs), cols) == 255).double()[:, None]
    for on in bc.ONS:
        on32 = float(np.float32(on))
        for bias in (b, None):
            want = F.conv2d(unpacked * on32, torch.as_tensor(w).double(), None if bias is None else torch.as_tensor(bias).double(), stride=stride).numpy()
            bound = bc.gamma(kernel * kernel + 2) * (abs(on32) * np.abs(w.astype(np.float64)).sum(axis=(1, 2, 3)) + (0.0 if bias is None else np.abs(bias.astype(np.float64))))
            for relu in (False, True):
                got = bc.forward(imgs, w, bias, stride, on, relu)
                assert got.dtype == np.float32 and got.shape == (3, channels) + bc.out_size(rows, cols, kernel, stride)
                ref = np.maximum(want, 0.0) if relu else want
                excess = np.abs(got.astype(np.float64) - ref) - bound[None, :, None, None]
                print('on=%g bias=%s relu=%s: worst |diff| / bound = %.3f' % (on, bias is not None, relu, float((np.abs(got - ref) / bound[None, :, None, None]).max())))
                assert (excess <= 0).all()
    # the empty image gives the bias alone and the all-set one on * (the taps summed in order) + bias
    got = bc.forward(imgs, w, b, stride, 1.0, False)
    assert (got[2] == b[:, None, None]).all()
    acc = np.zeros(channels, np.float32)
    for t in range(kernel * kernel):
        acc = acc + w[:, 0, t // kernel, t % kernel]
    assert (got[1] == (acc * np.float32(1.0) + b)[:, None, None]).all()


def test_checker_gradients_against_autograd_in_fp64():
    import torch
    import torch.nn.functional as F
    rows, cols, kernel, stride, channels = bc.CASES[1]
    imgs = bc.many_images(rows, cols, 3)
    w, b = bc.params(kernel, channels)
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    g = np.random.default_rng(2).normal(size=(3, channels, oh, ow)).astype(np.float32)
    on = 255.0
    wt, bt = torch.as_tensor(w).double().requires_grad_(), torch.as_tensor(b).double().requires_grad_()
    x = torch.as_tensor(imgs == 255).double()[:, None] * on
    F.conv2d(x, wt, bt, stride=stride).backward(torch.as_tensor(g).double())
    gw, gb, aw, ab = bc.gradients(imgs, g, kernel, stride, on)
    assert np.allclose(gw, wt.grad.numpy(), rtol=1e-12, atol=1e-9) and np.allclose(gb, bt.grad.numpy(), rtol=1e-12, atol=1e-9)
    assert (aw >= np.abs(gw) / on - 1e-9).all() and (ab >= np.abs(gb) - 1e-9).all()


def test_validate_accepts_and_refuses():
    from red_gym_amd import bitconv
    ok = dict(rows=256, cols=256, kernel=8, stride=4, channels=16, on=1.0)
    bitconv.validate(**ok)
    # the corners: kernel 8, stride 8, channels 64, rows = kernel
    bitconv.validate(rows=8, cols=8, kernel=8, stride=8, channels=64, on=255.0)
    bitconv.validate(rows=1, cols=16384, kernel=1, stride=1, channels=1, on=-1.0 / 255.0, relu=True)
    bitconv.validate(rows=16384, cols=8, kernel=8, stride=1, channels=64)
    for bad, what in ((dict(kernel=0), 'kernel'), (dict(kernel=9), 'kernel'), (dict(stride=0), 'stride'), (dict(stride=9), 'stride'),
                      (dict(kernel=3, stride=4), 'stride'), (dict(channels=0), 'channels'), (dict(channels=65), 'channels'),
                      (dict(rows=7), 'pixels'), (dict(cols=7), 'pixels'), (dict(rows=16385), 'pixels'), (dict(cols=16385), 'pixels'),
                      (dict(on=float('nan')), 'finite'), (dict(on=float('inf')), 'finite'), (dict(on=-float('inf')), 'finite'), (dict(on=1e39), 'finite')):
        with pytest.raises(ValueError, match=what):
            bitconv.validate(**dict(ok, **bad))
    from red_gym_amd import _lib
    lib = _lib.load()
    assert lib.f110_bitconv_validate(None) == _lib.E_INVALID
    assert lib.f110_bitconv_workspace(None, 4) == 0
    c = bitconv.make_config(**ok)
    assert lib.f110_bitconv_workspace(C.byref(c), 0) == 0
    # G = min(n * tiles, 1024) partials of C * (kernel^2 + 1) floats: one image of 256 x 256 is 16 tiles
    assert lib.f110_bitconv_workspace(C.byref(c), 1) == 16 * 16 * 65 * 4
    assert lib.f110_bitconv_workspace(C.byref(c), 4096) == 1024 * 16 * 65 * 4
    c.kernel = 9
    assert lib.f110_bitconv_workspace(C.byref(c), 4) == 0
    # the stateless entries refuse before any HIP call
    c = bitconv.make_config(**ok)
    assert lib.f110_bitconv_forward(C.byref(c), None, 3, None, 3, None, None, None, None) == _lib.E_INVALID
    assert lib.f110_bitconv_forward_u8(C.byref(c), None, 3, None, -1, None, None, None, None) == _lib.E_INVALID
    assert lib.f110_bitconv_backward(C.byref(c), None, 3, None, 3, None, None, None, None, None) == _lib.E_INVALID
    assert lib.f110_replay_locate(None, None, 0, None, None, None) == _lib.E_INVALID


def test_abi_symbols_and_struct_layout():
    from red_gym_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'f110_hip.h')).read()
    declared = set(re.findall(r'\b(f110_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None, name
    assert lib.f110_bitconv_workspace.restype is C.c_int64
    body = hdr[hdr.rindex('typedef struct {', 0, hdr.index('} f110_bitconv_config;')):hdr.index('} f110_bitconv_config;')]
    fields = []
    for ctype, names in re.findall(r'^\s*(int32_t|float)\s+([a-z_, ]+);', body, re.M):
        fields += [(n.strip(), C.c_int32 if ctype == 'int32_t' else C.c_float) for n in names.split(',')]
    assert fields == list(_lib.BitconvConfig._fields_)
    assert C.sizeof(_lib.BitconvConfig) == 7 * 4
    # one argument per parameter of the declaration
    for name in NEW_SYMBOLS:
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, hdr).group(1)
        assert len(_lib.SYMBOLS[name]) == decl.count(',') + 1, name


def test_module_parameters_without_gpu():
    import torch
    from red_gym_amd.bitconv import BitConv2d
    conv = torch.nn.Conv2d(1, 16, 8, 4)
    m = BitConv2d.from_conv(conv)
    assert m.weight is conv.weight and m.bias is conv.bias
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in conv.state_dict().items()}
    fresh = BitConv2d(16, 8, 4)
    fresh.load_state_dict(conv.state_dict())
    other = torch.nn.Conv2d(1, 16, 8, 4)
    other.load_state_dict(fresh.state_dict())
    assert torch.equal(other.weight, conv.weight) and torch.equal(other.bias, conv.bias)
    for bad in (torch.nn.Conv2d(3, 16, 8, 4), torch.nn.Conv2d(1, 16, 8, 4, padding=1), torch.nn.Conv2d(1, 16, 8, 4, dilation=2),
                torch.nn.Conv2d(2, 16, 8, 4, groups=2), torch.nn.Conv2d(1, 16, 9, 4), torch.nn.Conv2d(1, 65, 8, 4),
                torch.nn.Conv2d(1, 16, (8, 4), 4), torch.nn.Linear(3, 3)):
        with pytest.raises(ValueError):
            BitConv2d.from_conv(bad)
