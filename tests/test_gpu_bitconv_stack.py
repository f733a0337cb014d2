"""The first convolution on a stack of frames (f110_bitconv_forward_stack / _backward_stack, conv_bits with a weight [C, k, K, K],
BitConv2d(in_channels=k), Trunk(stack=k)): the forward `==` the checker of tests/stack_cases.py bit for bit at every shape-selected
path, with -1, entries beyond the frames and repeats in the index; a stack of one `==` the one-frame entry; the backward, column by
column, `==` the one-frame entry and `==` the exact sums where grad_out is made of small integers, from a workspace of NaN; autograd
through the module; and the trunk's two paths."""
import ctypes as C

import numpy as np
import pytest

import bitconv_cases as bc
import gpu_checks as gk
import replay_cases as rc
import stack_cases as sc
from test_gpu_bitconv import _raw_backward, _raw_forward

pytestmark = pytest.mark.gpu

SAL = (24, 260, 8, 4, 16)                      # SAL's kernel and stride with OW exactly 64 and OH 5 (bc.SHAPES[8])
VARIANTS = [(on, relu, bias) for on in bc.ONS for relu in (False, True) for bias in (True, False)]


def _frames_pool(rows, cols):
    """The three images of bc.images and rc.edge_images (single pixels at columns 0, 63, 64 and cols - 1)."""
    return np.concatenate([bc.images(rows, cols), rc.edge_images(rows, cols)])


def _raw_forward_stack(frames, n_frames, index, cfg, w, b):
    """f110_bitconv_forward_stack itself, into an array of -7 with a margin either side that must stay as it was."""
    import torch
    from red_gym_amd import _lib
    lib = _lib.load()
    n, k = index.shape
    oh, ow = bc.out_size(cfg.rows, cfg.cols, cfg.kernel, cfg.stride)
    buf = gk.Guarded(n * cfg.channels * oh * ow, fill=-7.0)
    _lib.check(lib.f110_bitconv_forward_stack(C.byref(cfg), frames.data_ptr(), n_frames, index.data_ptr(), k, n, w.data_ptr(),
                                              None if b is None else b.data_ptr(), buf.ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf.read().reshape(n, cfg.channels, oh, ow)


def _forward_case(rows, cols, kernel, stride, channels, k, n=3):
    from red_gym_amd import bitconv
    imgs = _frames_pool(rows, cols)
    frames = gk.packed(imgs)
    w, b = sc.params_stack(kernel, channels, k, seed=3)
    wd, bd = gk.to_device(w), gk.to_device(b)
    index = sc.stack_index(n, k, len(imgs), seed=kernel)
    assert (index == -1).any() and (index >= len(imgs)).any() and (k == 1 or (index[n // 2, 0] == index[n // 2, 1]))
    idx = gk.to_device(index)
    total, outs = 0, {}
    for on, relu, bias in VARIANTS:
        want = sc.forward_stack(imgs, index, w, b if bias else None, stride, on, relu)
        cfg = bitconv.make_config(rows, cols, kernel, stride, channels, on, relu)
        got = _raw_forward_stack(frames, len(imgs), idx, cfg, wd, bd if bias else None)
        bad = gk.differing(got, want)
        print('%d x %d k%d s%d c%d stack %d on=%g relu=%s bias=%s: %d of %d elements differ' % (rows, cols, kernel, stride, channels, k, on, relu, bias, bad, want.size))
        total += bad
        outs[(on, relu, bias)] = got
        if k == 1:                              # a stack of one frame is the one-frame entry
            one = _raw_forward(frames, len(imgs), gk.to_device(index[:, 0].copy()), n, cfg, gk.to_device(w), bd if bias else None)
            assert np.array_equal(bc.bit_patterns(got), bc.bit_patterns(one))
    assert total == 0
    plain = outs[(1.0, False, True)]
    assert (plain[0] != plain[1]).any() and (channels < 5 or ((plain < 0).any() and (plain > 0).any()))
    # a row's output does not depend on the batch around it
    cfg = bitconv.make_config(rows, cols, kernel, stride, channels, 1.0, False)
    for i in range(n):
        alone = _raw_forward_stack(frames, len(imgs), gk.to_device(index[i:i + 1].copy()), cfg, wd, bd)
        assert np.array_equal(bc.bit_patterns(alone[0]), bc.bit_patterns(plain[i]))


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.SHAPES)
def test_forward_stack_equals_checker_at_every_path(rows, cols, kernel, stride, channels):
    """stack = 3, n = 3 at the ten shapes of bc.SHAPES (every kernel size, both branches of the mask, partial tiles, the tail word, one
    to 64 channels: whole and partly filled chunks of accumulators), times on, relu and bias."""
    _forward_case(rows, cols, kernel, stride, channels, 3)


@pytest.mark.parametrize('k', [1, 2, 8])
def test_forward_stack_at_sals_shape(k):
    _forward_case(*SAL, k)


def _raw_backward_stack(frames, n_frames, index, cfg, g, with_bias=True):
    """f110_bitconv_backward_stack itself from a workspace of NaN, outputs and workspace between guards."""
    import torch
    from red_gym_amd import _lib
    lib = _lib.load()
    n, k = index.shape
    kk = cfg.kernel * cfg.kernel
    gw, gb = gk.Guarded(cfg.channels * k * kk, fill=-7.0), gk.Guarded(cfg.channels, fill=-7.0)
    nbytes = lib.f110_bitconv_workspace_stack(C.byref(cfg), k, n)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = gk.Guarded(nbytes // 4, fill=float('nan'))
    _lib.check(lib.f110_bitconv_backward_stack(C.byref(cfg), frames.data_ptr(), n_frames, index.data_ptr(), k, n, g.data_ptr(), gw.ptr,
                                               gb.ptr if with_bias else None, ws.ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ws.read()
    assert with_bias or gb.untouched()
    return gw.read().reshape(cfg.channels, k, cfg.kernel, cfg.kernel), gb.read()


def _backward_index(n, k):
    """[n, k] over bc.EXACT_FRAMES frames: column j is bc.exact_index's (with -1 and entries beyond the frames) rolled by j; a lone
    sample reads the random frames 1, 2, 0."""
    if n == 1:
        return np.array([[1, 2, 0][:k]], np.int64)
    return np.ascontiguousarray(np.stack([np.roll(bc.exact_index(n, True), j) for j in range(k)], axis=1))


@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('rows,cols,kernel,stride,channels,n', bc.BACKWARD_SHAPES)
def test_backward_stack_is_the_one_frame_backward_column_by_column(rows, cols, kernel, stride, channels, n, k):
    """At bc.BACKWARD_SHAPES (every kernel size, one to four chunks of channels, workgroups that walk one, two and three tiles): with a
    grad_out of mixed magnitude every grad_weight[:, j] and grad_bias `==` f110_bitconv_backward on index[:, j], two calls give the same
    bits, and without grad_bias nothing is written there; with a grad_out of small integers both `==` the exact sums."""
    from red_gym_amd import bitconv
    imgs = bc.many_images(rows, cols, bc.EXACT_FRAMES)
    frames = gk.packed(imgs)
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    index = _backward_index(n, k)
    idx = gk.to_device(index)
    rng = np.random.default_rng([rows, cols, n, k])
    g = (rng.normal(size=(n, channels, oh, ow)) * 10.0 ** rng.integers(-2, 2, (n, channels, 1, 1))).astype(np.float32)
    gd = gk.to_device(g)
    cfg = bitconv.make_config(rows, cols, kernel, stride, channels, 255.0)
    gw, gb = _raw_backward_stack(frames, len(imgs), idx, cfg, gd)
    for j in range(k):
        one_w, one_b = _raw_backward(frames, len(imgs), gk.to_device(index[:, j].copy()), n, cfg, gd, ws_fill=float('nan'))
        assert np.array_equal(bc.bit_patterns(gw[:, j]), bc.bit_patterns(one_w[:, 0])), j
        assert np.array_equal(bc.bit_patterns(gb), bc.bit_patterns(one_b)), j
    assert np.isfinite(gw).all() and (gw != 0).any() and (k < 2 or (gw[:, 0] != gw[:, 1]).any())
    gw2, gb2 = _raw_backward_stack(frames, len(imgs), idx, cfg, gd)
    assert np.array_equal(bc.bit_patterns(gw), bc.bit_patterns(gw2)) and np.array_equal(bc.bit_patterns(gb), bc.bit_patterns(gb2))
    gw3, _ = _raw_backward_stack(frames, len(imgs), idx, cfg, gd, with_bias=False)
    assert np.array_equal(bc.bit_patterns(gw), bc.bit_patterns(gw3))
    # small integers: every partial sum is exact, the kernels have no freedom left
    gi = bc.exact_grad_out(n, channels, oh, ow)
    for on in (1.0, 255.0):
        cfg = bitconv.make_config(rows, cols, kernel, stride, channels, on)
        gw, gb = _raw_backward_stack(frames, len(imgs), idx, cfg, gk.to_device(gi))
        for j in range(k):
            want_w, want_b = bc.exact_gradients(bc.exact_sums(bc.pick(imgs, index[:, j]), gi, kernel, stride), on)
            assert np.array_equal(bc.bit_patterns(gw[:, j]), bc.bit_patterns(want_w[:, 0])), (on, j)
            assert np.array_equal(bc.bit_patterns(gb), bc.bit_patterns(want_b))


@pytest.mark.parametrize('rows,cols,kernel,stride,channels,n', [bc.BACKWARD_SHAPES[3], bc.BACKWARD_SHAPES[2]])
def test_a_stack_of_one_is_the_one_frame_entry_forward_and_backward(rows, cols, kernel, stride, channels, n):
    """stack = 1 with an index [3, 1], at one chunk of channels (16) and at four (64): the raw stacked entries' out, grad_weight and
    grad_bias `==` f110_bitconv_forward / f110_bitconv_backward on index[:, 0], outputs and workspaces between guards."""
    from red_gym_amd import bitconv
    assert n == 3 and (channels + 15) // 16 in (1, 4)
    imgs = bc.many_images(rows, cols, bc.EXACT_FRAMES)
    frames = gk.packed(imgs)
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    index = _backward_index(n, 1)
    assert index.shape == (n, 1) and (index == -1).any()
    idx, flat = gk.to_device(index), gk.to_device(index[:, 0].copy())
    w, b = sc.params_stack(kernel, channels, 1, seed=3)
    wd, bd = gk.to_device(w), gk.to_device(b)
    rng = np.random.default_rng([rows, cols, n, 1])
    gd = gk.to_device((rng.normal(size=(n, channels, oh, ow)) * 10.0 ** rng.integers(-2, 2, (n, channels, 1, 1))).astype(np.float32))
    cfg = bitconv.make_config(rows, cols, kernel, stride, channels, 255.0, True)
    out = _raw_forward_stack(frames, len(imgs), idx, cfg, wd, bd)
    assert np.array_equal(bc.bit_patterns(out), bc.bit_patterns(_raw_forward(frames, len(imgs), flat, n, cfg, wd, bd)))
    assert (out > 0).any() and (out[0] != out[2]).any()
    gw, gb = _raw_backward_stack(frames, len(imgs), idx, cfg, gd)
    one_w, one_b = _raw_backward(frames, len(imgs), flat, n, cfg, gd, ws_fill=float('nan'))
    assert gw.shape == one_w.shape and np.array_equal(bc.bit_patterns(gw), bc.bit_patterns(one_w))
    assert np.array_equal(bc.bit_patterns(gb), bc.bit_patterns(one_b))
    assert np.isfinite(gw).all() and (gw != 0).any() and (gb != 0).any()


def test_autograd_through_the_module():
    """BitConv2d(in_channels=3): weight.grad[:, j] and bias.grad `==` the one-frame conv_bits' gradients on index[:, j] for the same
    grad_out; with relu the mask is the output's; the forward is the raw entry's; dtype and shape mismatches are refused."""
    import torch
    from red_gym_amd.bitconv import BitConv2d, conv_bits
    rows, cols, kernel, stride, channels, k, n = 30, 150, 5, 2, 16, 3, 4
    imgs = _frames_pool(rows, cols)
    frames = gk.packed(imgs)
    index = sc.stack_index(n, k, len(imgs))
    idx = gk.to_device(index)
    torch.manual_seed(3)
    conv = BitConv2d(channels, kernel, stride, on=255.0, cols=cols, device='cuda', in_channels=k)
    assert tuple(conv.weight.shape) == (channels, k, kernel, kernel)
    out = conv(frames, idx)
    want = sc.forward_stack(imgs, index, gk.to_host(conv.weight), gk.to_host(conv.bias), stride, 255.0, False)
    assert gk.differing(out, want) == 0 and out.requires_grad
    g = torch.randn_like(out)
    out.backward(g)
    for j in range(k):
        w1 = conv.weight.detach()[:, j:j + 1].clone().requires_grad_()
        b1 = conv.bias.detach().clone().requires_grad_()
        conv_bits(frames, w1, b1, stride=stride, on=255.0, index=idx[:, j].contiguous(), cols=cols).backward(g)
        assert torch.equal(conv.weight.grad[:, j:j + 1].view(torch.int32), w1.grad.view(torch.int32))
        assert torch.equal(conv.bias.grad.view(torch.int32), b1.grad.view(torch.int32))
    # relu: the gradient of the plain layer for grad_out masked where the output is 0
    plain_w, plain_b = conv.weight.grad.clone(), conv.bias.grad.clone()
    relu = BitConv2d.from_conv(torch.nn.Conv2d(k, channels, kernel, stride).cuda(), on=255.0, relu=True, cols=cols, in_channels=k)
    with torch.no_grad():
        relu.weight.copy_(conv.weight)
        relu.bias.copy_(conv.bias)
    out_r = relu(frames, idx)
    assert torch.equal(out_r, out.detach().clamp(min=0.0)) and bool((out_r == 0).any()) and bool((out_r > 0).any())
    out_r.backward(g)
    conv.weight.grad, conv.bias.grad = None, None
    conv(frames, idx).backward(g * (out_r > 0))
    assert torch.equal(relu.weight.grad, conv.weight.grad) and torch.equal(relu.bias.grad, conv.bias.grad) and not torch.equal(plain_w, conv.weight.grad)
    assert not torch.equal(plain_b, conv.bias.grad)
    # refusals
    w = conv.weight.detach()
    for bad in (lambda: conv_bits(frames, w, None, stride=stride, index=None, cols=cols), lambda: conv_bits(frames, w, None, stride=stride, index=idx[:, 0].contiguous(), cols=cols),
                lambda: conv_bits(frames, w, None, stride=stride, index=idx[:, :2].contiguous(), cols=cols), lambda: conv_bits(gk.to_device(imgs), w, None, stride=stride, index=idx),
                lambda: conv_bits(frames, torch.zeros((4, 9, 5, 5), device='cuda'), None, stride=stride, index=torch.zeros((n, 9), dtype=torch.int64, device='cuda'), cols=cols),
                lambda: conv_bits(frames, w, None, stride=stride, index=idx.int(), cols=cols)):
        with pytest.raises(ValueError):
            bad()


def test_the_trunks_two_paths_return_the_same_bits():
    """Trunk(stack=3): without gradients and with them the features are torch.equal, and the backward reaches conv1's [16, 3, 8, 8]."""
    import torch
    from red_gym_amd.featconv import Trunk
    rows, cols, k, n = 60, 76, 3, 5
    imgs = rc.random_images(rows, cols, n=6, seed=2)
    frames = gk.packed(imgs)
    idx = gk.to_device(sc.stack_index(n, k, 6))
    torch.manual_seed(5)
    trunk = Trunk(on=255.0, cols=cols, device='cuda', stack=k)
    assert trunk.stack == k and tuple(trunk.conv1.weight.shape) == (16, k, 8, 8)
    with torch.no_grad():
        acting = trunk(frames, idx)
    learning = trunk(frames, idx)
    assert not acting.requires_grad and learning.requires_grad and torch.equal(acting, learning.detach())
    assert acting.shape[0] == n and bool((acting > 0).any())
    learning.sum().backward()
    grad = trunk.conv1.weight.grad
    assert tuple(grad.shape) == (16, k, 8, 8) and bool(torch.isfinite(grad).all()) and all(bool((grad[:, j] != 0).any()) for j in range(k))
    shared = Trunk.from_convs(torch.nn.Conv2d(k, 16, 8, 4).cuda(), torch.nn.Conv2d(16, 32, 4, 2).cuda(), torch.nn.Conv2d(32, 32, 3, 1).cuda(), on=255.0, cols=cols, stack=k)
    assert shared.stack == k
    with torch.no_grad():
        assert shared(frames, idx).shape == acting.shape
    assert Trunk(on=255.0, cols=cols, device='cuda').stack == 1
