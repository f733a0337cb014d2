"""Bit convolution on the GPU (csrc/f110_bitconv.h): the forward pass `==` the checker of tests/bitconv_cases.py bit for bit, the
backward pass inside the bound of an fp32 sum around the checker's fp64 gradients and `==` the exact sums where grad_out is made
of small integers, both at every shape-selected path (bc.paths), and the closed loop from the env's bitmap and the replay ring's
frames to features."""
import ctypes as C
import os

import numpy as np
import pytest

import bitconv_cases as bc
import gpu_checks as gk
import replay_cases as rc
import shaping_cases as sc

pytestmark = pytest.mark.gpu


_forward_cache = {}


def _want(key, imgs, w, b, stride, on, relu):
    """The checker's output, computed once per (case, batch, on, relu, bias) and left unchanged."""
    if key not in _forward_cache:
        out = bc.forward(imgs, w, b, stride, on, relu)
        out.setflags(write=False)
        _forward_cache[key] = out
    return _forward_cache[key]


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.CASES)
def test_forward_equals_checker(golden, rows, cols, kernel, stride, channels):
    """f110_bitconv_forward on packed frames `==` the checker as raw 32-bit patterns: three images (arbitrary bytes, all set,
    empty), on in {1, 255, 1 / 255}, relu both ways, bias present and NULL; SAL's shape also on five FILL images of g16."""
    from red_gym_amd.bitconv import conv_bits
    w, b = bc.params(kernel, channels)
    wd, bd = gk.to_device(w), gk.to_device(b)
    batches = [('abc', bc.images(rows, cols))]
    if (rows, cols) == (256, 256):
        imgs = sc.unpack_images(golden('g16_shaping.npz'), 'a')
        filled = (imgs.reshape(imgs.shape[0], -1) == 255).sum(axis=1)
        filled = np.where(filled == 256 * 256, -1, filled)                      # (an all-set image is one of the three above)
        fill = imgs[np.argsort(-filled, kind='stable')[:5]]                     # the five fullest that hold both values
        assert fill.shape == (5, 256, 256) and all((im == 255).any() and (im == 0).any() for im in fill)
        batches.append(('fill', fill))
    total = 0
    for name, imgs in batches:
        frames = gk.packed(imgs)
        for on in bc.ONS:
            for relu in (False, True):
                for bias, bias_dev in ((b, bd), (None, None)):
                    got = conv_bits(frames, wd, bias_dev, stride=stride, on=on, relu=relu, cols=cols)
                    want = _want((rows, cols, name, on, relu, bias is not None), imgs, w, bias, stride, on, relu)
                    assert tuple(got.shape) == want.shape
                    bad = gk.differing(got, want)
                    print('%d x %d k%d s%d c%d %s on=%g relu=%s bias=%s: %d of %d elements differ' % (rows, cols, kernel, stride, channels, name, on, relu, bias is not None, bad, want.size))
                    total += bad
    assert total == 0
    # the comparison holds something: the random image's output is neither the empty one's nor the full one's, and relu cut some
    plain = _want((rows, cols, 'abc', 1.0, False, True), None, None, None, None, None, None)
    assert (plain[0] != plain[1]).any() and (plain[0] != plain[2]).any()
    if channels >= 5:
        assert (plain < 0).any() and (plain > 0).any()


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.CASES)
def test_uint8_entry_and_index(rows, cols, kernel, stride, channels):
    """The uint8 entry `==` the packed entry on the same images (arbitrary bytes: only 255 is set, 254 is not); an index with -1, an
    entry beyond the frames and repeats."""
    import torch
    from red_gym_amd.bitconv import conv_bits
    w, b = bc.params(kernel, channels, seed=1)
    wd, bd = gk.to_device(w), gk.to_device(b)
    imgs = bc.images(rows, cols)
    assert (imgs[0] == 254).any() and (imgs[0] == 255).any()
    frames = gk.packed(imgs)
    for on, relu in ((1.0, False), (255.0, True)):
        a = conv_bits(frames, wd, bd, stride=stride, on=on, relu=relu, cols=cols)
        u = conv_bits(gk.to_device(imgs), wd, bd, stride=stride, on=on, relu=relu)
        assert torch.equal(a, u) and gk.differing(u, bc.forward(imgs, w, b, stride, on, relu)) == 0
    # an image of 254 everywhere is an empty image; one 255 in it is one set pixel
    almost = np.full((2, rows, cols), 254, np.uint8)
    almost[1, rows // 2, cols // 2] = 255
    u = conv_bits(gk.to_device(almost), wd, bd, stride=stride)
    empty = bc.forward(np.zeros((1, rows, cols), np.uint8), w, b, stride, 1.0, False)
    assert gk.differing(u[:1], empty) == 0 and gk.differing(u, bc.forward(almost, w, b, stride, 1.0, False)) == 0
    assert not torch.equal(u[0], u[1])
    index = [2, -1, 0, 0, imgs.shape[0] + 5]
    for src in (frames, gk.to_device(imgs)):
        got = conv_bits(src, wd, bd, stride=stride, index=gk.to_device(np.array(index, np.int64)), cols=cols)
        full = bc.forward(imgs, w, b, stride, 1.0, False)
        assert got.shape[0] == 5
        assert gk.differing(got[0], full[2]) == 0 and gk.differing(got[2], full[0]) == 0
        assert gk.differing(got[1], empty[0]) == 0 and gk.differing(got[4], empty[0]) == 0          # -1 and out of range: the empty frame
        assert torch.equal(got[2], got[3])                                                         # the repeated rows


def _raw_backward(frames, n_frames, index, n, cfg, g, with_bias=True, ws_fill=-7.0):
    """f110_bitconv_backward itself, into arrays with a margin that must stay as it was; the workspace starts as `ws_fill` (NaN:
    a partial that is read without having been written shows in the result)."""
    import torch
    from red_gym_amd import _lib
    lib = _lib.load()
    kk = cfg.kernel * cfg.kernel
    gw, gb = gk.Guarded(cfg.channels * kk, fill=-7.0), gk.Guarded(cfg.channels, fill=-7.0)
    ws = gk.Guarded(lib.f110_bitconv_workspace(C.byref(cfg), n) // 4, fill=ws_fill)
    _lib.check(lib.f110_bitconv_backward(C.byref(cfg), frames.data_ptr(), n_frames, None if index is None else index.data_ptr(), n, g.data_ptr(),
                                         gw.ptr, gb.ptr if with_bias else None, ws.ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ws.read()
    assert with_bias or gb.untouched()
    return gw.read().reshape(cfg.channels, 1, cfg.kernel, cfg.kernel), gb.read()


def _backward_within_the_bound(rows, cols, kernel, stride, channels, n):
    from red_gym_amd import bitconv
    imgs = bc.many_images(rows, cols, max(n, 3))[:n]
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    rng = np.random.default_rng([rows, cols, n])
    g = (rng.normal(size=(n, channels, oh, ow)) * 10.0 ** rng.integers(-2, 2, (n, channels, 1, 1))).astype(np.float32)
    frames, gd = gk.packed(imgs), gk.to_device(g)
    for on in (255.0, 1.0 / 255.0):
        cfg = bitconv.make_config(rows, cols, kernel, stride, channels, on)
        gw, gb = _raw_backward(frames, n, None, n, cfg, gd)
        want_w, want_b, _, _ = bc.gradients(imgs, g, kernel, stride, on)
        bound_w, bound_b = bc.grad_bounds(imgs, g, kernel, stride, on)
        ew, eb = np.abs(gw - want_w), np.abs(gb - want_b)
        print('%d x %d k%d s%d c%d n=%d on=%g: worst error / bound: weight %.4f, bias %.4f' % (rows, cols, kernel, stride, channels, n, on,
              float((ew / np.maximum(bound_w, 1e-300)).max()), float((eb / np.maximum(bound_b, 1e-300)).max())))
        assert (ew <= bound_w).all() and (eb <= bound_b).all()
        assert np.abs(want_w).max() > 0 and np.abs(want_b).max() > 0
        gw2, gb2 = _raw_backward(frames, n, None, n, cfg, gd)
        assert np.array_equal(bc.bit_patterns(gw), bc.bit_patterns(gw2)) and np.array_equal(bc.bit_patterns(gb), bc.bit_patterns(gb2))
        gw3, _ = _raw_backward(frames, n, None, n, cfg, gd, with_bias=False)
        assert np.array_equal(bc.bit_patterns(gw), bc.bit_patterns(gw3))
    # an index: -1 and an entry beyond the frames read zeros, frame 0 three times
    index = np.array([0, -1, n - 1, 0, n + 3, 1, 0], np.int64)
    m = len(index)
    picked = np.stack([imgs[i] if 0 <= i < n else np.zeros((rows, cols), np.uint8) for i in index])
    gi = np.ascontiguousarray(g[np.arange(m) % n])
    cfg = bitconv.make_config(rows, cols, kernel, stride, channels, 1.0)
    gw, gb = _raw_backward(frames, n, gk.to_device(index), m, cfg, gk.to_device(gi))
    want_w, want_b, _, _ = bc.gradients(picked, gi, kernel, stride, 1.0)
    bound_w, bound_b = bc.grad_bounds(picked, gi, kernel, stride, 1.0)
    assert (np.abs(gw - want_w) <= bound_w).all() and (np.abs(gb - want_b) <= bound_b).all()


@pytest.mark.parametrize('n', bc.BACKWARD_N)
@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.BACKWARD_CASES)
def test_backward_within_the_bound_of_an_fp32_sum(rows, cols, kernel, stride, channels, n):
    """grad_weight and grad_bias against the checker's fp64 gradients: |d grad_weight| <= gamma_(M + 1) |on| sum |grad_out bit|,
    |d grad_bias| <= gamma_M sum |grad_out|, M = n OH OW; two calls give the same bits; without grad_bias nothing is written
    there; and with an index that holds -1 and repeats."""
    _backward_within_the_bound(rows, cols, kernel, stride, channels, n)


@pytest.mark.parametrize('rows,cols,kernel,stride,channels,n', bc.BACKWARD_SHAPES)
def test_backward_within_the_bound_at_every_path(rows, cols, kernel, stride, channels, n):
    """The same test, bound and two-calls-give-the-same-bits check at the shapes of bc.BACKWARD_SHAPES: every kernel size, one to
    four chunks of channels, and workgroups that walk one, two and three tiles."""
    _backward_within_the_bound(rows, cols, kernel, stride, channels, n)


def _raw_forward(src, n_frames, index, n, cfg, w, b):
    """f110_bitconv_forward (int64 frames) or f110_bitconv_forward_u8 (uint8 images) itself, into an array of -7 with a margin
    before and after it that must stay as it was -> the output on the host."""
    import torch
    from red_gym_amd import _lib
    lib = _lib.load()
    oh, ow = bc.out_size(cfg.rows, cfg.cols, cfg.kernel, cfg.stride)
    size = n * cfg.channels * oh * ow
    buf = gk.Guarded(size, fill=-7.0)
    fn = lib.f110_bitconv_forward_u8 if src.dtype == torch.uint8 else lib.f110_bitconv_forward
    _lib.check(fn(C.byref(cfg), src.data_ptr(), n_frames, None if index is None else index.data_ptr(), n, w.data_ptr(),
                  None if b is None else b.data_ptr(), buf.ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf.read().reshape(n, cfg.channels, oh, ow)


FORWARD_VARIANTS = ((255.0, True, True), (1.0 / 255.0, False, False))      # (on, relu, bias); the cross product runs on bc.CASES


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.SHAPES)
def test_forward_equals_checker_at_every_path(rows, cols, kernel, stride, channels):
    """Both entries `==` the checker as raw bit patterns at the shapes of bc.SHAPES (every kernel size, both branches of the mask,
    the largest LDS footprint, full and partial tiles, the tail word, more than 16 channels on several tiles): the three images
    of bc.images and rc.edge_images (single pixels at columns 0, 63, 64 and cols - 1), on = 255 with relu and bias, on = 1 / 255
    without either, and an index with -1, a repeat and an entry beyond the frames; the output's margins stay as they were."""
    from red_gym_amd import bitconv
    w, b = bc.params(kernel, channels, seed=3)
    wd, bd = gk.to_device(w), gk.to_device(b)
    batches = (('abc', bc.images(rows, cols)), ('edge', rc.edge_images(rows, cols)))
    total = 0
    for name, imgs in batches:
        srcs = (('packed', gk.packed(imgs)), ('uint8', gk.to_device(imgs)))
        for on, relu, bias in FORWARD_VARIANTS:
            want = bc.forward(imgs, w, b if bias else None, stride, on, relu)
            cfg = bitconv.make_config(rows, cols, kernel, stride, channels, on, relu)
            for entry, src in srcs:
                got = _raw_forward(src, len(imgs), None, len(imgs), cfg, wd, bd if bias else None)
                bad = gk.differing(got, want)
                print('%d x %d k%d s%d c%d %s %s on=%g relu=%s bias=%s: %d of %d elements differ' % (rows, cols, kernel, stride, channels, name, entry, on, relu, bias, bad, want.size))
                total += bad
            if name == 'abc':
                assert (want[0] != want[1]).any() and (want[0] != want[2]).any()
                assert not relu or channels < 5 or ((want == 0).any() and (want > 0).any())
            elif not relu:      # the pixel at (row 0, column 0) is under window (0, 0); the arbitrary image is no other one
                assert (want[2] != want[0]).any() and (want[-1] != want[0]).any() and (want[-1] != want[1]).any()
    imgs = batches[0][1]
    index = np.array([1, -1, 0, 0, len(imgs) + 5, 2], np.int64)
    want = bc.forward(bc.pick(imgs, index), w, b, stride, 1.0, False)
    assert (want[0] != want[2]).any() and (want[2] != want[1]).any() and (want[1] == want[4]).all() and (want[1] == want[5]).all()
    cfg = bitconv.make_config(rows, cols, kernel, stride, channels, 1.0, False)
    for src in (gk.packed(imgs), gk.to_device(imgs)):
        total += gk.differing(_raw_forward(src, len(imgs), gk.to_device(index), len(index), cfg, wd, bd), want)
    assert total == 0


@pytest.mark.parametrize('rows,cols,kernel,stride,channels,n', bc.BACKWARD_SHAPES)
def test_backward_exact_on_integer_gradients(rows, cols, kernel, stride, channels, n):
    """grad_out of integers in [-4, 4] with n OH OW 4 < 2^24 (bc.exact_sums asserts it before anything runs here): every fp32
    partial sum is an integer below 2^24, exact in any order and under any tiling, so grad_bias must `==` the sum and
    grad_weight `==` fp32(sum) * fp32(on) -- every (sample, pixel, channel, tap) term present once, in its own place.  With
    on in {1, 255, 1 / 255}, with and without grad_bias, with and without an index (-1, beyond the frames, repeats), and on a
    workspace of NaN once per case."""
    from red_gym_amd import bitconv
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    frames5 = bc.many_images(rows, cols, bc.EXACT_FRAMES)
    g = bc.exact_grad_out(n, channels, oh, ow)
    gd = gk.to_device(g)
    bad = 0
    for with_index in (False, True):
        idx = bc.exact_index(n, with_index)
        picked = bc.pick(frames5, idx)
        sums = bc.exact_sums(picked, g, kernel, stride)
        assert bc.holds_something(sums)
        frames, n_frames, index = (gk.packed(frames5), bc.EXACT_FRAMES, gk.to_device(idx)) if with_index else (gk.packed(picked), n, None)
        for on in bc.EXACT_ONS:
            want_w, want_b = bc.exact_gradients(sums, on)
            cfg = bitconv.make_config(rows, cols, kernel, stride, channels, on)
            for with_bias in (True, False):
                gw, gb = _raw_backward(frames, n_frames, index, n, cfg, gd, with_bias=with_bias,
                                       ws_fill=float('nan') if on == 255.0 and with_bias else -7.0)
                dw, db = int((gw != want_w).sum()), int((gb != want_b).sum()) if with_bias else 0
                print('%d x %d k%d s%d c%d n=%d index=%s on=%g bias=%s: %d of %d weights and %d of %d biases differ' % (
                      rows, cols, kernel, stride, channels, n, with_index, on, with_bias, dw, want_w.size, db, want_b.size))
                bad += dw + db
    assert bad == 0


def test_autograd_exact_beyond_one_chunk():
    """conv_bits(...).backward() at 33 channels and kernel 7 (the wrapper sizes the workspace of three chunks): integer grad_out,
    on = 1, no relu, from uint8 images and from packed frames with an index; weight.grad and bias.grad `==` the exact sums."""
    from red_gym_amd.bitconv import conv_bits
    rows, cols, kernel, stride, channels, n = 20, 400, 7, 5, 33, 4
    assert (rows, cols, kernel, stride, channels) in [s[:5] for s in bc.BACKWARD_SHAPES]
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    frames5 = bc.many_images(rows, cols, bc.EXACT_FRAMES)
    idx = np.array([2, -1, 0, bc.EXACT_FRAMES - 1], np.int64)                  # two random frames, an empty sample, the all-set frame
    picked = bc.pick(frames5, idx)
    g = bc.exact_grad_out(n, channels, oh, ow)
    sums = bc.exact_sums(picked, g, kernel, stride)
    assert bc.holds_something(sums)
    want_w, want_b = bc.exact_gradients(sums, 1.0)
    w, b = bc.params(kernel, channels, seed=5)
    out32 = bc.forward(picked, w, b, stride, 1.0, False)
    for src, kw in ((gk.to_device(picked), {}), (gk.packed(frames5), dict(cols=cols, index=gk.to_device(idx)))):
        wd, bd = gk.to_device(w).requires_grad_(), gk.to_device(b).requires_grad_()
        out = conv_bits(src, wd, bd, stride=stride, on=1.0, relu=False, **kw)
        assert gk.differing(out, out32) == 0
        out.backward(gk.to_device(g))
        assert wd.grad.shape == wd.shape and (gk.to_host(wd.grad) == want_w).all() and (gk.to_host(bd.grad) == want_b).all()


def test_forward_in_two_launches():
    """2^23 + 3 samples of one tile each: bitconv_forward launches 2^23 workgroups and then 3 more from a.first = 2^23.  8 x 8
    images, kernel 8, stride 8, one channel; an index over five packed frames (random, all-set, empty) with -1 entries, the last
    three samples on three different frames; every output `==` the checker's for its frame."""
    import torch
    from red_gym_amd import _lib, bitconv
    n = (1 << 23) + 3
    assert bc.paths(8, 8, 8, 8, 1, n)['launches'] == 2 and bc.paths(8, 8, 8, 8, 1, n)['group'] == n - 3
    rnd = rc.random_images(8, 8, n=3, seed=23)
    imgs = np.stack([rnd[0], np.full((8, 8), 255, np.uint8), rnd[1], np.zeros((8, 8), np.uint8), rnd[2]])
    w, b = bc.params(8, 1, seed=4)
    want = bc.forward(np.concatenate([imgs, np.zeros((1, 8, 8), np.uint8)]), w, b, 8, 1.0, False)[:, 0, 0, 0]
    assert len(set(bc.bit_patterns(want[:5]).tolist())) == 5 and want[5] == want[3]
    idx = np.random.default_rng(23).integers(0, 5, n).astype(np.int64)
    idx[5::1001] = -1
    idx[-3:] = [0, 1, 2]
    assert (idx[:-3] == -1).sum() > 8000 and all((idx[:-3] == f).sum() > 1000000 for f in range(5))
    index, frames, wd, bd = gk.to_device(idx), gk.packed(imgs), gk.to_device(w), gk.to_device(b)
    out = gk.Guarded(n, fill=-7.0)
    buf = out.data
    cfg = bitconv.make_config(8, 8, 8, 8, 1, 1.0)
    _lib.check(_lib.load().f110_bitconv_forward(C.byref(cfg), frames.data_ptr(), 5, index.data_ptr(), n, wd.data_ptr(), bd.data_ptr(),
                                                out.ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    gathered = gk.to_device(want)[torch.where(index < 0, 5, index)]
    out.read()
    wrong = int((buf.view(torch.int32) != gathered.view(torch.int32)).sum())
    print('%d of %d outputs differ; the last three: %s, wanted %s' % (wrong, n, gk.to_host(buf[n - 3:n]), want[idx[-3:]]))
    assert wrong == 0 and torch.equal(buf.view(torch.int32), gathered.view(torch.int32))
    assert np.array_equal(bc.bit_patterns(gk.to_host(buf[n - 16:n])), bc.bit_patterns(want[np.where(idx[-16:] < 0, 5, idx[-16:])]))


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.BACKWARD_CASES)
def test_autograd_with_relu(rows, cols, kernel, stride, channels):
    """conv_bits(..., relu=True).backward() against torch.autograd on F.relu(F.conv2d(unpacked.double() * on, ...)) in fp64, within
    the bounds of the masked grad_out; from packed frames with an index and from uint8 images; frames receive no gradient."""
    import torch
    import torch.nn.functional as F
    from red_gym_amd.bitconv import conv_bits
    n = 3
    imgs = bc.many_images(rows, cols, n)
    w, b = bc.params(kernel, channels, seed=2)
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    g = np.random.default_rng(9).normal(size=(n, channels, oh, ow)).astype(np.float32)
    on = 255.0
    wt, bt = torch.as_tensor(w).double().requires_grad_(), torch.as_tensor(b).double().requires_grad_()
    ref = F.relu(F.conv2d(torch.as_tensor(imgs == 255).double()[:, None] * on, wt, bt, stride=stride))
    ref.backward(torch.as_tensor(g).double())
    out32 = bc.forward(imgs, w, b, stride, on, True)
    masked = g * (out32 > 0)
    # the mask is the fp32 output's: it equals the fp64 one unless an output sits within rounding of 0
    assert ((out32 > 0) == (ref.detach().numpy() > 0)).all()
    bound_w, bound_b = bc.grad_bounds(imgs, masked, kernel, stride, on)
    for src, kw in ((gk.packed(imgs), dict(cols=cols, index=gk.to_device(np.arange(n, dtype=np.int64)))), (gk.to_device(imgs), {})):
        wd, bd = gk.to_device(w).requires_grad_(), gk.to_device(b).requires_grad_()
        out = conv_bits(src, wd, bd, stride=stride, on=on, relu=True, **kw)
        assert out.requires_grad and gk.differing(out, out32) == 0
        out.backward(gk.to_device(g))
        assert src.grad is None and not src.requires_grad
        ew, eb = np.abs(gk.to_host(wd.grad) - gk.to_host(wt.grad)), np.abs(gk.to_host(bd.grad) - gk.to_host(bt.grad))
        print('%d x %d: worst error / bound: weight %.4f, bias %.4f' % (rows, cols, float((ew / bound_w).max()), float((eb / bound_b).max())))
        assert wd.grad.shape == wd.shape and (ew <= bound_w).all() and (eb <= bound_b).all()
    # weight alone: no bias, and a weight that needs no gradient gets none
    wd = gk.to_device(w).requires_grad_()
    conv_bits(gk.packed(imgs), wd, None, stride=stride, on=on, cols=cols).backward(gk.to_device(g))
    want_w = bc.gradients(imgs, g, kernel, stride, on)[0]
    assert (np.abs(gk.to_host(wd.grad) - want_w) <= bc.grad_bounds(imgs, g, kernel, stride, on)[0]).all()
    assert not conv_bits(gk.packed(imgs), gk.to_device(w), None, stride=stride, cols=cols).requires_grad


def test_module_shares_parameters_and_refuses(golden):
    import torch
    from red_gym_amd.bitconv import BitConv2d, conv_bits
    conv = torch.nn.Conv2d(1, 16, 8, 4).cuda()
    m = BitConv2d.from_conv(conv, on=1.0 / 255.0)
    assert m.weight.data_ptr() == conv.weight.data_ptr() and m.bias.data_ptr() == conv.bias.data_ptr()
    imgs = bc.images(256, 256)
    out = m(gk.to_device(imgs))
    assert gk.differing(out, bc.forward(imgs, gk.to_host(conv.weight), gk.to_host(conv.bias), 4, 1.0 / 255.0, False)) == 0
    # training the module trains the layer it shares with
    out.sum().backward()
    assert conv.weight.grad is not None and conv.bias.grad is not None and float(conv.bias.grad[0]) == 3 * 63 * 63
    # state_dict round trip with nn.Conv2d, both ways
    fresh = BitConv2d(16, 8, 4, cols=256).cuda()
    fresh.load_state_dict(conv.state_dict())
    back = torch.nn.Conv2d(1, 16, 8, 4).cuda()
    back.load_state_dict(fresh.state_dict())
    assert torch.equal(back.weight, conv.weight) and torch.equal(back.bias, conv.bias)
    assert torch.equal(fresh(gk.packed(imgs)), conv_bits(gk.packed(imgs), conv.weight, conv.bias, stride=4, cols=256))
    for bad in (torch.nn.Conv2d(3, 16, 8, 4), torch.nn.Conv2d(1, 16, 8, 4, padding=2), torch.nn.Conv2d(1, 16, 8, 4, dilation=2),
                torch.nn.Conv2d(4, 16, 8, 4, groups=4)):
        with pytest.raises(ValueError):
            BitConv2d.from_conv(bad)
    w, b, f = conv.weight.detach(), conv.bias.detach(), gk.packed(imgs)
    for args, kw in (((f, w, b), dict(stride=4)),                                            # packed frames without cols
                     ((f, w, b), dict(stride=4, cols=100)),                                  # words that do not hold cols
                     ((f.float(), w, b), dict(stride=4, cols=256)),                          # a dtype that is neither
                     ((f, w.double(), b), dict(stride=4, cols=256)),
                     ((f, w[:, 0], b), dict(stride=4, cols=256)),
                     ((f, w, b[:3]), dict(stride=4, cols=256)),
                     ((f, w, b), dict(stride=9, cols=256)),                                  # what validate refuses
                     ((f, w, b), dict(stride=4, cols=256, on=float('nan'))),
                     ((f[:, :7], w, b), dict(stride=4, cols=256)),                           # rows < kernel
                     ((f, w, b), dict(stride=4, cols=256, index=torch.zeros(3, dtype=torch.int32, device='cuda'))),
                     ((f.cpu(), w, b), dict(stride=4, cols=256))):
        with pytest.raises(ValueError):
            conv_bits(*args, **kw)


def test_closed_loop_from_bitmap_and_ring_to_features(assets):
    """6 envs with shaper, path follower and replay ring (T = 4) on, 30 steps with autoreset: every 7 steps BitConv2d on
    info['lidar_bitmap'] `==` the checker on that bitmap, and for all T * B indices frames_at + conv_bits(index = s_idx / ns_idx)
    `==` the checker on the s / ns sample_at returns, with a, r, d, ok equal to sample_at's; then the same after steps replayed
    through step_graph (locate follows the device-side counter)."""
    import torch
    from red_gym_amd import F110VecEnv, workload
    from red_gym_amd.bitconv import BitConv2d, conv_bits
    B, T, AD, rows, cols = 6, 4, 16, 75, 100
    env = F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=1, autoreset=True, timestep=0.025)
    env.shape_rewards(rows=rows, cols=cols)
    env.follow_paths()
    env.record_replay(capacity=T * B + 3, action_dim=AD)
    assert env.replay.steps == T
    torch.manual_seed(3)
    layer = BitConv2d(16, 8, 4, on=1.0, relu=True, cols=cols).cuda()
    w, b = gk.to_host(layer.weight), gk.to_host(layer.bias)
    spawn = workload.spawn_poses(B, 1)
    crash = np.arange(B) % 4 == 1
    spawn[crash, 0, 2] += np.pi / 2
    crash_dev = torch.as_tensor(crash, device=env.device)
    rng = np.random.default_rng(18)
    all_idx = torch.arange(T * B, device=env.device)
    empty = bc.forward(np.zeros((1, rows, cols), np.uint8), w, b, 4, 1.0, True)[0]
    checks = {'bitmap': 0, 'ring': 0, 'valid': 0, 'invalid': 0}

    def check_bitmap(info):
        feats = layer(info['lidar_bitmap'])
        bitmap = gk.to_host(info['lidar_bitmap'])
        assert feats.shape == (B, 16, 17, 24) and gk.differing(feats, bc.forward(bitmap, w, b, 4, 1.0, True)) == 0
        assert 2 * sum(bool((im == 255).any() and (im == 0).any()) for im in bitmap) >= B
        checks['bitmap'] += 1

    def check_ring(what):
        s, a, r, ns, d, ok = env.replay.sample_at(all_idx)
        at = env.replay.frames_at(all_idx)
        frames, s_idx, ns_idx, a2, r2, d2, ok2 = (at[k] for k in ('frames', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok'))
        assert frames.data_ptr() == env.replay.buf['frames'].data_ptr() and tuple(frames.shape) == ((T + 1) * B, rows, 2)
        for x, y in ((a, a2), (r, r2), (d, d2), (ok, ok2)):
            assert x.dtype == y.dtype and torch.equal(x, y), what
        fs = conv_bits(frames, layer.weight, layer.bias, stride=4, relu=True, index=s_idx, cols=cols)
        fns = layer(frames, index=ns_idx)
        s, ns, okn = gk.to_host(s), gk.to_host(ns), gk.to_host(ok)
        bad = gk.differing(fs, bc.forward(s, w, b, 4, 1.0, True)) + gk.differing(fns, bc.forward(ns, w, b, 4, 1.0, True))
        held = np.flatnonzero(okn)
        both = sum(bool((s[i] == 0).any() and (s[i] == 255).any()) for i in held)
        print('%s: %d differing feature elements, %d valid, s holds 0 and 255 in %d' % (what, bad, held.size, both))
        assert bad == 0 and held.size > 0 and 2 * both >= held.size
        assert ((gk.to_host(s_idx) >= 0) == (okn == 1)).all() and ((gk.to_host(ns_idx) >= 0) == (okn == 1)).all()
        for i in np.flatnonzero(okn == 0):
            assert gk.differing(fs[i], empty) == 0 and gk.differing(fns[i], empty) == 0
        checks['ring'] += 1
        checks['valid'] += held.size
        checks['invalid'] += int((okn == 0).sum())

    def actions():
        raw = rng.uniform(-1.0, 1.0, (B, AD))
        acts = env.path_actions(torch.as_tensor(raw, device=env.device))
        acts[:, 0, 0] = torch.where(crash_dev, 0.0, acts[:, 0, 0])
        acts[:, 0, 1] = torch.where(crash_dev, 8.0, acts[:, 0, 1])
        return acts

    env.reset(spawn)
    for k in range(30):
        _, _, _, info = env.step(actions())
        if k % 7 == 6 or k == 29:
            check_bitmap(info)
            check_ring('after step %d' % k)
    env.capture_step()
    for k in range(2):
        _, _, _, info = env.step_graph(actions())
    check_bitmap(info)
    check_ring('after step_graph')
    # the same draws as sample(): sample_frames moves the one draw counter
    first = env.replay._draws
    batch = env.replay.sample_frames(64, seed=5)
    frames, s_idx, ns_idx, a, r, d, ok = (batch[k] for k in ('frames', 's_idx', 'ns_idx', 'a', 'r', 'd', 'ok'))
    drawn = gk.to_host(env.replay._keep)
    want_idx, want_ok, _ = rc.draw(gk.to_host(env.replay.buf['valid']), int(env.replay.buf['count']), 5, first, 64)
    assert np.array_equal(drawn, want_idx) and np.array_equal(gk.to_host(ok), want_ok) and env.replay._draws == first + 64
    s2 = env.replay.sample_at(torch.as_tensor(drawn, device=env.device))
    assert torch.equal(a, s2[1]) and torch.equal(r, s2[2]) and torch.equal(d, s2[4]) and torch.equal(ok, s2[5])
    assert gk.differing(layer(frames, index=s_idx), bc.forward(gk.to_host(s2[0]), w, b, 4, 1.0, True)) == 0
    print(checks)
    assert checks['bitmap'] >= 5 and checks['ring'] >= 5 and checks['valid'] > 0
    assert env.eng.device_errors() == 0
    env.close()
