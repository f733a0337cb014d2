"""Bit convolution without a GPU: the checker of tests/bitconv_cases.py against the reference's own operator (torch's conv2d in
fp64 on the unpacked image), and the library's host-only validate entry."""
import ctypes as C

import numpy as np
import pytest

import bitconv_cases as bc
import replay_cases as rc
from test_launch_plans_cpu import constant, lib as launch_plans  # noqa: F401 (the fixture: the plan headers compiled for the host)


@pytest.mark.parametrize('rows,cols,kernel,stride,channels', bc.CASES + bc.SHAPES)
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


def test_shape_tables_reach_every_path(launch_plans):
    """tests/bitconv_cases.py: paths() restates the header's arithmetic, and the tables the GPU tests run reach every kernel
    size, both branches of the mask, the largest LDS footprint, full and partial tiles, the tail word, every count of channel
    chunks and every kind of walk over the tiles.  Removing a row that is the only one to reach a path fails here."""
    from red_gym_amd import _lib, bitconv
    # the constants as the compiler sees them in csrc/f110_bitconv_plan.h (the shim of test_launch_plans_cpu.py)
    assert [constant(launch_plans, n) for n in ('BC_TX', 'BC_TY', 'BC_MAX_K', 'BC_LROWS', 'BC_LWORDS', 'BC_CHUNK', 'BC_MAX_PARTIALS')] == \
        [bc.BC_TX, bc.BC_TY, bc.BC_MAX_K, bc.BC_LROWS, bc.BC_LWORDS, bc.BC_CHUNK, bc.BC_MAX_PARTIALS]
    assert constant(launch_plans, 'BC_FORWARD_GROUP') == bc.FORWARD_GROUP == 1 << 23
    # the validated range by brute force: every kernel, every stride, every count of outputs of a row of up to three tiles
    widest = offs = 0
    for kernel in range(1, bc.BC_MAX_K + 1):
        for stride in range(1, kernel + 1):
            for ow in range(1, 3 * bc.BC_TX + 1):
                p = bc.paths(kernel, kernel + (ow - 1) * stride, kernel, stride, 1, 1)
                assert p['ow'] == ow and p['last_word'] < p['words'] and p['nrows'] == kernel
                widest, offs = max(widest, p['nwords']), max(offs, p['off'])
    print('widest tile: %d words of BC_LWORDS = %d; largest off: %d' % (widest, bc.BC_LWORDS, offs))
    assert widest <= bc.BC_LWORDS
    # forward, packed and uint8 entry alike (both run the whole of SHAPES and CASES; the uint8 one adds the row's end)
    fwd = [(s, bc.paths(*s, 3)) for s in bc.SHAPES + bc.CASES]
    for s, p in fwd:
        bitconv.validate(*s)
        assert p['last_word'] < p['words'] and p['nrows'] <= bc.BC_LROWS and p['nwords'] <= bc.BC_LWORDS and p['launches'] == 1, s
    assert {s[2] for s, p in fwd} == set(range(1, 9))
    assert {s[2] for s, p in fwd if p['straddles']} == set(range(2, 9))
    assert any(s[2] == s[3] and s[2] > 1 and not p['straddles'] and p['tiles_x'] > 1 for s, p in fwd)
    assert {p['straddles'] for s, p in fwd if s[2] == 2} == {False, True}              # the narrowest window that can: both branches
    assert max(p['nrows'] for s, p in fwd) == bc.BC_LROWS
    assert max(p['nwords'] for s, p in fwd) == widest
    assert any(p['tiles_x'] >= 3 for s, p in fwd) and any(p['tiles_y'] >= 3 for s, p in fwd)
    for key in ('partial_x', 'partial_y'):
        assert {p[key] for s, p in fwd if p['tiles_x'] * p['tiles_y'] > 1} == {False, True}, key
    assert {64, 65} <= {p['ow'] for s, p in fwd}
    assert any(p['tail_word'] and p['wbase'] == p['words'] - 1 for s, p in fwd)        # a tile that stages the tail word alone
    assert {False, True} == {p['u8_bytes'] for s, p in fwd}
    assert {1, 64} <= {s[4] for s, p in fwd if p['tiles_x'] * p['tiles_y'] > 1}
    assert any(p['chunks'] > 1 and p['tiles_x'] * p['tiles_y'] > 1 for s, p in fwd)
    # backward: tile, staging and mask are the forward pass's, so it runs only where the forward `==` has pinned them
    bwd = [(s, bc.paths(*s)) for s in bc.BACKWARD_SHAPES]
    assert {s[:5] for s in bc.BACKWARD_SHAPES} <= set(bc.SHAPES)
    assert {s[2] for s, p in bwd} == set(range(1, 9))
    assert {s[2] for s, p in bwd if p['straddles']} == set(range(2, 9))
    assert max(p['nrows'] for s, p in bwd) == bc.BC_LROWS and max(p['nwords'] for s, p in bwd) == widest
    assert any(p['tail_word'] and p['wbase'] == p['words'] - 1 for s, p in bwd) and any(p['tiles_x'] >= 3 for s, p in bwd)
    assert {p['chunks'] for s, p in bwd} == {1, 2, 3, 4}
    assert {0, 1, 15} <= {p['rem'] for s, p in bwd}
    assert any(p['rem'] and p['chunks'] > 1 for s, p in bwd)
    assert any(p['passes'] == 1 and p['G'] < bc.BC_MAX_PARTIALS for s, p in bwd)
    assert any(p['passes'] == 2 and p['uneven'] for s, p in bwd) and any(p['passes'] >= 3 for s, p in bwd)
    assert sum(p['G'] == bc.BC_MAX_PARTIALS for s, p in bwd) >= 2
    assert any(p['passes'] >= 2 and p['chunks'] > 1 for s, p in bwd)
    assert {1, 3} <= {s[5] for s, p in bwd}
    lib = _lib.load()
    for s, p in bwd:
        rows, cols, kernel, stride, channels, n = s
        cfg = bitconv.validate(rows, cols, kernel, stride, channels)
        assert lib.f110_bitconv_workspace(C.byref(cfg), n) == p['G'] * channels * (kernel * kernel + 1) * 4, s
        # the precondition of the exact backward test, on the inputs it uses: integers of [-4, 4] and n OH OW 4 < 2^24
        g = bc.exact_grad_out(n, channels, p['oh'], p['ow'])
        assert g.dtype == np.float32 and (g == np.rint(g)).all() and g.min() == -4 and g.max() == 4
        assert n * p['oh'] * p['ow'] * 4 < 2 ** 24, s
        for with_index in (False, True):
            idx = bc.exact_index(n, with_index)
            assert idx.shape == (n,) and idx.max() >= 0 and (not with_index or n < 2 or (idx == -1).any())
            assert 0 <= idx[-1] < bc.EXACT_FRAMES                              # the last tile of the walk reads a frame
            # and its sums are worth comparing: nonzero, different from channel to channel and from chunk to chunk
            picked = bc.pick(bc.many_images(rows, cols, bc.EXACT_FRAMES), idx)
            sums = bc.exact_sums(picked, g, kernel, stride)
            assert bc.holds_something(sums) and max(np.abs(sums[0]).max(), np.abs(sums[1]).max()) < 2 ** 24
            if p['passes'] >= 2:
                # the last tile of the walk (sample n - 1, last tile row and column) counts: its frame is all set and its
                # grad_out does not sum to zero, so a walk that stops one tile short changes grad_weight and grad_bias
                last = g[-1, :, (p['tiles_y'] - 1) * bc.BC_TY:, (p['tiles_x'] - 1) * bc.BC_TX:]
                assert (picked[-1] == 255).all() and (last.sum(axis=(1, 2)) != 0).any(), s
    # the split launch of the forward pass is reached by test_forward_in_two_launches alone
    p = bc.paths(8, 8, 8, 8, 1, (1 << 23) + 3)
    assert p['group'] == 1 << 23 and p['launches'] == 2 and bc.paths(8, 8, 8, 8, 1, 1 << 23)['launches'] == 1


def test_exact_sums_against_the_fp64_gradients():
    """bc.exact_sums / exact_gradients (integer grad_out) agree with bc.gradients in fp64 where both apply, and refuse a
    grad_out that is no integer or too large for exact fp32 sums."""
    rows, cols, kernel, stride, channels, n = 7, 70, 3, 3, 20, 4
    oh, ow = bc.out_size(rows, cols, kernel, stride)
    imgs = bc.pick(bc.many_images(rows, cols, bc.EXACT_FRAMES), bc.exact_index(n, True))
    g = bc.exact_grad_out(n, channels, oh, ow)
    sums = bc.exact_sums(imgs, g, kernel, stride)
    for on in bc.EXACT_ONS:
        gw, gb = bc.exact_gradients(sums, on)
        want_w, want_b, _, _ = bc.gradients(imgs, g, kernel, stride, on)
        assert (gb == want_b).all() and (np.abs(gw - want_w) <= bc.U * np.abs(want_w)).all() and np.abs(gw).max() > 0
    assert (bc.exact_gradients(sums, 1.0)[0] == sums[0]).all()
    with pytest.raises(AssertionError):
        bc.exact_sums(imgs, g + np.float32(0.5), kernel, stride)
    with pytest.raises(AssertionError):
        bc.exact_sums(imgs, g * np.float32(2.0 ** 20), kernel, stride)


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
