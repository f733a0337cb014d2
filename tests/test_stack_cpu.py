"""The frame stacks' checker (tests/stack_cases.py) without a GPU: the census of the base ring -- every way a stack ends, both seams --
counted from the checker alone before anything is compared with it; the contract `==` the brute-force statement over per-env runs on
every scripted ring; the shift between the stacks of a transition's two frames; the stacked convolution's checker against
bitconv_cases.forward and against torch's fp64 convolution; and the ABI's refusals, which need no device (tests/test_gpu_stack.py and
tests/test_gpu_bitconv_stack.py run the kernels against the same checker)."""
import ctypes as C

import numpy as np
import pytest

import bitconv_cases as bc
import nstep_cases as nc
import stack_cases as sc


def test_census_of_the_base_ring():
    """From stack() alone, at stack = 4: at least three stacks for each way one ends; among those that ask across the step-slot seam (slot
    0, then T - 1) and among those that hold frames across the frame-slot seam (slot 0, then T) a full one and a cut one."""
    valid, _, _, count = sc.base_ring()
    T, B = valid.shape
    assert (T, B, count) == (9, 8, 22) and count > 2 * T
    got = sc.census(4)
    print({k: (v if isinstance(v, int) else sorted(set(v))) for k, v in got.items()})
    assert all(got[e] >= 3 for e in sc.ENDS), got
    assert sum(got[e] for e in sc.ENDS) == (T + 1) * B
    for seam in ('step_seam', 'frame_seam'):
        assert 'full' in got[seam] and set(got[seam]) - {'full'}, (seam, got[seam])
    assert sorted(got['step_seam']) != sorted(got['frame_seam'])          # the two seams lie apart: the moduli differ
    s = sc.stack(valid, count, np.arange((T + 1) * B), 4)
    assert set(s['depth'].tolist()) == {1, 2, 3, 4}


@pytest.mark.parametrize('name', sorted(sc.rings()))
def test_stack_equals_brute_force_on_scripted_rings(name):
    valid, dones, rewards, count = sc.rings()[name]
    T, B = valid.shape
    rows = sc.all_rows(T, B)
    assert rows[0] == -1 and rows[-1] == (T + 1) * B
    pushes = nc.pushes_of_arrays(valid, dones, rewards, count)
    for k in sc.STACKS:
        s = sc.stack(valid, count, rows, k)
        b_rows, b_depth = sc.brute(pushes, T, B, count, rows, k)
        assert np.array_equal(s['rows'], b_rows) and np.array_equal(s['depth'], b_depth), (name, k)
        assert s['rows'].dtype == np.int64 and s['depth'].dtype == np.int32
        # column 0 is the row itself; a refused row is -1 everywhere with depth 0; k = 1 copies
        live = s['depth'] > 0
        assert s['depth'][0] == 0 and s['depth'][-1] == 0 and live.any() and (s['depth'] <= k).all()
        assert np.array_equal(s['rows'][live, 0], rows[live]) and (s['rows'][~live] == -1).all()
        assert live.sum() == min(count, T + 1) * B
        for i in np.flatnonzero(live):
            d = int(s['depth'][i])
            assert len(set(s['rows'][i, :d].tolist())) == d and (s['rows'][i, d:] == s['rows'][i, d - 1]).all()
            assert (s['rows'][i] % B == rows[i] % B).all()                                  # one env
    # the latest mode is the stack of the newest frame's row
    for k in (1, 4):
        latest = sc.stack(valid, count, None, k)
        newest = ((count - 1) % (T + 1)) * B + np.arange(B)
        named = sc.stack(valid, count, newest, k)
        assert np.array_equal(latest['rows'], named['rows']) and np.array_equal(latest['depth'], named['depth'])
    empty = sc.stack(np.zeros_like(valid), 0, None, 3)
    assert (empty['rows'] == -1).all() and not empty['depth'].any()


@pytest.mark.parametrize('name', sorted(sc.rings()))
def test_the_stack_of_the_frame_after_is_the_stack_of_the_frame_before_shifted(name):
    """For every transition the locate accepts: stack(ns_frame)[1:] == stack(s_frame)[:-1] wherever depth(s_frame) = stack, and
    depth(ns_frame) = min(depth(s_frame) + 1, stack) everywhere."""
    valid, dones, rewards, count = sc.rings()[name]
    T, B = valid.shape
    one = nc.one_step(valid, dones, rewards, count, nc.all_indices(T, B))
    ok = one['ok'] == 1
    assert ok.any()
    seen = 0
    for k in (2, 3, 4, 8):
        s, ns = sc.stack(valid, count, one['s_frame'][ok], k), sc.stack(valid, count, one['ns_frame'][ok], k)
        assert (s['depth'] >= 1).all() and np.array_equal(ns['depth'], np.minimum(s['depth'] + 1, k))
        full = s['depth'] == k
        seen += int(full.sum())
        assert np.array_equal(ns['rows'][full, 1:], s['rows'][full, :-1])
        assert np.array_equal(ns['rows'][:, 1], s['rows'][:, 0])
    assert seen > 0 or name == 'nstep_not_wrapped'


def test_forward_stack_of_one_frame_is_the_one_frame_checker():
    for rows, cols, kernel, stride, channels in bc.SHAPES[:3] + bc.SHAPES[-2:]:
        imgs = bc.images(rows, cols)
        w, b = bc.params(kernel, channels)
        index = np.array([[2], [0], [-1], [1], [7]], np.int64)
        for on in bc.ONS:
            for relu in (False, True):
                got = sc.forward_stack(imgs, index, w, b, stride, on, relu)
                want = bc.forward(bc.pick(imgs, index[:, 0]), w, b, stride, on, relu)
                assert got.dtype == np.float32 and np.array_equal(bc.bit_patterns(got), bc.bit_patterns(want))


def test_forward_stack_against_the_framework_in_fp64():
    """stack = 3 within gamma_m (|on| sum |w| + |b|) of F.conv2d in fp64 on the unpacked stack, m = k kernel^2 + 2: the one-frame bound
    with the longer chain."""
    import torch
    k = 3
    for rows, cols, kernel, stride, channels in bc.SHAPES[:4] + bc.SHAPES[-2:]:
        imgs = bc.images(rows, cols)
        w, b = sc.params_stack(kernel, channels, k)
        index = sc.stack_index(4, k, imgs.shape[0])
        x = torch.as_tensor((sc.unpacked_stack(imgs, index) == 255).astype(np.float64))
        for on in bc.ONS:
            on32 = float(np.float32(on))
            want = torch.nn.functional.conv2d(x * on32, torch.as_tensor(w.astype(np.float64)), torch.as_tensor(b.astype(np.float64)), stride=stride).numpy()
            got = sc.forward_stack(imgs, index, w, b, stride, on, False)
            bound = bc.gamma(k * kernel * kernel + 2) * (abs(on32) * np.abs(w.astype(np.float64)).sum(axis=(1, 2, 3)) + np.abs(b.astype(np.float64)))
            err = np.abs(got.astype(np.float64) - want).max(axis=(0, 2, 3))
            print((rows, cols, kernel, stride, channels), on, float((err / bound).max()))
            assert got.shape == want.shape and (err <= bound).all()
            relu = sc.forward_stack(imgs, index, w, b, stride, on, True)
            assert np.array_equal(relu, np.maximum(got, np.float32(0.0)))
    # the order of the frames matters to the bits: it is part of the contract
    imgs = bc.images(33, 520)
    w, b = sc.params_stack(8, 17, k)
    index = sc.stack_index(4, k, 3)
    swapped = sc.forward_stack(imgs, index[:, ::-1], w[:, ::-1], b, 8, 1.0, False)
    straight = sc.forward_stack(imgs, index, w, b, 8, 1.0, False)
    assert np.allclose(swapped, straight, rtol=1e-4, atol=1e-3) and not np.array_equal(swapped, straight)


def test_mirror_and_constants():
    from red_gym_amd import _lib, bitconv, replay, sac
    assert _lib.F110_REPLAY_MAX_STACK == sc.MAX_STACK == replay.MAX_STACK == sac.MAX_STACK == max(sc.STACKS)
    assert _lib.F110_BITCONV_MAX_STACK == bitconv.MAX_STACK == _lib.F110_REPLAY_MAX_STACK
    for name in ('f110_replay_stack', 'f110_bitconv_forward_stack', 'f110_bitconv_workspace_stack', 'f110_bitconv_backward_stack'):
        assert name in _lib.SYMBOLS
    assert _lib.RESTYPES['f110_bitconv_workspace_stack'] is C.c_int64


def test_refusals_need_no_device():
    """What is refused on the arguments alone comes back as F110_E_INVALID without a launch."""
    import torch
    from red_gym_amd import _lib, bitconv, build, replay
    build.build()
    lib = _lib.load()
    one = 4096                                   # never dereferenced
    assert lib.f110_replay_stack(None, one, 4, 3, one, one, None) == _lib.E_INVALID and b'null handle' in lib.f110_last_error()
    cfg = bitconv.make_config(24, 260, 8, 4, 16)
    fwd = lambda stack, index=one, n=4, c=cfg: lib.f110_bitconv_forward_stack(C.byref(c), one, 5, index, stack, n, one, one, one, None)  # noqa: E731
    bwd = lambda stack, index=one, n=4, ws=one, c=cfg: lib.f110_bitconv_backward_stack(C.byref(c), one, 5, index, stack, n, one, one, one, ws, None)  # noqa: E731
    for stack in (0, -1, 9, 2 ** 31 - 1):
        assert fwd(stack) == _lib.E_INVALID and b'stack' in lib.f110_last_error()
        assert bwd(stack) == _lib.E_INVALID and b'stack' in lib.f110_last_error()
        assert lib.f110_bitconv_workspace_stack(C.byref(cfg), stack, 4) == 0
    assert fwd(3, index=None) == _lib.E_INVALID and b'index' in lib.f110_last_error()
    assert bwd(3, index=None) == _lib.E_INVALID and b'index' in lib.f110_last_error()
    assert fwd(3, n=-1) == _lib.E_INVALID and bwd(3, n=0) == _lib.E_INVALID and bwd(3, ws=None) == _lib.E_INVALID and bwd(3, ws=4104) == _lib.E_INVALID
    assert fwd(3, n=0) == 0                                      # nothing to do is no error, and no launch
    bad = bitconv.make_config(24, 260, 9, 4, 16)
    assert fwd(3, c=bad) == _lib.E_INVALID and bwd(3, c=bad) == _lib.E_INVALID and lib.f110_bitconv_workspace_stack(C.byref(bad), 3, 4) == 0
    # the workspace: the one-frame partial sums rounded up to 16 bytes, then the index transposed
    for n in (1, 3, 67):
        for stack in (1, 3, 8):
            part = lib.f110_bitconv_workspace(C.byref(cfg), n)
            assert part > 0 and lib.f110_bitconv_workspace_stack(C.byref(cfg), stack, n) == (part + 15) // 16 * 16 + 8 * stack * n
    assert lib.f110_bitconv_workspace_stack(C.byref(cfg), 3, 0) == 0
    # the host side
    for bad_stack in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError):
            replay.ReplayBuffer._stack(bad_stack)
        with pytest.raises(ValueError):
            bitconv.BitConv2d(16, 8, 4, in_channels=bad_stack)
    assert replay.ReplayBuffer._stack(8) == 8
    conv = bitconv.BitConv2d(16, 8, 4, in_channels=3)
    assert tuple(conv.weight.shape) == (16, 3, 8, 8)
    shared = bitconv.BitConv2d.from_conv(torch.nn.Conv2d(3, 16, 8, 4), in_channels=3)
    assert tuple(shared.weight.shape) == (16, 3, 8, 8)
    for conv, k in ((torch.nn.Conv2d(9, 16, 8, 4), 9), (torch.nn.Conv2d(3, 16, 8, 4), 1), (torch.nn.Conv2d(3, 16, 8, 4), 2), (torch.nn.Conv2d(1, 16, 8, 4), 3)):
        with pytest.raises(ValueError):
            bitconv.BitConv2d.from_conv(conv, in_channels=k)
