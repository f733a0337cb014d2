"""No-GPU checks of the policy head (csrc/f110_policyhead.h): what f110_policyhead_validate accepts, the workspace against the
checker's tiling, the shape tables against paths(), the checker's analytic gradients against torch autograd in fp64, the size of
its tail bounds, and the checker pinned on the recording of the reference's own Actor (tests/golden/g20_head.npz)."""
import ctypes as C

import numpy as np
import pytest

import policyhead_cases as ph

from red_gym_amd import _lib, build


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _lib.load()


def test_validate_accepts_and_refuses_at_the_limits(lib):
    from red_gym_amd import policyhead
    for K in (0, 1, 4096, 4097):
        for A in (0, 1, 32, 33):
            ok = 1 <= K <= ph.MAX_K and 1 <= A <= ph.MAX_A
            cfg = policyhead.make_config(K, A)
            rc = lib.f110_policyhead_validate(C.byref(cfg))
            assert rc == (0 if ok else _lib.E_INVALID), (K, A)
            if not ok:
                msg = lib.f110_last_error().decode()
                assert ('in_features' if not 1 <= K <= ph.MAX_K else 'action_dim') in msg
                with pytest.raises(ValueError):
                    policyhead.validate(K, A)
    assert lib.f110_policyhead_validate(None) == _lib.E_INVALID and b'null' in lib.f110_last_error()
    assert (policyhead.MAX_IN_FEATURES, policyhead.MAX_ACTION_DIM) == (ph.MAX_K, ph.MAX_A)
    assert _lib.F110_POLICYHEAD_SLICE_ROWS == ph.R


def test_null_pointers_are_refused_before_any_launch(lib):
    """F110_E_INVALID on the host: no device is touched (this runs without one)."""
    from red_gym_amd import policyhead
    cfg = policyhead.make_config(512, 16)
    one = 16                                                     # (any non-null address: the checks come before the launch)
    args = [one] * 9
    for hole in (0, 1, 3, 6, 7):                                 # h, w_mean, w_log_std, pre, action
        a = list(args)
        a[hole] = None
        assert lib.f110_policyhead_forward(C.byref(cfg), a[0], 4, *a[1:], None) == _lib.E_INVALID
    # log_prob without eps and eps without log_prob
    assert lib.f110_policyhead_forward(C.byref(cfg), one, 4, one, None, one, None, None, one, one, one, None) == _lib.E_INVALID
    assert lib.f110_policyhead_forward(C.byref(cfg), one, 4, one, None, one, None, one, one, one, None, None) == _lib.E_INVALID
    assert lib.f110_policyhead_forward(C.byref(cfg), one, -1, one, None, one, None, one, one, one, one, None) == _lib.E_INVALID
    assert lib.f110_policyhead_forward(C.byref(cfg), None, 0, None, None, None, None, None, None, None, None, None) == 0
    assert lib.f110_policyhead_backward(C.byref(cfg), one, 4, one, one, one, one, None, None, None, None, None, None, None, None, one, None) == _lib.E_INVALID
    assert lib.f110_policyhead_backward(C.byref(cfg), one, 4, one, one, one, None, one, one, None, None, None, None, None, None, one, None) == _lib.E_INVALID
    assert lib.f110_policyhead_backward(C.byref(cfg), one, 4, one, one, one, one, one, None, None, None, None, None, None, None, 8, None) == _lib.E_INVALID


def test_memory_of_no_device_is_refused_before_any_launch(lib):
    """Every required pointer set but none of them device memory: the call is refused on the host -- F110_E_INVALID where a device
    can say that the address is not its memory, the runtime's error where there is no device at all -- and nothing is launched (a
    launch on these addresses would fault)."""
    from red_gym_amd import policyhead
    cfg = policyhead.make_config(512, 16)
    buf = np.zeros(4 * 512, np.float32)
    p = buf.ctypes.data
    rc = lib.f110_policyhead_forward(C.byref(cfg), p, 4, p, None, p, None, None, p, p, None, None)
    assert rc in (_lib.E_INVALID, _lib.E_HIP), rc
    if rc == _lib.E_INVALID:
        assert b'not device memory' in lib.f110_last_error()
    rc = lib.f110_policyhead_backward(C.byref(cfg), p, 4, p, p, p, None, p, None, None, None, None, None, None, None, p - p % 16 + 16, None)
    assert rc in (_lib.E_INVALID, _lib.E_HIP), rc


def test_workspace_is_what_the_tiling_needs(lib):
    from red_gym_amd import policyhead
    for n, K, A in ph.BACKWARD_SHAPES + ph.FORWARD_SHAPES + [(65536, 512, 16)]:
        got = policyhead.workspace_bytes(K, A, n)
        assert got == ph.workspace_bytes(n, K, A) and got % 4 == 0, (n, K, A)
        assert got >= 4 * (n * 2 * A + ph.paths(n, K, A)['slices'] * 2 * A * (K + 1))
    assert policyhead.workspace_bytes(512, 16, 0) == 0 and policyhead.workspace_bytes(0, 16, 4) == 0 and policyhead.workspace_bytes(512, 33, 4) == 0


def test_shape_tables_reach_every_path():
    """The GPU shape tables against paths(): every branch the kernels take on a shape is taken by some shape of the tables."""
    P = [ph.paths(*s) for s in ph.FORWARD_SHAPES]
    by = dict(zip(ph.FORWARD_SHAPES, P))
    assert all(p['lds'] <= ph.PH_LDS_BYTES and p['kc'] % 64 == 0 for p in P)
    assert {p['T'] for p in P} == {1, 2}
    assert any(p['lds'] == ph.PH_LDS_BYTES for p in P)                                   # the whole LDS
    assert any(p['chunks'] == 1 and p['pad_cols'] == 0 for p in P) and any(p['chunks'] == 1 and p['pad_cols'] > 0 for p in P)
    for T in (1, 2):                                                                     # chunked K in both layouts, with a short last chunk
        assert any(p['T'] == T and p['restage'] and p['last_chunk'] < 16 for p in P)
        assert any(p['T'] == T and not p['restage'] for p in P)
    assert any(p['restage'] and p['pad_cols'] == 0 for p in P)                           # (4096: the last chunk is full)
    assert any(p['vec_stage'] and not p['scalar_stage'] for p in P) and any(p['scalar_stage'] and not p['vec_stage'] for p in P)
    assert any(p['vec_stage'] and p['scalar_stage'] for p in P)
    assert any(p['idle_lanes'] == 0 for p in P) and any(p['idle_lanes'] == 15 for p in P) and any(p['idle_lanes'] == 1 for p in P)
    assert by[(65, 515, 17)]['idle_lanes'] == 15 and by[(65, 515, 17)]['T'] == 2 and by[(65, 515, 17)]['chunks'] == 3
    assert by[(3, 4096, 32)]['live_rows'] == 64 and by[(3, 4096, 32)]['chunks'] == 16
    assert by[(64, 512, 16)] == dict(by[(64, 512, 16)], tiles=1, idle_waves=0, partial_wave=False, chunks=1, kc=512, lds=65536)
    assert any(p['walks'] > 1 for p in P) and by[(32835, 8, 2)]['tiles'] == ph.PH_MAX_GRID + 2 and by[(32835, 8, 2)]['last_tile_rows'] == 3
    assert {p['idle_waves'] for p in P} >= {0, 2, 3} and any(p['partial_wave'] for p in P) and any(not p['partial_wave'] for p in P)
    assert any(p['tiles'] > 1 and p['last_tile_rows'] == 1 for p in P)
    B = [ph.paths(*s) for s in ph.BACKWARD_SHAPES]
    assert [s[0] for s in ph.BACKWARD_SHAPES] == [1, ph.R - 1, ph.R, ph.R + 1, 2 * ph.R + 3]
    assert [p['slices'] for p in B] == [1, 1, 1, 2, 3] and [p['last_slice_rows'] for p in B] == [1, ph.R - 1, ph.R, 1, 3]
    assert any(p['gh_kblocks'] == 2 and p['gh_partial_k'] for p in B) and any(p['gh_kblocks'] == 2 and not p['gh_partial_k'] for p in B)
    assert any(p['gw_kblocks'] > 1 and p['gw_partial_k'] for p in B) and any(not p['gw_partial_k'] for p in B)
    assert {p['chains'] for p in B} >= {2, 64} and any(p['gh_last_rows'] < ph.PH_GH_ROWS for p in B) and any(p['gh_last_rows'] == ph.PH_GH_ROWS for p in B)
    assert {p['T'] for p in B} == {1, 2}


def test_fma_chain_is_not_a_plain_sum():
    """The pre-activations of the checker are the fp32 chain: they differ from a float64 dot product rounded once somewhere, and
    stay within gamma_K of it everywhere; a bias of None is + 0.0f."""
    h, wm, bm, wl, bl, _ = ph.inputs(33, 515, 17, special=False)
    pre = ph.pre_activations(h, wm, bm, wl, bl)
    w = np.concatenate([wm, wl]).astype(np.float64)
    exact = h.astype(np.float64) @ w.T + np.concatenate([bm, bl]).astype(np.float64)
    assert pre.dtype == np.float32 and pre.shape == (33, 34)
    assert (pre != exact.astype(np.float32)).any()
    mag = np.abs(h.astype(np.float64)) @ np.abs(w).T + np.abs(np.concatenate([bm, bl]).astype(np.float64))
    assert (np.abs(pre - exact) <= ph.bc.gamma(517) * mag).all()
    nob = ph.pre_activations(h, wm, None, wl, None)
    assert np.array_equal(nob[:, 3] + bm[3], pre[:, 3]) and not np.signbit(nob).all()


def _torch_reference(pre, eps, g_y, g_lp):
    """torch autograd in fp64 on the CPU of the contract's formula with pre as the leaf."""
    import torch
    A = pre.shape[1] // 2
    p = torch.tensor(pre.astype(np.float64), requires_grad=True)
    mean, ls = p[:, :A], torch.clamp(p[:, A:], -20, 2)
    if eps is None:
        y = torch.tanh(mean)
        y.backward(torch.tensor(g_y))
        return y.detach().numpy(), None, p.grad.numpy()
    e = torch.tensor(eps.astype(np.float64))
    y = torch.tanh(mean + ls.exp() * e)
    lp = (-(e * e) / 2 - ls - ph.HALF_LOG_2PI - torch.log(1.0 - y * y + 1e-6)).sum(1)
    (y * torch.tensor(g_y)).sum().add((lp * torch.tensor(g_lp)).sum()).backward()
    return y.detach().numpy(), lp.detach().numpy(), p.grad.numpy()


def test_checker_gradients_agree_with_autograd():
    """The tail and g_pre of the checker against torch autograd in fp64, rows at exactly -20.0 and 2.0 and beyond them included
    (zero weights, bias only: inputs(special=True) has such a row, and here every row is one): within the checker's own bound, and
    the clamp's gradient mask is inclusive."""
    rng = np.random.default_rng(3)
    for n, K, A in ((9, 5, 15), (6, 3, 1), (12, 7, 32)):
        h, wm, bm, wl, bl, eps = ph.inputs(n, K, A)
        pre = ph.pre_activations(h, wm, bm, wl, bl)
        zero = ph.pre_activations(h, 0 * wm, bm, 0 * wl, bl)                 # bias only: exactly at and beyond the clamps
        assert np.array_equal(zero[0, A:], bl) and np.array_equal(pre[n // 2], zero[0])
        pre = np.concatenate([pre, zero[:2]])
        eps = np.concatenate([eps, eps[:2]])
        g_y, g_lp = rng.normal(size=(n + 2, A)), rng.normal(size=n + 2)
        if A >= 4:
            assert {-20.0, 2.0, -25.0, 3.0} <= set(pre[-1, A:].tolist())
        for e, glp in ((eps, g_lp), (None, None)):
            y, lp, grad = _torch_reference(pre, e, g_y, glp)
            t = ph.tail(pre, e)
            act_b, lp_b = ph.tail_bounds(pre, e)
            assert (np.abs(t['y'] - y) <= act_b).all()
            g, bound = ph.g_pre(pre, e, g_y, glp)
            if e is not None:
                assert (np.abs(t['log_prob'] - lp) <= lp_b).all()
                at = (pre[:, A:] == -20.0) | (pre[:, A:] == 2.0)
                beyond = (pre[:, A:] < -20.0) | (pre[:, A:] > 2.0)
                assert at.any() and beyond.any() and (g[:, A:][beyond] == 0).all() and (g[:, A:][at] != 0).all()
                assert (grad[:, A:][beyond] == 0).all() and (grad[:, A:][at] != 0).all()
            else:
                assert (g[:, A:] == 0).all() and (grad[:, A:] == 0).all()
            # torch's own error: its tanh backward forms 1 - y y with one rounding where the forward's log argument has two, and
            # the chain rule multiplies that difference (at most u64 y^2) by g_y + g_lp 2 y / (om + 1e-6), up to 2e6 |g_lp|
            ref = ph.U64 * np.abs(g_y + (0.0 if glp is None else glp[:, None]) * 2.0 * t['y'] / (t['om'] + 1e-6))
            ref = np.concatenate([ref, ref * np.abs(t['std'] * t['eps']) if e is not None else 0.0 * ref], axis=1)
            err, own = np.abs(g - grad), bound - ph.U32 * np.abs(g)          # (without the fp32 rounding: both sides are fp64 here)
            print('n=%d K=%d A=%d %s: worst g_pre error / bound %.3g' % (n, K, A, 'sampling' if e is not None else 'evaluate',
                                                                          float((err / np.maximum(own + ref, 1e-300)).max())))
            assert (err <= own + ref).all()


def test_tail_bounds_stay_tight_at_the_default_scale():
    """On default-scale data (no special rows) the tail bounds stay below 1e-12 for the action and 1e-10 for log_prob; a bound grown
    loose fails here."""
    for n, K, A in ((64, 512, 16), (33, 5, 15), (65, 515, 17)):
        h, wm, bm, wl, bl, eps = ph.inputs(n, K, A, special=False)
        pre = ph.pre_activations(h, wm, bm, wl, bl)
        act_b, lp_b = ph.tail_bounds(pre, eps)
        print('n=%d K=%d A=%d: action bound %.3g, log_prob bound %.3g' % (n, K, A, act_b.max(), lp_b.max()))
        assert act_b.max() < 1e-12 and lp_b.max() < 1e-10
        assert ph.tail_bounds(pre, None)[0].max() < 1e-12


def test_checker_pinned_on_the_reference_recording(golden):
    """g20: the reference's own Actor on the CPU.  mean and log_std of the checker within gamma_{K + 2} (sum |w| |h| + |b|) of the
    recording, clamped entries `==`; action and log_prob within the first-order fp32 bound (ph.reference_bounds) where it is at
    most 1e-3, and where it is not the branch is pinned: |y| >= 1 - 2^-24 where the recording is +-1.  In the default group every
    element is value-pinned and none differs by more than 1e-4."""
    g = golden('g20_head.npz')
    R, A = ph.GROUP_ROWS, 16
    assert list(g['keys']) == ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias', 'fc1.weight', 'fc1.bias',
                               'fc_mean.weight', 'fc_mean.bias', 'fc_log_std.weight', 'fc_log_std.bias']
    for gi, name in enumerate(ph.GROUPS):
        rows = slice(gi * R, (gi + 1) * R)
        wm, bm, wl, bl = ph.group_weights(g, gi)
        h, eps = g['h'][rows], g['eps'][rows]
        rec = {k: g[k][rows].astype(np.float64) for k in ('mean', 'log_std', 'action', 'log_prob')}
        pre = ph.pre_activations(h, wm, bm, wl, bl)
        t = ph.tail(pre, eps)
        dpre, dy, dlp = ph.reference_bounds(h, wm, bm, wl, bl, eps, pre)
        assert (np.abs(t['mean'] - rec['mean']) <= dpre[:, :A]).all()
        clamped = (rec['log_std'] == 2.0) | (rec['log_std'] == -20.0)
        sure = clamped & ((pre[:, A:] > 2.0 + dpre[:, A:]) | (pre[:, A:] < -20.0 - dpre[:, A:]))
        assert (t['ls'][sure] == rec['log_std'][sure]).all()
        assert (np.abs(t['ls'] - rec['log_std']) <= dpre[:, A:]).all()
        pin_a, pin_l = dy <= 1e-3, dlp <= 1e-3
        err_a, err_l = np.abs(t['y'] - rec['action']), np.abs(t['log_prob'] - rec['log_prob'])
        print('%-16s action: %5.1f %% value-pinned, worst error %.3g (bound %.3g); log_prob: %5.1f %%, worst error %.3g (bound %.3g)'
              % (name, 100 * pin_a.mean(), err_a[pin_a].max() if pin_a.any() else 0, dy[pin_a].max() if pin_a.any() else 0,
                 100 * pin_l.mean(), err_l[pin_l].max() if pin_l.any() else 0, dlp[pin_l].max() if pin_l.any() else 0))
        assert (err_a[pin_a] <= dy[pin_a]).all() and (err_l[pin_l] <= dlp[pin_l]).all()
        # beyond 1e-3 the bound pins no digits, but where it is finite it still pins the terms: a dropped -ls is worth 320 per row
        # in the last two groups, whose acting-scale rows are bounded by about 15
        fin = np.isfinite(dlp)
        print('%-16s log_prob: %5.1f %% of the rows inside a finite bound, median bound %.3g, worst error / bound %.3g'
              % (name, 100 * fin.mean(), float(np.median(dlp[fin])), float((err_l[fin] / dlp[fin]).max())))
        assert (err_l[fin] <= dlp[fin]).all() and fin.mean() >= 0.9
        sat = np.abs(rec['action']) == 1.0
        assert (np.abs(t['y'][sat]) >= 1.0 - 2.0 ** -24).all() and (np.sign(t['y'][sat]) == rec['action'][sat]).all()
        if name == 'default':                                                 # (every element value-pinned, and none further than 1e-4)
            assert pin_a.all() and pin_l.all() and err_a.max() <= 1e-4 and err_l.max() <= 1e-4
