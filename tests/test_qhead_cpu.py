"""No-GPU checks of the critic head (csrc/f110_qhead.h): what f110_qhead_validate, _workspace, _forward and _backward refuse on the
host, the workspace against the checker's tiling, the shape tables against paths(), the checker pinned on the recording of the
reference's own SACAgent.update (tests/golden/g21_critic.npz), its tie rule against torch.minimum's autograd, and its gradients
against fp64 autograd of the restated tail."""
import ctypes as C

import numpy as np
import pytest

import qhead_cases as qc

from red_gym_amd import _lib, build


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _lib.load()


def test_validate_accepts_and_refuses_at_the_limits(lib):
    from red_gym_amd import qhead
    for H in (0, 1, 4096, 4097):
        for A in (0, 1, 32, 33):
            for nc in (0, 1, 2, 3):
                for ld in (A - 1, A, A + 5):
                    ok = 1 <= H <= qc.MAX_H and 1 <= A <= qc.MAX_A and 1 <= nc <= qc.MAX_C and ld >= A
                    cfg = qhead.make_config(H, A, nc, ld)
                    assert lib.f110_qhead_validate(C.byref(cfg)) == (0 if ok else _lib.E_INVALID), (H, A, nc, ld)
                    if not ok:
                        msg = lib.f110_last_error().decode()
                        word = 'hidden' if not 1 <= H <= qc.MAX_H else 'action_dim' if not 1 <= A <= qc.MAX_A else 'critics' if not 1 <= nc <= qc.MAX_C else 'ld'
                        assert word in msg, (msg, H, A, nc, ld)
                        with pytest.raises(ValueError):
                            qhead.validate(H, A, nc, ld)
                        assert lib.f110_qhead_workspace(C.byref(cfg), 4) == 0
    assert lib.f110_qhead_validate(None) == _lib.E_INVALID and b'null' in lib.f110_last_error()
    assert (qhead.MAX_HIDDEN, qhead.MAX_ACTION_DIM, qhead.MAX_CRITICS) == (qc.MAX_H, qc.MAX_A, qc.MAX_C)
    assert _lib.F110_QHEAD_SLICE_ROWS == qc.R


def _critics(nc, hole=None):
    p = _lib.QheadCritics()
    for c in range(2):
        for name in _lib.QHEAD_CRITIC_FIELDS:
            getattr(p, name)[c] = None if (name, c) == hole or c >= nc else 16      # (any non-null address: the checks come before the launch)
    return p


def test_bad_calls_are_refused_before_any_launch(lib):
    """F110_E_INVALID on the host: no device is touched (this runs without one).  Null required pointers, a target without all
    three of its inputs, n out of range, a gamma that is not finite, a misaligned or missing workspace."""
    from red_gym_amd import qhead
    cfg = qhead.make_config(512, 16, 2, 25104)
    one, g = 16, _lib.QheadGrads()
    fwd = lambda p, action=one, n=4, r=None, d=None, lp=None, gamma=0.99, q=one, tv=None: lib.f110_qhead_forward(  # noqa: E731
        C.byref(cfg), p, action, n, r, d, lp, gamma, 0.2, q, None, tv, None)
    assert fwd(None) == _lib.E_INVALID and fwd(C.byref(_critics(2)), action=None) == _lib.E_INVALID and fwd(C.byref(_critics(2)), q=None) == _lib.E_INVALID
    for name in ('pre', 'w_act', 'w2'):
        for c in range(2):
            assert fwd(C.byref(_critics(2, (name, c)))) == _lib.E_INVALID and ('critic %d' % c).encode() in lib.f110_last_error()
    for r, d, lp in ((None, one, one), (one, None, one), (one, one, None), (None, None, None)):
        assert fwd(C.byref(_critics(2)), r=r, d=d, lp=lp, tv=one) == _lib.E_INVALID and b'target' in lib.f110_last_error()
    assert fwd(C.byref(_critics(2)), r=one, d=one, lp=one, tv=one, gamma=float('inf')) == _lib.E_INVALID
    assert fwd(C.byref(_critics(2)), n=-1) == _lib.E_INVALID and fwd(C.byref(_critics(2)), n=qc.MAX_ROWS + 1) == _lib.E_INVALID
    assert fwd(None, action=None, n=0, q=None) == 0                                  # n == 0 does nothing
    bad = qhead.make_config(512, 16, 2, 15)
    assert lib.f110_qhead_forward(C.byref(bad), C.byref(_critics(2)), one, 4, None, None, None, 0.99, 0.2, one, None, None, None) == _lib.E_INVALID
    bwd = lambda p, action=one, n=4, q=one, grads=C.byref(g), ws=None: lib.f110_qhead_backward(  # noqa: E731
        C.byref(cfg), p, action, n, q, one, None, grads, None, ws, None)
    assert bwd(None) == _lib.E_INVALID and bwd(C.byref(_critics(2)), action=None) == _lib.E_INVALID
    assert bwd(C.byref(_critics(2)), q=None) == _lib.E_INVALID and bwd(C.byref(_critics(2)), grads=None) == _lib.E_INVALID
    assert bwd(C.byref(_critics(2, ('w2', 1)))) == _lib.E_INVALID
    assert bwd(C.byref(_critics(2)), ws=one + 8) == _lib.E_INVALID and b'aligned' in lib.f110_last_error()
    g.grad_b1[1] = one                                                               # a parameter gradient without the workspace
    assert bwd(C.byref(_critics(2))) == _lib.E_INVALID and b'workspace' in lib.f110_last_error()
    assert bwd(None, action=None, n=0, q=None, grads=None) == 0
    # every required pointer set, none of them device memory: refused on the host, by the check the policy head uses
    buf = np.zeros(4 * 25104, np.float32)
    p = _lib.QheadCritics()
    for name in _lib.QHEAD_CRITIC_FIELDS:
        getattr(p, name)[0] = getattr(p, name)[1] = buf.ctypes.data
    rc = lib.f110_qhead_forward(C.byref(cfg), C.byref(p), buf.ctypes.data, 4, None, None, None, 0.99, 0.2, buf.ctypes.data, None, None, None)
    assert rc in (_lib.E_INVALID, _lib.E_HIP), rc
    if rc == _lib.E_INVALID:
        assert b'not device memory' in lib.f110_last_error()


def test_workspace_is_what_the_tiling_needs(lib):
    from red_gym_amd import qhead
    for n, H, A in qc.BACKWARD_SHAPES + qc.FORWARD_SHAPES + [(65536, 512, 16)]:
        for nc in (1, 2):
            got = qhead.workspace_bytes(H, A, nc, n)
            assert got == qc.workspace_bytes(n, H, A, nc) and got % 16 == 0, (n, H, A, nc)
            assert got >= 4 * nc * -(-n // qc.R) * (H * (A + 2) + 1)
    assert qhead.workspace_bytes(512, 16, 2, 0) == 0 and qhead.workspace_bytes(0, 16, 2, 4) == 0 and qhead.workspace_bytes(512, 33, 2, 4) == 0
    assert qhead.workspace_bytes(512, 16, 3, 4) == 0 and qhead.workspace_bytes(512, 16, 2, qc.MAX_ROWS + 1) == 0


def test_shape_tables_reach_every_path():
    """The GPU shape tables against paths(): every branch the kernels take on a shape is taken by some shape of the tables."""
    by = {s: qc.paths(*s) for s in qc.FORWARD_SHAPES}
    P = list(by.values())
    assert [s[:3] for s in qc.FORWARD_SHAPES[:7]] == [(1, 1, 1), (1, 64, 1), (3, 65, 2), (17, 63, 15), (64, 512, 16), (65, 515, 17), (5, 4096, 32)]
    assert all(p['lds'] <= qc.QH_LDS_BYTES and p['hc'] % 64 == 0 and p['lds'] % 4 == 0 for p in P)
    assert by[(1, 1, 1)] == dict(by[(1, 1, 1)], hc=64, chunks=1, partial_pass_lanes=1, tiles=1, idle_waves=3, odd_row=True)
    assert by[(1, 64, 1)]['partial_pass_lanes'] == 64 and by[(1, 64, 1)]['passes'] == 1
    assert by[(3, 65, 2)] == dict(by[(3, 65, 2)], hc=128, partial_pass_lanes=1, tiles=1, idle_waves=2, odd_row=True)
    assert by[(17, 63, 15)] == dict(by[(17, 63, 15)], partial_pass_lanes=63, tiles=3, last_tile_rows=1)
    assert by[(64, 512, 16)] == dict(by[(64, 512, 16)], hc=512, chunks=1, restage=False, lds=36928, tiles=8, last_tile_rows=8, idle_waves=0, odd_row=False)
    assert by[(65, 515, 17)] == dict(by[(65, 515, 17)], hc=576, chunks=1, partial_pass_lanes=3, passes=5, tiles=9, last_tile_rows=1)
    assert by[(5, 4096, 32)] == dict(by[(5, 4096, 32)], hc=448, chunks=10, last_chunk=64, restage=True, lds=61056)
    big = by[qc.FORWARD_SHAPES[7]]
    assert big['tiles'] == qc.QH_MAX_GRID + 1 and big['grid'] == qc.QH_MAX_GRID and big['walks'] == 2 and big['last_tile_rows'] == 1
    assert qc.FORWARD_SHAPES[7][1:] == (8, 2)
    assert qc.paths(64, 512, 16)['lds'] > qc.QH_LDS_BYTES // 2                       # (why the critics are staged one after the other)
    B = [qc.paths(*s) for s in qc.BACKWARD_SHAPES]
    assert [s[0] for s in qc.BACKWARD_SHAPES[:5]] == [1, qc.R - 1, qc.R, qc.R + 1, 2 * qc.R + 3]
    assert [p['slices'] for p in B[:5]] == [1, 1, 1, 2, 3] and [p['last_slice_rows'] for p in B[:5]] == [1, qc.R - 1, qc.R, 1, 3]
    assert {p['amax'] for p in B} == {16, 32} and any(p['gw_blocks'] == 2 and not p['gw_partial'] for p in B) and any(p['gw_blocks'] == 2 and p['gw_partial'] for p in B)
    assert any(p['restage'] and p['btiles'] == 2 and p['b_last_tile_rows'] == 2 for p in B) and any(p['b_last_tile_rows'] == 4 for p in B)
    assert any(p['b_last_tile_rows'] == 1 for p in B) and all(p['bwalks'] == 1 for p in B)
    # the specials of inputs(): ties, both sides of the min at least a quarter each, z == 0, both values of done, an all-zero action
    for n, H, A in [s for s in qc.FORWARD_SHAPES + qc.BACKWARD_SHAPES if s[0] >= 8 and s[1] >= 4 and s[0] <= 1024]:
        inp = qc.inputs(n, H, A)
        f = qc.forward(inp)
        ties, zero_row, z0_row = qc.special_rows(n, H)
        assert len(ties) == 2 and (f['q'][0][ties] == f['q'][1][ties]).all()
        assert (f['q'][0] < f['q'][1]).mean() >= 0.25 and (f['q'][1] < f['q'][0]).mean() >= 0.25, (n, H, A)
        assert f['z'][0][z0_row, H // 2] == 0 and f['z'][1][z0_row, H // 2] == 0 and not inp['action'][zero_row].any()
        assert set(inp['done'].tolist()) == {0, 1}
        assert (f['target'][inp['done'] == 1] == inp['reward'].astype(np.float32)[inp['done'] == 1]).all()


def test_checker_pinned_on_the_reference_recording(golden):
    """g21: the reference's own SACAgent.update on the CPU.  q of the four critics, tv, both critic losses and the four recorded
    gradients per critic agree with the checker within bounds built from the recording's own fc1 error and the formulas
    (qc.g21_check); the fixture's conditions hold."""
    g = golden('g21_critic.npz')
    assert list(g['keys']) == ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias', 'fc1.weight', 'fc1.bias',
                               'fc2.weight', 'fc2.bias']
    tq = g['ret'][:, :2]
    assert (tq[:, 0] < tq[:, 1]).mean() >= 0.25 and (tq[:, 1] < tq[:, 0]).mean() >= 0.25
    assert 0.25 <= g['done'].mean() <= 0.75 and (g['fc1_rel_err'] < 1e-6).all() and (g['fc1_rel_err'] > 0).all()

    def run_forward(inp, target):
        return qc.forward(inp, fp32_action=True, target=target, gamma=qc.GAMMA, alpha=qc.ALPHA)

    def run_backward(inp, q, G):
        return qc.backward(inp, qc.forward(inp, fp32_action=True, target=False), grad_q=G)
    qc.g21_check(g, run_forward, run_backward)
    for gi in range(len(qc.GROUPS)):
        for which in ('target', 'online'):
            inp, mags, _ = qc.g21_pass(g, gi, which)
            f = qc.forward(inp, fp32_action=True, target=False)
            for c in range(2):
                assert 0.2 <= (f['z'][c] > 0).mean() <= 0.8
                assert (np.abs(f['z'][c]) <= qc.dz_bound(mags[c], float(g['fc1_rel_err'][gi]), 16)).mean() <= 0.01


def test_tie_rule_is_torch_minimum(golden):
    """The checker's masks `==` the gradient torch.minimum's autograd gives each side on the CPU: 1 / 0 off a tie, halves on it."""
    import torch
    inp = qc.inputs(64, 512, 16)
    f = qc.forward(inp)
    ties = qc.special_rows(64, 512)[0]
    q = torch.tensor(f['q'], requires_grad=True)
    gm = torch.tensor(np.random.default_rng(0).normal(size=64).astype(np.float32))
    torch.minimum(q[0], q[1]).backward(gm)
    m = qc.min_masks(f['q'])
    assert np.array_equal(q.grad.numpy(), m * gm.numpy()[None, :])
    assert (m[:, ties] == 0.5).all() and set(np.unique(m).tolist()) == {0.0, 0.5, 1.0}
    assert np.array_equal(torch.minimum(q[0], q[1]).detach().numpy(), f['qmin'])
    assert (qc.min_masks(f['q'][:1]) == 1).all()


@pytest.mark.parametrize('shape', [(37, 70, 3), (qc.R + 3, 33, 17)])
def test_checker_gradients_agree_with_autograd(shape):
    """The checker's backward against fp64 autograd of the restated tail (cat-free: pre + a @ W.T + b, relu, fc2, min) with pre, the
    action and the parameters as leaves.  Both sides share the forward's masks where |z| is not tiny (inputs() puts z == 0 exactly on
    one unit, where both give 0), so every gradient agrees within the fp32 sums' gamma bounds."""
    import torch
    n, H, A = shape
    inp = qc.inputs(n, H, A)
    f = qc.forward(inp)
    rng = np.random.default_rng([n, H, A])
    gq, gm = rng.normal(size=(2, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    got = qc.backward(inp, f, gq, gm)
    act = torch.tensor(f['act32'].astype(np.float64), requires_grad=True)
    leaves, qs = [], []
    for c in range(2):
        t = {k: torch.tensor(np.asarray(inp[k][c], np.float64), requires_grad=True) for k in ('pre', 'w_act', 'b1', 'w2', 'b2')}
        z = t['pre'] + act @ t['w_act'].T + t['b1']
        assert np.array_equal(z.detach().numpy() > 0, f['z'][c] > 0)                 # (no unit's sign differs between fp32 and fp64 here)
        qs.append(torch.relu(z) @ t['w2'] + t['b2'])
        leaves.append(t)
    q = torch.stack(qs)
    assert np.array_equal(q.detach().numpy()[:, qc.special_rows(n, H)[0]], f['q'][:, qc.special_rows(n, H)[0]])   # the ties are ties in fp64 too
    ((q * torch.tensor(gq.astype(np.float64))).sum() + (torch.minimum(q[0], q[1]) * torch.tensor(gm.astype(np.float64))).sum()).backward()
    # the masks off the tie rows must agree for the comparison to mean anything: q's fp32 error could flip a near-tie
    off = np.ones(n, bool)
    off[qc.special_rows(n, H)[0]] = False
    assert np.array_equal((q[0] < q[1]).numpy()[off], (f['q'][0] < f['q'][1])[off])
    G = np.abs(got['G']).astype(np.float64)
    act_abs = np.abs(f['act32']).astype(np.float64)
    m = min(n, qc.R) + -(-n // qc.R) + 2
    ga_bound = np.zeros((n, A))
    for c in range(2):
        w2a, wa = np.abs(inp['w2'][c]).astype(np.float64), np.abs(inp['w_act'][c]).astype(np.float64)
        gz = np.where(f['z'][c] > 0, G[c][:, None] * w2a[None, :], 0.0)
        h = f['h'][c].astype(np.float64)
        # h itself carries the forward's fp32 error: A fused steps and two additions on |pre| + sum |w||a| + |b1|
        dh = qc.bc.gamma(A + 2) * (np.abs(inp['pre'][c]) + act_abs @ wa.T + np.abs(inp['b1'][c]))
        want = {'grad_pre': (leaves[c]['pre'].grad.numpy(), 3 * qc.U32 * gz),
                'grad_w_act': (leaves[c]['w_act'].grad.numpy(), qc.bc.gamma(m + 3) * (gz.T @ act_abs)),
                'grad_b1': (leaves[c]['b1'].grad.numpy(), qc.bc.gamma(m + 3) * gz.sum(0)),
                'grad_w2': (leaves[c]['w2'].grad.numpy(), qc.bc.gamma(m + 3) * (G[c] @ h) + G[c] @ dh),
                'grad_b2': (leaves[c]['b2'].grad.numpy(), qc.bc.gamma(m + 3) * G[c].sum(keepdims=True))}
        for key, (ref, bound) in want.items():
            err = np.abs(got[key][c].astype(np.float64) - ref)
            print('%s critic %d %s: worst error / bound %.3g' % (shape, c, key, float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all() and (ref != 0).any(), (key, c)
        ga_bound += qc.bc.gamma(-(-H // 64) + 6 + 3 + 2) * (gz @ wa)
    err = np.abs(got['grad_action'].astype(np.float64) - act.grad.numpy())
    print('%s grad_action: worst error / bound %.3g' % (shape, float((err / np.maximum(ga_bound, 1e-300)).max())))
    assert (err <= ga_bound).all()
    for c in range(2):
        assert got['grad_pre'][c][n // 2, H // 2] == 0 and leaves[c]['pre'].grad[n // 2, H // 2] == 0     # z == 0: torch's ReLU gives 0 too
