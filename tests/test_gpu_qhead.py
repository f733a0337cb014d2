"""The critic head on the GPU (csrc/f110_qhead.h): q, qmin and the target `==` the checker of tests/qhead_cases.py as raw bit patterns
at every shape-selected path (qc.paths), for fp64 and fp32 actions, with and without biases, one and two critics, a dense and a
strided, misaligned w_act; margins, batch independence, repeatability; every output of the backward pass `==` the checker, the
tie rows' halves, NULL outputs, the columns between grad_w_act's rows; the module against the torch sequence it replaces and against
the recording of the reference's own update (g21); a captured graph."""
import ctypes as C

import numpy as np
import pytest

import gpu_checks as gk
import qhead_cases as qc

pytestmark = pytest.mark.gpu

SENT = -7.0                                   # fill of every output and guard: no result of these inputs equals it


_cache = {}


def _case(shape, seed=0):
    """inputs() of a shape and the checker's forward in every variant asked for, computed once and left unchanged."""
    key = (shape, seed)
    if key not in _cache:
        _cache[key] = (qc.inputs(*shape, seed=seed), {})
    return _cache[key]


def _forward_ref(shape, nc, fp64, bias, seed=0):
    inp, memo = _case(shape, seed)
    key = (nc, fp64, bias)
    if key not in memo:
        memo[key] = qc.forward(inp, C=nc, fp32_action=not fp64, bias=bias)
        for v in memo[key].values():
            for a in (v if isinstance(v, list) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return inp, memo[key]


class _Raw:
    """The arrays of one raw-ABI call on the device: w_act of every critic inside a [H, ld] block of SENT that starts `off` floats
    into its allocation (off = 1: a base aligned to 4 bytes only), every output between two guards of SENT."""

    def __init__(self, inp, nc, fp64, bias, ld_extra=0, off=0):
        import torch
        from red_gym_amd import _lib, qhead
        self.lib, self._lib = _lib.load(), _lib
        self.n, self.H = inp['pre'][0].shape
        self.A = inp['w_act'][0].shape[1]
        self.nc, self.fp64, self.ld, self.off = nc, fp64, self.A + ld_extra, off
        self.cfg = qhead.make_config(self.H, self.A, nc, self.ld, fp64)
        dt = torch.float64 if fp64 else torch.float32
        self.dt = dt
        self.keep = []
        self.p = _lib.QheadCritics()
        self.wblocks = []
        for c in range(nc):
            block = np.full(self.H * self.ld + off, SENT, np.float32)
            block[off:].reshape(self.H, self.ld)[:, :self.A] = inp['w_act'][c]
            wb = gk.to_device(block)
            t = [gk.to_device(inp['pre'][c]), wb, gk.to_device(inp['b1'][c]) if bias else None, gk.to_device(inp['w2'][c]), gk.to_device(inp['b2'][c]) if bias else None]
            self.keep.append(t)
            self.wblocks.append(block)
            self.p.pre[c], self.p.w_act[c], self.p.b1[c] = t[0].data_ptr(), wb.data_ptr() + 4 * off, _lib.ptr(t[2])
            self.p.w2[c], self.p.b2[c] = t[3].data_ptr(), _lib.ptr(t[4])
        self.action = gk.to_device(inp['action']).to(dt)
        self.nlp, self.reward, self.done = gk.to_device(inp['nlp']).to(dt), gk.to_device(inp['reward']), gk.to_device(inp['done'])
        self.stream = torch.cuda.current_stream().cuda_stream

    def forward(self, target=True, qmin=True, gamma=0.99, alpha=0.2):
        import torch
        n, nc = self.n, self.nc
        bufs = [gk.Guarded(size, fill=SENT) for size in (nc * n, n, n)]
        ptr = [b.ptr for b in bufs]
        self._lib.check(self.lib.f110_qhead_forward(C.byref(self.cfg), C.byref(self.p), self.action.data_ptr(), n, self.reward.data_ptr() if target else None,
                                                    self.done.data_ptr() if target else None, self.nlp.data_ptr() if target else None, gamma, alpha,
                                                    ptr[0], ptr[1] if qmin else None, ptr[2] if target else None, self.stream))
        torch.cuda.synchronize()
        for c in range(nc):                                               # the weights, and what lies between their rows, are as they were
            assert gk.same(self.keep[c][1], self.wblocks[c])
        return bufs[0].read().reshape(nc, n), bufs[1].read(), bufs[2].read()

    def backward(self, q, grad_q, grad_qmin, skip=(), ws_fill=float('nan')):
        """f110_qhead_backward from a workspace of `ws_fill` -> dict of host arrays; outputs named in `skip` are passed as NULL.
        grad_w_act comes back as the whole [H, ld] block."""
        import torch
        from red_gym_amd import qhead
        n, H, A, nc, ld = self.n, self.H, self.A, self.nc, self.ld
        sizes = dict(grad_pre=n * H, grad_w_act=H * ld, grad_b1=H, grad_w2=H, grad_b2=1)
        g = self._lib.QheadGrads()
        bufs = {k: [gk.Guarded(s, fill=SENT) for _ in range(nc)] for k, s in sizes.items()}
        for k in sizes:
            for c in range(nc):
                getattr(g, k)[c] = None if k in skip else bufs[k][c].ptr
        ga = gk.Guarded(n * A, dtype=self.dt, fill=SENT)
        nbytes = qhead.workspace_bytes(H, A, nc, n)
        assert nbytes == qc.workspace_bytes(n, H, A, nc)
        ws = gk.Guarded(nbytes // 4, fill=ws_fill)
        qd, gq, gm = gk.to_device(np.ascontiguousarray(q, np.float32)), gk.to_device(grad_q), gk.to_device(grad_qmin)
        self._lib.check(self.lib.f110_qhead_backward(C.byref(self.cfg), C.byref(self.p), self.action.data_ptr(), n, qd.data_ptr(), self._lib.ptr(gq),
                                                     self._lib.ptr(gm), C.byref(g), None if 'grad_action' in skip else ga.ptr,
                                                     ws.ptr, self.stream))
        torch.cuda.synchronize()
        ws.read()
        res = {k: [b.read() for b in bufs[k]] for k in sizes}
        res['grad_action'] = ga.read().reshape(n, A)
        res['grad_pre'] = [a.reshape(n, H) for a in res['grad_pre']]
        res['grad_w_act'] = [a.reshape(H, ld) for a in res['grad_w_act']]
        for k in skip:
            assert all((a == SENT).all() for a in (res[k] if isinstance(res[k], list) else [res[k]])), k
        return res


VARIANTS = [(nc, fp64, bias) for nc in (2, 1) for fp64 in (True, False) for bias in (True, False)]


@pytest.mark.parametrize('shape', qc.FORWARD_SHAPES)
def test_forward_equals_checker(shape):
    """q, qmin and the target `==` the checker as raw bit patterns, for one and two critics, fp64 and fp32 actions, with and without
    biases; with biases w_act is a view with row stride A + 3 that starts 4 bytes past a 16-byte boundary, without them it is dense;
    nothing is written outside the outputs or into the weights; a second call gives the same bits; without the target's inputs the
    target is not touched, and neither is a NULL qmin."""
    n, H, A = shape
    for nc, fp64, bias in VARIANTS:
        inp, want = _forward_ref(shape, nc, fp64, bias)
        raw = _Raw(inp, nc, fp64, bias, ld_extra=3 if bias else 0, off=1 if bias else 0)
        q, qmin, tv = raw.forward()
        what = '%s C=%d fp64=%s bias=%s' % (shape, nc, fp64, bias)
        bad = [gk.differing(a, b) for a, b in ((q, want['q']), (qmin, want['qmin']), (tv, want['target']))]
        print('%s: %d q, %d qmin, %d target values differ' % ((what,) + tuple(bad)))
        assert bad == [0, 0, 0], what
        q2, qmin2, tv2 = raw.forward()
        assert gk.same(q2, q) and gk.same(qmin2, qmin) and gk.same(tv2, tv)
        q3, qmin3, tv3 = raw.forward(target=False, qmin=False)
        assert gk.same(q3, q) and (qmin3 == SENT).all() and (tv3 == SENT).all()
    inp, want = _forward_ref(shape, 2, True, True)
    ties, zero_row, z0_row = qc.special_rows(n, H)
    if H >= 4:
        assert want['z'][0][z0_row, H // 2] == 0.0 and want['z'][1][z0_row, H // 2] == 0.0
    if ties:
        assert (want['q'][0][ties] == want['q'][1][ties]).all() and (want['q'][:, ties] == qc.TIE_Q).all()
        assert (want['q'][0] < want['q'][1]).mean() >= 0.25 and (want['q'][1] < want['q'][0]).mean() >= 0.25
        assert set(inp['done'].tolist()) == {0, 1} and not inp['action'][zero_row].any()


def test_rows_do_not_depend_on_the_batch():
    """A row's q, qmin and target are the same bits alone, in a batch of 131 and at another place of a batch of 4099."""
    import torch
    n, H, A = 131, 515, 17
    inp, want = _forward_ref((n, H, A), 2, True, True, seed=3)
    full = _Raw(inp, 2, True, True).forward()
    assert gk.same(full[0], want['q'])

    def pick(rows, total=None):
        sub = dict(inp)
        for k in ('action', 'reward', 'done', 'nlp'):
            sub[k] = inp[k][rows]
        sub['pre'] = [p[rows] for p in inp['pre']]
        if total is not None:                                             # scattered into a larger batch of zeros
            perm = np.random.default_rng(1).permutation(total)[:len(rows)]
            for k in ('action', 'reward', 'done', 'nlp'):
                big = np.zeros((total,) + sub[k].shape[1:], sub[k].dtype)
                big[perm] = sub[k]
                sub[k] = big
            pres = []
            for p in sub['pre']:
                big = np.zeros((total, H), np.float32)
                big[perm] = p
                pres.append(big)
            sub['pre'] = pres
            return sub, perm
        return sub, None
    for i in (0, 1, 7, 8, 130):
        one = _Raw(pick(np.array([i]))[0], 2, True, True).forward()
        assert all(gk.same(a[..., i:i + 1], b) for a, b in zip(full, one)), i
    sub, perm = pick(np.arange(n), 4099)
    big = _Raw(sub, 2, True, True).forward()
    assert all(gk.same(a, b[..., perm]) for a, b in zip(full, big))
    assert full[0][0, 0] != full[0][0, 1]


def _grads_for(shape, mode, rng):
    nc, n = 2, shape[0]
    gq = rng.normal(size=(nc, n)).astype(np.float32) if mode in ('q', 'both') else None
    gm = rng.normal(size=n).astype(np.float32) if mode in ('qmin', 'both') else None
    return gq, gm


def _compare_backward(res, want, inp, A, what, skip=()):
    bad = {}
    for c in range(len(want['grad_pre'])):
        for k in ('grad_pre', 'grad_b1', 'grad_w2', 'grad_b2'):
            if k not in skip:
                bad['%s[%d]' % (k, c)] = gk.differing(res[k][c].reshape(-1), want[k][c].reshape(-1))
        if 'grad_w_act' not in skip:
            block = res['grad_w_act'][c]
            bad['grad_w_act[%d]' % c] = gk.differing(block[:, :A], want['grad_w_act'][c])
            assert (block[:, A:] == SENT).all(), '%s: the columns between the rows of grad_w_act[%d] were written' % (what, c)
    if 'grad_action' not in skip:
        ga = res['grad_action']
        bad['grad_action'] = gk.differing(ga.astype(np.float32), want['grad_action']) + int((ga.astype(np.float32) != ga).sum())
    print('%s: values that differ: %s' % (what, bad))
    assert not any(bad.values()), (what, bad)


@pytest.mark.parametrize('shape', qc.BACKWARD_SHAPES)
def test_backward_equals_checker(shape):
    """Every output `==` the checker with grad_q only, grad_qmin only and both, for an fp64 action and a strided grad_w_act whose
    columns between the rows keep their fill (fp32 and dense once); the tie rows get halves; one critic; a second call from a
    workspace of another fill gives the same bits; NULL outputs are skipped and the others unchanged by that."""
    n, H, A = shape
    rng = np.random.default_rng([n, H, A, 7])
    inp, fwd = _forward_ref(shape, 2, True, True)
    raw = _Raw(inp, 2, True, True, ld_extra=3, off=1)
    ties, _, z0_row = qc.special_rows(n, H)
    for mode in ('q', 'qmin', 'both'):
        gq, gm = _grads_for(shape, mode, rng)
        want = qc.backward(inp, fwd, gq, gm)
        res = raw.backward(fwd['q'], gq, gm)
        _compare_backward(res, want, inp, A, '%s %s' % (shape, mode))
        if H >= 4:
            assert all(res['grad_pre'][c][z0_row, H // 2] == 0.0 for c in range(2))          # z == 0: gradient 0, as torch's ReLU
        if mode == 'qmin':
            side = fwd['q'][0] < fwd['q'][1]
            assert (res['grad_pre'][0][~side & (fwd['q'][0] != fwd['q'][1])] == 0).all()
            for r in ties:                                                                    # w2[0] = 1: g_z of unit 0 is G itself
                assert all(res['grad_pre'][c][r, 0] == np.float32(0.5) * gm[r] for c in range(2)) and gm[r] != 0
        if mode == 'both':
            again = raw.backward(fwd['q'], gq, gm, ws_fill=3.0e38)
            assert all(gk.same(a, b) for k in res for a, b in zip(res[k], again[k]))
            part = raw.backward(fwd['q'], gq, gm, skip=('grad_pre', 'grad_b1', 'grad_w_act'))
            _compare_backward(part, want, inp, A, '%s NULL grad_pre, grad_b1, grad_w_act' % (shape,), skip=('grad_pre', 'grad_b1', 'grad_w_act'))
            part = raw.backward(fwd['q'], gq, gm, skip=('grad_action', 'grad_w2', 'grad_b2'))
            _compare_backward(part, want, inp, A, '%s NULL grad_action, grad_w2, grad_b2' % (shape,), skip=('grad_action', 'grad_w2', 'grad_b2'))
    gq, gm = _grads_for(shape, 'both', rng)
    inp, fwd32 = _forward_ref(shape, 2, False, False)
    dense = _Raw(inp, 2, False, False)
    _compare_backward(dense.backward(fwd32['q'], gq, gm), qc.backward(inp, fwd32, gq, gm, bias=False), inp, A, '%s fp32 action, no biases, dense' % (shape,))
    inp, fwd1 = _forward_ref(shape, 1, True, True)
    one = _Raw(inp, 1, True, True, ld_extra=1)
    _compare_backward(one.backward(fwd1['q'], gq[:1], gm), qc.backward(inp, fwd1, gq[:1], gm), inp, A, '%s one critic' % (shape,))


def _torch_sequence(feats, action, fc1s, fc2s):
    """The launches twin_q replaces: .float(), cat, fc1, relu, fc2 per critic, min."""
    import torch
    import torch.nn.functional as F
    a = action.float()
    qs = [F.linear(torch.relu(F.linear(torch.cat([f, a], 1), l1.weight, l1.bias)), l2.weight, l2.bias) for f, l1, l2 in zip(feats, fc1s, fc2s)]
    return qs, (torch.min(qs[0], qs[1]) if len(qs) == 2 else qs[0])


def _module_case(n=64, F=1000, A=16, H=512, seed=5):
    import torch
    torch.manual_seed(seed)
    fc1s = [torch.nn.Linear(F + A, H).cuda() for _ in range(2)]
    fc2s = [torch.nn.Linear(H, 1).cuda() for _ in range(2)]
    with torch.no_grad():
        for l in fc1s:
            l.weight[:, F:].mul_(30.0)                                    # (the action part weighs as much as the features)
        fc2s[1].bias.add_(0.01)
    feats = [torch.randn((n, F), device='cuda').relu_() for _ in range(2)]
    action = torch.tanh(torch.randn((n, A), dtype=torch.float64, device='cuda'))
    return feats, action, fc1s, fc2s


def test_module_against_the_torch_sequence():
    """QHead.from_linears shares tensors and has the reference Critic's keys; twin_q and td_target agree with the restated torch
    sequence within bounds derived as for g21 (the fp32 GEMM's own error against fp64 measured on the torch side, the rest by
    formula); every gradient agrees with autograd of that sequence; ONE fc1.weight gradient of the full shape comes out with both
    column ranges filled; mismatches raise ValueError."""
    import torch
    import torch.nn.functional as Fn
    from red_gym_amd.qhead import QHead, td_target, twin_q
    n, F, A, H = 64, 1000, 16, 512
    feats, action, fc1s, fc2s = _module_case(n, F, A, H)
    head = QHead.from_linears(fc1s[0], fc2s[0])
    assert head.fc1.weight.data_ptr() == fc1s[0].weight.data_ptr() and head.fc2.bias.data_ptr() == fc2s[0].bias.data_ptr()
    assert sorted(head.state_dict()) == ['fc1.bias', 'fc1.weight', 'fc2.bias', 'fc2.weight']
    fresh = QHead(F, A, H).cuda()
    fresh.load_state_dict(head.state_dict())
    assert torch.equal(fresh.fc1.weight, fc1s[0].weight)
    q, qmin = twin_q(feats, action, fc1s, fc2s)
    assert tuple(q.shape) == (2, n) and tuple(qmin.shape) == (n,) and q.dtype == qmin.dtype == torch.float32
    assert torch.equal(head(feats[0], action), q[0].unsqueeze(1)) and tuple(head(feats[0], action).shape) == (n, 1)
    ref_q, ref_min = _torch_sequence(feats, action, fc1s, fc2s)
    a32 = action.float()
    side = gk.to_host(q[0] < q[1])
    assert 0.1 < side.mean() < 0.9                                         # both sides of the min occur
    dq = []
    for c in range(2):
        x = torch.cat([feats[c], a32], 1)
        z32 = Fn.linear(x, fc1s[c].weight, fc1s[c].bias)
        z64 = Fn.linear(x.double(), fc1s[c].weight.double(), fc1s[c].bias.double())
        mag = Fn.linear(x.double().abs(), fc1s[c].weight.double().abs(), fc1s[c].bias.double().abs())
        rel = float(((z32.double() - z64).abs() / mag).max())
        dz = qc.dz_bound(gk.to_host(mag), rel, A, gemm_sides=2)
        bound = qc.q_bound(dz, gk.to_host(torch.relu(z64)), gk.to_host(fc2s[c].weight.double()).reshape(-1), float(fc2s[c].bias))
        err = np.abs(gk.to_host(q[c]).astype(np.float64) - gk.to_host(ref_q[c][:, 0]).astype(np.float64))
        print('critic %d: fc1 relative error %.3g of sum |w||x|; worst q error %.3g, its bound %.3g' % (c, rel, err.max(), bound[err.argmax()]))
        assert (err <= bound).all() and bound.max() < 1e-3
        dq.append(bound)
    dmin = np.maximum(dq[0], dq[1])
    assert (np.abs(gk.to_host(qmin).astype(np.float64) - gk.to_host(ref_min[:, 0])) <= dmin).all()
    # the target against the reference's two fp32 lines
    gamma, alpha = 0.99, 0.2
    reward = torch.randn(n, dtype=torch.float64, device='cuda')
    done = (torch.rand(n, device='cuda') < 0.5).to(torch.uint8)
    nlp = torch.randn(n, dtype=torch.float64, device='cuda') * 10 - 20
    tv = td_target(feats, action, nlp, reward, done, fc1s, fc2s, gamma, alpha)
    assert tv.dtype == torch.float32 and tuple(tv.shape) == (n,) and tv.grad_fn is None
    tq = ref_min - alpha * nlp.float().unsqueeze(1)
    ref_tv = reward.float().unsqueeze(1) + (1 - done.float().unsqueeze(1)) * gamma * tq
    tb = qc.target_bound(dmin, gk.to_host(qmin), gk.to_host(nlp), gk.to_host(reward), gk.to_host(done), gamma, alpha)
    err = np.abs(gk.to_host(tv).astype(np.float64) - gk.to_host(ref_tv[:, 0]))
    print('target: worst error %.3g, its bound %.3g' % (err.max(), tb[err.argmax()]))
    assert (err <= tb).all() and set(gk.to_host(done).tolist()) == {0, 1}
    assert torch.equal(td_target(feats, action, nlp.unsqueeze(1), reward, done.bool(), fc1s, fc2s, gamma, alpha), tv)
    # gradients: a loss that uses q and qmin, features and action require grad
    f_req = [f.clone().requires_grad_() for f in feats]
    a_req = action.clone().requires_grad_()
    params = [p for l in fc1s + fc2s for p in (l.weight, l.bias)]
    tvd = tv.detach()
    q, qmin = twin_q(f_req, a_req, fc1s, fc2s)
    (Fn.mse_loss(q[0], tvd) + Fn.mse_loss(q[1], tvd) - qmin.mean()).backward()
    got = [p.grad.clone() for p in params + f_req + [a_req]]
    for l in fc1s:
        assert l.weight.grad.shape == (H, F + A) and bool((l.weight.grad[:, :F] != 0).any()) and bool((l.weight.grad[:, F:] != 0).any())
    for p in params:
        p.grad = None
    f64 = [f.detach().double().requires_grad_() for f in feats]
    a64 = action.detach().float().double().requires_grad_()
    p64 = [p.detach().double().requires_grad_() for p in params]
    qs = [Fn.linear(torch.relu(Fn.linear(torch.cat([f64[c], a64], 1), p64[2 * c], p64[2 * c + 1])), p64[4 + 2 * c], p64[5 + 2 * c])[:, 0] for c in range(2)]
    (Fn.mse_loss(qs[0], tvd.double()) + Fn.mse_loss(qs[1], tvd.double()) - torch.min(qs[0], qs[1]).mean()).backward()
    names = ['fc1[0].weight', 'fc1[0].bias', 'fc1[1].weight', 'fc1[1].bias', 'fc2[0].weight', 'fc2[0].bias', 'fc2[1].weight', 'fc2[1].bias', 'feat[0]', 'feat[1]', 'action']
    for name, g, r in zip(names, got, p64 + f64 + [a64]):
        err, scale = float((g.double() - r.grad).abs().max()), float(r.grad.abs().max())
        print('%s.grad: largest difference from fp64 autograd %.3g (largest entry %.3g)' % (name, err, scale))
        # fp32 against fp64: z differs by about 1e-6, which moves G by as much relative to its size and flips the mask of the few
        # units within that of zero, each worth one term of a sum of n * H; a lost or doubled term changes an entry by its own size
        assert g.shape == r.grad.shape and scale > 0 and err <= 1e-3 * scale
    assert got[-1].dtype == torch.float64
    # mismatches
    bad_fc1 = torch.nn.Linear(F + A + 1, H).cuda()
    for args in ((feats, action.half(), fc1s, fc2s), (feats[:1], action, fc1s, fc2s), ([f.double() for f in feats], action, fc1s, fc2s),
                 (feats, action[:5], fc1s, fc2s), (feats, action.cpu(), fc1s, fc2s), (feats, action, [bad_fc1, fc1s[1]], fc2s),
                 (feats, action, fc1s, [fc2s[0], torch.nn.Linear(H, 2).cuda()]), (feats, action, [l.weight for l in fc1s], fc2s),
                 (feats + feats[:1], action, fc1s + fc1s[:1], fc2s + fc2s[:1])):
        with pytest.raises(ValueError):
            twin_q(*args)
    for kw in (dict(reward=reward.float()), dict(done=done.float()), dict(nlp=nlp.float()), dict(reward=reward[:5]), dict(gamma=float('nan'))):
        a = dict(nlp=nlp, reward=reward, done=done, gamma=gamma)
        a.update(kw)
        with pytest.raises(ValueError):
            td_target(feats, action, a['nlp'], a['reward'], a['done'], fc1s, fc2s, a['gamma'], alpha)
    with pytest.raises(ValueError):
        QHead(F, 33, H)
    with pytest.raises(ValueError):
        QHead.from_linears(torch.nn.Linear(10, 4097), torch.nn.Linear(4097, 1))
    empty = twin_q([f[:0] for f in feats], action[:0], fc1s, fc2s)
    assert tuple(empty[0].shape) == (2, 0) and tuple(empty[1].shape) == (0,)


def test_fc1_gradient_is_one_allocation():
    """The backward pass of twin_q at SAL's width allocates one [H, F + A] gradient per fc1.weight and lets the framework's GEMM
    write its feature columns through the view: its peak stays below what two full-size temporaries per critic (the zero-filled
    halves autograd would add) need on top."""
    import torch
    from red_gym_amd.qhead import twin_q
    n, F, A, H = 64, 25088, 16, 512
    feats, action, fc1s, fc2s = _module_case(n, F, A, H, seed=6)
    wbytes = H * (F + A) * 4
    for warm in (True, False):
        for l in fc1s + fc2s:
            l.weight.grad = l.bias.grad = None
        q, qmin = twin_q(feats, action, fc1s, fc2s)
        loss = q.sum() + qmin.sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    print('backward peak %.1f MB over the state before it; one fc1 gradient is %.1f MB' % (peak / 1e6, wbytes / 1e6))
    assert all(l.weight.grad.data_ptr() % 16 == 0 and l.weight.grad.is_contiguous() for l in fc1s)
    assert peak < 2 * wbytes + wbytes // 2                                # two gradients and the small tensors; a temporary would be a third


def test_graph_replay_equals_eager():
    """twin_q's forward captured in a torch.cuda.graph on one stream replays `==` eager after the inputs changed."""
    import torch
    from red_gym_amd.qhead import twin_q
    feats, action, fc1s, fc2s = _module_case(33, 200, 16, 512, seed=8)
    with torch.no_grad():
        twin_q(feats, action, fc1s, fc2s)                                 # warm up: the GEMM's first call is not captured
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            twin_q(feats, action, fc1s, fc2s)
            with torch.cuda.graph(graph, stream=s):
                q, qmin = twin_q(feats, action, fc1s, fc2s)
        torch.cuda.current_stream().wait_stream(s)
        first = (q.clone(), qmin.clone())
        for f in feats:
            f.copy_(torch.randn_like(f).relu_())
        action.copy_(torch.tanh(torch.randn_like(action)))
        graph.replay()
        torch.cuda.synchronize()
        eager = twin_q(feats, action, fc1s, fc2s)
        assert torch.equal(q, eager[0]) and torch.equal(qmin, eager[1]) and not torch.equal(q, first[0])


def test_g21_on_the_device(golden):
    """The recording of the reference's own SACAgent.update: the kernels, fed the fixture's pre, fp32 actions and next_log_prob, give
    q of the four critics, tv, both critic losses and the four recorded gradients per critic within the reference bounds
    (qc.g21_check, as test_qhead_cpu pins the checker), and `==` the checker on the way."""
    g = golden('g21_critic.npz')
    A = g['w_act'].shape[2]

    def run_forward(inp, target):
        q, qmin, tv = _Raw(inp, 2, False, True, ld_extra=5).forward(target=target, gamma=qc.GAMMA, alpha=qc.ALPHA)
        want = qc.forward(inp, fp32_action=True, target=target, gamma=qc.GAMMA, alpha=qc.ALPHA)
        assert gk.same(q, want['q']) and gk.same(qmin, want['qmin'])
        assert not target or gk.same(tv, want['target'])
        return dict(q=q, qmin=qmin, target=tv if target else None)

    def run_backward(inp, q, G):
        res = _Raw(inp, 2, False, True, ld_extra=5).backward(q, G, None)
        res['grad_w_act'] = [b[:, :A] for b in res['grad_w_act']]
        return res
    qc.g21_check(g, run_forward, run_backward)
