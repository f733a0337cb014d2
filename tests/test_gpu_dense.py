"""The dense layer on the GPU (red_gym_amd/dense.py, csrc/f110_dense.h) against the NumPy checkers of tests/dense_cases.py, `==` as
raw 32-bit patterns: forward and backward over the shape table, through the raw ABI on guarded buffers with the weight dense and
as a column view, the batch independence the layer exists for, SAL's own fc1, the critics' opt-in path, and the reference pin."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
import gpu_checks as gk
import qhead_cases as qh

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


class _Raw:
    """f110_dense_forward / f110_dense_backward on guarded buffers, for one shape and one layout of weight and grad_weight."""

    def __init__(self, shape, layout, relu):
        from red_gym_amd import _lib, dense
        self.n, self.K, self.H, self.S = shape
        ld, self.off = dc.LAYOUTS[layout]
        self.ld = ld(self.K)
        self.cfg = dense.validate(self.K, self.H, self.ld, self.S, relu)
        self.lib, self._lib, self.dense = _lib.load(), _lib, dense

    def weight(self, w):
        return gk.Guarded.matrix(self.H, self.K, self.ld, self.off, w, fill=SENTINEL)

    def forward(self, x, wm, b, n=None):
        """-> out [n, H] as numpy; the workspace is NaN beforehand and the guards of out and the workspace are checked."""
        import torch
        n = self.n if n is None else n
        out = gk.Guarded(n * self.H, fill=SENTINEL)
        nbytes = self.dense.workspace_bytes(self.cfg, n)
        assert nbytes == dc.paths(n, self.K, self.H, self.S)['workspace'] if n else nbytes == 0
        ws = gk.Guarded(nbytes // 4, fill=float('nan')) if nbytes else None
        before = wm.whole.clone()
        self._lib.check(self.lib.f110_dense_forward(C.byref(self.cfg), x.data_ptr(), n, wm.ptr, self._lib.ptr(b), out.ptr,
                                                    None if ws is None else ws.ptr, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(wm.whole, before)
        if ws is not None:
            ws.read()
        got = out.read().reshape(n, self.H)
        assert n == 0 or not (got == SENTINEL).any()
        return got

    def backward(self, x, out, go, wm, want=(True, True, True)):
        """-> (grad_x [n, K], grad_weight [H, K], grad_bias [H]) as numpy, None for what `want` leaves out; the guards, the floats
        between the rows of grad_weight and the weight itself are checked."""
        import torch
        gx = gk.Guarded(self.n * self.K, fill=SENTINEL) if want[0] else None
        gw = gk.Guarded.matrix(self.H, self.K, self.ld, self.off, fill=SENTINEL) if want[1] else None
        gb = gk.Guarded(self.H, fill=SENTINEL) if want[2] else None
        before = wm.whole.clone()
        ptr = lambda g: None if g is None else g.ptr       # noqa: E731
        self._lib.check(self.lib.f110_dense_backward(C.byref(self.cfg), x.data_ptr(), self._lib.ptr(out), go.data_ptr(), self.n, wm.ptr,
                                                     ptr(gx), ptr(gw), ptr(gb), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(wm.whole, before)
        return (None if gx is None else gx.read().reshape(self.n, self.K), None if gw is None else gw.read(), None if gb is None else gb.read())


def _layer(shape, r, relu, with_bias):
    """linear_feat forward and backward on leaves made from the reference's arrays -> (out, x.grad, w.grad, b.grad)."""
    from red_gym_amd.dense import linear_feat
    x, w = gk.to_device(r['x']).requires_grad_(), gk.to_device(r['w']).requires_grad_()
    b = gk.to_device(r['b']).requires_grad_() if with_bias else None
    out = linear_feat(x, w, b, relu=relu, segment=shape[3])
    out.backward(gk.to_device(r['grad_out']))
    return out, x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize('shape', dc.SHAPES, ids=str)
def test_forward_equals_checker(shape):
    """`==` the checker as raw bit patterns under dc.VARIANTS (relu on and off, bias present and NULL); a second call gives the same bits."""
    from red_gym_amd.dense import linear_feat
    r = dc.reference(shape)
    x, w, b = gk.to_device(r['x']), gk.to_device(r['w']), gk.to_device(r['b'])
    total = 0
    for v in dc.VARIANTS:
        relu, with_bias = v
        got = linear_feat(x, w, b if with_bias else None, relu=relu, segment=shape[3])
        again = linear_feat(x, w, b if with_bias else None, relu=relu, segment=shape[3])
        assert got.grad_fn is None and gk.differing(again, gk.to_host(got)) == 0
        bad = gk.differing(got, r['out'][v])
        print('%s relu=%s bias=%s: %d of %d elements differ' % (shape, relu, with_bias, bad, got.numel()))
        total += bad
    assert total == 0


@pytest.mark.parametrize('shape', dc.SHAPES, ids=str)
def test_backward_equals_checker_and_repeats(shape):
    """grad_x, grad_weight and grad_bias `==` their checkers through autograd, with and without relu and bias; twice the same bits."""
    for v in ((True, True), (False, False)):
        r = dc.reference(shape)
        out, gx, gw, gb = _layer(shape, r, *v)
        bad = (gk.differing(out, r['out'][v]), gk.differing(gx, r['grad_x'][v]), gk.differing(gw, r['grad_weight'][v]), 0 if gb is None else gk.differing(gb, r['grad_bias'][v]))
        print('%s relu=%s bias=%s: differing elements of out, grad_x, grad_weight, grad_bias: %s' % ((shape,) + v + (bad,)))
        assert bad == (0, 0, 0, 0)
        again = _layer(shape, r, *v)
        assert all(a is None or gk.differing(a, gk.to_host(c)) == 0 for a, c in zip(again, (out, gx, gw, gb)))
    n, K, H, S = shape
    if n * H >= 64:
        g = dc.reference(shape)['g'][(True, True)]
        assert (g == 0).any() and (g != 0).any()


@pytest.mark.parametrize('layout', list(dc.LAYOUTS))
@pytest.mark.parametrize('shape', dc.SHAPES[:6], ids=str)
def test_margins_through_the_raw_abi(shape, layout):
    """Sentinel buffers with 64 guard floats either side; weight and grad_weight dense, as the ld = K + 3 view that starts 4 bytes
    past a 16-byte boundary, and as an aligned view: every result `==` its checker, the guards, the floats between the rows and the
    weights themselves untouched, the workspace NaN beforehand; each output NULL in turn; n == 0 writes nothing; null inputs,
    host memory and n out of range are refused."""
    import torch
    from red_gym_amd import _lib
    n, K, H, S = shape
    r = dc.reference(shape)
    x, b, go = gk.to_device(r['x']), gk.to_device(r['b']), gk.to_device(r['grad_out'])
    for v in ((True, True), (False, False)):
        relu, with_bias = v
        raw = _Raw(shape, layout, relu)
        wm = raw.weight(r['w'])
        out = raw.forward(x, wm, b if with_bias else None)
        assert gk.differing(out, r['out'][v]) == 0
        assert raw.forward(x, wm, None, 0).size == 0
        o = gk.to_device(r['out'][v]) if relu else None
        gx, gw, gb = raw.backward(x, o, go, wm)
        assert (gk.differing(gx, r['grad_x'][v]), gk.differing(gw, r['grad_weight'][v]), gk.differing(gb, r['grad_bias'][v])) == (0, 0, 0)
        for hole in range(3):
            want = tuple(i != hole for i in range(3))
            got = raw.backward(x, o, go, wm, want)
            for i, (a, name) in enumerate(zip(got, ('grad_x', 'grad_weight', 'grad_bias'))):
                assert (a is None) == (i == hole) and (a is None or gk.differing(a, r[name][v]) == 0)
    raw = _Raw(shape, layout, False)
    wm = raw.weight(r['w'])
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    keep = torch.empty(max(n * H, n * K, raw.dense.workspace_bytes(raw.cfg, n) // 4) + 8, device='cuda')
    ptrs = [x.data_ptr(), wm.ptr, keep.data_ptr()]
    for hole in range(3):
        a = [None if i == hole else p for i, p in enumerate(ptrs)]
        assert lib.f110_dense_forward(C.byref(raw.cfg), a[0], n, a[1], None, a[2], keep.data_ptr(), stream) == _lib.E_INVALID
    if raw.dense.workspace_bytes(raw.cfg, n):
        assert lib.f110_dense_forward(C.byref(raw.cfg), ptrs[0], n, ptrs[1], None, ptrs[2], None, stream) == _lib.E_INVALID
    host = np.zeros(H, np.float32)                                  # a bias in host memory is refused before any launch
    assert lib.f110_dense_forward(C.byref(raw.cfg), ptrs[0], n, ptrs[1], host.ctypes.data, ptrs[2], keep.data_ptr(), stream) == _lib.E_INVALID
    for bad_n in (-1, dc.MAX_ROWS + 1):
        assert lib.f110_dense_forward(C.byref(raw.cfg), ptrs[0], bad_n, ptrs[1], None, ptrs[2], keep.data_ptr(), stream) == _lib.E_INVALID
        assert lib.f110_dense_backward(C.byref(raw.cfg), ptrs[0], None, go.data_ptr(), bad_n, ptrs[1], keep.data_ptr(), None, None, stream) == _lib.E_INVALID
    assert lib.f110_dense_backward(C.byref(raw.cfg), ptrs[0], None, None, n, ptrs[1], keep.data_ptr(), None, None, stream) == _lib.E_INVALID
    assert lib.f110_dense_backward(C.byref(raw.cfg), ptrs[0], None, go.data_ptr(), n, None, keep.data_ptr(), None, None, stream) == _lib.E_INVALID
    assert lib.f110_dense_backward(C.byref(raw.cfg), None, None, go.data_ptr(), n, ptrs[1], None, keep.data_ptr(), None, stream) == _lib.E_INVALID
    relu_cfg = _Raw(shape, layout, True).cfg
    assert lib.f110_dense_backward(C.byref(relu_cfg), ptrs[0], None, go.data_ptr(), n, ptrs[1], keep.data_ptr(), None, None, stream) == _lib.E_INVALID


def test_a_row_does_not_depend_on_its_batch():
    """The property the layer exists for: one row alone, in a batch whose segments go through the workspace, and at another place
    in a batch that one workgroup walks adding in registers, gives the same bits -- forward and grad_x."""
    import torch
    from red_gym_amd.dense import linear_feat
    shape = (40, 100, 130, 36)
    n, K, H, S = shape
    r = dc.reference(shape)
    v = (True, True)
    w, b = gk.to_device(r['w']), gk.to_device(r['b'])
    big_n, at_small, at_big = 2753, 17, 2000
    assert [dc.paths(m, K, H, S)['path'] for m in (1, n, big_n)] == ['split', 'split', 'registers']
    big = dc.tensor((big_n, K), 77)
    big[at_big] = r['x'][at_small]
    big_go = dc.tensor((big_n, H), 78)
    big_go[at_big] = r['grad_out'][at_small]
    rows = []
    for xs, gos, at in ((r['x'][at_small:at_small + 1], r['grad_out'][at_small:at_small + 1], 0), (r['x'], r['grad_out'], at_small), (big, big_go, at_big)):
        x = gk.to_device(xs).requires_grad_()
        out = linear_feat(x, w, b, relu=True, segment=S)
        gx, = torch.autograd.grad(out, x, gk.to_device(gos))
        rows.append((gk.to_host(out)[at], gk.to_host(gx)[at]))
    for out, gx in rows:
        assert gk.differing(out, r['out'][v][at_small]) == 0 and gk.differing(gx, r['grad_x'][v][at_small]) == 0
    assert (r['out'][v][at_small] != 0).any() and (r['grad_x'][v][at_small] != 0).any()


def test_sal_shape_on_the_critics_view():
    """SAL's own fc1 once: (2, 25088, 512, 784) on the feature columns of a [512, 25104] matrix, forward and backward; the action
    columns of the weight and of the gradient are not touched.  grad_weight is compared on dc.SAL_COLS."""
    import torch
    from red_gym_amd import _lib, dense
    n, K, H, S = dc.SAL
    A = 16
    r = dc.reference(dc.SAL, cols=dc.SAL_COLS, variants=((True, True),))
    v = (True, True)
    full = torch.full((H, K + A), SENTINEL, device='cuda')
    full[:, :K] = gk.to_device(r['w'])
    gfull = torch.full((H, K + A), SENTINEL, device='cuda')
    cfg = dense.validate(K, H, K + A, S, True)
    x, b, go = gk.to_device(r['x']), gk.to_device(r['b']), gk.to_device(r['grad_out'])
    out = dense.forward_into(cfg, x, full.data_ptr(), b, torch.empty((n, H), device='cuda'))
    assert dense.workspace_bytes(cfg, n) == 32 * n * H * 4
    assert gk.differing(out, r['out'][v]) == 0
    gx, gb = torch.empty((n, K), device='cuda'), torch.empty((H,), device='cuda')
    dense.backward_into(cfg, x, out, go, full.data_ptr(), gx, gfull.data_ptr(), gb)
    assert gk.differing(gx, r['grad_x'][v]) == 0 and gk.differing(gb, r['grad_bias'][v]) == 0
    assert gk.differing(gk.to_host(gfull[:, :K])[:, dc.SAL_COLS], r['grad_weight'][v]) == 0
    assert bool((gfull[:, K:] == SENTINEL).all()) and bool((full[:, K:] == SENTINEL).all()) and not bool((gfull[:, :K] == SENTINEL).any())
    assert _lib.load().f110_dense_workspace(C.byref(cfg), 4096) == 0


def test_against_the_reference_actor():
    """fc1 of the reference's own Actor on the two recorded feature rows (tests/golden/g23_dense.npz): the GPU's pre-activation,
    grad_input, weight.grad on the recorded columns and bias.grad within the bounds of tests/test_dense_cpu.py's pin, and `==` the checker."""
    import torch
    from red_gym_amd.dense import linear_feat
    g, x, w, b = dc.golden_inputs()
    xd, wd, bd = gk.to_device(x).requires_grad_(), gk.to_device(w).requires_grad_(), gk.to_device(b).requires_grad_()
    pre = linear_feat(xd, wd, bd, relu=False)
    assert gk.differing(pre, dc.forward(x, w, b, dc.DEFAULT_SEGMENT, False)) == 0
    # the backward on the recording's own forward: relu's mask from the recorded pre-activation
    rec = gk.to_device(g['pre'])
    gm = torch.where(rec > 0, gk.to_device(g['cotangent']), torch.zeros_like(rec))
    pre.backward(gm)
    dc.golden_check(g, x, w, b, gk.to_host(pre), gk.to_host(xd.grad), gk.to_host(wd.grad)[:, g['cols']], gk.to_host(bd.grad))


def _critic_case(n, F, A, H, seed):
    import torch
    rng = np.random.default_rng([n, F, A, H, seed])
    fc1s, fc2s, feats = [], [], []
    for c in range(2):
        l1, l2 = torch.nn.Linear(F + A, H).cuda(), torch.nn.Linear(H, 1).cuda()
        with torch.no_grad():
            l1.weight.copy_(gk.to_device(dc.tensor((H, F + A), seed + c)))
            l1.bias.copy_(gk.to_device((0.5 * rng.normal(size=H)).astype(np.float32)))
            l2.weight.copy_(gk.to_device((rng.normal(size=(1, H)) / np.sqrt(H)).astype(np.float32)))
        fc1s.append(l1)
        fc2s.append(l2)
        feats.append(gk.to_device(dc.tensor((n, F), seed + 10 + c)).requires_grad_())
    action = gk.to_device(np.tanh(rng.normal(size=(n, A)))).requires_grad_()
    return feats, action, fc1s, fc2s


def test_twin_q_dense_equals_the_chained_checkers():
    """twin_q(dense=True), td_target and QHead: q, qmin, the target and every gradient `==` dense_cases' checker chained into
    qhead_cases' checker."""
    import torch
    from red_gym_amd.qhead import QHead, td_target, twin_q
    n, F, A, H, S = 17, 37, 3, 33, 8
    feats, action, fc1s, fc2s = _critic_case(n, F, A, H, 3)
    W = [gk.to_host(l.weight) for l in fc1s]
    inp = dict(pre=[dc.chains(gk.to_host(f), w[:, :F], S) for f, w in zip(feats, W)], w_act=[np.ascontiguousarray(w[:, F:]) for w in W],
               b1=[gk.to_host(l.bias) for l in fc1s], w2=[gk.to_host(l.weight).reshape(-1) for l in fc2s], b2=[gk.to_host(l.bias) for l in fc2s], action=gk.to_host(action),
               reward=np.linspace(-1.0, 1.0, n), done=(np.arange(n) % 3 == 0).astype(np.uint8), nlp=np.linspace(-5.0, 2.0, n))
    fwd = qh.forward(inp, target=True, gamma=0.99, alpha=0.2)
    rng = np.random.default_rng(5)
    cq, cm = rng.normal(size=(2, n)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    bwd = qh.backward(inp, fwd, cq, cm)
    q, qmin = twin_q(feats, action, fc1s, fc2s, dense=True, segment=S)
    assert gk.differing(q, fwd['q']) == 0 and gk.differing(qmin, fwd['qmin']) == 0
    ((q * gk.to_device(cq)).sum() + (qmin * gk.to_device(cm)).sum()).backward()
    for c in range(2):
        gw = gk.to_host(fc1s[c].weight.grad)
        assert gk.differing(np.ascontiguousarray(gw[:, :F]), dc.grad_weight(bwd['grad_pre'][c], gk.to_host(feats[c]))) == 0
        assert gk.differing(np.ascontiguousarray(gw[:, F:]), bwd['grad_w_act'][c]) == 0
        assert gk.differing(feats[c].grad, dc.grad_x(bwd['grad_pre'][c], W[c][:, :F])) == 0
        assert gk.differing(fc1s[c].bias.grad, bwd['grad_b1'][c]) == 0 and gk.differing(gk.to_host(fc2s[c].weight.grad).reshape(-1), bwd['grad_w2'][c]) == 0
        assert gk.differing(fc2s[c].bias.grad, bwd['grad_b2'][c]) == 0 and (gw[:, :F] != 0).any() and (gw[:, F:] != 0).any()
    assert np.array_equal(gk.to_host(action.grad), bwd['grad_action'].astype(np.float64))
    with torch.no_grad():
        tv = td_target(feats, action, gk.to_device(inp['nlp']), gk.to_device(inp['reward']), gk.to_device(inp['done']), fc1s, fc2s, 0.99, 0.2, dense=True, segment=S)
        assert gk.differing(tv, fwd['target']) == 0
        head = QHead.from_linears(fc1s[0], fc2s[0], dense=True, segment=S)
        assert gk.differing(head(feats[0], action)[:, 0], fwd['q'][0]) == 0
    with pytest.raises(ValueError):
        twin_q(feats, action, fc1s, fc2s, dense=True, segment=6)


def test_twin_q_dense_backward_allocates_no_more():
    """The backward's peak with dense=True is no more than with dense=False: still one [H, F + A] gradient per critic, its feature
    columns written in place with the row stride."""
    import torch
    from red_gym_amd.qhead import twin_q
    n, F, A, H = 64, 4096, 16, 512
    feats, action, fc1s, fc2s = _critic_case(n, F, A, H, 6)
    peaks = {}
    for dense in (False, True, False, True):
        for l in fc1s + fc2s:
            l.weight.grad = l.bias.grad = None
        for t in feats + [action]:
            t.grad = None
        q, qmin = twin_q(feats, action, fc1s, fc2s, dense=dense)
        loss = q.sum() + qmin.sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        peaks[dense] = torch.cuda.max_memory_allocated() - before
        assert all(bool((l.weight.grad[:, :F] != 0).any()) and bool((l.weight.grad[:, F:] != 0).any()) for l in fc1s)
    print('backward peak over the state before it: dense %.2f MB, default %.2f MB; one fc1 gradient is %.2f MB' % (
        peaks[True] / 1e6, peaks[False] / 1e6, H * (F + A) * 4 / 1e6))
    assert peaks[True] <= peaks[False]


def test_dense_module_shares_tensors_and_keys():
    import torch
    from red_gym_amd.dense import Dense, linear_feat
    torch.manual_seed(3)
    lin = torch.nn.Linear(100, 130).cuda()
    m = Dense.from_linear(lin, relu=True, segment=36)
    assert m.weight is lin.weight and m.bias is lin.bias and list(m.state_dict()) == ['weight', 'bias'] == list(lin.state_dict())
    fresh = Dense(100, 130, relu=True, segment=36).cuda()
    fresh.load_state_dict(lin.state_dict())
    lin2 = torch.nn.Linear(100, 130).cuda()
    lin2.load_state_dict(fresh.state_dict())
    x = gk.to_device(dc.tensor((40, 100), 4))
    want = dc.forward(gk.to_host(x), gk.to_host(lin.weight), gk.to_host(lin.bias), 36, True)
    assert gk.differing(m(x), want) == 0 and gk.differing(fresh(x), want) == 0 and torch.equal(lin2.weight, lin.weight)
    m(x).sum().backward()
    assert lin.weight.grad is not None and lin.bias.grad is not None
    nobias = Dense(8, 4, bias=False).cuda()
    assert nobias.bias is None and list(nobias.state_dict()) == ['weight'] and nobias(torch.ones(2, 8, device='cuda')).shape == (2, 4)
    w, b = lin.weight.detach(), lin.bias.detach()
    for args, kw in (((x.double(), w, b), {}), ((x, w.half(), b), {}), ((x, w, b.double()), {}), ((x[:, :50], w, b), {}), ((x, w[:, :50], b), {}),
                     ((x, w, b[:3]), {}), ((x, w.cpu(), b), {}), ((x, w, b.cpu()), {}), ((x.t(), w, b), {}), ((x[0], w, b), {}),
                     ((x, w.t().contiguous().t(), b), {}), ((x, w, b), dict(segment=6)), ((x, w, b), dict(segment=0)), ((x, w, b), dict(segment=4100))):
        with pytest.raises(ValueError):
            linear_feat(*args, **kw)
    with pytest.raises(ValueError):
        Dense.from_linear(torch.nn.Conv2d(1, 1, 1))
    with pytest.raises(ValueError):
        Dense(8, 5000)


def test_graph_replay():
    """linear_feat forward and backward captured in a torch.cuda.graph replay twice with the inputs refilled in place between the
    replays; each replay equals the eager result.  The shape takes the workspace path: its workspace lives in the graph's pool."""
    import torch
    from red_gym_amd.dense import linear_feat
    shape = (40, 100, 130, 36)
    fills = [dc.reference(shape, seed=s) for s in (0, 12)]
    w, b = gk.to_device(fills[0]['w']), gk.to_device(fills[0]['b'])
    v = (True, True)

    def run(x, go, wl, bl):
        out = linear_feat(x, wl, bl, relu=True, segment=shape[3])
        gx, gw, gb = torch.autograd.grad(out, (x, wl, bl), go)
        return out, gx, gw, gb

    eager = []
    for r in fills:
        eager.append([t.clone() for t in run(gk.to_device(r['x']).requires_grad_(), gk.to_device(r['grad_out']), w.clone().requires_grad_(), b.clone().requires_grad_())])
    assert gk.differing(eager[0][0], fills[0]['out'][v]) == 0 and gk.differing(eager[0][2], fills[0]['grad_weight'][v]) == 0
    assert not torch.equal(eager[0][0], eager[1][0])
    x, go = torch.zeros_like(gk.to_device(fills[0]['x'])).requires_grad_(), torch.zeros_like(gk.to_device(fills[0]['grad_out']))
    wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x, go, wl, bl)                                        # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(x, go, wl, bl)
    for r, want in zip(fills, eager):
        with torch.no_grad():
            x.copy_(gk.to_device(r['x']))
            go.copy_(gk.to_device(r['grad_out']))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(outs, want))
