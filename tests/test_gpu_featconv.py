"""The dense feature-map convolution on the GPU (csrc/f110_featconv.h): conv_feat forward, grad_x, grad_weight and grad_bias `==` the
checkers of tests/featconv_cases.py as raw 32-bit patterns at every shape-selected path (fc.paths), repeatability, batch
independence down to the per-sample partials in the workspace, the reference's own Actor (g22_trunk.npz, g22_trunk_unit.npz), margins through the raw
ABI, more work items than workgroups, the Trunk's two paths and its gradients chained through the checkers, and graph replay."""
import ctypes as C

import numpy as np
import pytest

import bitconv_cases as bc
import featconv_cases as fc
import gpu_checks as gk

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _conv(case, x, w, b, relu):
    from red_gym_amd.featconv import conv_feat
    return conv_feat(x, w, b, stride=case[5], relu=relu)


def _backward(case, r, relu, with_bias=True):
    """conv_feat forward and backward on leaves made from the reference's arrays -> (out, x.grad, w.grad, b.grad)."""
    x, w = gk.to_device(r['x']).requires_grad_(), gk.to_device(r['w']).requires_grad_()
    b = gk.to_device(r['b']).requires_grad_() if with_bias else None
    out = _conv(case, x, w, b, relu)
    out.backward(gk.to_device(r['grad_out']))
    return out, x.grad, w.grad, None if b is None else b.grad


@pytest.mark.parametrize('case', fc.CASES)
def test_forward_equals_checker(case):
    """`==` the checker as raw bit patterns on three samples under fc.VARIANTS (relu on and off, bias present and NULL)."""
    total = 0
    for relu, with_bias in fc.VARIANTS:
        r = fc.reference(case, 3, relu)
        want = fc.finish2(r['acc'], r['b'] if with_bias else None, relu)
        got = _conv(case, gk.to_device(r['x']), gk.to_device(r['w']), gk.to_device(r['b']) if with_bias else None, relu)
        assert got.grad_fn is None
        bad = gk.differing(got, want)
        print('%s relu=%s bias=%s: %d of %d elements differ' % (case, relu, with_bias, bad, want.size))
        total += bad
        if want[0].size >= 8:
            assert (want[0] != want[1]).any() and (want != 0).any()
    assert total == 0


@pytest.mark.parametrize('case', fc.CASES)
def test_backward_equals_checker_and_repeats(case):
    """grad_x, grad_weight and grad_bias `==` their checkers with and without ReLU on three samples; a second call gives the
    same bits; without a bias (another output, another mask) grad_x and grad_weight `==` the checkers again; with only the weight or
    only x requiring grad, that gradient stays the same."""
    import torch
    total = 0
    for relu in (True, False):
        r = fc.reference(case, 3, relu)
        out, gx, gw, gb = _backward(case, r, relu)
        bad = [gk.differing(out, r['out']), gk.differing(gx, r['grad_x']), gk.differing(gw, r['grad_weight']), gk.differing(gb, r['grad_bias'])]
        print('%s relu=%s: out, grad_x, grad_weight, grad_bias differ in %s elements' % (case, relu, bad))
        total += sum(bad)
        again = _backward(case, r, relu)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((out, gx, gw, gb), again))
        if not relu:
            assert (r['grad_x'] != 0).any() and (r['grad_weight'] != 0).any() and (r['grad_bias'] != 0).any()
    assert total == 0
    # without a bias the output changes, and with it the mask; grad_x and grad_weight follow the checkers, no grad_bias comes back
    r = fc.reference(case, 3, True)
    nb = fc.finish2(r['acc'], None, True)
    g = fc.masked(nb, r['grad_out'], True)
    out, gx, gw, gb = _backward(case, r, True, with_bias=False)
    assert gb is None and gk.differing(out, nb) == 0 and gk.differing(gx, fc.grad_x(g, r['w'], case[5], case[1], case[2])) == 0
    assert gk.differing(gw, fc.reduce(fc.partials(g, r['x'], case[4], case[5])[0])) == 0
    # only what needs_input_grad asks: weight alone, x alone
    w = gk.to_device(r['w']).requires_grad_()
    _conv(case, gk.to_device(r['x']), w, gk.to_device(r['b']), True).backward(gk.to_device(r['grad_out']))
    assert gk.differing(w.grad, r['grad_weight']) == 0
    x = gk.to_device(r['x']).requires_grad_()
    _conv(case, x, gk.to_device(r['w']), gk.to_device(r['b']), True).backward(gk.to_device(r['grad_out']))
    assert gk.differing(x.grad, r['grad_x']) == 0


@pytest.mark.parametrize('case', fc.GAP_CASES)
def test_grad_x_is_plus_zero_where_no_window_reaches(case):
    """kernel < stride: the input pixels between two windows (fc.holes) get no term; grad_x is +0 there as a bit pattern, through
    conv_feat and through the raw ABI into a buffer of sentinels, and not zero everywhere else; the whole array `==` the checker."""
    ci, h, wd, co, k, s = case
    unreached, inside = fc.holes(h, wd, k, s)
    assert inside.sum() > 0 and unreached.sum() >= inside.sum() and not unreached.all()
    r = fc.reference(case, 3, False)
    assert (bc.bit_patterns(r['grad_x'][:, :, unreached]) == 0).all() and (r['grad_x'][:, :, ~unreached] != 0).any()
    _, gx, _, _ = _backward(case, r, False)
    raw = _Raw(case, False)
    gx_raw = raw.backward(gk.to_device(r['x']), None, gk.to_device(r['grad_out']), gk.to_device(r['w']), 3, want=(True, False, False), with_ws=False)[0].reshape(r['x'].shape)
    for got in (gk.to_host(gx), gx_raw):
        assert int((bc.bit_patterns(got[:, :, inside]) != 0).sum()) == 0 and int((bc.bit_patterns(got[:, :, unreached]) != 0).sum()) == 0
        assert gk.differing(got, r['grad_x']) == 0


class _Raw:
    """The two entry points themselves on buffers of SENTINEL with 64 guard floats either side of every output."""

    def __init__(self, case, relu):
        from red_gym_amd import _lib, featconv
        self.lib, self._lib = _lib.load(), _lib
        ci, h, w, co, k, s = case
        self.case, self.cfg = case, featconv.make_config(ci, h, w, co, k, s, relu)
        self.oh, self.ow = fc.out_size(h, w, k, s)

    def forward(self, x, w, b, n):
        import torch
        ci, h, wd, co, k, s = self.case
        size = n * co * self.oh * self.ow
        buf = gk.Guarded(size, fill=SENTINEL)
        self._lib.check(self.lib.f110_featconv_forward(C.byref(self.cfg), x.data_ptr(), n, w.data_ptr(), self._lib.ptr(b), buf.ptr,
                                                       torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return buf.read().reshape(n, co, self.oh, self.ow)

    def backward(self, x, out, go, w, n, want=(True, True, True), with_ws=True):
        """-> (grad_x, grad_weight, grad_bias, workspace) on the host, None for an output passed as NULL."""
        import torch
        ci, h, wd, co, k, s = self.case
        sizes = (n * ci * h * wd, co * ci * k * k, co, n * co * (ci * k * k + 1))
        bufs = [gk.Guarded(z, fill=SENTINEL) if on else None for z, on in zip(sizes, tuple(want) + (with_ws,))]
        ptrs = [None if t is None else t.ptr for t in bufs]
        rc_ = self.lib.f110_featconv_backward(C.byref(self.cfg), self._lib.ptr(x), self._lib.ptr(out), self._lib.ptr(go), n, self._lib.ptr(w), ptrs[0], ptrs[1], ptrs[2],
                                              ptrs[3], torch.cuda.current_stream().cuda_stream)
        self._lib.check(rc_)
        torch.cuda.synchronize()
        return [None if t is None else t.read() for t in bufs]


@pytest.mark.parametrize('case', (fc.CONV3, fc.CASES[2], fc.CASES[6]))
def test_batch_independence(case):
    """Samples 0..1 alone equal samples 0..1 inside a batch of 3: the forward and grad_x through conv_feat, the per-sample partials P
    read back from the workspace through the raw ABI, where they also `==` the checker's."""
    import torch
    ci, h, wd, co, k, s = case
    r = fc.reference(case, 3, True)
    x, w, b, go = (gk.to_device(r[key]) for key in ('x', 'w', 'b', 'grad_out'))
    full = _backward(case, r, True)
    two = {key: r[key][:2] for key in ('x', 'grad_out')}
    two.update(w=r['w'], b=r['b'])
    part = _backward(case, two, True)
    assert torch.equal(full[0][:2], part[0]) and torch.equal(full[1][:2], part[1]) and not torch.equal(full[0][0], full[0][2])
    raw = _Raw(case, True)
    out = raw.forward(x, w, b, 3)
    assert gk.differing(out, r['out']) == 0
    row = co * (ci * k * k + 1)
    ws3 = raw.backward(x, gk.to_device(out), go, w, 3)[3].reshape(3, row)
    ws2 = raw.backward(x[:2].contiguous(), gk.to_device(out[:2]), go[:2].contiguous(), w, 2)[3].reshape(2, row)
    assert np.array_equal(bc.bit_patterns(ws3[:2]), bc.bit_patterns(ws2))
    assert gk.differing(ws3[:, :co * ci * k * k].reshape(r['P'].shape), r['P']) == 0 and gk.differing(ws3[:, co * ci * k * k:], r['B']) == 0
    assert (ws3[0] != ws3[2]).any()


@pytest.mark.parametrize('fixture', fc.GOLDEN)
def test_against_the_reference_actor(golden, fixture):
    """conv2 and conv3 through the raw ABI on the inputs the reference's Actor recorded (the raw 0 / 255 row, the / 255 row), its own `out` as the mask
    of the backward: every array within 2 * gamma * mag of the recording."""
    g = golden(fixture)
    rows = int(g['a1'].shape[0])
    for name, xin, s, go in fc.golden_layers(g):
        w, b, out = g[name + '_weight'], g[name + '_bias'], g[name + '_out']
        co, ci, k, _ = w.shape
        case = (ci, xin.shape[2], xin.shape[3], co, k, s)
        raw = _Raw(case, True)
        got = raw.forward(gk.to_device(xin), gk.to_device(w), gk.to_device(b), rows)

        def within(what, v, ref, mag, terms):
            err, bound = np.abs(v.astype(np.float64) - ref.astype(np.float64)), 2.0 * fc.gamma(terms) * mag
            print('%s %s: worst error / bound %.4f' % (name, what, float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all(), (name, what)

        within('out', got, out, fc.forward_fp64(xin, w, b, s)[1], ci * k * k + 1)
        gm = fc.masked(out, go, True)
        gx, gw, gb, _ = raw.backward(gk.to_device(xin), gk.to_device(out), gk.to_device(go), gk.to_device(w), rows)
        within('grad_input', gx.reshape(xin.shape), g[name + '_grad_input'], fc.grad_x_fp64(gm, w, s, xin.shape[2], xin.shape[3])[1], co * (-(-k // s)) ** 2)
        _, mw, _, mb = fc.grad_w_fp64(gm, xin, k, s)
        pixels = rows * out.shape[2] * out.shape[3]
        within('weight.grad', gw.reshape(w.shape), g[name + '_weight_grad'], mw, pixels)
        within('bias.grad', gb, g[name + '_bias_grad'], mb, pixels)


@pytest.mark.parametrize('case', fc.CASES)
def test_margins_through_the_raw_abi(case):
    """The guards around out, grad_x, grad_weight, grad_bias and the workspace stay as they were and no element between them keeps
    the sentinel; an output passed as NULL is skipped (without parameter gradients the workspace may be NULL and is not touched);
    n == 0 writes nothing; null inputs are refused."""
    import torch
    from red_gym_amd import _lib
    ci, h, wd, co, k, s = case
    r = fc.reference(case, 3, False)
    x, w, b, go = (gk.to_device(r[key]) for key in ('x', 'w', 'b', 'grad_out'))
    raw = _Raw(case, False)
    out = raw.forward(x, w, b, 3)
    assert (r['out'] != SENTINEL).all() and gk.differing(out, r['out']) == 0
    assert raw.forward(x, w, b, 0).size == 0
    gx, gw, gb, ws = raw.backward(x, None, go, w, 3)
    assert gk.differing(gx.reshape(r['x'].shape), r['grad_x']) == 0 and gk.differing(gw.reshape(r['w'].shape), r['grad_weight']) == 0
    assert gk.differing(gb, r['grad_bias']) == 0 and (ws != SENTINEL).all()
    gx, gw, gb, ws = raw.backward(x, None, go, w, 3, want=(True, False, False), with_ws=False)
    assert gw is None and gb is None and ws is None and gk.differing(gx.reshape(r['x'].shape), r['grad_x']) == 0
    gx, gw, gb, ws = raw.backward(x, None, go, None, 3, want=(False, True, False))
    assert gx is None and gb is None and gk.differing(gw.reshape(r['w'].shape), r['grad_weight']) == 0
    gx, gw, gb, ws = raw.backward(x, None, go, None, 3, want=(False, False, True))
    assert gx is None and gw is None and gk.differing(gb, r['grad_bias']) == 0
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    ptrs = [x.data_ptr(), w.data_ptr(), gk.to_device(out).data_ptr()]
    for hole in range(3):
        a = [None if i == hole else p for i, p in enumerate(ptrs)]
        assert lib.f110_featconv_forward(C.byref(raw.cfg), a[0], 3, a[1], None, a[2], stream) == _lib.E_INVALID
    host_bias = np.zeros(co, np.float32)                          # a bias in host memory is refused before any launch
    assert lib.f110_featconv_forward(C.byref(raw.cfg), ptrs[0], 3, ptrs[1], host_bias.ctypes.data, ptrs[2], stream) == _lib.E_INVALID
    keep = torch.empty(co * (ci * k * k + 1) * 3 + 8, device='cuda')
    assert lib.f110_featconv_backward(C.byref(raw.cfg), x.data_ptr(), None, None, 3, w.data_ptr(), keep.data_ptr(), None, None, None, stream) == _lib.E_INVALID
    assert lib.f110_featconv_backward(C.byref(raw.cfg), x.data_ptr(), None, go.data_ptr(), 3, w.data_ptr(), None, keep.data_ptr(), None, None, stream) == _lib.E_INVALID
    assert lib.f110_featconv_backward(C.byref(raw.cfg), x.data_ptr(), None, go.data_ptr(), 3, None, keep.data_ptr(), None, None, None, stream) == _lib.E_INVALID
    relu_cfg = _Raw(case, True).cfg
    assert lib.f110_featconv_backward(C.byref(relu_cfg), x.data_ptr(), None, go.data_ptr(), 3, w.data_ptr(), keep.data_ptr(), None, None, None, stream) == _lib.E_INVALID
    assert lib.f110_featconv_backward(C.byref(raw.cfg), x.data_ptr(), None, go.data_ptr(), -1, w.data_ptr(), keep.data_ptr(), None, None, None, stream) == _lib.E_INVALID


def test_more_items_than_workgroups():
    """fc.LOOP_N samples of a tiny shape on fc.FC_MAX_GRID workgroups: each walks two or three in the forward, in grad_x and in the
    partials; every result `==` its checker, the reduction over 4 101 partials included."""
    case, n = fc.LOOP_CASE, fc.LOOP_N
    r = fc.reference(case, n, True)
    out, gx, gw, gb = _backward(case, r, True)
    assert (gk.differing(out, r['out']), gk.differing(gx, r['grad_x']), gk.differing(gw, r['grad_weight']), gk.differing(gb, r['grad_bias'])) == (0, 0, 0, 0)
    assert (r['out'][-1] != r['out'][0]).any() and (r['grad_x'][-1] != 0).any()


def test_refuses_mismatched_tensors():
    import torch
    from red_gym_amd.featconv import conv_feat
    x, w, b = torch.zeros(2, 32, 30, 30, device='cuda'), torch.zeros(32, 32, 3, 3, device='cuda'), torch.zeros(32, device='cuda')
    conv_feat(x, w, b)
    for args, kw in (((x.double(), w, b), {}), ((x, w.half(), b), {}), ((x, w, b.double()), {}), ((x[:, :16], w, b), {}), ((x, w[:, :, :, :2], b), {}),
                     ((x, w, b[:3]), {}), ((x, w.cpu(), b), {}), ((x, w, b.cpu()), {}), ((x.permute(0, 1, 3, 2), w, b), {}), ((x[0], w, b), {}),
                     ((x, w.permute(0, 1, 3, 2), b), {}), ((x, w, b), dict(stride=5)), ((x, w, b), dict(stride=0)),
                     ((torch.zeros(2, 32, 30, 65, device='cuda'), w, b), {}), ((torch.zeros(2, 32, 2, 30, device='cuda'), w, b), {})):
        with pytest.raises(ValueError):
            conv_feat(*args, **kw)


def _trunk_checker(imgs, host, on, cot):
    """The three layers and their backward, checker by checker -> (features, grads of conv2 and conv3's weight and bias, the
    gradient that arrives at conv1's output)."""
    w1, b1, w2, bb2, w3, bb3 = host
    a1 = bc.forward(imgs, w1, b1, 4, on, True)
    a2 = fc.forward(a1, w2, bb2, 2, True)
    a3 = fc.forward(a2, w3, bb3, 1, True)
    g3 = fc.masked(a3, cot.reshape(a3.shape), True)
    P3, B3 = fc.partials(g3, a2, 3, 1)
    g2 = fc.masked(a2, fc.grad_x(g3, w3, 1, a2.shape[2], a2.shape[3]), True)
    P2, B2 = fc.partials(g2, a1, 4, 2)
    return a3.reshape(a3.shape[0], -1), (fc.reduce(P2), fc.reduce(B2), fc.reduce(P3), fc.reduce(B3)), fc.grad_x(g2, w2, 2, a1.shape[2], a1.shape[3])


def test_trunk_acts_and_learns_on_the_same_bits():
    """Trunk.from_convs shares the six tensors and loads a reference-keyed state dict; the no-grad path and the learning path are
    torch.equal on uint8 bitmaps and on ring frames with an index, and `==` the checkers; backward() reaches all six parameters
    with the checkers' gradients chained layer by layer (conv1's from conv_bits' own backward fed the checker's gradient)."""
    import torch
    from red_gym_amd.bitconv import conv_bits
    from red_gym_amd.featconv import Trunk
    torch.manual_seed(7)
    nn = torch.nn
    c1, c2, c3 = nn.Conv2d(1, 16, 8, 4).cuda(), nn.Conv2d(16, 32, 4, 2).cuda(), nn.Conv2d(32, 32, 3, 1).cuda()
    on = 255.0
    trunk = Trunk.from_convs(c1, c2, c3, on=on, cols=256)
    theirs = (c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias)
    mine = (trunk.conv1.weight, trunk.conv1.bias, trunk.conv2.weight, trunk.conv2.bias, trunk.conv3.weight, trunk.conv3.bias)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(mine, theirs))
    keys = ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias']
    assert list(trunk.state_dict()) == keys
    fresh = Trunk(on=on, cols=256).cuda()
    fresh.load_state_dict(dict(zip(keys, theirs)))
    imgs = np.kron(np.random.default_rng(7).random((2, 32, 32)) < 0.5, np.ones((8, 8), bool)).astype(np.uint8) * 255
    packed = gk.packed(imgs)
    index = gk.to_device(np.array([1, -1, 0, 1], np.int64))
    with torch.no_grad():
        act, act_ring = trunk(gk.to_device(imgs)), fresh(packed, index=index)
    learn, learn_ring = trunk(gk.to_device(imgs)), fresh(packed, index=index)
    assert act.grad_fn is None and learn.grad_fn is not None and act.shape == (2, 32 * 28 * 28) and act_ring.shape == (4, 32 * 28 * 28)
    assert torch.equal(act.view(torch.int32), learn.view(torch.int32)) and torch.equal(act_ring.view(torch.int32), learn_ring.view(torch.int32))
    assert torch.equal(act_ring[0], act[1]) and torch.equal(act_ring[2], act[0]) and not torch.equal(act[0], act[1]) and bool((act_ring[1] != act_ring[0]).any())
    host = tuple(gk.to_host(p) for p in theirs)
    cot = fc.tensor(tuple(act.shape), 9)
    feats, grads, g_a1 = _trunk_checker(imgs, host, on, cot)
    assert gk.differing(act, feats) == 0 and (feats > 0).any()
    learn.backward(gk.to_device(cot))
    for name, p, want in zip(keys[2:], theirs[2:], grads):
        assert p.grad is not None and (want != 0).any()
        assert gk.differing(p.grad, want.reshape(p.shape)) == 0, name
    leaves = [p.detach().clone().requires_grad_() for p in theirs[:2]]
    conv_bits(gk.to_device(imgs), leaves[0], leaves[1], stride=4, on=on, relu=True).backward(gk.to_device(g_a1))
    assert torch.equal(c1.weight.grad, leaves[0].grad) and torch.equal(c1.bias.grad, leaves[1].grad) and bool((c1.weight.grad != 0).any())
    # frozen parameters take the acting path even with grad enabled
    for p in theirs:
        p.requires_grad_(False)
    frozen = trunk(gk.to_device(imgs))
    assert frozen.grad_fn is None and torch.equal(frozen, act)


def test_graph_replay():
    """conv_feat forward and backward captured in a torch.cuda.graph replay twice with the inputs refilled in place between the
    replays; each replay equals the eager result."""
    import torch
    case = fc.CASES[2]
    fills = [fc.reference(case, 3, True, seed=s) for s in (11, 12)]
    w, b = gk.to_device(fills[0]['w']), gk.to_device(fills[0]['b'])

    def run(x, go, wl, bl):
        out = _conv(case, x, wl, bl, True)
        gx, gw, gb = torch.autograd.grad(out, (x, wl, bl), go)
        return out, gx, gw, gb

    eager = []
    for r in fills:
        eager.append([t.clone() for t in run(gk.to_device(r['x']).requires_grad_(), gk.to_device(r['grad_out']), w.clone().requires_grad_(), b.clone().requires_grad_())])
    assert gk.differing(eager[0][0], fills[0]['out']) == 0 and gk.differing(eager[0][2], fills[0]['grad_weight']) == 0
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
