"""The parameter update on the GPU (csrc/f110_adam.h, red_gym_amd/optim.py): params, moments, targets and the device state `==` the
checker of tests/optim_cases.py as raw bit patterns at every size-selected path, on misaligned views between canaries, with more
tensors than one launch holds, with a missing gradient, for soft_update alone, through a captured graph, across a state_dict
exchange with torch.optim.Adam in both directions and on SAL's critic; and as close to fp64 Adam as torch's own fp32 Adam is."""
import numpy as np
import pytest

import gpu_checks as gk
import optim_cases as oc

pytestmark = pytest.mark.gpu

CANARY = -7.0                                 # fill around every view: no result of these inputs equals it


def _state_words(opt):
    return gk.to_host(opt._state)


_cache = {}


def _sizes_case():
    """Parameters, targets and 20 steps of gradients for oc.SIZES, and the checker's results after 5 steps with and without targets:
    computed once, left unchanged."""
    if 'sizes' not in _cache:
        rng = np.random.default_rng(1)
        params = [oc.values(rng, n) for n in oc.SIZES]
        targets = [oc.values(rng, n) for n in oc.SIZES]
        grads = [[oc.gradients(rng, n) for n in oc.SIZES] for _ in range(20)]
        ref = {False: oc.run(params, grads[:5]), True: oc.run(params, grads[:5], targets)}
        for a in params + targets + [g for gs in grads for g in gs]:
            a.setflags(write=False)
        _cache['sizes'] = (params, targets, grads, ref)
    return _cache['sizes']


def _run(opt, params, grads):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = None if g is None else gk.to_device(g)
        opt.step()


def _assert_equal(opt, params, targets, want):
    ps, ms, vs, ts, state = want
    for i, p in enumerate(params):
        m, v = opt.moments(i)
        assert gk.same(p, ps[i]), ('p', i)
        assert gk.same(m, ms[i]), ('m', i)
        assert gk.same(v, vs[i]), ('v', i)
        if targets is not None:
            assert gk.same(targets[i], ts[i]), ('target', i)
    assert np.array_equal(_state_words(opt), oc.state_words(state)), (_state_words(opt), oc.state_words(state))


@pytest.mark.parametrize('with_targets', [False, True])
def test_every_size_equals_the_checker(with_targets):
    """One tensor each of 1 .. 2 CHUNK + 3 elements and an empty one, 5 steps with fresh gradients: p, m, v, the targets and the device
    state `==` the checker."""
    from red_gym_amd.optim import SacAdam
    p0, t0, grads, ref = _sizes_case()
    params = [gk.to_device(p) for p in p0]
    targets = [gk.to_device(t) for t in t0] if with_targets else None
    opt = SacAdam(params, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, targets=targets, tau=oc.TAU)
    assert opt.device_state()[:3] == (0, 1.0, 1.0)
    _run(opt, params, grads[:5])
    _assert_equal(opt, params, targets, ref[with_targets])
    assert opt.device_state()[0] == 5
    if not with_targets:
        opt.zero_grad()
        assert all(p.grad is None for p in params)


@pytest.mark.parametrize('which', ['p', 'g', 'target', 'all'])
def test_misaligned_views_between_canaries(which):
    """p, g and the target in turn, and together, a view at element offset 1, 2, 3 of a larger buffer of canaries (so the tensor takes
    the 4-byte path), for 5 and CHUNK + 1 elements, two steps: the results `==` the checker and every canary is unchanged."""
    from red_gym_amd.optim import SacAdam
    rng = np.random.default_rng(2)
    for n in oc.MISALIGNED_SIZES:
        p0, t0 = oc.values(rng, n), oc.values(rng, n)
        grads = [[oc.gradients(rng, n)] for _ in range(2)]
        want = oc.run([p0], grads, [t0])
        for off in ((0, 1, 2, 3) if which == 'all' else (1, 2, 3)):
            offs = {k: off if which in (k, 'all') else 0 for k in ('p', 'g', 'target')}
            bufs = {k: gk.Guarded(n, off=offs[k], fill=CANARY) for k in offs}
            view = {k: bufs[k].data for k in offs}
            assert all(view[k].data_ptr() % 16 == 4 * offs[k] for k in offs)
            view['p'].copy_(gk.to_device(p0))
            view['target'].copy_(gk.to_device(t0))
            opt = SacAdam([view['p']], lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, targets=[view['target']], tau=oc.TAU)
            for gs in grads:
                view['g'].copy_(gk.to_device(gs[0]))
                view['p'].grad = view['g']
                opt.step()
            _assert_equal(opt, [view['p']], [view['target']], want)
            assert gk.same(view['g'], grads[-1][0])
            for k in offs:
                bufs[k].read()


def test_more_tensors_than_one_launch_holds():
    """MAX_TENSORS + 3 tensors of 1 .. 7 elements with targets, two steps: `==` the checker, and the state advanced by exactly 2 (the
    second launch of a step reads the state the first one's advance left)."""
    from red_gym_amd.optim import SacAdam
    rng = np.random.default_rng(3)
    sizes = [1 + i % 7 for i in range(oc.MAX_TENSORS + 3)]
    p0, t0 = [oc.values(rng, n) for n in sizes], [oc.values(rng, n) for n in sizes]
    grads = [[oc.values(rng, n, 3.0) for n in sizes] for _ in range(2)]
    params, targets = [gk.to_device(p) for p in p0], [gk.to_device(t) for t in t0]
    opt = SacAdam(params, targets=targets)
    _run(opt, params, grads)
    want = oc.run(p0, grads, t0)
    _assert_equal(opt, params, targets, want)
    t, pow1, pow2, _, _ = opt.device_state()
    assert (t, pow1, pow2) == (2, 0.9 * 0.9, 0.999 * 0.999)


def test_a_missing_gradient_leaves_the_parameter_and_moves_its_target():
    from red_gym_amd.optim import SacAdam
    rng = np.random.default_rng(4)
    sizes = [65, 300, oc.CHUNK + 1, 7]
    p0, t0 = [oc.values(rng, n) for n in sizes], [oc.values(rng, n) for n in sizes]
    grads = [[oc.gradients(rng, n) for n in sizes] for _ in range(3)]
    grads[1][1] = grads[2][1] = None                                     # parameter 1 has a gradient at the first step only
    params, targets = [gk.to_device(p) for p in p0], [gk.to_device(t) for t in t0]
    opt = SacAdam(params, targets=targets)
    _run(opt, params, grads[:1])
    after_first = [x.clone() for x in (params[1],) + opt.moments(1)]
    target_first = targets[1].clone()
    _run(opt, params, grads[1:])
    for got, was in zip((params[1],) + opt.moments(1), after_first):
        assert gk.same(got, gk.to_host(was))
    assert not gk.same(targets[1], gk.to_host(target_first))
    _assert_equal(opt, params, targets, oc.run(p0, grads, t0))
    # no gradient anywhere: nothing is stepped, the counter stands, the targets still move
    before = [t.clone() for t in targets]
    _run(opt, params, [[None] * len(sizes)])
    assert opt.device_state()[0] == 3
    for i, t in enumerate(targets):
        assert gk.same(t, oc.lerp(gk.to_host(before[i]), gk.to_host(params[i])))


def test_soft_update_alone():
    from red_gym_amd.optim import soft_update
    p0, t0, _, _ = _sizes_case()
    sources, targets = [gk.to_device(p) for p in p0], [gk.to_device(t) for t in t0]
    soft_update(targets, sources, oc.TAU)
    for i in range(len(p0)):
        assert gk.same(targets[i], oc.lerp(t0[i], p0[i])), i
        assert gk.same(sources[i], p0[i]), i
    soft_update(targets, sources, 0.0)
    assert all(gk.same(targets[i], oc.lerp(t0[i], p0[i])) for i in range(len(p0)))
    with pytest.raises(ValueError, match='tau'):
        soft_update(targets, sources, 1.5)


def test_refusals_on_device_tensors():
    import torch
    from red_gym_amd.optim import SacAdam, soft_update
    a, b = torch.zeros((8, 8), device='cuda'), torch.zeros((8, 8), device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        SacAdam([a.t()])
    with pytest.raises(ValueError, match='alias'):
        SacAdam([a, a[2:4]])
    with pytest.raises(ValueError, match='alias'):
        SacAdam([a], targets=[a])
    with pytest.raises(ValueError, match='alias'):
        soft_update([a], [a.view(64)[0:64].view(8, 8)], 0.005)
    with pytest.raises(ValueError, match='1 targets for 2'):
        SacAdam([a, b], targets=[torch.zeros((8, 8), device='cuda')])
    with pytest.raises(ValueError, match='shape'):
        SacAdam([a], targets=[torch.zeros((8, 4), device='cuda')])
    with pytest.raises(ValueError, match='CPU'):
        SacAdam([a], targets=[torch.zeros((8, 8))])
    with pytest.raises(ValueError, match='float32'):
        SacAdam([a.double()])
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(tau=2.0, targets=[b]), dict(lr=float('inf'))):
        with pytest.raises(ValueError):
            SacAdam([a], **kw)
    opt = SacAdam([a])
    a.grad = torch.ones((8, 8), device='cuda').t()
    with pytest.raises(ValueError, match='gradient'):
        opt.step()
    a.grad = torch.ones((8, 8), device='cuda')
    opt.lr = float('nan')
    with pytest.raises(ValueError, match='lr'):
        opt.step()
    assert opt.device_state()[0] == 0 and not a.any()


def test_captured_step_replays():
    """step() captured once on a side stream (a linear chain: the advance, then the update) and replayed 3 times with the gradients
    rewritten in place between replays: params, moments, targets and t are bitwise those of 3 eager steps."""
    import torch
    from red_gym_amd.optim import SacAdam
    rng = np.random.default_rng(6)
    sizes = [3, 257, oc.CHUNK + 1, 2 * oc.CHUNK + 3]
    p0, t0 = [oc.values(rng, n) for n in sizes], [oc.values(rng, n) for n in sizes]
    grads = [[oc.gradients(rng, n) for n in sizes] for _ in range(3)]
    eager_p, eager_t = [gk.to_device(p) for p in p0], [gk.to_device(t) for t in t0]
    eager = SacAdam(eager_p, targets=eager_t)
    _run(eager, eager_p, grads)                                          # (also the warm-up: the kernels are loaded before the capture)
    params, targets = [gk.to_device(p) for p in p0], [gk.to_device(t) for t in t0]
    static = [torch.zeros_like(p) for p in params]
    for p, g in zip(params, static):
        p.grad = g
    opt = SacAdam(params, targets=targets)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert opt.device_state()[0] == 0 and all(gk.same(p, p0[i]) for i, p in enumerate(params))    # capturing runs nothing
    for gs in grads:
        for g, new in zip(static, gs):
            g.copy_(gk.to_device(new))
        graph.replay()
    torch.cuda.synchronize()
    for i in range(len(sizes)):
        assert torch.equal(params[i], eager_p[i]) and torch.equal(targets[i], eager_t[i]), i
        assert all(torch.equal(a, b) for a, b in zip(opt.moments(i), eager.moments(i))), i
    assert np.array_equal(_state_words(opt), _state_words(eager)) and opt.device_state()[0] == 3
    _assert_equal(opt, params, targets, oc.run(p0, grads, t0))


def test_state_dict_interchange_with_torch_adam():
    """Three steps of torch.optim.Adam on the GPU, SacAdam.load_state_dict(its state), two steps: `==` the checker started from that
    state (the powers beta ** 3 computed on the host).  SacAdam.state_dict() loads into a fresh torch.optim.Adam, which steps on;
    unequal step counts are refused."""
    import torch
    from red_gym_amd.optim import SacAdam
    rng = np.random.default_rng(7)
    sizes = [5, 257, oc.CHUNK + 1]
    grads = [[oc.gradients(rng, n) for n in sizes] for _ in range(6)]
    params = [gk.to_device(oc.values(rng, n)) for n in sizes]
    adam = torch.optim.Adam(params, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS)
    for gs in grads[:3]:
        for p, g in zip(params, gs):
            p.grad = gk.to_device(g)
        adam.step()
    sd = adam.state_dict()
    p3 = [gk.to_host(p).copy() for p in params]
    moments = ([gk.to_host(sd['state'][i]['exp_avg']).copy() for i in range(3)], [gk.to_host(sd['state'][i]['exp_avg_sq']).copy() for i in range(3)])
    opt = SacAdam(params, lr=1.0, betas=(0.5, 0.5), eps=1.0)            # (every hyperparameter comes from the state_dict)
    opt.load_state_dict(sd)
    assert (opt.lr, opt.betas, opt.eps) == (oc.LR, oc.BETAS, oc.EPS)
    assert opt.device_state()[:3] == (3, 0.9 ** 3, 0.999 ** 3)
    _run(opt, params, grads[3:5])
    want = oc.run(p3, grads[3:5], state=oc.new_state(oc.BETAS, 3), moments=moments)
    _assert_equal(opt, params, None, want)
    # and back
    out = opt.state_dict()
    assert sorted(out['state']) == [0, 1, 2] and all(float(out['state'][i]['step']) == 5.0 for i in range(3))
    assert set(out['param_groups'][0]) == set(sd['param_groups'][0]) and out['param_groups'][0]['params'] == [0, 1, 2]
    fresh = torch.optim.Adam(params, lr=1.0)
    fresh.load_state_dict(out)
    assert fresh.param_groups[0]['lr'] == oc.LR and tuple(fresh.param_groups[0]['betas']) == oc.BETAS
    assert all(torch.equal(fresh.state[p]['exp_avg'], opt.moments(i)[0]) for i, p in enumerate(params))
    for p, g in zip(params, grads[5]):
        p.grad = gk.to_device(g)
    before = [p.clone() for p in params]
    fresh.step()
    assert all(float(fresh.state[p]['step']) == 6.0 for p in params) and all(not torch.equal(p, b) for p, b in zip(params, before))
    assert all(bool(torch.isfinite(p).all()) for p in params)
    # SacAdam -> SacAdam, and the refusal of unequal steps
    out = opt.state_dict()                                               # (torch's load_state_dict kept the step tensors and stepped them)
    again = SacAdam(params)
    again.load_state_dict(out)
    assert np.array_equal(_state_words(again)[:3], oc.state_words(oc.new_state(oc.BETAS, 5))[:3])
    assert SacAdam(params).state_dict()['state'] == {}
    out['state'][1]['step'] = torch.tensor(4.0)
    with pytest.raises(ValueError, match='step'):
        again.load_state_dict(out)


def test_sal_critic_once():
    """A critic's ten tensors (fc1.weight [512, 25104]: 12.87 M parameters, 3 143 chunks) with targets, one step: `==` the checker."""
    from red_gym_amd.optim import SacAdam
    rng = np.random.default_rng(8)
    ns = [int(np.prod(s)) for s in oc.SAL_CRITIC]
    assert sum(ns) == 12872785
    p0 = [oc.values(rng, n, 0.05) for n in ns]
    t0 = [p + oc.values(rng, n, 0.001) for p, n in zip(p0, ns)]
    grads = [[oc.values(rng, n, 0.01) for n in ns]]
    params = [gk.to_device(p).view(s) for p, s in zip(p0, oc.SAL_CRITIC)]
    targets = [gk.to_device(t).view(s) for t, s in zip(t0, oc.SAL_CRITIC)]
    opt = SacAdam(params, targets=targets)
    for p, g, s in zip(params, grads[0], oc.SAL_CRITIC):
        p.grad = gk.to_device(g).view(s)
    opt.step()
    ps, ms, vs, ts, state = oc.run(p0, grads, t0)
    for i, s in enumerate(oc.SAL_CRITIC):
        m, v = opt.moments(i)
        assert gk.same(params[i], ps[i].reshape(s)) and gk.same(m, ms[i].reshape(s)) and gk.same(v, vs[i].reshape(s)), i
        assert gk.same(targets[i], ts[i].reshape(s)), i
    assert np.array_equal(_state_words(opt), oc.state_words(state))


def test_as_close_to_fp64_adam_as_torch_on_the_gpu():
    """20 steps on the first case's tensors against torch.optim.Adam(foreach=False) on the GPU: per element |SacAdam - p64| <= 2
    max|torch32 - p64| + 1 ulp32(p64), the condition test_optim_cpu puts on the checker."""
    import torch
    from red_gym_amd.optim import SacAdam
    p0, _, grads, _ = _sizes_case()
    want = oc.adam64(p0, grads)
    ours, theirs = [gk.to_device(p) for p in p0], [gk.to_device(p) for p in p0]
    opt = SacAdam(ours, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS)
    ref = torch.optim.Adam(theirs, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, foreach=False)
    for gs in grads:
        for a, b, g in zip(ours, theirs, gs):
            a.grad = gk.to_device(g)
            b.grad = gk.to_device(g)
        opt.step()
        ref.step()
    for i, n in enumerate(oc.SIZES):
        if n == 0:
            continue
        e_torch = np.abs(gk.to_host(theirs[i]).astype(np.float64) - want[i])
        e_ours = np.abs(gk.to_host(ours[i]).astype(np.float64) - want[i])
        print('%d elements: max |torch32 - p64| %.3e, max |SacAdam - p64| %.3e' % (n, e_torch.max(), e_ours.max()))
        assert (e_ours <= 2.0 * e_torch.max() + oc.ulp32(want[i])).all(), n
