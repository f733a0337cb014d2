"""The stacked fused stem on the GPU (f110_bitconv2_forward_stack, conv_bits2 with a w1 [C1, k, k1, k1], BitConvStem(in_channels=k),
Trunk(stack=k) without gradients, SACAgent(stack=k)): the forward `==` the checker of tests/stem_stack_cases.py as raw bit patterns
with the output between guards; a stack of one `==` the one-frame entry; a workgroup that walks several items; the order of the frames;
batch independence; the Python layers' refusals and their two paths; the memory the feature exists for; and the agent's acting path and
replayed updates."""
import ctypes as C

import numpy as np
import pytest

import bitconv2_cases as b2
import gpu_checks as gk
import replay_cases as rc
import stack_cases as sc
import stem_stack_cases as ss
from test_gpu_bitconv2 import _raw_forward2

pytestmark = pytest.mark.gpu


def _raw_stack(frames, n_frames, index, cfg, P):
    """f110_bitconv2_forward_stack itself into an array of -7 between guards that must stay as they were -> the output on the host."""
    import torch
    from red_gym_amd import _lib, bitconv
    lib = _lib.load()
    n, k = index.shape
    oh2, ow2 = bitconv.output_size2(cfg.rows, cfg.cols, cfg.kernel, cfg.stride, cfg.kernel2, cfg.stride2)
    buf = gk.Guarded(n * cfg.channels2 * oh2 * ow2, fill=-7.0)
    _lib.check(lib.f110_bitconv2_forward_stack(C.byref(cfg), frames.data_ptr(), n_frames, index.data_ptr(), k, n,
                                               *[None if t is None else t.data_ptr() for t in P], buf.ptr, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return buf.read().reshape(n, cfg.channels2, oh2, ow2)


def _cfg(case, on=1.0, relu1=True, relu2=True):
    from red_gym_amd import bitconv
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    return bitconv.make_config2(rows, cols, k1, s1, c1, k2, s2, c2, on, relu1, relu2)


def _pick(P, with_b1=True, with_b2=True):
    return (P[0], P[1] if with_b1 else None, P[2], P[3] if with_b2 else None)


@pytest.mark.parametrize('k', ss.STACKS)
@pytest.mark.parametrize('case', ss.STACK_CASES)
def test_forward_equals_checker(case, k):
    """n = 3 samples over 6 frames with sc.stack_index (a -1, an entry beyond the frames, a repeat inside a row) under every tuple of
    b2.VARIANTS: `on`, bias and relu1 are applied once, after the last frame."""
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = ss.frames_pool(rows, cols)
    frames = gk.packed(imgs)
    host = ss.params_stem_stack(k1, c1, k, k2, c2, seed=3)
    P = tuple(gk.to_device(x) for x in host)
    index = sc.stack_index(3, k, len(imgs), seed=k1)
    assert (index == -1).any() and (index >= len(imgs)).any() and index[1, 0] == index[1, 1]
    idx = gk.to_device(index)
    total = 0
    for on, relu1, relu2, wb1, wb2 in b2.VARIANTS:
        w1, b1, w2, bb = _pick(host, wb1, wb2)
        want = ss.forward_stem_stack(imgs, index, w1, b1, s1, on, relu1, w2, bb, s2, relu2)
        got = _raw_stack(frames, len(imgs), idx, _cfg(case, on, relu1, relu2), _pick(P, wb1, wb2))
        bad = gk.differing(got, want)
        print('%s stack %d on=%g relu=%s/%s bias=%s/%s: %d of %d elements differ' % (case, k, on, relu1, relu2, wb1, wb2, bad, want.size))
        total += bad
        if not relu2:                           # (0 is no hiding place: the sentinel would have to be computed, and the samples differ)
            assert (got != -7.0).all() and (want[0].size < 8 or ((want[0] != want[1]).any() and (want[1] != want[2]).any()))
    assert total == 0


@pytest.mark.parametrize('case', (ss.SAL, ss.ODD))
def test_a_stack_of_one_is_the_one_frame_entry(case):
    """index [n, 1] and stack = 1 `==` f110_bitconv2_forward with index [n]; conv_bits2 sends an [n, 1] index with a one-channel w1 there."""
    import torch
    from red_gym_amd.bitconv import conv_bits2
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = ss.frames_pool(rows, cols)
    frames = gk.packed(imgs)
    host = ss.params_stem_stack(k1, c1, 1, k2, c2, seed=4)
    P = tuple(gk.to_device(x) for x in host)
    index = np.array([[3], [-1], [0]], np.int64)
    for on, relu1, relu2, wb1, wb2 in b2.VARIANTS[:2]:
        cfg = _cfg(case, on, relu1, relu2)
        got = _raw_stack(frames, len(imgs), gk.to_device(index), cfg, _pick(P, wb1, wb2))
        one = _raw_forward2(frames, len(imgs), gk.to_device(index[:, 0].copy()), 3, cfg, _pick(P, wb1, wb2))
        assert gk.same(got, one) and (got[0] != got[1]).any() and (got[0] != got[2]).any()
    py = conv_bits2(frames, P[0], P[1], P[2], P[3], stride1=s1, stride2=s2, index=gk.to_device(index), cols=cols)
    flat = conv_bits2(frames, P[0], P[1], P[2], P[3], stride1=s1, stride2=s2, index=gk.to_device(index[:, 0].copy()), cols=cols)
    assert torch.equal(py.view(torch.int32), flat.view(torch.int32))


def test_a_workgroup_walks_several_items():
    """b2.LOOP_CASE with n = b2.LOOP_N and stack = 2 through an index over five frames with -1 entries: every workgroup walks two or
    three items, each `==` the checker (stale sums in a1 or a stale mask from the previous item would show)."""
    case, n, k = b2.LOOP_CASE, b2.LOOP_N, 2
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = ss.frames_pool(rows, cols)[[0, 1, 3, 4, 5]]
    host = ss.params_stem_stack(k1, c1, k, k2, c2, seed=4)
    index = np.random.default_rng(4).integers(0, len(imgs), (n, k)).astype(np.int64)
    index[7::101, 1] = -1
    index[11::103, 0] = -1
    want = ss.forward_stem_stack(imgs, index, host[0], host[1], s1, 1.0, True, host[2], host[3], s2, False)
    assert len(np.unique(want.reshape(n, -1), axis=0)) > 10
    got = _raw_stack(gk.packed(imgs), len(imgs), gk.to_device(index), _cfg(case, 1.0, True, False), tuple(gk.to_device(x) for x in host))
    assert gk.same(got, want)


def test_the_order_of_the_frames():
    """SAL's shape, stack = 3: reversing the columns of the index changes bits, and permuting w1's j axis alike gives the same sum added
    in the other order -- `==` the checker fed the same way, and the straight call's values to rounding (not its bits: the order of
    the frames is part of the contract, tests/test_stack_cpu.py)."""
    case, k = ss.SAL, 3
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = ss.frames_pool(rows, cols)
    frames = gk.packed(imgs)
    host = ss.params_stem_stack(k1, c1, k, k2, c2, seed=5)
    P = tuple(gk.to_device(x) for x in host)
    index = np.array([[0, 3, 4], [5, 0, 3]], np.int64)
    cfg = _cfg(case)
    straight = _raw_stack(frames, len(imgs), gk.to_device(index), cfg, P)
    turned = _raw_stack(frames, len(imgs), gk.to_device(index[:, ::-1].copy()), cfg, P)
    assert gk.differing(turned, straight) > 0
    assert gk.same(turned, ss.forward_stem_stack(imgs, index[:, ::-1], host[0], host[1], s1, 1.0, True, host[2], host[3], s2, True))
    w1r = np.ascontiguousarray(host[0][:, ::-1])
    both = _raw_stack(frames, len(imgs), gk.to_device(index[:, ::-1].copy()), cfg, (gk.to_device(w1r),) + P[1:])
    assert gk.same(both, ss.forward_stem_stack(imgs, index[:, ::-1], w1r, host[1], s1, 1.0, True, host[2], host[3], s2, True))
    assert np.allclose(both, straight, rtol=1e-3, atol=1e-3 * float(np.abs(straight).max()))
    assert gk.differing(both, turned) > 0


@pytest.mark.parametrize('case', (ss.TALL, ss.ODD))
def test_batch_independence(case):
    """A sample's result is the same alone and among 67 samples (stack = 3, seeded index over 6 frames)."""
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = ss.frames_pool(rows, cols)
    frames = gk.packed(imgs)
    P = tuple(gk.to_device(x) for x in ss.params_stem_stack(k1, c1, 3, k2, c2, seed=1))
    index = sc.stack_index(67, 3, len(imgs), seed=9)
    cfg = _cfg(case)
    batch = _raw_stack(frames, len(imgs), gk.to_device(index), cfg, P)
    for i in (0, 31, 33, 66):
        alone = _raw_stack(frames, len(imgs), gk.to_device(index[i:i + 1].copy()), cfg, P)
        assert gk.same(alone[0], batch[i])
    assert (batch[0] != batch[31]).any()


def test_the_raw_entry_refuses():
    from red_gym_amd import _lib
    lib = _lib.load()
    case = ss.ODD
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = ss.frames_pool(rows, cols)
    frames = gk.packed(imgs)
    P = tuple(gk.to_device(x) for x in ss.params_stem_stack(k1, c1, 2, k2, c2))
    idx = gk.to_device(sc.stack_index(3, 2, len(imgs)))
    out = gk.Guarded(3 * c2 * 9 * 24)
    cfg = _cfg(case)

    def call(cfg=cfg, frames=frames.data_ptr(), index=idx.data_ptr(), stack=2, n=3, w1=P[0].data_ptr(), w2=P[2].data_ptr(), o=out.ptr):
        return lib.f110_bitconv2_forward_stack(C.byref(cfg), frames, len(imgs), index, stack, n, w1, None, w2, None, o, None)

    assert b2.out_size2(rows, cols, k1, s1, k2, s2) == (9, 24) and call() == 0
    for kw in (dict(stack=0), dict(stack=sc.MAX_STACK + 1), dict(index=None), dict(n=0), dict(n=-1), dict(frames=None), dict(w1=None), dict(w2=None),
               dict(o=None), dict(cfg=_cfg((rows, 8 * cols, k1, s1, c1, k2, s2, c2)))):
        assert call(**kw) == _lib.E_INVALID, kw
    import torch
    torch.cuda.synchronize()
    out.read()


def test_conv_bits2_stem_and_trunk():
    """conv_bits2's refusals for a stacked w1; BitConvStem(in_channels=3) under no_grad is torch.equal to its gradient path's layers
    composed by hand, conv_bits(relu) -> conv_feat(relu); Trunk(stack=3)'s acting features are torch.equal to its learning features."""
    import torch
    from red_gym_amd.bitconv import MAX_STACK, BitConvStem, conv_bits, conv_bits2
    from red_gym_amd.featconv import Trunk, conv_feat
    rows, cols, k, n = 60, 76, 3, 5
    imgs = rc.random_images(rows, cols, n=6, seed=2)
    frames = gk.packed(imgs)
    index = sc.stack_index(n, k, 6)
    idx = gk.to_device(index)
    torch.manual_seed(7)
    stem = BitConvStem(on=255.0, cols=cols, device='cuda', in_channels=k)
    assert tuple(stem.conv1.weight.shape) == (16, k, 8, 8)
    c1, c2 = stem.conv1, stem.conv2
    with torch.no_grad():
        acting = stem(frames, idx)
        a1 = conv_bits(frames, c1.weight, c1.bias, stride=4, on=255.0, relu=True, index=idx, cols=cols)
        by_hand = conv_feat(a1, c2.weight, c2.bias, stride=2, relu=True)
    assert acting.grad_fn is None and torch.equal(acting.view(torch.int32), by_hand.view(torch.int32)) and bool((acting > 0).any())
    host = tuple(gk.to_host(p) for p in (c1.weight, c1.bias, c2.weight, c2.bias))
    assert gk.same(acting, ss.forward_stem_stack(imgs, index, host[0], host[1], 4, 255.0, True, host[2], host[3], 2, True))
    learning = stem(frames, idx)
    assert learning.grad_fn is not None and torch.allclose(learning.detach(), acting, rtol=1e-3, atol=1e-3 * float(acting.max()))
    learning.sum().backward()
    assert tuple(c1.weight.grad.shape) == (16, k, 8, 8) and all(bool((c1.weight.grad[:, j] != 0).any()) for j in range(k))
    shared = BitConvStem.from_convs(torch.nn.Conv2d(k, 16, 8, 4).cuda(), torch.nn.Conv2d(16, 32, 4, 2).cuda(), on=255.0, cols=cols, in_channels=k)
    with torch.no_grad():
        assert shared(frames, idx).shape == acting.shape
    with pytest.raises(ValueError):
        BitConvStem.from_convs(torch.nn.Conv2d(k, 16, 8, 4).cuda(), torch.nn.Conv2d(16, 32, 4, 2).cuda(), on=255.0, cols=cols)
    # the trunk: the paths differ now, the bits do not
    trunk = Trunk(on=255.0, cols=cols, device='cuda', stack=k)
    with torch.no_grad():
        feats = trunk(frames, idx)
    assert torch.equal(feats, trunk(frames, idx).detach()) and bool((feats > 0).any())
    # refusals
    w1, b1, w2, bb = (p.detach() for p in (c1.weight, c1.bias, c2.weight, c2.bias))
    kw = dict(stride1=4, stride2=2, cols=cols)
    big = MAX_STACK + 1
    for bad in (lambda: conv_bits2(gk.to_device(imgs), w1, b1, w2, bb, stride1=4, stride2=2, index=idx),            # uint8 frames
                lambda: conv_bits2(frames, w1, b1, w2, bb, **kw),                                                       # no index
                lambda: conv_bits2(frames, w1, b1, w2, bb, index=idx[:, 0].contiguous(), **kw),
                lambda: conv_bits2(frames, w1, b1, w2, bb, index=idx[:, :2].contiguous(), **kw),                        # the wrong width
                lambda: conv_bits2(frames, w1, b1, w2, bb, index=idx.int(), **kw),                                      # the wrong dtype
                lambda: conv_bits2(frames, w1, b1, w2, bb, index=idx.cpu(), **kw),
                lambda: conv_bits2(frames, torch.zeros((16, big, 8, 8), device='cuda'), b1, w2, bb, index=torch.zeros((n, big), dtype=torch.int64, device='cuda'), **kw),
                lambda: conv_bits2(frames, w1, b1, w2, bb, index=idx, stride1=4, stride2=2)):                           # packed frames without cols
        with pytest.raises(ValueError):
            bad()
    assert tuple(conv_bits2(frames, w1, b1, w2, bb, index=idx[:0].contiguous(), **kw).shape) == (0, 32, 6, 8)


def test_acting_holds_no_first_layer_activations():
    """SAL's shape, n = 256, stack = 2.  The rise of max_memory_allocated over a conv_bits2 call stays below the output's 29.5 MB + 1
    MiB; over Trunk(stack=2) under no_grad it stays below conv1's activations alone (n 16 63 63 4 B = 65.0 MB): the path holds
    conv2's and conv3's outputs (55.2 MB), where conv_bits -> conv_feat -> conv_feat holds conv1's and conv2's at once (94.5 MB)."""
    import torch
    from red_gym_amd.bitconv import conv_bits2
    from red_gym_amd.featconv import Trunk
    rows, cols, k1, s1, c1, k2, s2, c2 = ss.SAL
    n, k = 256, 2
    frames = gk.packed(rc.random_images(rows, cols, n=8, seed=2))
    idx = gk.to_device(np.random.default_rng(3).integers(0, 8, (n, k)).astype(np.int64))
    w1, b1, w2, bb = (gk.to_device(x) for x in ss.params_stem_stack(k1, c1, k, k2, c2))
    torch.manual_seed(2)
    trunk = Trunk(on=1.0, cols=cols, device='cuda', stack=k)
    out_bytes, a1_bytes = n * 32 * 30 * 30 * 4, n * 16 * 63 * 63 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = conv_bits2(frames, w1, b1, w2, bb, stride1=s1, stride2=s2, index=idx, cols=cols)
    torch.cuda.synchronize()
    fused = torch.cuda.max_memory_allocated() - base
    del out
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        feats = trunk(frames, idx)
    torch.cuda.synchronize()
    acting = torch.cuda.max_memory_allocated() - base
    print('peak bytes above the start: conv_bits2 %d (out %d), Trunk(stack=2) under no_grad %d (a1 %d)' % (fused, out_bytes, acting, a1_bytes))
    assert tuple(feats.shape) == (n, 32 * 28 * 28)
    assert out_bytes <= fused < out_bytes + (1 << 20)
    assert acting < a1_bytes


def test_act_from_by_hand_and_replays_equal_eager_updates(assets):
    """SACAgent(stack=3) on a ring of 8 envs after a dozen steps with a reset among them: act_from(evaluate=True) `==` the action
    computed by hand through conv_bits -> conv_feat -> conv_feat -> fc1 -> head from stack_latest's rows; three replayed updates `==`
    three eager ones (the captured graph holds the stacked stem in its no_grad block)."""
    import torch
    from red_gym_amd import workload
    from red_gym_amd.bitconv import conv_bits
    from red_gym_amd.featconv import conv_feat
    from red_gym_amd.policyhead import sample_actions
    from test_gpu_sac_agent import SMALL, _differing, _ring_env, _snapshot
    from test_gpu_sac_stack import K, _agent, _eps, _same_bits
    c = SMALL
    n, A = c['n'], c['action_dim']
    env = _ring_env(assets, c, steps=10)
    B = env.num_envs
    mask = torch.zeros(B, dtype=torch.uint8, device=env.device)
    mask[2] = 1
    env.reset(workload.spawn_poses(B, 1), mask=mask)
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    agent, _ = _agent(c, K)
    t, head = agent.actor.trunk, agent.actor.head
    depths = []
    for steps in (1, 2):                         # right behind the reset the stacks are cut short and repeat a row; later they fill up again
        for _ in range(steps):
            env.step(acts)
        rows, depth = env.replay.stack_latest(K)
        depths.append(gk.to_host(depth))
        assert tuple(rows.shape) == (B, K) and bool((depth >= 1).all())
        got = agent.act_from(env.replay, evaluate=True)
        with torch.no_grad():
            a1 = conv_bits(env.replay.frame_view(), t.conv1.weight, t.conv1.bias, stride=t.conv1.stride, on=t.conv1.on, relu=True, index=rows, cols=c['cols'])
            a2 = conv_feat(a1, t.conv2.weight, t.conv2.bias, stride=t.conv2.stride, relu=True)
            a3 = conv_feat(a2, t.conv3.weight, t.conv3.bias, stride=t.conv3.stride, relu=True).flatten(1)
            want = sample_actions(agent.actor.fc1(a3), head.fc_mean.weight, head.fc_mean.bias, head.fc_log_std.weight, head.fc_log_std.bias, eps=None,
                                  dtype=torch.float64)[0]
        assert got.dtype == torch.float64 and tuple(got.shape) == (B, A) and torch.equal(got, want) and bool((got[0] != got[1]).any())
    print('depth of the newest stacks, one and three steps behind the reset:', depths)
    assert (depths[0] < K).any() and (depths[1] == K).any()
    (eager, _), (graph, _) = _agent(c, K), _agent(c, K)
    losses = graph.capture_update(env.replay, n, draws=False)
    torch.cuda.synchronize()
    gen = torch.Generator(device='cuda').manual_seed(17)
    for u in range(3):
        eps = _eps(gen, n, A)
        want = eager.update(env.replay, n, eps=eps)
        got = graph.update_graph(eps=eps)
        torch.cuda.synchronize()
        assert got is losses and not graph.recaptured and graph.captures == 1
        assert _same_bits(got, want) and bool(torch.isfinite(got).all()) and _differing(_snapshot(graph), _snapshot(eager)) == [], u
    assert env.eng.device_errors() == 0
    env.close()
