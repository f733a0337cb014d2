"""Times the frame-stack path (csrc/f110_replay.h replay_stack_kernel, csrc/f110_bitconv.h's stacked kernels, SACAgent(stack=k)),
alternating in one process, with events on the stream and the wall clock, the median of 20 after warm-up (tools/time_update.py's harness),
two rounds:
    python tools/time_stack.py [--batches 64,4096] [--envs 65536] [--skip walk,conv,update]
walk      f110_replay_stack on the two halves of a sample (2 n rows, one launch) for stack 1, 2, 4 and 8, against the sample it follows
          (f110_replay_sample, two launches), on a ring of --envs envs (64 x 64 images: the walk never reads a frame) and 12 step slots
          after 16 pushes; the mean depth of the last walk is printed.
conv      f110_bitconv_forward_stack at SAL's shape (256 x 256, kernel 8, stride 4, 16 channels, relu) on n samples for stack 1, 2 and 4
          against the one-frame entry, and against what a framework does with the same stacks: torch.stack of the unpacked uint8 frames
          -> .float() -> F.conv2d -> relu.  Then forward + backward likewise (conv_bits's autograd against the framework's).
update    the whole SACAgent update of batch 64 at SAL's shape (tools/time_update.py's setup), replayed from its graph and eager, with
          stack = 1 against stack = 4: two agents on one ring.
The step path (bench.py) launches nothing of this; it is timed against the parent commit by running both trees' bench.py alternately."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from red_gym_amd import F110VecEnv, SACAgent, _lib, workload
from red_gym_amd.bitconv import conv_bits, make_config
from red_gym_amd.replay import pack_bitmaps, unpack_bitmaps
from time_update import AD, alternate, setup

T, PUSHES = 12, 16
ROUNDS = 2


def walk(envs, batches):
    env = F110VecEnv(envs, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.shape_rewards(rows=64, cols=64)
    env.record_replay(steps=T, action_dim=AD)
    env.reset(torch.as_tensor(workload.spawn_poses(envs, 1), device=env.device))
    acts = torch.zeros((envs, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for _ in range(PUSHES):
        env.step(acts)
    rp, eng = env.replay, env.eng
    print('ring: %d envs x %d step slots, %d pushes, %d of %d transitions valid' % (envs, T, int(rp.buf['count']), len(rp), T * envs), flush=True)
    for n in batches:
        counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
        outs = {k: rp.sample_out(n, stack=k) for k in (2, 4, 8)}
        p, plain = outs[8], rp.sample_out(n)
        one = dict(stacks=torch.empty((2, n, 1), dtype=torch.int64, device=env.device), depth=p['depth'])
        seed, cp, st = rp._seed(0), counter.data_ptr(), eng._stream()

        def raw_sample():        # the library calls themselves, without the wrapper's checks of `out`: like against like
            return eng.lib.f110_replay_sample(eng._h, seed, cp, n, p['indices'].data_ptr(), p['s_idx'].data_ptr(), p['ns_idx'].data_ptr(), p['a'].data_ptr(),
                                              p['r'].data_ptr(), p['d'].data_ptr(), p['ok'].data_ptr(), st)

        def raw_walk(k):
            o = one if k == 1 else outs[k]
            return lambda: eng.lib.f110_replay_stack(eng._h, p['pair'].data_ptr(), 2 * n, k, o['stacks'].data_ptr(), o['depth'].data_ptr(), st)
        _lib.check(raw_sample())
        _lib.check(raw_walk(8)())
        for r in range(ROUNDS):
            alternate('round %d batch %4d library calls:' % (r, n), {'sample': raw_sample, 'walk k=1': raw_walk(1), 'walk k=2': raw_walk(2), 'walk k=4': raw_walk(4),
                                                                       'walk k=8': raw_walk(8)})
            alternate('round %d batch %4d sample_frames_dev:' % (r, n), {'stack=1': lambda: rp.sample_frames_dev(n, counter, seed=0, out=plain),
                                                                          'stack=4': lambda: rp.sample_frames_dev(n, counter, seed=0, out=outs[4], stack=4)})
        raw_walk(8)()
        print('batch %4d walk: mean depth at stack 8: %.3f' % (n, outs[8]['depth'].double().mean().item()), flush=True)
    env.close()


def conv(dev, batches, rows=256, cols=256, pool=512):
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    images = ((torch.rand((pool, rows, cols), device=dev, generator=gen) < 0.3) * 255).to(torch.uint8)
    frames = pack_bitmaps(images)
    assert torch.equal(unpack_bitmaps(frames, cols), images)
    for n in batches:
        for k in (1, 2, 4):
            ref = torch.nn.Conv2d(k, 16, 8, 4, device=dev)
            w, b = ref.weight.detach().clone().requires_grad_(), ref.bias.detach().clone().requires_grad_()
            index = torch.randint(0, pool, (n, k), device=dev, generator=gen)
            g = torch.randn((n, 16, 63, 63), device=dev, generator=gen)

            def stacked(backward):
                def fn():
                    out = conv_bits(frames, w if backward else w.detach(), b if backward else b.detach(), stride=4, on=255.0, relu=True, index=index, cols=cols)
                    if backward:
                        w.grad = b.grad = None
                        out.backward(g)
                return fn

            def framework(backward):
                def fn():
                    x = torch.stack([images[index[:, j]] for j in range(k)], dim=1).float()
                    out = F.relu(F.conv2d(x, ref.weight if backward else ref.weight.detach(), ref.bias if backward else ref.bias.detach(), stride=4))
                    if backward:
                        ref.weight.grad = ref.bias.grad = None
                        out.backward(g)
                return fn
            contestants = {False: {'stack': stacked(False), 'torch': framework(False)}, True: {'stack': stacked(True), 'torch': framework(True)}}
            if k == 1:
                w1, flat = w.detach().clone().requires_grad_(), index[:, 0].contiguous()

                def one_frame(backward):
                    def fn():
                        out = conv_bits(frames, w1 if backward else w1.detach(), b if backward else b.detach(), stride=4, on=255.0, relu=True, index=flat, cols=cols)
                        if backward:
                            w1.grad = b.grad = None
                            out.backward(g)
                    return fn
                lib = _lib.load()
                cfg = make_config(rows, cols, 8, 4, 16, 255.0, True)
                out = torch.empty((n, 16, 63, 63), device=dev)
                st = torch.cuda.current_stream(dev).cuda_stream
                wd, bd, idx2 = w.detach(), b.detach(), index.contiguous()
                contestants[False]['one-frame'] = one_frame(False)
                contestants[True]['one-frame'] = one_frame(True)
                contestants[False]['raw stack'] = lambda: lib.f110_bitconv_forward_stack(C.byref(cfg), frames.data_ptr(), pool, idx2.data_ptr(), 1, n, wd.data_ptr(),
                                                                                         bd.data_ptr(), out.data_ptr(), st)
                contestants[False]['raw one'] = lambda: lib.f110_bitconv_forward(C.byref(cfg), frames.data_ptr(), pool, flat.data_ptr(), n, wd.data_ptr(), bd.data_ptr(),
                                                                                 out.data_ptr(), st)
            for r in range(ROUNDS):
                alternate('round %d batch %4d stack %d forward:           ' % (r, n, k), contestants[False])
                alternate('round %d batch %4d stack %d forward + backward:' % (r, n, k), contestants[True])


def update(n=64):
    env, one = setup()
    torch.manual_seed(0)
    four = SACAgent(action_dim=AD, rows=one.rows, cols=one.cols, device=env.device, stack=4)
    one.capture_update(env.replay, n)
    four.capture_update(env.replay, n)
    for r in range(ROUNDS):
        got = alternate('round %d batch %4d update, replayed:' % (r, n), {'stack=1': one.update_graph, 'stack=4': four.update_graph})
        print('round %d batch %4d update, replayed: stack=4 / stack=1 %.4f; mean depth of the last batch %.3f' % (
            r, n, got['stack=4'] / got['stack=1'], four.sample['depth'].double().mean().item()), flush=True)
        got = alternate('round %d batch %4d update, eager:   ' % (r, n), {'stack=1': lambda: one.update(env.replay, n), 'stack=4': lambda: four.update(env.replay, n)})
        print('round %d batch %4d update, eager: stack=4 / stack=1 %.4f' % (r, n, got['stack=4'] / got['stack=1']), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,4096')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--skip', default='')
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(',')]
    skip = set(a.skip.split(','))
    if 'walk' not in skip:
        walk(a.envs, batches)
    if 'conv' not in skip:
        conv(torch.device('cuda', torch.cuda.current_device()), batches)
    if 'update' not in skip:
        update()


if __name__ == '__main__':
    main()
