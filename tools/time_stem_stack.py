"""Times the stacked fused stem (csrc/f110_bitconv2.h bitconv2_forward_kernel<true>; conv_bits2 with a w1 [16, k, 8, 8]) at SAL's shape
(256 x 256, conv1 8 / 4 / 16, conv2 4 / 2 / 32) beside the path it replaces for acting, conv_bits(relu) -> conv_feat(relu), in one
process, alternating, with events on the stream, the median of 20 after warm-up (tools/time_update.py's harness), two rounds:
    python tools/time_stem_stack.py [--batches 64,4096,65536] [--stacks 1,2,4] [--envs 65536] [--skip stem,act]
    python tools/time_stem_stack.py --update [--tree PATH]
stem      conv_bits2 against conv_bits(relu) -> conv_feat(relu) on n stacks of k frames drawn from a pool of 512 packed frames, and
          torch.cuda.max_memory_allocated() above the starting level over one call of either path.
act       SACAgent(stack=4).act_from(replay, evaluate=True) on --envs envs against the same action composed by hand through the unfused
          trunk (conv_bits -> conv_feat -> conv_feat -> fc1 -> head), and the peak memory of each.
--update  one process, nothing else: the replayed update of batch 64 with stack=4 (tools/time_update.py's setup), 20 single replays.
          --tree PATH imports red_gym_amd from another checkout (the parent commit's, built there), so that the two trees are timed by
          running this file on each in turn, processes alternating.
Its output belongs in profiles/r27_stem_stack.txt."""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def peak(fn):
    """Bytes allocated above the starting level at the peak of one call (its result is dropped before the next)."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated() - base
    del out
    return top


def stem(batches, stacks, rounds, rows=256, cols=256, pool=512):
    import torch
    from red_gym_amd.bitconv import conv_bits, conv_bits2
    from red_gym_amd.featconv import conv_feat
    from red_gym_amd.replay import pack_bitmaps
    from time_update import alternate
    dev = torch.device('cuda', torch.cuda.current_device())
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    frames = pack_bitmaps(((torch.rand((pool, rows, cols), device=dev, generator=gen) < 0.3) * 255).to(torch.uint8))
    conv2 = torch.nn.Conv2d(16, 32, 4, 2, device=dev)
    w2, b2 = conv2.weight.detach(), conv2.bias.detach()
    for n in batches:
        for k in stacks:
            conv1 = torch.nn.Conv2d(k, 16, 8, 4, device=dev)
            w1, b1 = conv1.weight.detach(), conv1.bias.detach()
            index = torch.randint(0, pool, (n, k), device=dev, generator=gen)

            def fused():
                return conv_bits2(frames, w1, b1, w2, b2, stride1=4, stride2=2, on=255.0, index=index, cols=cols)

            def unfused():
                return conv_feat(conv_bits(frames, w1, b1, stride=4, on=255.0, relu=True, index=index, cols=cols), w2, b2, stride=2, relu=True)

            if n <= 4096:
                assert torch.equal(fused(), unfused())
            print('---- n %d stack %d (a1: %.3f GB, out: %.3f GB): peak bytes above the start over one call: conv_bits2 %d, conv_bits -> conv_feat %d' % (
                n, k, n * 16 * 63 * 63 * 4 / 1e9, n * 32 * 30 * 30 * 4 / 1e9, peak(fused), peak(unfused)), flush=True)
            for r in range(rounds):
                got = alternate('round %d n %5d stack %d stem:' % (r, n, k), {'fused': fused, 'unfused': unfused})
                print('round %d n %5d stack %d stem: fused / unfused %.3f' % (r, n, k, got['fused'] / got['unfused']), flush=True)
            torch.cuda.empty_cache()


def act(envs, rounds, stack=4, rows=256, cols=256, T=5, AD=16):
    import torch
    from red_gym_amd import F110VecEnv, SACAgent, workload
    from red_gym_amd.bitconv import conv_bits
    from red_gym_amd.featconv import conv_feat
    from red_gym_amd.policyhead import sample_actions
    from time_update import alternate
    env = F110VecEnv(envs, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.shape_rewards(rows=rows, cols=cols)
    env.record_replay(steps=T, action_dim=AD)
    env.reset(torch.as_tensor(workload.spawn_poses(envs, 1), device=env.device))
    acts = torch.zeros((envs, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for _ in range(T + 2):
        env.step(acts)
    torch.manual_seed(0)
    agent = SACAgent(action_dim=AD, rows=rows, cols=cols, device=env.device, stack=stack)
    t, head, rp = agent.actor.trunk, agent.actor.head, env.replay

    def new():
        return agent.act_from(rp, evaluate=True)

    def by_hand():
        idx, _ = rp.stack_latest(stack)
        with torch.no_grad():
            a1 = conv_bits(rp.frame_view(), t.conv1.weight, t.conv1.bias, stride=t.conv1.stride, on=t.conv1.on, relu=True, index=idx, cols=cols)
            a2 = conv_feat(a1, t.conv2.weight, t.conv2.bias, stride=t.conv2.stride, relu=True)
            del a1
            h = agent.actor.fc1(conv_feat(a2, t.conv3.weight, t.conv3.bias, stride=t.conv3.stride, relu=True).flatten(1))
            return sample_actions(h, head.fc_mean.weight, head.fc_mean.bias, head.fc_log_std.weight, head.fc_log_std.bias, eps=None, dtype=torch.float64)[0]

    same = torch.equal(new(), by_hand())
    print('---- act_from on %d envs, stack %d: the two paths give %s actions; peak bytes above the start over one call: act_from %d, unfused trunk by hand %d' % (
        envs, stack, 'the same' if same else 'DIFFERENT', peak(new), peak(by_hand)), flush=True)
    for r in range(rounds):
        got = alternate('round %d act_from %d envs stack %d:' % (r, envs, stack), {'act_from': new, 'by hand': by_hand})
        print('round %d act_from %d envs stack %d: act_from / by hand %.3f' % (r, envs, stack, got['act_from'] / got['by hand']), flush=True)
    assert env.eng.device_errors() == 0
    env.close()


def update(tree, n=64, stack=4, reps=20):
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    import torch
    import red_gym_amd                                   # (from `tree`, before time_update puts this checkout in front)
    from red_gym_amd import SACAgent
    from time_update import AD, setup
    env, one = setup()
    torch.manual_seed(0)
    agent = SACAgent(action_dim=AD, rows=one.rows, cols=one.cols, device=env.device, stack=stack)
    agent.capture_update(env.replay, n)
    for _ in range(3):
        agent.update_graph()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        agent.update_graph()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print('%s: replayed update, batch %d, stack %d: median %.3f ms (fastest %.3f, slowest %.3f) of %d single replays' % (
        os.path.dirname(os.path.dirname(os.path.abspath(red_gym_amd.__file__))), n, stack, statistics.median(ms), min(ms), max(ms), reps), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,4096,65536')
    ap.add_argument('--stacks', default='1,2,4')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--skip', default='')
    ap.add_argument('--update', action='store_true')
    ap.add_argument('--tree', default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    if a.update:
        if not a.tree:
            sys.path.insert(0, os.path.dirname(HERE))
        return update(a.tree)
    sys.path.insert(0, os.path.dirname(HERE))
    skip = set(a.skip.split(','))
    if 'stem' not in skip:
        stem([int(x) for x in a.batches.split(',')], [int(x) for x in a.stacks.split(',')], a.rounds)
    if 'act' not in skip:
        act(a.envs, a.rounds)


if __name__ == '__main__':
    main()
