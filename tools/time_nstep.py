"""Times the n-step path (csrc/f110_replay.h replay_walk, f110_qhead_forward_rows, SACAgent(nstep=k)), alternating in one process, with
events on the stream and the wall clock, the median of 20 after warm-up (tools/time_update.py's harness):
    python tools/time_nstep.py [--batches 64,4096] [--envs 65536] [--skip sample,target,update]
sample    ReplayBuffer.sample_frames_dev on a ring of --envs envs (64 x 64 images: the walk never reads a frame) and 12 step slots, 16
          pushes: the one-step call (f110_replay_sample) against f110_replay_sample_nstep at nstep 1, 3 and 8, once as the bare library
          calls and once through the Python wrapper.  Each is two launches, the sample and the one-lane advance; the walk adds up to
          nstep - 1 dependent rounds of three loads per lane, one step slot = envs cells apart.  The mean span of the last batch is
          printed.
target    qhead.td_target(dense=True) at SAL's widths (25 088 features, hidden 512, 16 action values, two critics) with gamma by value
          against an [n] fp64 discount per row: the same launches, one fp64 load per row more in the last of them.
update    the whole SACAgent update of batch 64 at SAL's shape (tools/time_update.py's setup: 256 envs, 256 x 256 images), replayed from
          its graph, with nstep = 1 against nstep = 3: two agents on one ring.
The step path (bench.py) launches nothing of this; it is timed against the parent commit by running both trees' bench.py alternately."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from red_gym_amd import F110VecEnv, SACAgent, _lib, workload
from red_gym_amd.qhead import td_target
from time_update import AD, alternate, setup

GAMMA = 0.99
T, PUSHES = 12, 16


def sample(envs, batches):
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
        outs = {k: rp.sample_out(n, 2) for k in (1, 3, 8)}       # (the raw entry at nstep = 1 writes discount and span too)
        plain = rp.sample_out(n)
        p = plain
        seed, cp, st = rp._seed(0), counter.data_ptr(), eng._stream()

        def raw_one():           # the library calls themselves, without the wrapper's checks of `out`: like against like
            return eng.lib.f110_replay_sample(eng._h, seed, cp, n, p['indices'].data_ptr(), p['s_idx'].data_ptr(), p['ns_idx'].data_ptr(), p['a'].data_ptr(),
                                              p['r'].data_ptr(), p['d'].data_ptr(), p['ok'].data_ptr(), st)

        def raw_walk(k):
            o = outs[k]
            return lambda: eng.lib.f110_replay_sample_nstep(eng._h, seed, cp, n, k, GAMMA, o['indices'].data_ptr(), o['s_idx'].data_ptr(),
                                                            o['ns_idx'].data_ptr(), o['a'].data_ptr(), o['r'].data_ptr(), o['d'].data_ptr(),
                                                            o['ok'].data_ptr(), o['discount'].data_ptr(), o['span'].data_ptr(), st)
        _lib.check(raw_one())
        _lib.check(raw_walk(1)())
        alternate('batch %4d sample, library calls:' % n, {'one-step': raw_one, 'walk n=1': raw_walk(1), 'walk n=3': raw_walk(3), 'walk n=8': raw_walk(8)})
        alternate('batch %4d sample_frames_dev:   ' % n, {'nstep=1': lambda: rp.sample_frames_dev(n, counter, seed=0, out=plain),
                                                           'nstep=3': lambda: rp.sample_frames_dev(n, counter, seed=0, out=outs[3], nstep=3, gamma=GAMMA),
                                                           'nstep=8': lambda: rp.sample_frames_dev(n, counter, seed=0, out=outs[8], nstep=8, gamma=GAMMA)})
        print('batch %4d sample: mean span at nstep 3: %.3f, at 8: %.3f; ok %.3f' % (
            n, outs[3]['span'].double().mean().item(), outs[8]['span'].double().mean().item(), outs[8]['ok'].double().mean().item()), flush=True)
    env.close()


def target(dev, batches, F=25088, H=512):
    torch.manual_seed(0)
    fc1s = [torch.nn.Linear(F + AD, H, device=dev) for _ in range(2)]
    fc2s = [torch.nn.Linear(H, 1, device=dev) for _ in range(2)]
    for n in batches:
        feats = [torch.randn((n, F), device=dev).relu_() for _ in range(2)]
        action = torch.tanh(torch.randn((n, AD), dtype=torch.float64, device=dev))
        nlp = torch.randn((n,), dtype=torch.float64, device=dev) * 10.0 - 5.0
        reward = torch.randn((n,), dtype=torch.float64, device=dev)
        done = (torch.rand((n,), device=dev) < 0.1).to(torch.uint8)
        rows = torch.full((n,), GAMMA ** 3, dtype=torch.float64, device=dev)
        alternate('batch %4d td_target:' % n, {'by value': lambda: td_target(feats, action, nlp, reward, done, fc1s, fc2s, GAMMA, 0.2, dense=True),
                                                'per row': lambda: td_target(feats, action, nlp, reward, done, fc1s, fc2s, rows, 0.2, dense=True)})


def update(n=64):
    env, one = setup()
    torch.manual_seed(0)
    three = SACAgent(action_dim=AD, rows=one.rows, cols=one.cols, device=env.device, nstep=3)
    one.capture_update(env.replay, n)
    three.capture_update(env.replay, n)
    r = alternate('batch %4d update, replayed:' % n, {'nstep=1': one.update_graph, 'nstep=3': three.update_graph})
    print('batch %4d update, replayed: nstep=3 / nstep=1 %.4f; mean span of the last batch %.3f' % (
        n, r['nstep=3'] / r['nstep=1'], three.sample['span'].double().mean().item()), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,4096')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--skip', default='')
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(',')]
    skip = set(a.skip.split(','))
    if 'sample' not in skip:
        sample(a.envs, batches)
    if 'target' not in skip:
        target(torch.device('cuda', torch.cuda.current_device()), batches)
    if 'update' not in skip:
        update()


if __name__ == '__main__':
    main()
