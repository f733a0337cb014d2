"""Times prioritized replay (csrc/f110_priority.h, SACAgent(per=True)), alternating in one process, with events on the stream and the
wall clock, the median of 20 after warm-up (tools/time_update.py's harness), two rounds:
    python tools/time_priority.py [--batches 64,4096] [--envs 65536] [--push-envs 4096,65536] [--skip sample,update_tree,push,update]
sample       f110_priority_sample (two launches: one wave per draw, then one workgroup for the weights and the advances) against
             f110_replay_sample_nstep (two launches: one lane per draw, the one-lane advance) on one ring of --envs envs and 12 step slots,
             at nstep 1 and 3, as bare library calls.
update_tree  f110_priority_update (two launches: clear, raise) on the rows the last sample drew.
push         the step with the priorities' push hook against the step without, on rings of --push-envs envs: eager step() and
             step_lib_graph(), two envs in one process.  The hook is one launch per step, two where the tree has more than one level.
update       the whole SACAgent update of batch 64 at SAL's shape (tools/time_update.py's setup), replayed from its graph: per=True
             against per=False, two agents on one ring.
The default step path (bench.py) launches nothing of this; it is timed against the parent commit by running both trees' bench.py
alternately."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from red_gym_amd import F110VecEnv, SACAgent, _lib, workload
from time_update import AD, alternate, setup

GAMMA = 0.99
T, PUSHES = 12, 16


def ring(envs, priorities):
    env = F110VecEnv(envs, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.shape_rewards(rows=64, cols=64)
    env.record_replay(steps=T, action_dim=AD, priorities=priorities)
    env.reset(torch.as_tensor(workload.spawn_poses(envs, 1), device=env.device))
    acts = torch.zeros((envs, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for _ in range(PUSHES):
        env.step(acts)
    return env, acts


def sample(envs, batches, skip):
    env, _ = ring(envs, True)
    rp, eng, p = env.replay, env.eng, env.replay.priorities
    L = p.leaf.numel()
    gen = torch.Generator(device=env.device).manual_seed(0)
    words = torch.randint(1 << 10, 1 << 24, (L,), device=env.device, generator=gen, dtype=torch.int32)
    p.set(torch.arange(L, device=env.device), words)
    print('ring: %d envs x %d step slots, %d of %d transitions valid, %d node words' % (envs, T, len(rp), L, p.node.numel()), flush=True)
    for rnd in range(2):
        for n in batches:
            counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
            o, u = rp.sample_out(n, 3, priorities=True), rp.sample_out(n, 3)
            seed, cp, st = rp._seed(0), counter.data_ptr(), eng._stream()

            def uniform(k):
                return lambda: eng.lib.f110_replay_sample_nstep(eng._h, seed, cp, n, k, GAMMA, u['indices'].data_ptr(), u['s_idx'].data_ptr(),
                                                                u['ns_idx'].data_ptr(), u['a'].data_ptr(), u['r'].data_ptr(), u['d'].data_ptr(),
                                                                u['ok'].data_ptr(), u['discount'].data_ptr(), u['span'].data_ptr(), st)

            def prioritized(k):
                return lambda: eng.lib.f110_priority_sample(eng._h, seed, cp, n, k, GAMMA, o['indices'].data_ptr(), o['s_idx'].data_ptr(),
                                                            o['ns_idx'].data_ptr(), o['a'].data_ptr(), o['r'].data_ptr(), o['d'].data_ptr(),
                                                            o['ok'].data_ptr(), o['discount'].data_ptr(), o['span'].data_ptr(), o['prio'].data_ptr(),
                                                            o['weight'].data_ptr(), st)
            _lib.check(uniform(1)())
            _lib.check(prioritized(1)())
            if 'sample' not in skip:
                alternate('round %d batch %4d sample, library calls:' % (rnd, n), {'uniform n=1': uniform(1), 'priority n=1': prioritized(1),
                                                                                  'uniform n=3': uniform(3), 'priority n=3': prioritized(3)})
            if 'update_tree' not in skip:
                td = torch.rand((n,), device=env.device, generator=gen) * 4.0
                q = torch.empty((n,), dtype=torch.int32, device=env.device)
                alternate('round %d batch %4d write-back:' % (rnd, n), {
                    'f110_priority_update': lambda: eng.lib.f110_priority_update(eng._h, o['indices'].data_ptr(), o['ok'].data_ptr(), td.data_ptr(), n, q.data_ptr(), st)})
    env.close()


def push(env_counts):
    for envs in env_counts:
        (plain, acts), (prio, _) = ring(envs, None), ring(envs, True)
        levels, cur = 0, envs * T
        while cur > 64:
            levels, cur = levels + 1, -(-cur // 64)
        print('push: %d envs, %d node words, %d levels above the leaves' % (envs, prio.replay.priorities.node.numel(), levels), flush=True)
        plain.build_step_graph()
        prio.build_step_graph()
        for rnd in range(2):
            r = alternate('round %d %5d envs step, eager:' % (rnd, envs), {'uniform ring': lambda: plain.step(acts), 'with priorities': lambda: prio.step(acts)})
            g = alternate('round %d %5d envs step_lib_graph:' % (rnd, envs), {'uniform ring': lambda: plain.step_lib_graph(acts), 'with priorities': lambda: prio.step_lib_graph(acts)})
            print('round %d %5d envs: the hook adds %.4f ms eager, %.4f ms through step_lib_graph' % (
                rnd, envs, r['with priorities'] - r['uniform ring'], g['with priorities'] - g['uniform ring']), flush=True)
        plain.close()
        prio.close()


def update(n=64):
    env, plain = setup()
    env.replay.set_priorities(True)
    torch.manual_seed(0)
    per = SACAgent(action_dim=AD, rows=plain.rows, cols=plain.cols, device=env.device, per=True)
    plain.capture_update(env.replay, n)
    per.capture_update(env.replay, n)
    for rnd in range(2):
        r = alternate('round %d batch %4d update, replayed:' % (rnd, n), {'per=False': plain.update_graph, 'per=True': per.update_graph})
        print('round %d batch %4d update, replayed: per=True / per=False %.4f; mean weight of the last batch %.4f, beta %.6f' % (
            rnd, n, r['per=True'] / r['per=False'], per.sample['weight'].mean().item(), env.replay.priorities.beta), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,4096')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--push-envs', default='4096,65536')
    ap.add_argument('--skip', default='')
    a = ap.parse_args()
    skip = set(a.skip.split(','))
    if not {'sample', 'update_tree'} <= skip:
        sample(a.envs, [int(x) for x in a.batches.split(',')], skip)
    if 'push' not in skip:
        push([int(x) for x in a.push_envs.split(',')])
    if 'update' not in skip:
        update()


if __name__ == '__main__':
    main()
