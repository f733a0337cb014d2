"""Times one SAC update at SAL's shape (256 envs, 256 x 256 images, hidden 512, 16 action values) three ways, alternating in one
process, with events on the stream and the wall clock, the median of 20:
    python tools/time_update.py [--parent PATH] [--batches 64,4096] [--count KIND --updates K]
graph     SACAgent.update_graph(): the captured update, one host call
eager     SACAgent.update(): the same launches from the host
parent    update() of another commit's examples/sac_update.py (PATH: that file; it builds its own env and networks when loaded)
and, at each batch size, the pieces this commit replaced: ReplayBuffer.sample_frames_dev against draw + frames_at, critic_loss against
F.mse_loss twice with its backward, actor_loss against (alpha * logp - qn).mean() with its backward.
--count KIND --updates K runs K updates of one kind and nothing else, for a kernel trace of its own: the launches of an update are the
difference of two such runs' dispatch counts divided by the difference of their K."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from red_gym_amd import F110VecEnv, SACAgent, workload
from red_gym_amd.sacloss import actor_loss, critic_loss

B, STEPS, AD, REPS = 256, 40, 16, 20


def setup():
    env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.shape_rewards()
    env.follow_paths()
    env.record_replay(capacity=16 * B, action_dim=AD)
    cfg = env.eng.shaper.cfg
    torch.manual_seed(0)
    agent = SACAgent(action_dim=AD, rows=cfg.rows, cols=cfg.cols, device=env.device)
    gen = torch.Generator(device=env.device).manual_seed(0)
    env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
    for _ in range(STEPS):
        env.step(env.path_actions(torch.rand((B, AD), dtype=torch.float64, device=env.device, generator=gen) * 2.0 - 1.0))
    return env, agent


def load_parent(path, batch):
    spec = importlib.util.spec_from_file_location('parent_sac_update', path)
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, [path, str(B), str(STEPS), str(batch)]
    try:
        spec.loader.exec_module(mod)              # (not '__main__', so its env stays open)
    finally:
        sys.argv = argv
    return mod


def alternate(title, contestants, warm=3):
    """Every contestant once per round, REPS rounds -> {name: median ms on the stream}; prints stream and wall medians."""
    for fn in contestants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in contestants}, {k: [] for k in contestants}
    for _ in range(REPS):
        for name, fn in contestants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            wall[name].append(1e3 * (time.perf_counter() - t0))
            ev[name].append(e0.elapsed_time(e1))
    out = {}
    for name in contestants:
        out[name] = statistics.median(ev[name])
        print('%s %-10s stream %8.3f ms (fastest %8.3f, slowest %8.3f)   wall %8.3f ms' % (
            title, name, out[name], min(ev[name]), max(ev[name]), statistics.median(wall[name])), flush=True)
    return out


def pieces(env, agent, n):
    rp, dev = env.replay, env.device
    counter = torch.zeros((1,), dtype=torch.int64, device=dev)
    out = rp.sample_out(n)
    alternate('batch %4d sample:' % n, {'device': lambda: rp.sample_frames_dev(n, counter, out=out), 'host': lambda: rp.sample_frames(n)})
    q = torch.randn((2, n), device=dev).requires_grad_()
    tv = torch.randn((n,), device=dev)
    logp = torch.randn((n,), dtype=torch.float64, device=dev).requires_grad_()
    qn = torch.randn((n,), device=dev).requires_grad_()
    losses = torch.zeros((3,), device=dev)
    grad = torch.empty((2, n), device=dev)

    def framework_critic():
        q.grad = None
        (F.mse_loss(q[0], tv) + F.mse_loss(q[1], tv)).backward()

    def framework_actor():
        logp.grad = qn.grad = None
        (agent.alpha * logp - qn).mean().backward()

    alternate('batch %4d critic loss + gradients:' % n, {'kernel': lambda: critic_loss(q[0], q[1], tv, loss=losses[1:3], grad=grad), 'framework': framework_critic})
    alternate('batch %4d actor loss + gradients: ' % n, {'kernel': lambda: actor_loss(logp, qn, agent.alpha, loss=losses[0:1]), 'framework': framework_actor})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--batches', default='64,4096')
    ap.add_argument('--count', default=None, choices=('graph', 'eager', 'parent'))
    ap.add_argument('--updates', type=int, default=5)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(',')]
    if a.count:
        n = batches[0]
        if a.count == 'parent':
            mod = load_parent(a.parent, n)
            fn, env = mod.update, mod.env
        else:
            env, agent = setup()
            if a.count == 'graph':
                agent.capture_update(env.replay, n)
            fn = agent.update_graph if a.count == 'graph' else (lambda: agent.update(env.replay, n))
        for _ in range(a.updates):
            fn()
        torch.cuda.synchronize()
        print('%d %s updates of batch %d' % (a.updates, a.count, n))
        env.close()
        return
    env, agent = setup()
    print('%d envs, %d x %d images, features %d wide, hidden %d; ring: %d of %d transitions valid; median of %d, alternating' % (
        B, agent.rows, agent.cols, agent.width, agent.hidden, len(env.replay), env.replay.steps * B, REPS), flush=True)
    for n in batches:
        contestants = {'graph': agent.update_graph, 'eager': lambda: agent.update(env.replay, n)}
        agent.capture_update(env.replay, n)
        mod = None
        if a.parent:
            mod = load_parent(a.parent, n)
            contestants['parent'] = mod.update
        r = alternate('batch %4d update:' % n, contestants)
        print('batch %4d update: eager / graph %.2f%s' % (n, r['eager'] / r['graph'], ', parent / graph %.2f, parent / eager %.2f' % (
            r['parent'] / r['graph'], r['parent'] / r['eager']) if mod else ''), flush=True)
        if mod:
            mod.env.close()
        pieces(env, agent, n)
    print('captures: %d' % agent.captures)
    env.close()


if __name__ == '__main__':
    main()
