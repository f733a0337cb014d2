"""Times the learnt temperature (red_gym_amd.temperature, csrc/f110_temperature.h) at SAL's shape, alternating in one process, with
events on the stream and the wall clock, the median of 20 after warm-up (tools/time_update.py's harness):
    python tools/time_temperature.py [--batches 64,4096] [--count KIND --updates K]
step      Temperature.step(logp), one launch, against the framework sequence it replaces: (-(log_alpha * (logp + H).detach()).mean())
          .backward(), torch.optim.Adam.step() on the one parameter and .exp()
update    the whole SACAgent update, replayed from its graph and eager, for alpha='auto' against alpha=0.2: two agents on one ring
The same update of the parent commit is timed by that commit's own tools/time_update.py in its own tree and process, run alternately
with this one (a process holds one build of the library); its `graph` and `eager` lines stand beside `fixed graph` and `fixed eager`.
--count KIND --updates K (KIND: auto or fixed) runs K eager updates of batch 64 and nothing else, for a kernel trace of its own: the
launches of an update are the difference of two such runs' dispatch counts divided by the difference of their K."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from red_gym_amd import SACAgent
from red_gym_amd.temperature import Temperature
from time_update import AD, alternate, setup

H = -float(AD)


def agents(env, fixed):
    """(the fixed-alpha agent setup() built, an alpha='auto' agent from the same seed) on the env's ring."""
    torch.manual_seed(0)
    auto = SACAgent(action_dim=AD, rows=fixed.rows, cols=fixed.cols, device=env.device, alpha='auto')
    return fixed, auto


def step_alone(dev, n):
    logp = (10.0 * torch.randn((n,), dtype=torch.float64, device=dev) - 5.0)
    temp = Temperature(target_entropy=H, device=dev)
    log_alpha = torch.tensor([float(temp.log_alpha.item())], device=dev, requires_grad=True)
    opt = torch.optim.Adam([log_alpha], lr=3e-4)

    def framework():
        opt.zero_grad()
        (-(log_alpha * (logp + H).detach()).mean()).backward()
        opt.step()
        return log_alpha.detach().exp()

    alternate('n %4d temperature step:' % n, {'kernel': lambda: temp.step(logp), 'framework': framework})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,4096')
    ap.add_argument('--count', default=None, choices=('auto', 'fixed'))
    ap.add_argument('--updates', type=int, default=5)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(',')]
    env, fixed = setup()
    fixed, auto = agents(env, fixed)
    if a.count:
        agent = auto if a.count == 'auto' else fixed
        for _ in range(a.updates):
            agent.update(env.replay, batches[0])
        torch.cuda.synchronize()
        print('%d %s updates of batch %d' % (a.updates, a.count, batches[0]))
        env.close()
        return
    for n in batches:
        step_alone(env.device, n)
    for n in batches:
        fixed.capture_update(env.replay, n)
        auto.capture_update(env.replay, n)
        r = alternate('batch %4d update:' % n, {'fixed graph': fixed.update_graph, 'auto graph': auto.update_graph,
                                                 'fixed eager': lambda: fixed.update(env.replay, n), 'auto eager': lambda: auto.update(env.replay, n)})
        print('batch %4d update: auto / fixed: graph %.4f, eager %.4f; alpha now %.9f' % (
            n, r['auto graph'] / r['fixed graph'], r['auto eager'] / r['fixed eager'], auto.alpha.item()), flush=True)
    env.close()


if __name__ == '__main__':
    main()
