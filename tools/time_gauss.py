"""Times the policy's Gaussian draws made on the device (red_gym_amd/gauss.py) two ways, alternating in one process, with events on the
stream and the wall clock, the median of 20 (the protocol of tools/time_update.py):
    python tools/time_gauss.py [--rows 64,4096,65536] [--batch 64] [--no-update]
fill      GaussianSource.normal(n, 16) into a static tensor (the fill and the advance of its counter) against torch.randn((n, 16))
          into one, at each n of --rows
update    one SAC update of --batch transitions at SAL's shape with SACAgent(draws='device') against draws='torch', both replayed
          from their graphs and both launched eagerly, two agents on one ring"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import GaussianSource, SACAgent
from time_update import AD, alternate, setup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', default='64,4096,65536')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--no-update', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', torch.cuda.current_device())
    src = GaussianSource(0, dev)
    for n in (int(x) for x in a.rows.split(',')):
        mine, theirs = (torch.empty((n, AD), dtype=torch.float32, device=dev) for _ in range(2))
        r = alternate('%6d x %d draws:' % (n, AD), {'fill': lambda: src.normal(n, AD, out=mine), 'fill_at': lambda: src.normal_at(0, 0, n, AD, out=mine),
                                                   'torch.randn': lambda: torch.randn((n, AD), out=theirs)})
        print('%6d x %d draws: fill / torch.randn %.2f' % (n, AD, r['fill'] / r['torch.randn']), flush=True)
    if a.no_update:
        return
    env, tor = setup()
    cfg = env.eng.shaper.cfg
    torch.manual_seed(0)
    own = SACAgent(action_dim=AD, rows=cfg.rows, cols=cfg.cols, device=env.device, draws='device', seed=0)
    n = a.batch
    tor.capture_update(env.replay, n)
    own.capture_update(env.replay, n)
    r = alternate('batch %4d update:' % n, {'graph device': own.update_graph, 'graph torch': tor.update_graph,
                                           'eager device': lambda: own.update(env.replay, n), 'eager torch': lambda: tor.update(env.replay, n)})
    print('batch %4d update: device / torch replayed %.3f, eager %.3f; calls %s' % (
        n, r['graph device'] / r['graph torch'], r['eager device'] / r['eager torch'], own.source.calls()), flush=True)
    env.close()


if __name__ == '__main__':
    main()
