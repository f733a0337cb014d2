"""Times gradient clipping (SacAdam(max_grad_norm=...), csrc/f110_adam_clip.h) at SAL's shapes, in one process:
    python tools/time_clip.py [repetitions] [--update]
One update's worth of optimizer steps (two critics of 12 872 785 parameters with their targets, then the actor of 12 880 496):
  SacAdam clipped         per network: the norm kernel, the one-workgroup clip kernel, the guarded advance, the clipped update
  SacAdam unclipped       tools/time_optim.py's first line, in this process
  torch clip + fused      torch.nn.utils.clip_grad_norm_(foreach=True) per network, torch.optim.Adam(fused=True).step() and
                          torch._foreach_lerp_ over both target critics
  device copy             a copy whose reads and writes add up to the bytes the clipped step must move (g is read twice: 32 B per
                          parameter, 40 with a target): the floor
max_grad_norm is far below the gradients' norm, so every step is clipped (with coef = 1.0f the kernels do the same work).  hipEvents
around `repetitions` back-to-back calls after a warm-up; five alternating windows per variant; the median, the five values and their
spread are printed (the protocol of tools/time_optim.py).
--update adds tools/time_update.py's whole update of batch 64 with max_grad_norm set and unset, replayed and eager, alternating in
this process, median of 20.  Its output belongs in profiles/r29_clip.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from red_gym_amd.optim import SacAdam
from timing import report

ARGS = [a for a in sys.argv[1:] if not a.startswith('--')]
N = int(ARGS[0]) if ARGS else 20
CRITIC = [(16, 1, 8, 8), (16,), (32, 16, 4, 4), (32,), (32, 32, 3, 3), (32,), (512, 25104), (512,), (1, 512), (1,)]
ACTOR = CRITIC[:6] + [(512, 25088), (512,), (16, 512), (16,), (16, 512), (16,)]
LR, TAU, MAX_NORM = 3e-4, 0.005, 1.0


def network(shapes):
    ps = [torch.randn(s, device='cuda') * 0.05 for s in shapes]
    for p in ps:
        p.grad = torch.randn_like(p) * 0.01
    return ps


def nets():
    """(critic, its target) twice, and the actor."""
    critics = [network(CRITIC) for _ in range(2)]
    targets = [[p.clone() for p in c] for c in critics]
    return critics, targets, network(ACTOR)


def sac_adam(**kw):
    critics, targets, actor = nets()
    return [SacAdam(c, lr=LR, targets=t, tau=TAU, **kw) for c, t in zip(critics, targets)] + [SacAdam(actor, lr=LR, **kw)]


def torch_variant():
    cs, ts, a = nets()
    opts = [torch.optim.Adam(c, lr=LR, fused=True) for c in cs] + [torch.optim.Adam(a, lr=LR, fused=True)]
    grads = [[p.grad.clone() for p in ps] for ps in cs + [a]]

    def run():
        for ps, gs, o in zip(cs + [a], grads, opts):
            torch._foreach_copy_([p.grad for p in ps], gs)     # (clip_grad_norm_ scales .grad in place: without this the norm decays to 0;
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=True)      # the copy's 8 B per parameter are reported on their own below)
            o.step()
        with torch.no_grad():
            for t, c in zip(ts, cs):
                torch._foreach_lerp_(t, c, TAU)

    def restore_only():
        for ps, gs in zip(cs + [a], grads):
            torch._foreach_copy_([p.grad for p in ps], gs)
    return run, restore_only


def steps():
    n_critic, n_actor = (sum(int(np.prod(s)) for s in shapes) for shapes in (CRITIC, ACTOR))
    nbytes = 2 * 40 * n_critic + 32 * n_actor
    print('parameters: critic %d, actor %d; the clipped step moves %.3f GB per update (the unclipped one %.3f); %d repetitions per window' % (
        n_critic, n_actor, nbytes / 1e9, (2 * 36 * n_critic + 28 * n_actor) / 1e9, N), flush=True)
    clipped, plain = sac_adam(max_grad_norm=MAX_NORM), sac_adam()
    fused, restore = torch_variant()
    src = torch.empty(nbytes // 8, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    fns = {'SacAdam clipped: 3 steps (2 with targets)': lambda: [o.step() for o in clipped],
           'SacAdam unclipped: 3 steps (2 with targets)': lambda: [o.step() for o in plain],
           'torch: copy .grad + clip_grad_norm_(foreach) + Adam(fused) + lerp': fused,
           'torch: the copy of .grad alone': restore,
           'device copy, reads + writes = %.3f GB' % (2 * src.numel() * 4 / 1e9): lambda: dst.copy_(src)}
    med = report(fns, N, 3, 5)
    keys = list(med)
    print('clipped / unclipped %.3f (+%.1f us); clipped / floor %.3f; torch (without its copy) / clipped %.3f' % (
        med[keys[0]] / med[keys[1]], med[keys[0]] - med[keys[1]], med[keys[0]] / med[keys[4]], (med[keys[2]] - med[keys[3]]) / med[keys[0]]), flush=True)
    stats = [o.clip_stats() for o in clipped]
    print('clip_stats (norm, coef, skip, steps_clipped, steps_skipped): %s' % stats, flush=True)
    assert all(s[1] < 1.0 and not s[2] and s[4] == 0 for s in stats)
    assert all(bool(torch.isfinite(p).all()) for o in clipped for p in o.params)


def update():
    import time_update as tu
    from red_gym_amd import SACAgent
    env, plain = tu.setup()
    cfg = env.eng.shaper.cfg
    torch.manual_seed(0)
    clipped = SACAgent(action_dim=tu.AD, rows=cfg.rows, cols=cfg.cols, device=env.device, max_grad_norm=10.0)
    n = 64
    plain.capture_update(env.replay, n)
    clipped.capture_update(env.replay, n)
    r = tu.alternate('batch %4d update:' % n, {'graph': plain.update_graph, 'graph+clip': clipped.update_graph,
                                                'eager': lambda: plain.update(env.replay, n), 'eager+clip': lambda: clipped.update(env.replay, n)})
    print('batch %4d update: clipped / unclipped, replayed %.3f (+%.1f us), eager %.3f (+%.1f us)' % (
        n, r['graph+clip'] / r['graph'], 1e3 * (r['graph+clip'] - r['graph']), r['eager+clip'] / r['eager'], 1e3 * (r['eager+clip'] - r['eager'])), flush=True)
    stats = clipped.grad_stats()
    print('grad_stats after %d updates: norm %s coef %s steps_clipped %s steps_skipped %s' % (
        int(clipped.actor_opt.device_state()[0]), stats['norm'].tolist(), stats['coef'].tolist(), stats['steps_clipped'].tolist(), stats['steps_skipped'].tolist()), flush=True)
    env.close()


torch.manual_seed(0)
steps()
if '--update' in sys.argv[1:]:
    update()
