"""Times one SACAgent.update's worth of parameter stepping at SAL's shapes (two critics of 12 872 785 parameters with their targets,
then the actor of 12 880 496) beside the framework's optimizers, in the same process:
    python tools/time_optim.py [repetitions]
  SacAdam                 two SacAdam(critic, targets=...).step() and one SacAdam(actor).step(): three state advances, three updates
  SacAdam, no advance     the same with the one-wave state-advance launches left out (what they cost is the difference), and the
                          advance launch alone, back to back
  torch Adam (default)    three torch.optim.Adam.step() (the foreach form on a GPU) and torch._foreach_lerp_ over both target critics
  torch Adam (fused=True) the same with fused=True, if this torch accepts it on the device
  device copy             a copy whose reads and writes add up to the bytes a single pass needs (28 B per parameter, 36 with a
                          target: 1.29 GB for the three networks): the floor
The gradients are fixed random tensors, so every variant reads and writes the same amount; hipEvents around `repetitions` back-to-back
calls after a warm-up; five alternating windows per variant; the median, the five values and their spread are printed.  Its output
belongs in profiles/r16_optim.txt."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from red_gym_amd import _lib
from red_gym_amd.optim import SacAdam
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
CRITIC = [(16, 1, 8, 8), (16,), (32, 16, 4, 4), (32,), (32, 32, 3, 3), (32,), (512, 25104), (512,), (1, 512), (1,)]
ACTOR = CRITIC[:6] + [(512, 25088), (512,), (16, 512), (16,), (16, 512), (16,)]
LR, TAU = 3e-4, 0.005


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


torch.manual_seed(0)
n_critic, n_actor = (sum(int(np.prod(s)) for s in shapes) for shapes in (CRITIC, ACTOR))
nbytes = 2 * 36 * n_critic + 28 * n_actor
print('parameters: critic %d, actor %d; a single pass moves %.3f GB per update; %d repetitions per window' % (n_critic, n_actor, nbytes / 1e9, N), flush=True)

critics, targets, actor = nets()
mine = [SacAdam(c, lr=LR, targets=t, tau=TAU) for c, t in zip(critics, targets)] + [SacAdam(actor, lr=LR)]
critics_n, targets_n, actor_n = nets()
mine_n = [SacAdam(c, lr=LR, targets=t, tau=TAU) for c, t in zip(critics_n, targets_n)] + [SacAdam(actor_n, lr=LR)]
for o in mine_n:                            # every launch a further one of the step begun at the warm-up: no advance kernel
    o.step()
    o._config = (lambda orig: lambda first: orig(False))(o._config)
adv_cfg = mine[2]._config(True)
adv_state = torch.zeros(4, dtype=torch.int64, device='cuda')
adv_state.view(torch.float64)[1:3] = 1.0
lib = _lib.load()


def advance_alone():
    _lib.check(lib.f110_adam_step(C.byref(adv_cfg), None, 0, adv_state.data_ptr(), LR, _lib.stream(adv_state.device)))


def torch_variant(**kw):
    cs, ts, a = nets()
    opts = [torch.optim.Adam(c, lr=LR, **kw) for c in cs] + [torch.optim.Adam(a, lr=LR, **kw)]

    def run():
        for o in opts:
            o.step()
        with torch.no_grad():
            for t, c in zip(ts, cs):
                torch._foreach_lerp_(t, c, TAU)
    return run


src = torch.empty(nbytes // 8, dtype=torch.float32, device='cuda').normal_()
dst = torch.empty_like(src)
fns = {'SacAdam: 3 steps (2 with targets)': lambda: [o.step() for o in mine],
       'SacAdam, no advance launches': lambda: [o.step() for o in mine_n],
       'torch Adam (default) x 3 + _foreach_lerp_': torch_variant()}
try:
    fused = torch_variant(fused=True)
    fused()
    torch.cuda.synchronize()
    fns['torch Adam (fused=True) x 3 + _foreach_lerp_'] = fused
except Exception as e:                     # (reported, not hidden: the variant is optional by the torch version)
    print('torch Adam (fused=True): not accepted here: %s' % str(e).splitlines()[0], flush=True)
fns['device copy, reads + writes = %.3f GB' % (2 * src.numel() * 4 / 1e9)] = lambda: dst.copy_(src)
med = report(fns, N, 3, 5)
for k, v in med.items():
    print('%-52s %.0f GB/s of the single pass\'s bytes' % (k, nbytes / v / 1e3), flush=True)
print('the advance launches: %.1f us per update by difference' % (med['SacAdam: 3 steps (2 with targets)'] - med['SacAdam, no advance launches']), flush=True)
report({'the state advance alone, back to back': advance_alone}, 200, 3, 5)
assert all(bool(torch.isfinite(p).all()) for p in critics[0] + targets[0] + actor)
