"""Times the policy head (red_gym_amd.policyhead.sample_actions, SAL's shape: K = 512 features, 16 actions) beside the torch
sequence it replaces, in the same process:
    python tools/time_policyhead.py [launches] [n ...]        n: rows (default: 64 4096 65536)
per n:  forward             sample_actions under no_grad  against  src/SAL.py:410-421 restated from the formula on the same tensors
                            (two F.linear, clamp, exp, mean + std * eps, tanh, the log_prob summed) and the .double() that
                            path_actions needs
        forward + backward  (alpha * logp - action.sum(1)).mean().backward() through either
        at the largest n    a device copy of h (read and write of its bytes; reading h once is the forward's floor)
hipEvents around `launches` back-to-back calls after a warm-up; three alternating windows per variant, the median and the three
values are printed (their spread is the run-to-run noise).  Its output belongs in profiles/r12_policyhead.txt."""
import math
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from red_gym_amd.policyhead import sample_actions
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SIZES = [int(a) for a in sys.argv[2:]] or [64, 4096, 65536]
K, A = 512, 16
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def torch_head(h, wm, bm, wl, bl, eps):
    """Actor.forward's end and Actor.sample (src/SAL.py:410-421) restated, with the fp64 copy of the action path_actions takes."""
    mean = F.linear(h, wm, bm)
    log_std = torch.clamp(F.linear(h, wl, bl), -20, 2)
    std = log_std.exp()
    x_t = mean + std * eps
    y_t = torch.tanh(x_t)
    log_prob = (-((x_t - mean) ** 2) / (2 * std * std) - log_std - HALF_LOG_2PI - torch.log(1 - y_t.pow(2) + 1e-6)).sum(1)
    return y_t.double(), log_prob, y_t


torch.manual_seed(0)
fc_mean, fc_log_std = torch.nn.Linear(K, A).cuda(), torch.nn.Linear(K, A).cuda()
params = (fc_mean.weight, fc_mean.bias, fc_log_std.weight, fc_log_std.bias)
print('policy head: K = %d, A = %d; %d launches per window (a quarter of them at 65 536 rows)' % (K, A, N), flush=True)
for n in SIZES:
    h = torch.randn((n, K), device='cuda').relu_()
    eps = torch.randn((n, A), device='cuda')
    launches = N if n <= 4096 else max(5, N // 4)
    print('---- n = %d (h: %.1f MB)' % (n, n * K * 4 / 1e6), flush=True)
    with torch.no_grad():
        mine, theirs = sample_actions(h, *params, eps=eps), torch_head(h, *params, eps)
        # (both compute the same thing; the fp32 sequence loses digits of 1 - y^2 near saturation, hence the loose log_prob figure)
        print('    largest difference from the torch sequence: action %.3g, log_prob %.3g' % (
            float((mine[0] - theirs[0]).abs().max()), float((mine[1] - theirs[1].double()).abs().max())), flush=True)
        assert torch.allclose(mine[0], theirs[0], rtol=0, atol=1e-4)

    def fwd_mine():
        with torch.no_grad():
            return sample_actions(h, *params, eps=eps)

    def fwd_torch():
        with torch.no_grad():
            return torch_head(h, *params, eps)

    hg = h.clone().requires_grad_()

    def both_mine():
        a, lp, _, _ = sample_actions(hg, *params, eps=eps)
        (0.2 * lp - a.sum(1)).mean().backward()

    def both_torch():
        a, lp, _ = torch_head(hg, *params, eps)
        (0.2 * lp - a.sum(1)).mean().backward()

    fns = {'forward: sample_actions': fwd_mine, 'forward: torch sequence + .double()': fwd_torch,
           'forward + backward: sample_actions': both_mine, 'forward + backward: torch sequence': both_torch}
    if n == max(SIZES):
        copy = torch.empty_like(h)
        fns['device copy of h (%.0f MB read + as much written)' % (n * K * 4 / 1e6)] = lambda: copy.copy_(h)
    r = report(fns, launches, 5, 3)
    print('    sample_actions / torch: forward %.2f, forward + backward %.2f' % (
        r['forward: sample_actions'] / r['forward: torch sequence + .double()'],
        r['forward + backward: sample_actions'] / r['forward + backward: torch sequence']), flush=True)
