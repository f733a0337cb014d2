"""Times the critic head (red_gym_amd.qhead, SAL's shape: F = 25 088 features, 16 actions, 512 hidden units, two critics) beside the
torch sequence it replaces, in the same process:
    python tools/time_qhead.py [launches] [n ...]        n: rows (default: 64 4096 65536)
per n:  the tail alone      one f110_qhead_forward with the TD target on a prepared `pre` (the feature GEMM excluded)  against  the
                            launches behind the same GEMM restated on the same tensors: .float() of the fp64 action, log_prob and
                            reward, the action part of fc1 added to `pre`, bias, relu, fc2 twice, min, the two target lines -- and
                            the cat([features, action]) copy of both critics, which the sequence needs and the kernel does not,
                            timed on its own line
        the feature GEMM    torch.mm on the strided view W[:, :F] of both critics (what twin_q runs) and F.linear on the concatenated
                            input (what the sequence runs), shown separately
        forward + backward  (mse(q0, tv) + mse(q1, tv) - qmin.mean()).backward() through twin_q and through the whole torch sequence,
                            GEMMs included on both sides; parameters require grad, features and action do not; and the same behind
                            a 16-wide feature part, where the GEMMs and the cat weigh nothing: the tail and its backward alone
        at the largest n    a device copy of both critics' `pre` (reading it once is the forward kernel's floor)
hipEvents around `launches` back-to-back calls after a warm-up; three alternating windows per variant, the median and the three
values are printed (their spread is the run-to-run noise).  Its output belongs in profiles/r14_qhead.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as Fn
from red_gym_amd import qhead
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SIZES = [int(a) for a in sys.argv[2:]] or [64, 4096, 65536]
F, A, H = 32 * 28 * 28, 16, 512
GAMMA, ALPHA = 0.99, 0.2


torch.manual_seed(0)
fc1s = [torch.nn.Linear(F + A, H).cuda() for _ in range(2)]
fc2s = [torch.nn.Linear(H, 1).cuda() for _ in range(2)]
params = [p for l in fc1s + fc2s for p in l.parameters()]
fc1s16 = [torch.nn.Linear(16 + A, H).cuda() for _ in range(2)]
params16 = [p for l in fc1s16 + fc2s for p in l.parameters()]
print('critic head: F = %d, A = %d, H = %d, two critics; %d launches per window (fewer where a call takes milliseconds)' % (F, A, H, N), flush=True)
for n in SIZES:
    feat = torch.randn((n, F), device='cuda').relu_()                 # (both critics read the same features here: 6.6 GB at 65 536 rows)
    feats = [feat, feat]
    action = torch.tanh(torch.randn((n, A), dtype=torch.float64, device='cuda'))
    nlp = torch.randn(n, dtype=torch.float64, device='cuda') * 10 - 20
    reward = torch.randn(n, dtype=torch.float64, device='cuda')
    done = (torch.rand(n, device='cuda') < 0.5).to(torch.uint8)
    print('---- n = %d (pre of both critics: %.1f MB)' % (n, 2 * n * H * 4 / 1e6), flush=True)
    with torch.no_grad():
        w1s = [l.weight.detach() for l in fc1s]
        pres = [torch.mm(f, w[:, :F].t()) for f, w in zip(feats, w1s)]
    cfg = qhead.validate(H, A, 2, F + A, True)

    def tail_mine():
        return qhead._launch_forward(cfg, pres, w1s, [l.bias for l in fc1s], [l.weight for l in fc2s], [l.bias for l in fc2s], F, action,
                                     (reward, done, nlp, GAMMA, ALPHA))

    def tail_torch():
        with torch.no_grad():
            a = action.float()
            qs = [Fn.linear(torch.relu(p + Fn.linear(a, l1.weight[:, F:], l1.bias)), l2.weight, l2.bias) for p, l1, l2 in zip(pres, fc1s, fc2s)]
            tq = torch.min(qs[0], qs[1]) - ALPHA * nlp.float().unsqueeze(1)
            return reward.float().unsqueeze(1) + (1 - done.float().unsqueeze(1)) * GAMMA * tq

    def cat_torch():
        a = action.float()
        return [torch.cat([f, a], 1) for f in feats]

    def gemm_view():
        with torch.no_grad():
            return [torch.mm(f, w[:, :F].t()) for f, w in zip(feats, w1s)]

    xs = cat_torch()

    def gemm_cat():
        with torch.no_grad():
            return [Fn.linear(x, l.weight, l.bias) for x, l in zip(xs, fc1s)]

    def torch_sequence():
        a = action.float()
        qs = [Fn.linear(torch.relu(Fn.linear(torch.cat([f, a], 1), l1.weight, l1.bias)), l2.weight, l2.bias)[:, 0] for f, l1, l2 in zip(feats, fc1s, fc2s)]
        return qs, torch.min(qs[0], qs[1])

    with torch.no_grad():
        mine, theirs = tail_mine()[2], tail_torch()[:, 0]
        print('    largest difference of the target from the torch sequence: %.3g (largest entry %.3g)' % (
            float((mine - theirs).abs().max()), float(theirs.abs().max())), flush=True)
        assert torch.allclose(mine, theirs, rtol=1e-4, atol=1e-3)
        tv = mine.clone()
    launches = N if n <= 4096 else max(3, N // 40)
    slow = max(3, launches // 10 if n > 64 else launches // 2)
    t = report({'the tail alone, forward: f110_qhead_forward (one launch)': tail_mine,
                'the tail alone, forward: torch launches behind the GEMM': tail_torch}, launches, 3, 3)
    t.update(report({'cat([features, action]) of both critics (the sequence only)': cat_torch,
                     'feature GEMM: torch.mm on the view W[:, :F], both critics': gemm_view,
                     'feature GEMM: F.linear on the concatenated input, both critics': gemm_cat}, slow, 3, 3))

    def fb_mine():
        for p in params:
            p.grad = None
        q, qmin = qhead.twin_q(feats, action, fc1s, fc2s)
        (Fn.mse_loss(q[0], tv) + Fn.mse_loss(q[1], tv) - qmin.mean()).backward()

    def fb_torch():
        for p in params:
            p.grad = None
        qs, qmin = torch_sequence()
        (Fn.mse_loss(qs[0], tv) + Fn.mse_loss(qs[1], tv) - qmin.mean()).backward()

    t.update(report({'forward + backward, GEMMs included: twin_q': fb_mine, 'forward + backward, GEMMs included: torch sequence': fb_torch}, slow, 3, 3))
    # the backward kernels on their own: the same tail behind a 16-wide feature part, where both sides' GEMMs and the cat are negligible
    small = torch.randn((n, 16), device='cuda').relu_()

    def fb_mine_small():
        for p in params16:
            p.grad = None
        q, qmin = qhead.twin_q([small, small], action, fc1s16, fc2s)
        (Fn.mse_loss(q[0], tv) + Fn.mse_loss(q[1], tv) - qmin.mean()).backward()

    def fb_torch_small():
        for p in params16:
            p.grad = None
        a = action.float()
        qs = [Fn.linear(torch.relu(Fn.linear(torch.cat([small, a], 1), l1.weight, l1.bias)), l2.weight, l2.bias)[:, 0] for l1, l2 in zip(fc1s16, fc2s)]
        (Fn.mse_loss(qs[0], tv) + Fn.mse_loss(qs[1], tv) - torch.min(qs[0], qs[1]).mean()).backward()

    t.update(report({'forward + backward at F = 16 (the tail and its backward alone): twin_q': fb_mine_small,
                     'forward + backward at F = 16: torch sequence': fb_torch_small}, launches, 3, 3))
    fb_mine()
    g_mine = [l.weight.grad.clone() for l in fc1s]
    fb_torch()
    print('    largest difference of fc1.weight.grad between the two: feature columns (both sides a GEMM of the framework) %.3g, action columns '
          '(the kernel) %.3g; largest entry %.3g' % (max(float((a - l.weight.grad)[:, :F].abs().max()) for a, l in zip(g_mine, fc1s)),
                                                    max(float((a - l.weight.grad)[:, F:].abs().max()) for a, l in zip(g_mine, fc1s)),
                                                    max(float(l.weight.grad.abs().max()) for l in fc1s)), flush=True)
    if n == max(SIZES):
        both = torch.stack(pres)
        out = torch.empty_like(both)
        report({'device copy of pre (%.0f MB read + as much written)' % (both.numel() * 4 / 1e6): lambda: out.copy_(both)}, launches, 3, 3)
    keys = list(t)
    print('    kernel / torch: the tail alone %.2f; forward + backward with GEMMs %.2f; forward + backward at F = 16 %.2f' % (
        t[keys[0]] / t[keys[1]], t[keys[5]] / t[keys[6]], t[keys[7]] / t[keys[8]]), flush=True)
    del feat, feats, xs, pres, g_mine
    torch.cuda.empty_cache()
