"""Times the dense layer (red_gym_amd.dense.linear_feat, SAL's fc1: 25 088 features -> 512 units, segments of 784) beside torch's GEMM
on the same tensors, in the same process:
    python tools/time_dense.py [launches] [sections ...]        sections: layer critics update[:path] (default: all)
layer     linear_feat(relu)  against  F.linear -> relu_: forward, and forward + backward, at 64, 4 096 and 65 536 rows; at 64 rows
          beside a device copy of fc1.weight's bytes, at 65 536 beside the arithmetic at the fp32 matrix-core rate; torch's one call
          on 65 536 rows is compared with torch in pieces of 4 096 rows, and a row of linear_feat with the same row alone
critics   twin_q(dense=True) against twin_q(dense=False), forward + backward, at 64 and 4 096 rows (two critics, 16 actions)
update    examples/sac_update.py's update() at its defaults (batch 64): the file (or the one at `path`, for another commit's) is run
          in this process, then 20 further updates are timed one by one on the host clock between synchronisations
hipEvents around `launches` back-to-back calls after a warm-up; three alternating windows per variant, the median and the three
values are printed (their spread is the run-to-run noise).  Its output belongs in profiles/r18_dense.txt."""
import importlib.util
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from red_gym_amd.dense import DEFAULT_SEGMENT, linear_feat, make_config, workspace_bytes
from red_gym_amd.qhead import twin_q
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
SECTIONS = sys.argv[2:] or ['layer', 'critics', 'update']
MFMA_F32_FLOPS = 157.3e12                     # 256 CUs x 4 SIMDs x 64 FLOP / clk at 2.4 GHz: the fp32 matrix-core (= vector) peak
K, H, A = 32 * 28 * 28, 512, 16


def layer():
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, H).cuda()
    w, b = lin.weight.detach(), lin.bias.detach()
    src = torch.empty_like(w)
    dst = torch.empty_like(w)
    for rows in (64, 4096, 65536):
        x = torch.relu(torch.randn((rows, K), device='cuda'))
        mine, theirs = lambda: linear_feat(x, w, b, relu=True), lambda: F.linear(x, w, b).relu_()
        got, ref = mine(), theirs()
        assert torch.equal(got[-3:], linear_feat(x[-3:].contiguous(), w, b, relu=True))       # (a row does not depend on its batch)
        pieces = torch.cat([F.linear(x[i:i + 4096], w, b).relu_() for i in range(0, rows, 4096)])
        alone = F.linear(x[-3:].contiguous(), w, b).relu_()
        print('fc1, %5d rows (workspace %d bytes): largest difference from torch in pieces of 4 096 rows: linear_feat %.3g, torch in one call %.3g; '
              'torch\'s last 3 rows against the same rows alone: %.3g (outputs up to %.3g)'
              % (rows, workspace_bytes(make_config(K, H, None, DEFAULT_SEGMENT, True), rows), float((got - pieces).abs().max()),
                 float((ref - pieces).abs().max()), float((ref[-3:] - alone).abs().max()), float(pieces.max())), flush=True)
        assert torch.allclose(got, pieces, rtol=1e-3, atol=1e-3)
        del pieces, got, ref
        fns = {'linear_feat(relu)': mine, 'F.linear -> relu_': theirs}
        if rows == 64:
            fns['device copy of fc1.weight\'s bytes'] = lambda: dst.copy_(src)
        few = N if rows <= 4096 else max(2, N // 4)
        r = report(fns, few, 3, 3, name='fc1 forward, %5d rows: ' % rows)
        print('    linear_feat / torch: %.2f' % (r['linear_feat(relu)'] / r['F.linear -> relu_']), flush=True)
        flops = 2.0 * rows * H * K
        floor = flops / MFMA_F32_FLOPS * 1e6
        print('    arithmetic %.2f GFLOP = %.0f us at the fp32 matrix-core rate (%.1f TFLOP/s): the forward stands at %.2f x that'
              % (flops / 1e9, floor, MFMA_F32_FLOPS / 1e12, r['linear_feat(relu)'] / floor), flush=True)
        xg, wg, bg = x.requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        go = torch.randn((rows, H), device='cuda')

        def both(f):
            def run():
                xg.grad = wg.grad = bg.grad = None
                f(xg, wg, bg).backward(go)
            return run
        r = report({'linear_feat(relu)': both(lambda a, c, d: linear_feat(a, c, d, relu=True)),
                  'F.linear -> relu': both(lambda a, c, d: torch.relu(F.linear(a, c, d)))}, few, 3, 3, name='fc1 forward + backward, %5d rows: ' % rows)
        print('    linear_feat / torch: %.2f (three GEMMs: %.0f us at the matrix-core rate)' % (r['linear_feat(relu)'] / r['F.linear -> relu'], 3 * floor), flush=True)
        del x, xg, go
        torch.cuda.empty_cache()


def critics():
    torch.manual_seed(1)
    fc1s = [torch.nn.Linear(K + A, H).cuda() for _ in range(2)]
    fc2s = [torch.nn.Linear(H, 1).cuda() for _ in range(2)]
    for rows in (64, 4096):
        feats = [torch.randn((rows, K), device='cuda').relu_().requires_grad_() for _ in range(2)]
        action = torch.tanh(torch.randn((rows, A), dtype=torch.float64, device='cuda'))

        def both(dense):
            def run():
                for l in fc1s + fc2s:
                    l.weight.grad = l.bias.grad = None
                for f in feats:
                    f.grad = None
                q, qmin = twin_q(feats, action, fc1s, fc2s, dense=dense)
                (q.sum() + qmin.sum()).backward()
            return run
        with torch.no_grad():
            qd, qt = twin_q(feats, action, fc1s, fc2s, dense=True)[0], twin_q(feats, action, fc1s, fc2s)[0]
        print('critics, %5d rows: largest difference of q between dense=True and dense=False %.3g (q up to %.3g)'
              % (rows, float((qd - qt).abs().max()), float(qt.abs().max())), flush=True)
        r = report({'dense=True': both(True), 'dense=False': both(False)}, N, 3, 3, name='twin_q forward + backward, %5d rows: ' % rows)
        print('    dense / default: %.2f' % (r['dense=True'] / r['dense=False']), flush=True)
        del feats
        torch.cuda.empty_cache()


def update(path=None):
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'sac_update.py')
    spec = importlib.util.spec_from_file_location('sac_update', path)
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, [path]
    try:
        spec.loader.exec_module(mod)              # (its defaults; not '__main__', so the env stays open)
    finally:
        sys.argv = argv
    times = []
    for _ in range(20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mod.update()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print('%s update(): median of 20 %.3f ms (fastest %.3f, slowest %.3f)' % (path, 1e3 * sorted(times)[10], 1e3 * min(times), 1e3 * max(times)), flush=True)
    mod.env.close()


print('%d launches per window' % N, flush=True)
for sec in SECTIONS:
    name, _, arg = sec.partition(':')
    {'layer': layer, 'critics': critics, 'update': update}[name](*([arg] if arg else []))
