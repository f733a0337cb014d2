"""Times the trunk's dense convolutions (red_gym_amd.featconv.conv_feat, SAL's shapes: conv2 16 x 63 x 63 -> 32 x 30 x 30, kernel 4,
stride 2; conv3 32 x 30 x 30 -> 32 x 28 x 28, kernel 3) beside torch's, in the same process:
    python tools/time_featconv.py [launches] [sections ...]        sections: layers trunk update (default: all)
layers    conv_feat(relu)  against  F.conv2d -> relu_: forward at 64, 4 096 and 65 536 rows, forward + backward at 64 and 4 096;
          the forward at 65 536 rows beside its arithmetic at the fp32 matrix-core rate and a device copy of its bytes
trunk     featconv.Trunk against the trunk examples/sac_update.py had before (BitConvStem -> nn.Conv2d -> relu), both paths
update    examples/sac_update.py's update() at its defaults (batch 64): the file is run in this process, then 20 further updates are
          timed one by one on the host clock between synchronisations; the median, the fastest and the slowest are printed
hipEvents around `launches` back-to-back calls after a warm-up; three alternating windows per variant, the median and the three
values are printed (their spread is the run-to-run noise).  Its output belongs in profiles/r17_featconv.txt."""
import importlib.util
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from red_gym_amd.bitconv import BitConvStem
from red_gym_amd.featconv import Trunk, conv_feat
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
SECTIONS = sys.argv[2:] or ['layers', 'trunk', 'update']
MFMA_F32_FLOPS = 157.3e12                     # 256 CUs x 4 SIMDs x 64 FLOP / clk at 2.4 GHz: the fp32 matrix-core (= vector) peak
LAYERS = {'conv2': (16, 63, 32, 4, 2, 30), 'conv3': (32, 30, 32, 3, 1, 28)}


def layers():
    torch.manual_seed(0)
    for name, (ci, hw, co, k, s, ohw) in LAYERS.items():
        conv = torch.nn.Conv2d(ci, co, k, s).cuda()
        w, b = conv.weight.detach(), conv.bias.detach()
        for rows in (64, 4096, 65536):
            x = torch.relu(torch.randn((rows, ci, hw, hw), device='cuda'))
            mine, theirs = lambda: conv_feat(x, w, b, stride=s, relu=True), lambda: F.conv2d(x, w, b, stride=s).relu_()
            got, ref = mine(), theirs()
            assert torch.equal(got[-3:], conv_feat(x[-3:].contiguous(), w, b, stride=s, relu=True))       # (a sample does not depend on its batch)
            # torch in pieces of 4 096 rows is the yardstick: its one call on 65 536 rows is reported beside it, not trusted
            pieces = torch.cat([F.conv2d(x[i:i + 4096], w, b, stride=s).relu_() for i in range(0, rows, 4096)])
            print('%s, %5d rows: largest difference from torch in pieces of 4 096 rows: conv_feat %.3g, torch in one call %.3g (outputs up to %.3g)'
                  % (name, rows, float((got - pieces).abs().max()), float((ref - pieces).abs().max()), float(pieces.max())), flush=True)
            assert torch.allclose(got, pieces, rtol=1e-3, atol=1e-3)
            del pieces
            del got, ref
            fns = {'conv_feat(relu)': mine, 'F.conv2d -> relu_': theirs}
            if rows == 65536:
                src = torch.empty((rows * (ci * hw * hw + co * ohw * ohw) // 2,), device='cuda')
                dst = torch.empty_like(src)
                fns['device copy of its bytes (x read, out written)'] = lambda: dst.copy_(src)
            r = report(fns, N if rows <= 4096 else max(2, N // 4), 3, 3, name='%s forward, %5d rows: ' % (name, rows))
            print('    conv_feat / torch: %.2f' % (r['conv_feat(relu)'] / r['F.conv2d -> relu_']), flush=True)
            if rows == 65536:
                flops = 2.0 * rows * co * ohw * ohw * ci * k * k
                print('    arithmetic %.1f GFLOP = %.0f us at the fp32 matrix-core rate (%.1f TFLOP/s): the kernel stands at %.2f x that, and at %.2f x the copy'
                      % (flops / 1e9, flops / MFMA_F32_FLOPS * 1e6, MFMA_F32_FLOPS / 1e12, r['conv_feat(relu)'] / (flops / MFMA_F32_FLOPS * 1e6),
                         r['conv_feat(relu)'] / r['device copy of its bytes (x read, out written)']), flush=True)
                del src, dst
            if rows <= 4096:
                xg, wg, bg = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
                go = torch.randn((rows, co, ohw, ohw), device='cuda')

                def both(f):
                    def run():
                        xg.grad = wg.grad = bg.grad = None
                        f(xg, wg, bg).backward(go)
                    return run
                r = report({'conv_feat(relu)': both(lambda a, c, d: conv_feat(a, c, d, stride=s, relu=True)),
                            'F.conv2d -> relu': both(lambda a, c, d: torch.relu(F.conv2d(a, c, d, stride=s)))},
                           N, 3, 3, name='%s forward + backward, %5d rows: ' % (name, rows))
                print('    conv_feat / torch: %.2f' % (r['conv_feat(relu)'] / r['F.conv2d -> relu']), flush=True)
            del x
            torch.cuda.empty_cache()


class OldTrunk(torch.nn.Module):
    """The trunk examples/sac_update.py had before featconv.Trunk."""

    def __init__(self):
        super().__init__()
        self.stem = BitConvStem(16, 8, 4, 32, 4, 2, on=255.0, cols=256)
        self.conv3 = torch.nn.Conv2d(32, 32, kernel_size=3, stride=1)

    def forward(self, frames, index=None):
        return torch.relu(self.conv3(self.stem(frames, index=index))).flatten(1)


def trunk():
    torch.manual_seed(0)
    new, old = Trunk(on=255.0, cols=256).cuda(), OldTrunk().cuda()
    old.load_state_dict({('stem.' + k if k[4] in '12' else k): v for k, v in new.state_dict().items()})
    for rows in (64, 4096):
        imgs = (torch.rand((rows, 32, 32), device='cuda') < 0.5).repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.uint8) * 255
        with torch.no_grad():
            assert torch.allclose(new(imgs), old(imgs), rtol=1e-4, atol=1e-2)

        def acting(m):
            def run():
                with torch.no_grad():
                    return m(imgs)
            return run

        def learning(m):
            go = torch.randn((rows, 32 * 28 * 28), device='cuda')

            def run():
                m.zero_grad(set_to_none=True)
                m(imgs).backward(go)
            return run
        r = report({'featconv.Trunk': acting(new), 'BitConvStem -> nn.Conv2d -> relu': acting(old)}, N, 3, 3, name='trunk, no grad, %5d uint8 bitmaps: ' % rows)
        print('    new / previous: %.2f' % (r['featconv.Trunk'] / r['BitConvStem -> nn.Conv2d -> relu']), flush=True)
        r = report({'featconv.Trunk': learning(new), 'BitConvStem -> nn.Conv2d -> relu': learning(old)}, N, 3, 3, name='trunk, forward + backward, %5d uint8 bitmaps: ' % rows)
        print('    new / previous: %.2f' % (r['featconv.Trunk'] / r['BitConvStem -> nn.Conv2d -> relu']), flush=True)


def update():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'sac_update.py')
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
    print('examples/sac_update.py update(): median of 20 %.3f ms (fastest %.3f, slowest %.3f)' % (1e3 * sorted(times)[10], 1e3 * min(times), 1e3 * max(times)), flush=True)
    mod.env.close()


print('%d launches per window' % N, flush=True)
for sec in SECTIONS:
    {'layers': layers, 'trunk': trunk, 'update': update}[sec]()
