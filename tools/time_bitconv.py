"""Times the first convolution from bits (red_gym_amd.bitconv, SAL's layer: 256 x 256, kernel 8, stride 4, 16 channels) beside the
torch path it replaces, in the same process:
    python tools/time_bitconv.py [launches] [sections ...]        sections: ring u8_4096 u8_65536 backward (default: all)
ring      4 096 samples of a replay ring: sample_frames + conv_bits on the s frames  against  sample_at(dtype=float32, scale) + F.conv2d
u8_N      N envs' uint8 lidar_bitmap: conv_bits  against  .float().mul_(scale).unsqueeze(1) + F.conv2d
backward  4 096 samples: f110_bitconv_backward (conv_bits' autograd) from the ring's bits  against  torch's conv2d weight gradient
          (+ the bias sum) on the fp32 images, which the torch path has kept from its forward pass
hipEvents around `launches` back-to-back calls after a warm-up; three alternating windows per variant, the median and the three
values are printed (their spread is the run-to-run noise).  Its output belongs in profiles/r10_bitconv.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from red_gym_amd import F110VecEnv, workload
from red_gym_amd.bitconv import conv_bits
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
SECTIONS = sys.argv[2:] or ['ring', 'u8_4096', 'u8_65536', 'backward']
ROWS = COLS = 256
K, STRIDE, CH = 8, 4, 16
SCALE = 1.0 / 255.0
T = 3


def filled_env(B):
    env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
    env.shape_rewards(rows=ROWS, cols=COLS)
    env.record_replay(steps=T)
    env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
    acts = torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device)
    acts[:, 0, 1] = 2.0
    for _ in range(T + 2):
        _, _, _, info = env.step(acts)
    return env, info


conv = torch.nn.Conv2d(1, CH, K, STRIDE).cuda()
w, b = conv.weight.detach(), conv.bias.detach()
OH = OW = (ROWS - K) // STRIDE + 1
out_bytes = lambda n: n * CH * OH * OW * 4  # noqa: E731

env, info = filled_env(4096)
rp = env.replay
print('SAL layer: %d x %d, kernel %d, stride %d, %d channels -> %d x %d; %d launches per window' % (ROWS, COLS, K, STRIDE, CH, OH, OW, N), flush=True)

if 'ring' in SECTIONS or 'backward' in SECTIONS:
    n = 4096
    idx, _ = rp.draw(n, seed=1)
    assert bool(rp.sample_at(idx)[5].all())

    def ours():
        at = rp.frames_at(idx)
        frames, s_idx = at['frames'], at['s_idx']
        return conv_bits(frames, w, b, stride=STRIDE, on=255.0 * SCALE, cols=COLS, index=s_idx)

    def ours_both():
        at = rp.frames_at(idx)
        frames, s_idx, ns_idx = at['frames'], at['s_idx'], at['ns_idx']
        return (conv_bits(frames, w, b, stride=STRIDE, on=255.0 * SCALE, cols=COLS, index=s_idx),
                conv_bits(frames, w, b, stride=STRIDE, on=255.0 * SCALE, cols=COLS, index=ns_idx))

    def theirs():
        s = rp.sample_at(idx, dtype=torch.float32, scale=SCALE)[0]
        return F.conv2d(s, w, b, stride=STRIDE)

    def theirs_both():
        got = rp.sample_at(idx, dtype=torch.float32, scale=SCALE)
        return F.conv2d(got[0], w, b, stride=STRIDE), F.conv2d(got[3], w, b, stride=STRIDE)

    if 'ring' in SECTIONS:
        assert torch.allclose(ours(), theirs(), rtol=0, atol=1e-4)
        print('---- forward, %d samples of the ring (out: %.2f GB per frame set)' % (n, out_bytes(n) / 1e9))
        report({'frames_at + conv_bits(s)': ours, 'sample_at(fp32, scale) + F.conv2d(s)   [unpacks s and ns]': theirs,
                'frames_at + conv_bits(s) + conv_bits(ns)': ours_both, 'sample_at(fp32, scale) + F.conv2d(s) + F.conv2d(ns)': theirs_both,
                'frames_at alone (locate + a, r, d, ok)': lambda: rp.frames_at(idx),
                'write of one out tensor alone (fill_)': (lambda o=torch.empty((n, CH, OH, OW), device='cuda'): o.fill_(1.0))}, N, 5, 3, name='ring  ')

    if 'backward' in SECTIONS:
        at = rp.frames_at(idx)
        frames, s_idx = at['frames'], at['s_idx']
        s32 = rp.sample_at(idx, dtype=torch.float32, scale=SCALE)[0]
        g = torch.randn((n, CH, OH, OW), device='cuda')
        wg = w.clone().requires_grad_()
        bg = b.clone().requires_grad_()

        def ours_bwd():
            wg.grad = bg.grad = None
            out = conv_bits(frames, wg, bg, stride=STRIDE, on=255.0 * SCALE, cols=COLS, index=s_idx)
            out.backward(g)

        def ours_fwd_only():
            conv_bits(frames, wg, bg, stride=STRIDE, on=255.0 * SCALE, cols=COLS, index=s_idx)

        def theirs_bwd():
            return torch.nn.grad.conv2d_weight(s32, w.shape, g, stride=STRIDE), g.sum(dim=(0, 2, 3))

        ours_bwd()
        ref_w, ref_b = theirs_bwd()
        assert torch.allclose(wg.grad, ref_w, rtol=1e-3, atol=1e-2) and torch.allclose(bg.grad, ref_b, rtol=1e-3, atol=1e-2)
        print('---- backward, %d samples (grad_out: %.2f GB)' % (n, out_bytes(n) / 1e9))
        r = report({'conv_bits forward + backward': ours_bwd, 'conv_bits forward alone': ours_fwd_only,
                    'torch: conv2d_weight on the fp32 images + grad_out.sum': theirs_bwd}, N, 5, 3, name='bwd   ')
        print('    f110_bitconv_backward alone (difference of the first two): %.1f us' % (r['conv_bits forward + backward'] - r['conv_bits forward alone']), flush=True)
        del s32, g

for sec in SECTIONS:
    if not sec.startswith('u8_'):
        continue
    n = int(sec[3:])
    bitmap = info['lidar_bitmap']
    images = bitmap.repeat((n + bitmap.shape[0] - 1) // bitmap.shape[0], 1, 1)[:n].contiguous()    # real FILL images, repeated
    out_holder = {}

    def ours_u8():
        out_holder['o'] = conv_bits(images, w, b, stride=STRIDE, on=255.0 * SCALE)

    def theirs_u8():
        out_holder['t'] = F.conv2d(images.float().mul_(SCALE).unsqueeze(1), w, b, stride=STRIDE)

    if n <= 4096:
        ours_u8(), theirs_u8()
        assert torch.allclose(out_holder['o'], out_holder['t'], rtol=0, atol=1e-4)
    fill = torch.empty((n, CH, OH, OW), device='cuda')
    print('---- forward, %d envs\' uint8 bitmaps (in: %.2f GB uint8 = %.2f GB as fp32; out: %.2f GB)' % (n, n * ROWS * COLS / 1e9, n * ROWS * COLS * 4 / 1e9, out_bytes(n) / 1e9))
    r = report({'conv_bits(lidar_bitmap)': ours_u8, '.float().mul_(scale).unsqueeze(1) + F.conv2d': theirs_u8,
                'write of out alone (fill_)': lambda: fill.fill_(1.0)}, N, 5, 3, name='u8    ')
    print('    output write share of conv_bits: %.0f %%' % (100.0 * r['write of out alone (fill_)'] / r['conv_bits(lidar_bitmap)']), flush=True)
    del images, fill
    out_holder.clear()
    torch.cuda.empty_cache()

assert env.eng.device_errors() == 0
env.close()
