"""Times the fused policy stem (red_gym_amd.bitconv.conv_bits2, SAL's shape: 256 x 256, conv1 8 / 4 / 16, conv2 4 / 2 / 32) beside
the path it replaces for acting, in the same process:
    python tools/time_bitconv2.py [launches] [sections ...]        sections: ring u8_4096 u8_65536 (default: all)
ring      4 096 samples of a replay ring (frames_at's s frames through an index)
u8_N      N envs' uint8 lidar_bitmap
each: conv_bits2  against  conv_bits(relu=True) -> F.conv2d(stride=2) -> relu_();  beside them F.conv2d alone on a kept a1 and the
write of `out` alone; and torch.cuda.max_memory_allocated() above the starting level over one call of either path.
hipEvents around `launches` back-to-back calls after a warm-up; three alternating windows per variant, the median and the three
values are printed (their spread is the run-to-run noise).  Its output belongs in profiles/r11_bitconv2.txt."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
from red_gym_amd import F110VecEnv, workload
from red_gym_amd.bitconv import conv_bits, conv_bits2
from timing import report

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
SECTIONS = sys.argv[2:] or ['ring', 'u8_4096', 'u8_65536']
ROWS = COLS = 256
T = 3


def peak(fn):
    """Bytes allocated above the starting level at the peak of one call (its result is dropped before the next)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated() - base
    del out
    return top


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


torch.manual_seed(0)
conv1, conv2 = torch.nn.Conv2d(1, 16, 8, 4).cuda(), torch.nn.Conv2d(16, 32, 4, 2).cuda()
w1, b1, w2, b2 = (p.detach() for p in (conv1.weight, conv1.bias, conv2.weight, conv2.bias))
env, info = filled_env(4096)
rp = env.replay
print('SAL stem: %d x %d -> 16 x 63 x 63 -> 32 x 30 x 30; %d launches per window' % (ROWS, COLS, N), flush=True)


def section(title, n, src, kw):
    def fused():
        return conv_bits2(src, w1, b1, w2, b2, stride1=4, stride2=2, on=1.0, **kw)

    def parent():
        return F.conv2d(conv_bits(src, w1, b1, stride=4, on=1.0, relu=True, **kw), w2, b2, stride=2).relu_()

    if n <= 4096:
        assert torch.allclose(fused(), parent(), rtol=1e-4, atol=1e-4)
    print('---- %s (a1: %.2f GB, out: %.2f GB)' % (title, n * 16 * 63 * 63 * 4 / 1e9, n * 32 * 30 * 30 * 4 / 1e9), flush=True)
    print('peak bytes above the start over one call: conv_bits2 %d, conv_bits -> F.conv2d -> relu_ %d' % (peak(fused), peak(parent)), flush=True)
    a1 = conv_bits(src, w1, b1, stride=4, on=1.0, relu=True, **kw)
    fill = torch.empty((n, 32, 30, 30), device='cuda')
    r = report({'conv_bits2': fused, 'conv_bits(relu) -> F.conv2d -> relu_': parent, 'F.conv2d alone on a kept a1': lambda: F.conv2d(a1, w2, b2, stride=2),
                'write of out alone (fill_)': lambda: fill.fill_(1.0)}, N if n <= 4096 else max(2, N // 4), 3, 3)
    print('    conv_bits2 / parent path: %.2f' % (r['conv_bits2'] / r['conv_bits(relu) -> F.conv2d -> relu_']), flush=True)
    del a1, fill
    torch.cuda.empty_cache()


for sec in SECTIONS:
    if sec == 'ring':
        idx, _ = rp.draw(4096, seed=1)
        at = rp.frames_at(idx)
        frames, s_idx = at['frames'], at['s_idx']
        section('4096 samples of the ring', 4096, frames, dict(cols=COLS, index=s_idx))
    elif sec.startswith('u8_'):
        n = int(sec[3:])
        bitmap = info['lidar_bitmap']
        images = bitmap.repeat((n + bitmap.shape[0] - 1) // bitmap.shape[0], 1, 1)[:n].contiguous()    # real FILL images, repeated
        section('%d envs\' uint8 bitmaps' % n, n, images, {})
        del images

assert env.eng.device_errors() == 0
env.close()
