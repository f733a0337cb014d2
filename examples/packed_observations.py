"""The SAC wrapper's closed loop with the observation held as bits from the renderer on: shape_rewards(image='bits') draws the
FILL bitmap as one bit per pixel (f110_bitmap_render_bits), the shaper reads bits, the replay push copies them into the ring
(whose frames are this format), and the policy's stem acts on info['lidar_bitmap_bits'] -- no byte image is ever written.
    python examples/packed_observations.py [envs] [steps] [bytes|bits]
info['lidar_bitmap_bits'] is int64 [B, rows, ceil(cols / 64)]: bit k of word w of a row = pixel 64 w + k is 255;
replay.unpack_bitmaps(info['lidar_bitmap_bits'], cols) gives the byte image back where one is wanted (a plot, a check)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import F110VecEnv, replay, workload
from red_gym_amd.bitconv import BitConvStem
from red_gym_amd.policyhead import PolicyHead

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
IMAGE = sys.argv[3] if len(sys.argv) > 3 else 'bits'
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.shape_rewards(image=IMAGE)
env.follow_paths()
env.record_replay(capacity=16 * B)
rows, cols = env.eng.shaper.cfg.rows, env.eng.shaper.cfg.cols
key = 'lidar_bitmap_bits' if IMAGE == 'bits' else 'lidar_bitmap'
torch.manual_seed(0)
stem = BitConvStem(cols=cols, device=env.device)                                  # the reference's Actor.conv1 + conv2, from bits
conv3 = torch.nn.Conv2d(32, 32, kernel_size=3, stride=1).to(env.device)
obs, reward, done, info = env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
with torch.no_grad():
    width = conv3(stem(info[key][:1])).numel()
fc1 = torch.nn.Linear(width, 512).to(env.device)
head = PolicyHead(512, 16).to(env.device)
raw = torch.zeros((B, 16), dtype=torch.float64, device=env.device)
total = torch.zeros((B,), dtype=torch.float64, device=env.device)
for k in range(STEPS):
    with torch.no_grad():
        feats = stem(info[key])                                                    # the same kernel reads either form
        head.sample(torch.relu(fc1(torch.relu(conv3(feats)).flatten(1))), out=raw)
    obs, reward, done, info = env.step(env.path_actions(raw))
    total += reward
print('%d envs, %d steps, image=%r: %s %s %s -> features %s; mean return %.2f, %d valid transitions held'
      % (B, STEPS, IMAGE, key, tuple(info[key].shape), info[key].dtype, tuple(feats.shape), float(total.mean()), len(env.replay)))
if IMAGE == 'bits':
    img = replay.unpack_bitmaps(info[key][:4], cols)
    print('unpack_bitmaps of 4 of them: %s %s, values %s' % (tuple(img.shape), img.dtype, sorted(int(v) for v in img.unique())))
held = env.eng.shaper.buf['bitmap']
for image, size in (('bytes', B * rows * cols), ('bits', B * rows * replay.words(cols) * 8)):
    print('observation buffer as %-5s: %9.1f MB written by the render and read by the push every step%s'
          % (image, size / 1e6, '   <- this run (%.1f MB held)' % (held.numel() * held.element_size() / 1e6) if image == IMAGE else ''))
print('ring: %.1f MB of frames either way (the ring is bits)' % (env.replay.buf['frames'].numel() * 8 / 1e6))
assert env.eng.device_errors() == 0
env.close()
