"""Closed loop of shaper + path follower + replay buffer in which the policy's stem reads bits: acting on the env's uint8
lidar_bitmap through conv1 + relu + conv2 in one kernel, conv3 and fc1 of the framework, and the policy's head (fc_mean, fc_log_std,
the sampling tail) in one kernel that writes the fp64 actions the path follower reads; and learning from the ring's packed frames
through the same modules with grad on, without an fp32 image ever existing.
    python examples/policy_features.py [envs] [steps]
The reference's Actor opens with nn.Conv2d(1, 16, kernel_size=8, stride=4) (src/SAL.py:397) on FloatTensor(state) / 255 (:510) when
it acts and on the raw 0 / 255 images when it learns (:536).  BitConv2d shares that layer's parameters and computes it from bits;
BitConvStem does the same for the pair conv1, conv2 = nn.Conv2d(16, 32, kernel_size=4, stride=2) (:398) that both networks continue
with, fused when it acts.  conv3 (:399) and fc1 (:400, sized to this image) are stock layers; PolicyHead is fc_mean, fc_log_std
(:401-402) and Actor.sample's tail (:414-421)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from red_gym_amd import F110VecEnv, workload
from red_gym_amd.bitconv import BitConv2d, BitConvStem
from red_gym_amd.policyhead import PolicyHead

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
env.shape_rewards()
env.follow_paths()
env.record_replay(capacity=16 * B)
torch.manual_seed(0)
conv1 = torch.nn.Conv2d(1, 16, kernel_size=8, stride=4).to(env.device)          # the reference's Actor.conv1
act_layer = BitConv2d.from_conv(conv1, on=1.0, relu=True)                      # select_action: state / 255
learn_layer = BitConv2d.from_conv(conv1, on=255.0, relu=True, cols=env.eng.shaper.cfg.cols)   # update: the raw 0 / 255 floats
conv2 = torch.nn.Conv2d(16, 32, kernel_size=4, stride=2).to(env.device)         # the reference's Actor.conv2
stem = BitConvStem.from_convs(conv1, conv2, on=1.0, cols=env.eng.shaper.cfg.cols)   # relu(conv2(relu(conv1(x)))), the same four tensors
conv3 = torch.nn.Conv2d(32, 32, kernel_size=3, stride=1).to(env.device)         # the reference's Actor.conv3
obs, reward, done, info = env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
with torch.no_grad():
    width = conv3(stem(info['lidar_bitmap'][:1])).numel()
fc1 = torch.nn.Linear(width, 512).to(env.device)                                # the reference's Actor.fc1
head = PolicyHead(512, 16).to(env.device)                                       # fc_mean, fc_log_std and the tail of Actor.sample


def features(frames, index=None):
    return torch.relu(fc1(torch.relu(conv3(stem(frames, index=index))).flatten(1)))


raw = torch.zeros((B, 16), dtype=torch.float64, device=env.device)              # the static buffer a captured step would read
for k in range(STEPS):
    with torch.no_grad():
        feats = stem(info['lidar_bitmap'])                                         # [B, 32, 30, 30]: fused, conv1's [B, 16, 63, 63] is never written
        h = torch.relu(fc1(torch.relu(conv3(feats)).flatten(1)))
        head.sample(h, out=raw)                                                    # one kernel: tanh(mean + std * eps) in fp64, into raw
    obs, reward, done, info = env.step(env.path_actions(raw))
print('acting: lidar_bitmap %s %s -> features %s %s' % (tuple(info['lidar_bitmap'].shape), info['lidar_bitmap'].dtype, tuple(feats.shape), feats.dtype))
n = 64
batch = env.replay.sample_frames(n)
frames, s_idx, ns_idx, r, ok = (batch[k] for k in ('frames', 's_idx', 'ns_idx', 'r', 'ok'))
f_s, f_ns = learn_layer(frames, index=s_idx), learn_layer(frames, index=ns_idx)
loss = ((f_s.mean(dim=(1, 2, 3)) - r.float()) ** 2).mean() + f_ns.mean()
loss.backward()
print('learning: frames %s %s (a view of the ring), %d of %d draws valid -> features %s, grad weight %s, grad bias %s'
      % (tuple(frames.shape), frames.dtype, int(ok.sum()), n, tuple(f_s.shape), tuple(conv1.weight.grad.shape), tuple(conv1.bias.grad.shape)))
f2 = stem(frames, index=s_idx)                                                     # grad on: conv_bits -> F.conv2d -> relu, differentiable
f2.mean().backward()
new_a, logp, mean, log_std = head.sample(features(frames, index=s_idx))             # one sample with gradients, as update() takes (:564)
(0.2 * logp - new_a.sum(dim=1)).mean().backward()                                 # (the critics: examples/sac_update.py)
print('head: actions %s %s, log_prob %s, grad fc_mean.weight %s, grad fc1.weight %s'
      % (tuple(new_a.shape), new_a.dtype, tuple(logp.shape), tuple(head.fc_mean.weight.grad.shape), tuple(fc1.weight.grad.shape)))
print('stem: acting features %s (no grad_fn: %s), learning features %s, grad conv2.weight %s' % (tuple(feats.shape), feats.grad_fn is None, tuple(f2.shape), tuple(conv2.weight.grad.shape)))
rows, cols = env.eng.shaper.cfg.rows, env.eng.shaper.cfg.cols
print('bytes not moved: acting %.1f MB per step (the fp32 copy of %d bitmaps, written and read again), learning %.1f MB per batch '
      '(two fp32 images per transition, written and read again)' % (2 * B * rows * cols * 4 / 1e6, B, 2 * 2 * n * rows * cols * 4 / 1e6))
env.close()
