"""Generates tests/golden/g20_head.npz from the reference's own Actor (src/SAL.py:390-421) on the CPU: the features h = relu(fc1(.))
that reach the head, the draws eps of rsample, and what Actor.forward and Actor.sample return, in six groups of 16 rows that drive
the head through its branches (policyhead_cases.GROUPS): the default initialisation, fc_mean.weight x 40, fc_log_std.weight x 400
(high clamp and saturation), fc_log_std.bias + 1.9 (saturation), - 19.9 and - 25 (low clamp).  The fixture holds data only: the
default head's weights, the per-group fp32 scalars applied to them, inputs, recorded outputs and the Actor's state-dict keys.
Run through make_golden.py, whose g20 row says which of these arrays follow the host's CPU kernels.
"""
import numpy as np
import torch

import reference
import policyhead_cases as ph

# per group: fc_mean.weight *=, fc_log_std.weight *=, fc_log_std.bias +=
MODS = ((1.0, 1.0, 0.0), (40.0, 1.0, 0.0), (1.0, 400.0, 0.0), (1.0, 1.0, 1.9), (1.0, 1.0, -19.9), (1.0, 1.0, -25.0))


def g20_head():
    sal = reference.load_sal()
    torch.manual_seed(20)
    torch.set_num_threads(1)
    actor = sal.Actor(action_dim=16)
    base = {k: v.clone() for k, v in actor.state_dict().items()}
    rng = np.random.default_rng(20)
    R, A = ph.GROUP_ROWS, 16
    rec = {k: [] for k in ('h', 'eps', 'mean', 'log_std', 'action', 'log_prob', 'seed')}
    feats = []
    hook = actor.fc1.register_forward_hook(lambda mod, inp, out: feats.append(torch.relu(out).detach().clone()))
    for gi, (ms, ls, shift) in enumerate(MODS):
        actor.load_state_dict(base)
        with torch.no_grad():
            actor.fc_mean.weight.mul_(ms)
            actor.fc_log_std.weight.mul_(ls)
            actor.fc_log_std.bias.add_(shift)
        # two-valued 256 x 256 images of random blocks of 8 x 8 pixels: even rows as select_action feeds them (FloatTensor(state) /
        # 255, :510), odd rows of every group but the default one as update() does (the raw 0 / 255 floats, :536): features some hundred times larger
        blocks = rng.random((R, 1, 32, 32)) < rng.uniform(0.2, 0.8, (R, 1, 1, 1))
        on = np.where((np.arange(R) % 2 == 1) & (gi > 0), 255.0, 1.0).reshape(R, 1, 1, 1)
        x = torch.from_numpy((np.kron(blocks, np.ones((8, 8))) * on).astype(np.float32))
        seed = 1000 + gi
        with torch.no_grad():
            feats.clear()
            mean, log_std = actor(x)
            torch.manual_seed(seed)
            y, lp = actor.sample(x)
            torch.manual_seed(seed)
            eps = torch.distributions.Normal(torch.zeros_like(mean), torch.ones_like(mean)).rsample()
            assert torch.equal(torch.tanh(mean + log_std.exp() * eps), y), 'the recovered draws do not reproduce the reference action'
        rec['h'].append(feats[-1].numpy())
        rec['eps'].append(eps.numpy())
        rec['mean'].append(mean.numpy())
        rec['log_std'].append(log_std.numpy())
        rec['action'].append(y.numpy())
        rec['log_prob'].append(lp.numpy()[:, 0])
        rec['seed'].append(seed)
    hook.remove()
    out = {k: np.concatenate(v) if k != 'seed' else np.array(v, np.int64) for k, v in rec.items()}
    y, ls = out['action'], out['log_std']
    sat, hi, lo = np.abs(y) == 1.0, ls == 2.0, ls == -20.0
    share = {name: float(m.mean()) for name, m in (('saturated', sat), ('high clamp', hi), ('low clamp', lo), ('untouched', ~(sat | hi | lo)))}
    print(share)
    assert min(share['saturated'], share['high clamp'], share['low clamp']) >= 0.05 and share['untouched'] >= 0.20, share
    out.update(w_mean=base['fc_mean.weight'].numpy(), b_mean=base['fc_mean.bias'].numpy(), w_log_std=base['fc_log_std.weight'].numpy(),
               b_log_std=base['fc_log_std.bias'].numpy(), mean_scale=np.array([m[0] for m in MODS], np.float32),
               log_std_scale=np.array([m[1] for m in MODS], np.float32), log_std_shift=np.array([m[2] for m in MODS], np.float32),
               keys=np.array(list(base.keys())))
    assert all(v.dtype == np.float32 for k, v in out.items() if k not in ('seed', 'keys'))
    reference.save('g20_head.npz', **out)
