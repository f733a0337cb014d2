"""One whole SACAgent.update through the library (tests/update_cases.py: LibAgent, the modules and the order of examples/sac_update.py)
against the mirror that test_update_cpu.py pins on the reference's own update.

Every phase is evaluated three ways from the library's own parameters (teacher forcing, per phase): by the library, by the fp32 mirror
on the GPU (the reference's arithmetic on this stack) and by the fp64 mirror on the CPU (the truth).  With e = ||x - x64|| / ||x64||
every forward quantity and every gradient tensor must keep e_lib <= 8 * max(e_torch32, 2^-23): e_torch32 is the framework's own error
on the same parameters, batch and draws, measured here, and the factor is a formula -- the library's longest chain is 784 sequential
fmaf's with an expected rounding error near sqrt(784) u, a GEMM blocked b wide stands near sqrt(784 / b) u, and sqrt(b) <= 8 up to
b = 64.  At on = 1.0 the batches are quiet: e_torch32 <= 1e-5 everywhere (a ReLU or a side of the min that the reference's own
arithmetic flips would fail that instead of widening the tolerance).  Config (c) feeds 0 / 255 as update() does: there tanh
saturates under the 1e-6 guard, e_torch32 reaches 1e-2, the cap is 5e-2, and the config is a structural check only.

    config  image    conv1 -> conv2 -> conv3   F    H   A   n   on     reaches
    a       68 x 76  16x18 -> 7x8 -> 5x6       960  96  16  24  1.0    two words per row with tail bits; two dense segments (784 + 176); a
                                                                        partial 64-output tile; F + A = 976, the 16-byte path
    b       68 x 76  as a                      960  96  15  24  1.0    F + A = 975: 4-byte accesses on the critics' view and its gradient
    c       68 x 76  as a                      960  96  16  24  255.0  what update() feeds
    d       44 x 44  10x10 -> 4x4 -> 2x2       128  64  16  3   1.0    one segment shorter than the default; a batch below one wave's rows

Seeds (chosen on the CPU, fp32 against fp64 mirror, profiles/r19_update.txt): the quiet seeds on which both critics win the min in
some row of the three updates.  Exact checks ride along: every Adam step and soft update `==` tests/optim_cases.py on the .grad
captured in front of it, the gradients the actor's loss leaves in the critics and their removal by the next zero_grad, repeatability
from a snapshot, acting against learning, batch independence, the ring's -1 row, SAL's own shape on g24's batch, and the example."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import optim_cases as oc
import update_cases as uc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = dict(a=6, b=5, c=5, d=4)
FACTOR, FLOOR, QUIET, LOUD = 8.0, 2.0 ** -23, 1e-5, 5e-2


def _kw(c):
    return dict(rows=c['rows'], cols=c['cols'], hidden=c['hidden'], action_dim=c['action_dim'], on=c['on'])


def _agents(c, seed):
    """(the library agent, the fp32 mirror on the GPU whose tensors it shares, the fp64 mirror on the CPU)."""
    import torch
    m32 = uc.MirrorAgent(dtype=torch.float32, device='cuda', seed=seed, **_kw(c))
    m64 = uc.MirrorAgent(dtype=torch.float64, device='cpu', **_kw(c))
    lib = uc.LibAgent.from_mirror(m32, c['cols'])
    for name, mod in lib.modules().items():
        shared = {uc.lib_key(k): p for k, p in mod.named_parameters()}
        assert list(shared) == uc.keys_of(name) and all(shared[k] is m32.net(name).get_parameter(k) for k in shared)
    return lib, m32, m64


def _batches(c, b):
    import torch
    return uc.lib_batch(b), uc.mirror_batch(b, c['on'], torch.float32, 'cuda'), uc.mirror_batch(b, c['on'], torch.float64, 'cpu')


def _judge(tag, got, t32, t64, cap, keys=None):
    """The tolerance rule on every key of the fp64 result -> the lines of those that miss it (printed: e_torch32, e_lib, ratio)."""
    missed = []
    for k in (sorted(t64) if keys is None else keys):
        e32, el = uc.rel_err(t32[k], t64[k]), uc.rel_err(got[k], t64[k])
        line = '%s %-34s e_torch32 %.3e e_lib %.3e ratio %.3f' % (tag, k, e32, el, el / max(e32, FLOOR))
        print(line)
        if not el <= FACTOR * max(e32, FLOOR):
            missed.append(line + '  ABOVE %g' % FACTOR)
        if not e32 <= cap:
            missed.append(line + '  e_torch32 ABOVE the cap %g: not a quiet batch' % cap)
    return missed


class _Steps:
    """The hook of LibAgent's phases: in front of each step() it keeps .grad, the parameters, moments, targets and the device state;
    check() then compares what the step left with tests/optim_cases.py, bit for bit."""

    def __init__(self, lib, grads_only=False):
        self.lib, self.seen, self.grads_only = lib, {}, grads_only

    def __call__(self, name, opt):
        mods = self.lib.modules()
        names = [k for k, _ in mods[name].named_parameters()]
        assert len(names) == len(opt.params) == (12 if name == 'actor' else 10) and all(p is q for p, (_, q) in zip(opt.params, mods[name].named_parameters()))
        if self.grads_only:
            self.seen[name] = dict(grads=self.lib.grads(name))
            return
        target = None if name == 'actor' else dict(mods[name + '_target'].named_parameters())
        host = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
        self.seen[name] = dict(
            names=names, grads=self.lib.grads(name), g=[host(p.grad) for p in opt.params], p=[host(p) for p in opt.params],
            m=[host(opt.moments(i)[0]) for i in range(len(names))], v=[host(opt.moments(i)[1]) for i in range(len(names))],
            t=None if target is None else [host(target[k]) for k in names], state=opt.device_state())

    def check(self, name):
        opt, s = self.lib.optimizers()[name], self.seen[name]
        t, pow1, pow2, k2, a = s['state']
        state = dict(t=t, pow1=pow1, pow2=pow2, k2=np.float32(k2), a=np.float32(a))
        ps, ms, vs, ts, state = oc.run(s['p'], [s['g']], targets=s['t'], state=state, moments=(s['m'], s['v']))
        bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
        host = lambda x: x.detach().cpu().numpy()  # noqa: E731
        target = None if name == 'actor' else dict(self.lib.modules()[name + '_target'].named_parameters())
        for i, k in enumerate(s['names']):
            assert np.array_equal(bits(host(opt.params[i])), bits(ps[i])), (name, k, 'parameter')
            assert np.array_equal(bits(host(opt.moments(i)[0])), bits(ms[i])) and np.array_equal(bits(host(opt.moments(i)[1])), bits(vs[i])), (name, k, 'moments')
            assert (ps[i] != s['p'][i]).any(), (name, k, 'was not stepped')
            if target is not None:                                      # paired by name, moved once from the parameter just written
                assert np.array_equal(bits(host(target[k])), bits(ts[i])) and (ts[i] != s['t'][i]).any(), (name, k, 'target')
        assert np.array_equal(opt._state.cpu().numpy(), oc.state_words(state)) and state['t'] == t + 1, (name, 'device state')


def _unchanged(before, after, nets):
    import torch
    for n in nets:
        assert all(torch.equal(before['params'][n][k], after['params'][n][k]) for k in before['params'][n]), n
        if n in before['opt']:
            assert all(torch.equal(x, y) for x, y in zip(before['opt'][n], after['opt'][n])), n


def _lib_flat(out, steps, nets):
    flat = uc.flatten(out)
    for n in nets:
        flat.update({'grads.%s.%s' % (n, k): g for k, g in steps.seen[n]['grads'].items()})
    return flat


@pytest.mark.parametrize('config', sorted(uc.CONFIGS))
def test_three_updates_against_the_mirror(config):
    """Three teacher-forced updates of one config: the tolerance rule on every forward quantity and gradient of both phases, the
    quiet-batch cap, every step against optim_cases, what the actor's loss leaves in the critics, and nothing else changed.  (c) is a
    structural check only (module docstring)."""
    import torch
    c, seed = uc.CONFIGS[config], SEEDS[config]
    cap = QUIET if c['on'] == 1.0 else LOUD
    lib, m32, m64 = _agents(c, seed)
    F, A = uc.feature_width(c['rows'], c['cols']), c['action_dim']
    assert lib.critics[0].head.fc1.weight.shape == (c['hidden'], F + A) and lib.actor.fc1.weight.shape == (c['hidden'], F)
    assert (F, -(-c['cols'] // 64), (F + A) % 4) == {'a': (960, 2, 0), 'b': (960, 2, 3), 'c': (960, 2, 0), 'd': (128, 1, 0)}[config]
    missed, sides = [], set()
    for u in range(uc.UPDATES):
        b = uc.batch(1000 * seed + u, c['n'], c['rows'], c['cols'], A, c['pool'])
        bl, b32, b64 = _batches(c, b)
        tag = '%s u%d' % (config, u)
        # ---- the critics
        m64.load_from(m32)
        c64, c32 = m64.critic_phase(b64, b64['eps_next']), m32.critic_phase(b32, b32['eps_next'])
        with torch.no_grad():
            tq = [m64.net(n)(b64['ns'], c64['next_a']) for n in ('critic1_target', 'critic2_target')]
            sides |= {('target', bool(x)) for x in (tq[0] < tq[1]).reshape(-1)}
        steps, before = _Steps(lib), lib.snapshot()
        out = lib.critic_phase(bl, bl['eps_next'], hook=steps)
        missed += _judge(tag + ' critic', _lib_flat(out, steps, ('critic1', 'critic2')), uc.flatten(c32), uc.flatten(c64), cap)
        steps.check('critic1')
        steps.check('critic2')
        after = lib.snapshot()
        _unchanged(before, after, ('actor',))
        # ---- the actor, from the critics the library just stepped
        m64.load_from(m32)
        a64, a32 = m64.actor_phase(b64, b64['eps_new']), m32.actor_phase(b32, b32['eps_new'])
        with torch.no_grad():
            qs = [m64.net(n)(b64['s'], a64['new_a']) for n in ('critic1', 'critic2')]
            sides |= {('actor', bool(x)) for x in (qs[0] < qs[1]).reshape(-1)}
        steps_a = _Steps(lib)
        out = lib.actor_phase(bl, bl['eps_new'], hook=steps_a)
        keys = [k for k in uc.flatten(a64) if not k.startswith('grads.critic')]
        missed += _judge(tag + ' actor ', _lib_flat(out, steps_a, ('actor',)), uc.flatten(a32), uc.flatten(a64), cap, keys)
        steps_a.check('actor')
        _unchanged(after, lib.snapshot(), ('critic1', 'critic2', 'critic1_target', 'critic2_target'))
        # the actor's loss flows into the critics' .grad, on top of what their own loss left, as in the reference
        left = {'grads.%s.%s' % (n, k): g for n in ('critic1', 'critic2') for k, g in lib.grads(n).items()}
        want = [{'grads.%s.%s' % (n, k): cp['grads'][n][k] + ap['grads'][n][k] for n in ('critic1', 'critic2') for k in uc.CRITIC_KEYS}
                for cp, ap in ((c32, a32), (c64, a64))]
        assert all(not torch.equal(left['grads.%s.%s' % (n, k)], steps.seen[n]['grads'][k]) for n in ('critic1', 'critic2') for k in uc.CRITIC_KEYS
                   if float(a64['grads'][n][k].abs().max()) > 0)
        missed += _judge(tag + ' left  ', left, want[0], want[1], cap)
    assert sides == {('target', True), ('target', False), ('actor', True), ('actor', False)}, sides
    assert not missed, '\n' + '\n'.join(missed)


def _one_update(lib, bl):
    """critic_phase + actor_phase -> everything they return, the gradients in front of each step and the snapshot after."""
    steps = _Steps(lib)
    out = lib.critic_phase(bl, bl['eps_next'], hook=steps)
    out.update(lib.actor_phase(bl, bl['eps_new'], hook=steps))
    flat = _lib_flat(out, steps, uc.TRAINED)
    snap = lib.snapshot()
    for n, nets in snap['params'].items():
        flat.update({'after.%s.%s' % (n, k): v for k, v in nets.items()})
    for n, (m, v, s) in snap['opt'].items():
        flat.update({'opt.%s.m' % n: m, 'opt.%s.v' % n: v, 'opt.%s.state' % n: s})
    return flat


def test_an_update_repeats_bit_for_bit():
    """Two updates, a snapshot of parameters, targets, moments and step state in between; restoring it and running the second update
    again gives the same bits in every output, gradient, parameter, moment and state word."""
    import torch
    c, seed = uc.CONFIGS['b'], SEEDS['b']
    lib, _, _ = _agents(c, seed)
    first, second = (uc.lib_batch(uc.batch(1000 * seed + u, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])) for u in range(2))
    _one_update(lib, first)
    snap = lib.snapshot()
    one = _one_update(lib, second)
    lib.restore(snap)
    two = _one_update(lib, second)
    assert sorted(one) == sorted(two) and len(one) > 100
    assert [k for k in one if not torch.equal(one[k], two[k])] == []
    assert not torch.equal(one['after.critic1.fc1.weight'], snap['params']['critic1']['fc1.weight']) and int(one['opt.actor.state'][0]) == 2


def test_acting_equals_learning_and_rows_do_not_depend_on_the_batch():
    """actor.sample under no_grad (Trunk's fused acting path) and with gradients (the learning path) on the same draws are
    torch.equal in action and log_prob; row i run alone through actor.sample and through twin_q(dense=True) equals row i of the batch,
    for the ring's -1 row too."""
    import torch
    from red_gym_amd.qhead import twin_q
    for config in ('a', 'd'):
        c, seed = uc.CONFIGS[config], SEEDS[config]
        lib, _, _ = _agents(c, seed)
        b = uc.batch(1000 * seed, c['n'], c['rows'], c['cols'], c['action_dim'], c['pool'])
        bl = uc.lib_batch(b)
        with torch.no_grad():
            act, act_lp = lib.actor.sample(bl['frames'], bl['s_idx'], bl['eps_new'])
        learn, learn_lp = lib.actor.sample(bl['frames'], bl['s_idx'], bl['eps_new'])
        assert act.grad_fn is None and learn.grad_fn is not None and act.dtype == torch.float64 and act_lp.shape == (c['n'],)
        assert torch.equal(act, learn) and torch.equal(act_lp, learn_lp) and not torch.equal(act[0], act[1])
        heads = uc._heads(lib.critics)
        with torch.no_grad():
            q, qmin = twin_q([k.trunk(bl['frames'], bl['s_idx']) for k in lib.critics], act, *heads, dense=True)
            for i in sorted({0, b['hole'], c['n'] - 1}):
                idx = bl['s_idx'][i:i + 1]
                a1, lp1 = lib.actor.sample(bl['frames'], idx, bl['eps_new'][i:i + 1])
                q1, qmin1 = twin_q([k.trunk(bl['frames'], idx) for k in lib.critics], a1, *heads, dense=True)
                assert torch.equal(a1[0], act[i]) and torch.equal(lp1[0], act_lp[i]), (config, i)
                assert torch.equal(q1[:, 0], q[:, i]) and torch.equal(qmin1[0], qmin[i]), (config, i)


def test_the_hole_adds_nothing_to_conv1_weight():
    """The ring's "no transition" row (index -1): its features are those of an all-zero frame, bit for bit; and n * conv1.weight.grad
    of the batch equals (n - 1) * that of the batch without the row (the losses are means), under the tolerance rule with the fp64
    mirror's full-batch gradient as the truth, for the critics' loss and for the actor's."""
    import torch
    c, seed = uc.CONFIGS['a'], SEEDS['a']
    n = c['n']
    b = uc.batch(1000 * seed, n, c['rows'], c['cols'], c['action_dim'], c['pool'])
    less = uc.without_row(b, b['hole'])
    results = {}
    for which, bb in (('full', b), ('less', less)):
        lib, m32, m64 = _agents(c, seed)
        bl, b32, b64 = _batches(c, bb)
        m64.load_from(m32)
        if which == 'full':
            zero = torch.cat([bl['frames'], torch.zeros_like(bl['frames'][:1])])
            at = torch.tensor([c['pool']], device='cuda')
            with torch.no_grad():
                for net in [lib.actor] + lib.critics:
                    f = net.trunk(bl['frames'], bl['s_idx'])
                    assert torch.equal(f[b['hole']], net.trunk(zero, at)[0]) and not torch.equal(f[b['hole']], f[0])
        rows = int(bb['a'].shape[0])
        c64, c32 = m64.critic_phase(b64, b64['eps_next']), m32.critic_phase(b32, b32['eps_next'])
        steps = _Steps(lib)
        lib.critic_phase(bl, bl['eps_next'], hook=steps)
        m64.load_from(m32)
        a64, a32 = m64.actor_phase(b64, b64['eps_new']), m32.actor_phase(b32, b32['eps_new'])
        lib.actor_phase(bl, bl['eps_new'], hook=steps)
        for net, p64, p32 in (('critic1', c64, c32), ('critic2', c64, c32), ('actor', a64, a32)):
            results[which, net] = tuple(g * rows for g in (steps.seen[net]['grads']['conv1.weight'], p32['grads'][net]['conv1.weight'], p64['grads'][net]['conv1.weight']))
    for net in uc.TRAINED:
        truth = results['full', net][2]
        e32, el = uc.rel_err(results['less', net][1], truth), uc.rel_err(results['less', net][0], truth)
        print('%s: (n - 1) grad without the row against n grad64 with it: e_torch32 %.3e e_lib %.3e' % (net, e32, el))
        # (in fp64 the two agree to 1e-12 on equal parameters, test_update_cpu.py; here the critics the actor's loss reads were stepped
        # from gradients that differ by n / (n - 1), which Adam's eps = 1e-8 turns into steps that differ by 1e-8 / |g| of lr)
        assert uc.rel_err(results['less', net][2], truth) <= 1e-7 and e32 <= QUIET
        assert el <= FACTOR * max(e32, FLOOR)


def test_sal_shape_on_the_recorded_batch(golden):
    """256 x 256, F = 25 088, H = 512, A = 16, n = 8, on = 255 on g24's batch and draws, the parameters rebuilt from its seed: one
    teacher-forced update under the tolerance rule with the 5e-2 cap; and the library's tv, cq and critic losses lie within 8 *
    max(||recorded - m64||, 2^-23 ||m64||) of what the reference's own update recorded."""
    import torch
    g = golden('g24_update.npz')
    c = dict(uc.SAL, on=255.0, n=8)
    lib, m32, m64 = _agents(c, int(g['seed']))
    b = uc.golden_batch(g)
    bl, b32, b64 = _batches(c, b)
    m64.load_from(m32)
    w = m64.net('critic2').fc1.weight.double()
    assert abs(w.sum().item() - g['critic2/fc1.weight/init'][0]) <= 2.0 ** -40 * w.abs().sum().item()
    c64, c32 = m64.critic_phase(b64, b64['eps_next']), m32.critic_phase(b32, b32['eps_next'])
    steps = _Steps(lib, grads_only=True)
    out = lib.critic_phase(bl, bl['eps_next'], hook=steps)
    missed = _judge('sal critic', _lib_flat(out, steps, ('critic1', 'critic2')), uc.flatten(c32), uc.flatten(c64), LOUD)
    recorded = {'tv': g['tv'], 'cq.0': g['cq1'], 'cq.1': g['cq2'], 'c_loss.0': g['losses'][1], 'c_loss.1': g['losses'][2]}
    flat, f64 = uc.flatten(out), uc.flatten(c64)
    for k, rec in recorded.items():
        truth = f64[k].numpy().astype(np.float64).reshape(-1)
        rec = np.asarray(rec, np.float64).reshape(-1)
        d = float(np.linalg.norm(flat[k].detach().cpu().numpy().astype(np.float64).reshape(-1) - rec))
        bound = FACTOR * max(float(np.linalg.norm(rec - truth)), FLOOR * float(np.linalg.norm(truth)))
        print('sal recorded %-10s ||lib - recorded|| %.3e bound %.3e' % (k, d, bound))
        if not d <= bound:
            missed.append('%s: %.3e from the recording, bound %.3e' % (k, d, bound))
    m64.load_from(m32)
    a64, a32 = m64.actor_phase(b64, b64['eps_new']), m32.actor_phase(b32, b32['eps_new'])
    steps_a = _Steps(lib, grads_only=True)
    out = lib.actor_phase(bl, bl['eps_new'], hook=steps_a)
    keys = [k for k in uc.flatten(a64) if not k.startswith('grads.critic')]
    missed += _judge('sal actor ', _lib_flat(out, steps_a, ('actor',)), uc.flatten(a32), uc.flatten(a64), LOUD, keys)
    assert not missed, '\n' + '\n'.join(missed)


def test_the_example_runs():
    """examples/sac_update.py 64 12 16 in a fresh child process: exit 0, three finite update lines, and both column ranges of a
    critic's one fc1.weight.grad filled."""
    import math
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'sac_update.py'), '64', '12', '16'], cwd=ROOT, capture_output=True, text=True,
                          timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    updates = [line for line in proc.stdout.splitlines() if line.startswith('update ')]
    assert len(updates) == 3, proc.stdout
    for line in updates:
        found = re.fullmatch(r'update \d: actor loss (\S+), critic losses (\S+) (\S+)', line)
        assert found and all(math.isfinite(float(v)) for v in found.groups()), line
    assert 'feature columns filled: True, action columns filled: True' in proc.stdout
