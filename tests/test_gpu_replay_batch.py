"""The replay batch as one record (ReplayBuffer.sample_frames_dev / sample_priority_dev / frames_at return dicts under sample_out's names):
for nstep 1 and 3, priorities off and on, stack 1 and 3 on the stack tests' scripted ring (T = 5, B = 7, wrapped, with resets inside it)
the returned keys are tests/test_replay_fields_cpu.py's table plus 'frames', the tensors are `out`'s own, `out` gains nothing, s_idx and
ns_idx are column 0 of the stacks, and every field `==` frames_at(indices); and SACAgent hands the target gamma by value with nstep = 1
-- with a priority draw's 'discount' column beside it too -- and the discounts per row with nstep = 3."""
import pytest

import nstep_cases as nc
import replay_cases as rc
import stack_cases as sc
import update_cases as uc
from test_gpu_nstep import _ring
from test_gpu_sac_agent import _ring_env
from test_replay_fields_cpu import COMBOS, TABLE

pytestmark = pytest.mark.gpu

G = nc.GAMMA
N = 64


@pytest.mark.parametrize('nstep,priorities,stack', COMBOS)
def test_a_drawn_batch_is_the_table_on_outs_tensors_and_equals_frames_at(assets, nstep, priorities, stack):
    import torch
    env = _ring(assets, sc.base_ring())
    rp = env.replay
    if priorities:
        rp.set_priorities(True)
    want = TABLE[(nstep, priorities, stack)]
    draw = rp.sample_priority_dev if priorities else rp.sample_frames_dev
    counter = torch.zeros((1,), dtype=torch.int64, device=env.device)
    out = rp.sample_out(N, nstep, priorities, stack)
    assert sorted(out) == sorted(want)
    kept = dict(out)
    batch = draw(N, counter, seed=rc.DRAW_CASE['seed'], out=out, nstep=nstep, gamma=G, stack=stack)
    assert int(counter) == N and sorted(batch) == sorted(list(want) + ['frames'])
    # a new dict on out's own tensors; out itself is as it was and holds no view of the ring
    assert batch is not out and 'frames' not in out and sorted(out) == sorted(kept) and all(out[k] is kept[k] for k in kept)
    for k, (_, dt) in want.items():
        assert batch[k] is out[k] and batch[k].data_ptr() == out[k].data_ptr() and batch[k].dtype == getattr(torch, dt), k
    frames = rp.frame_view()
    assert batch['frames'].data_ptr() == frames.data_ptr() and batch['frames'].shape == frames.shape
    assert tuple(batch['s_idx'].shape) == tuple(batch['ns_idx'].shape) == (N,) and bool(batch['ok'].any())
    if stack > 1:
        assert torch.equal(batch['s_stack'][:, 0], batch['s_idx']) and torch.equal(batch['ns_stack'][:, 0], batch['ns_idx'])
        assert tuple(batch['s_stack'].shape) == tuple(batch['ns_stack'].shape) == (N, stack) and tuple(batch['depth'].shape) == (2, N)
    # without out=: a batch of the same names on tensors of its own
    fresh = draw(N, counter, seed=rc.DRAW_CASE['seed'], nstep=nstep, gamma=G, stack=stack)
    assert sorted(fresh) == sorted(batch) and fresh['indices'].data_ptr() != batch['indices'].data_ptr() and int(counter) == 2 * N
    # field by field what frames_at gives for the drawn indices
    at = rp.frames_at(batch['indices'], nstep=nstep, gamma=G, stack=stack)
    assert sorted(at) == sorted(list(TABLE[(nstep, False, stack)]) + ['frames'])
    assert at['frames'].data_ptr() == batch['frames'].data_ptr() and at['frames'].shape == batch['frames'].shape
    for k in TABLE[(nstep, False, stack)]:
        g, w = batch[k], at[k]
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), k
    if priorities:                                                               # the walk's columns are there whatever nstep is
        walk = rp.nstep_at(batch['indices'], nstep, G)
        assert all(torch.equal(batch[k], w) for k, w in zip(('ns_idx', 'r', 'd', 'discount', 'span'), walk))
    assert env.eng.device_errors() == 0
    env.close()


TINY = dict(rows=36, cols=36, hidden=32, action_dim=16, on=1.0)                  # 36 x 36: conv3 leaves one pixel


@pytest.mark.parametrize('nstep,per', [(1, False), (1, True), (3, False)])
def test_the_target_takes_gamma_by_value_unless_nstep_walks(assets, monkeypatch, nstep, per):
    """One update of batch 8: td_target's discount is the Python float gamma with nstep = 1 -- with per=True as well, where the draw
    wrote a 'discount' column, which stays in agent.sample -- and the batch's [8] fp64 'discount' with nstep = 3."""
    import torch
    from red_gym_amd import SACAgent, sac
    n = 8
    env = _ring_env(assets, TINY)
    if per:
        env.replay.set_priorities(True)
    torch.manual_seed(7)
    agent = SACAgent(gamma=uc.GAMMA, tau=uc.TAU, alpha=uc.ALPHA, actor_lr=uc.LR, critic_lr=uc.LR, nstep=nstep, per=per, **TINY)
    seen, real = [], sac.td_target

    def spy(*args, **kw):
        seen.append(args[7])
        return real(*args, **kw)
    monkeypatch.setattr(sac, 'td_target', spy)
    losses = agent.update(env.replay, n)
    assert len(seen) == 1 and int(agent.draws) == n and bool(torch.isfinite(losses).all())
    s = agent.sample
    assert 'frames' not in s and sorted(s) == sorted(env.replay.sample_out(n, nstep, per))
    if nstep == 1:
        assert type(seen[0]) is float and seen[0] == uc.GAMMA == agent.gamma
        assert ('discount' in s) == per
        if per:
            assert bool((s['discount'] == uc.GAMMA).all())
    else:
        assert seen[0] is s['discount'] and seen[0].dtype == torch.float64 and tuple(seen[0].shape) == (n,)
    assert env.eng.device_errors() == 0
    env.close()
