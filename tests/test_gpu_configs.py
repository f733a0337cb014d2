"""The composed step path on the GPU (f110_reset / f110_step through F110VecEnv and the single-env F110Env facade) against
runs of the REFERENCE at off-default configurations: g14, tests/golden/make_golden.py g14_A ... g14_H.

Each case is ONE env of a batch of five and never env 0; the other envs start from jittered poses and drive seeded random
actions, so a result leaking from a neighbour shows.  Every record, agent and beam is compared (tests/config_cases.py:
compare): every boolean, index, counter, toggle and `done` ==; lap_times and current_time ==; state <= 1e-9; scans <= 1e-9;
the set of opponent-modified beams == (a beam counts as modified when it differs from the map scan of f110_scan at the
car's pose_snap plus its noise row); the fp32 observation == float32 of the fp64 one, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from config_cases import compare, load_case, map_arg, map_yaml  # noqa: E402

B, SLOT = 5, 2


def _np(t):
    return t.detach().cpu().numpy()


def _make(assets, case, **kw):
    from red_gym_amd import F110VecEnv, Integrator
    k = case.ctor()
    kw.setdefault('autoreset', False)
    kw.setdefault('params', k['params'])
    return F110VecEnv(B, map=map_arg(assets, k['map']), map_ext='.png', num_agents=k['num_agents'], timestep=k['timestep'],
                      ego_idx=k['ego_idx'], integrator=getattr(Integrator, k['integrator']), fov=k['fov'], seed=k['seed'],
                      keep_f64_scans=True, **kw)


class _Batch(object):
    """Drives env SLOT of a batch with the case's operations and the other envs with seeded filler."""

    def __init__(self, assets, case, env, graph=False, slots=False):
        self.assets, self.case, self.env, self.A = assets, case, env, case.kwargs['num_agents']
        self.rng = np.random.default_rng(1400 + len(case.kwargs['map']) + self.A)
        self.noise = oracle.noise_table(case.kwargs['seed'], int(case.noise_rows.max()) + 2)
        self.step_fn, self.graph = env.step, graph
        self.slots, self.first = slots, True

    def _filler_poses(self, poses):
        p = np.repeat(poses[None], B, axis=0)
        jit = np.concatenate([self.rng.uniform(-0.05, 0.05, (B, self.A, 2)), self.rng.uniform(-0.1, 0.1, (B, self.A, 1))], axis=2)
        jit[SLOT] = 0.0
        return p + jit

    def _filler_actions(self, action):
        a = np.stack([self.rng.uniform(-0.4, 0.4, (B, self.A)), self.rng.uniform(0.0, 5.0, (B, self.A))], axis=2)
        a[SLOT] = action
        return a

    def apply(self, op):
        import torch
        env = self.env
        if op[0] == 'update_params':
            if self.slots:   # the env's own params slot, agent by agent (an update never touches the Simulator's copy)
                from red_gym_amd import _lib
                from red_gym_amd.engine import params_vec
                pv = np.ascontiguousarray(params_vec(op[1]))
                for a in (range(self.A) if op[2] < 0 else [op[2]]):
                    _lib.check(env.eng.lib.f110_set_params_slot(env.eng._h, int(env.eng.env_params_assign[SLOT]),
                                                                pv.ctypes.data_as(C.c_void_p), a))
            else:
                env.update_params(op[1], op[2])
            return None
        if op[0] == 'update_map':
            env.update_map(map_yaml(self.assets, op[1]), '.png')
            return None
        r = op[1]
        if op[0] == 'reset':
            poses = self._filler_poses(op[2])
            if self.first:
                env.reset(poses)
                self.first = False
                if self.graph:   # every step from here on replays one captured graph
                    env.capture_step()
                    self.step_fn = env.step_graph
            elif env.eng.autoreset:
                # the batch's own reset: a done env restarts from its spawn pose on the next step
                assert bool(_np(env.eng.t['done'])[SLOT])
                env.eng.t['spawn'][SLOT] = torch.as_tensor(op[2], device=env.device)
                self.step_fn(self._filler_actions(np.zeros((self.A, 2))))
            else:
                mask = torch.zeros(B, dtype=torch.uint8)
                mask[SLOT] = 1
                env.reset(poses, mask=mask)
        else:
            self.step_fn(self._filler_actions(op[2]))
        return self.collect(r)

    def collect(self, r):
        env, t = self.env, self.env.eng.t
        got = {'state': _np(t['state'])[SLOT], 'scan_pose': _np(t['pose_snap'])[SLOT],
               'collisions': _np(t['collisions'])[SLOT], 'collision_idx': _np(t['collision_idx'])[SLOT],
               'toggles': _np(t['toggles'])[SLOT], 'lap_counts': _np(t['lap_counts'])[SLOT],
               'lap_times': _np(t['lap_times'])[SLOT], 'checkpoint_done': _np(t['checkpoint_done'])[SLOT],
               'done': bool(_np(t['done'])[SLOT]), 'current_time': float(_np(t['current_time'])[SLOT])}
        if r in self.case.expected['scan_records']:
            got.update(_scans(env.eng, SLOT, self.noise[self.case.noise_rows[r]]))
        return got


def _scans(eng, b, noise_row):
    s64, s32 = _np(eng.t['scans_f64'])[b], _np(eng.t['scans'])[b]
    assert np.array_equal(s32.view(np.uint32), s64.astype(np.float32).view(np.uint32))
    base = _np(eng.scan(eng.t['pose_snap'][b])) + noise_row
    return {'scans': s64, 'opp_mod': s64 != base}


def _replay(case, runner, name):
    seen, sampled = 0, 0
    for op in case.ops():
        got = runner.apply(op)
        if got is None:
            continue
        sampled += bool(compare(case, op[1], got, 1e-9, 1e-9, False, name))
        seen += 1
    assert seen == case.records and sampled == len(case.expected['scan_records'])


@pytest.mark.parametrize('name', ['A', 'B', 'C', 'D', 'E', 'F', 'G'])
def test_case_in_a_batch(golden, assets, name):
    case = load_case(golden, name)
    env = _make(assets, case)
    _replay(case, _Batch(assets, case, env), name)
    env.close()


def test_case_A_through_a_captured_graph(golden, assets):
    case = load_case(golden, 'A')
    env = _make(assets, case)
    _replay(case, _Batch(assets, case, env, graph=True), 'A graph')
    env.close()


def test_case_F_with_autoreset(golden, assets):
    """The batch path's own reset (a done env restarts from its spawn pose inside the next step) instead of a host-side
    reset call."""
    case = load_case(golden, 'F')
    env = _make(assets, case, autoreset=True)
    _replay(case, _Batch(assets, case, env), 'F autoreset')
    env.close()


def test_case_E_through_params_slots(golden, assets):
    """Every env has a vehicle (and so a params slot) of its own; the updates go to the case's slot alone."""
    case = load_case(golden, 'E')
    par = [dict(case.kwargs['params'], m=case.kwargs['params']['m'] + (0.05 * (b - SLOT))) for b in range(B)]
    env = _make(assets, case, params=par)
    assert len(set(env.eng.env_params_assign.tolist())) == B
    _replay(case, _Batch(assets, case, env, slots=True), 'E slots')
    env.close()


@pytest.mark.parametrize('name,mode', [('H_shared', 'shared'), ('H_own', 'per_env')])
def test_case_H_class_statics(golden, assets, name, mode):
    """Env 0 drives vehicle pa, the others pb: by default every env tests its beams against env 0's outline (the
    reference's class statics), with side_distances='per_env' against its own."""
    case = load_case(golden, name)
    pa = load_case(golden, 'H_shared').kwargs['statics_params']
    env = _make(assets, case, params=[pa] + [case.kwargs['params']] * (B - 1), side_distances=mode)
    _replay(case, _Batch(assets, case, env), name)
    env.close()


class _Facade(object):
    """The single-env red_gym_amd.F110Env (pack_env_kernel) driven by a case's operations."""

    def __init__(self, assets, case):
        from red_gym_amd import F110Env, Integrator
        k = case.ctor()
        self.assets, self.case = assets, case
        self.env = F110Env(map=map_arg(assets, k['map']), map_ext='.png', num_agents=k['num_agents'], timestep=k['timestep'],
                           ego_idx=k['ego_idx'], integrator=getattr(Integrator, k['integrator']), fov=k['fov'],
                           seed=k['seed'], params=k['params'])
        self.noise = oracle.noise_table(k['seed'], int(case.noise_rows.max()) + 2)

    def apply(self, op):
        env = self.env
        if op[0] == 'update_params':
            env.update_params(op[1], op[2])
            return None
        if op[0] == 'update_map':
            env.update_map(map_yaml(self.assets, op[1]), '.png')
            return None
        obs, reward, done, info = env.reset(op[2]) if op[0] == 'reset' else env.step(op[2])
        assert reward == self.case.kwargs['timestep']
        eng = env._vec.eng
        st = _np(eng.t['state'])[0]
        got = {'state': st, 'scan_pose': _np(eng.t['pose_snap'])[0], 'collisions': obs['collisions'],
               'collision_idx': _np(eng.t['collision_idx'])[0], 'toggles': env.toggle_list, 'lap_counts': obs['lap_counts'],
               'lap_times': obs['lap_times'], 'checkpoint_done': info['checkpoint_done'], 'done': done,
               'current_time': env.current_time}
        assert np.array_equal(st[:, 0], obs['poses_x']) and np.array_equal(st[:, 1], obs['poses_y'])
        assert np.array_equal(st[:, 4], obs['poses_theta']) and np.array_equal(st[:, 3], obs['linear_vels_x'])
        assert np.array_equal(st[:, 5], obs['ang_vels_z'])
        if op[1] in self.case.expected['scan_records']:
            got.update(_scans(eng, 0, self.noise[self.case.noise_rows[op[1]]]))
            assert np.array_equal(np.stack(obs['scans']), got['scans'])
        return got


@pytest.mark.parametrize('name', ['A', 'F'])
def test_case_through_the_single_env_facade(golden, assets, name):
    case = load_case(golden, name)
    f = _Facade(assets, case)
    _replay(case, f, name + ' facade')
    f.env.close()
