"""Golden fixtures of the COMPOSED step path at its off-default configurations, generated in the dev container by
RUNNING THE REFERENCE's own F110Env (reference.load_env(); never shipped, none of its text copied) through make_golden.py,
rows g14_A ... g14_H:

  g14_<case>.npz   one file per case (arrays and JSON strings only), cases A-H below.  Per case: the constructor kwargs,
                   every operation in order (reset poses, step actions, update_params / update_map calls), and after every
                   reset / step ("record") each agent's 7-state, the pose its scan was taken at (Simulator.agent_poses,
                   i.e. before the iTTC zeroing), collisions, Simulator.collision_idx, toggle_list, lap_counts, lap_times,
                   done, current_time and info['checkpoint_done'].  The fp64 scans of every agent, and which of their beams
                   a ray_cast call changed (opponent-modified beams, packed bits), at SAMPLED records: every 10th, every
                   record where a collision flag changes, each reset and the step after it, both sides of every
                   update_map / update_params call.

Noise is on in every case at the reference's own seed handling (12345, and 777 in cases C and D).  The reference's
class-level statics (RaceCar.scan_simulator / scan_angles / cosines / side_distances) are cleared before every case,
except inside case H, which is about them.  Every case asserts that what it is meant to exercise really occurred.

  A  3 cars, ego_idx=1, example_map, pure-pursuit train.  Car 2 is steered into the wall first (collisions[2] == 1 while
     done stays False, its iTTC zeroing repeating), then the ego rear-ends car 0 (done).
  B  4 cars, ego_idx=3, timestep 0.005: cars 0-2 drive into one another and overlap in the same step (collision_idx is
     last-writer-wins: asserted to differ from "first collider"); car 3 stays clear (collision_idx -1) and sees them.
  C  1 car, Euler, timestep 0.02, skirk (0.05 m cells), fov 4.7, seed 777, a non-default vehicle; runs into the wall.
  D  3 cars, ego_idx=2, timestep 0.02, berlin, seed 777: each circles through its start zone at its own speed; all reach
     toggle >= 4 at different steps; done comes from np.all(toggles >= 4); start_rot is the EGO's start angle (the three
     start yaws differ).
  E  2 cars; update_params(p2, index=1) after 40 steps, update_params(p3) for all after 80.  NOT as the issue words it:
     in the reference NO GJK decision can depend on update_params, because check_collision sizes its quads from
     Simulator.params (base_classes.py:542), which update_params never touches (:507-527).  What the case pins instead,
     and the generator asserts: (1) a re-run without the updates gives other opponent-modified beams (ray_cast_agents
     uses the VIEWING car's params, :221) and other states (dynamics use the car's params); (2) the recorded GJK flags
     are those of the constructor's size at steps where the updated size would decide otherwise, in both directions
     (no hit although the grown p2 quads overlap; a hit although the shrunk p3 quads do not).
  F  2 cars, one env: run to done (ego into the wall), reset at other poses, run to done again (ego rear-ends car 1),
     reset a third time, 30 steps.
  G  2 cars, update_map example_map -> berlin -> example_map mid-run.
  H  the class statics: env 1 with vehicle pa, then env 2 with vehicle pb (other width, lf, lr) in the same process
     WITHOUT clearing the statics; env 2 is driven into a wall-side iTTC hit.  Stored twice: 'H_shared' (env 2 tests its
     beams against pa's side distances: this project's default mode) and 'H_own' (statics cleared first, pb's own side
     distances: side_distances='per_env').  Asserted: the hit steps differ.

No trajectory had to be replaced for a rounding-decided flag (none was met: the oracle agrees on every flag of every case).
"""
import json

import numpy as np

import reference
from reference import PARAMS

NB = 1080
START = [0.7, 0.0, 1.37079632679]   # config_example_map.yaml


class RefBackend(object):
    """The reference's F110Env; the only place that reads its internals."""

    def __init__(self):
        self.lm, self.dm, self.cm, self.bc, self.fe = reference.load_env()
        self._mods = []
        orig = self.bc.ray_cast

        def ray_cast(pose, scan, angles, verts):   # records which beams each call changes; computes nothing itself
            before = scan.copy()
            out = orig(pose, scan, angles, verts)
            self._mods.append(np.nonzero(out != before)[0])
            return out
        self.bc.ray_cast = ray_cast

    def clear_statics(self):
        rc = self.bc.RaceCar
        rc.scan_simulator = rc.scan_angles = rc.cosines = rc.side_distances = None

    def map_arg(self, name):
        return reference.path('examples', 'example_map') if name == 'example_map' else name

    def map_yaml(self, name):
        return (reference.path('examples', 'example_map.yaml') if name == 'example_map'
                else reference.path('gym', 'f110_gym', 'envs', 'maps', name + '.yaml'))

    def make(self, kw):
        k = dict(kw)
        k['map'] = self.map_arg(k['map'])
        k['map_ext'] = '.png'
        k['integrator'] = getattr(self.bc.Integrator, k['integrator'])
        self.env = self.fe.F110Env(**k)
        self.A = kw['num_agents']

    def _snap(self, ret):
        obs, _, done, info = ret
        e, A = self.env, self.A
        mod = np.zeros((A, NB), dtype=bool)
        assert len(self._mods) == A * (A - 1)
        for i in range(A):
            for m in self._mods[i * (A - 1):(i + 1) * (A - 1)]:
                mod[i, m] = True
        self._mods = []
        return dict(state=np.stack([a.state for a in e.sim.agents]), scan_pose=e.sim.agent_poses.copy(),
                    collisions=np.array(e.sim.collisions), collision_idx=np.array(e.sim.collision_idx),
                    toggles=np.array(e.toggle_list), lap_counts=np.array(e.lap_counts), lap_times=np.array(e.lap_times),
                    done=bool(done), current_time=float(e.current_time), checkpoint_done=np.array(info['checkpoint_done']),
                    scans=np.stack(obs['scans']).astype(np.float64), opp_mod=mod)

    def reset(self, poses):
        return self._snap(self.env.reset(np.array(poses, dtype=np.float64)))

    def step(self, action):
        return self._snap(self.env.step(np.array(action, dtype=np.float64)))

    def update_params(self, params, index):
        self.env.update_params(dict(params), index=index)

    def update_map(self, name):
        self.env.update_map(self.map_yaml(name), '.png')

    def gjk(self, pose_a, pose_b, length, width):
        va, vb = self.cm.get_vertices(np.array(pose_a), length, width), self.cm.get_vertices(np.array(pose_b), length, width)
        return bool(self.cm.collision(np.ascontiguousarray(va), np.ascontiguousarray(vb)))


class Run(object):
    """One recorded run: forwards every operation to the backend and keeps what came back."""
    RESET, STEP = 0, 1

    def __init__(self, be, kw, make=True):
        self.be, self.kw, self.A = be, kw, kw['num_agents']
        if make:
            be.make(kw)
        self.rec, self.kind, self.arg, self.calls, self.force = [], [], [], [], set()
        self.last = None

    def _push(self, kind, arg, snap):
        a = np.zeros((self.A, 3))
        a[:, :np.shape(arg)[1]] = arg
        self.kind.append(kind); self.arg.append(a); self.rec.append(snap)
        self.last = snap
        return snap

    def reset(self, poses):
        r = len(self.rec)
        self.force |= {r, r + 1}
        return self._push(self.RESET, poses, self.be.reset(poses))

    def step(self, action):
        return self._push(self.STEP, action, self.be.step(action))

    def _mark(self):
        r = len(self.rec)
        self.force |= {r - 1, r}

    def update_params(self, params, index=-1):
        self._mark()
        self.calls.append({'before': len(self.rec), 'call': 'update_params', 'params': dict(params), 'index': index})
        self.be.update_params(params, index)

    def update_map(self, name):
        self._mark()
        self.calls.append({'before': len(self.rec), 'call': 'update_map', 'map': name})
        self.be.update_map(name)

    def pose(self, i):
        s = self.last['state'][i]
        return s[0], s[1], s[4]

    def col(self, key):
        return np.stack([r[key] for r in self.rec])

    def sampled(self):
        col = self.col('collisions')
        out = set(r for r in self.force if 0 <= r < len(self.rec))
        out |= set(range(0, len(self.rec), 10))
        out |= set((np.nonzero((col[1:] != col[:-1]).any(axis=1))[0] + 1).tolist())
        return sorted(out)

    def save(self, name, notes):
        R = len(self.rec)
        assert R <= 301, R
        s = self.sampled()
        if self.A > 1:
            assert any(self.rec[r]['opp_mod'].any() for r in s), 'no sampled record with an opponent-modified beam'
        out = dict(kwargs=np.array(json.dumps(self.kw)), calls=np.array(json.dumps(self.calls)),
                   op_kind=np.array(self.kind, dtype=np.int8), op_arg=np.stack(self.arg),
                   done=np.array([r['done'] for r in self.rec]), current_time=np.array([r['current_time'] for r in self.rec]),
                   scan_records=np.array(s, dtype=np.int32), scans=np.stack([self.rec[r]['scans'] for r in s]),
                   opp_mod=np.packbits(np.stack([self.rec[r]['opp_mod'] for r in s]), axis=-1))
        for k in ('state', 'scan_pose', 'collisions', 'collision_idx', 'toggles', 'lap_counts', 'lap_times', 'checkpoint_done'):
            out[k] = self.col(k)
        kb = reference.save('g14_%s.npz' % name, **out) / 1024
        assert kb < 1000, kb
        print('  %d records, %d with scans, %d opponent-modified beams; %s'
              % (R, len(s), int(sum(self.rec[r]['opp_mod'].sum() for r in s)), notes), flush=True)


class Planner(object):
    """The reference's own pure-pursuit caller (examples/waypoint_follow.py), as g7-g9 load it."""

    def __init__(self):
        mod, conf = reference.load_planner()
        self.p = mod.PurePursuitPlanner(conf, 0.17145 + 0.15875)
        self.rl = reference.raceline()

    def __call__(self, pose, vgain):
        sp, st = self.p.plan(pose[0], pose[1], pose[2], 0.82461887897713965, vgain)
        return [st, sp]

    def at(self, k, back=0.0):
        k %= self.rl.shape[0]
        th = self.rl[k, 3] + np.pi / 2
        return [self.rl[k, 1] - back * np.cos(th), self.rl[k, 2] - back * np.sin(th), th]


def kwargs(map='example_map', num_agents=2, ego_idx=0, timestep=0.01, integrator='RK4', fov=2 * np.pi, seed=12345,
           params=None):
    return dict(map=map, num_agents=num_agents, ego_idx=ego_idx, timestep=timestep, integrator=integrator, fov=fov,
                seed=seed, params=dict(PARAMS if params is None else params))


def first(mask):
    mask = np.asarray(mask)
    return int(np.argmax(mask)) if mask.any() else None


def case_A(be, plan):
    run = Run(be, kwargs(num_agents=3, ego_idx=1))
    run.reset([plan.at(18), START, plan.at(-10)])
    for k in range(300):
        act = [plan(run.pose(0), 0.45), plan(run.pose(1), 1.375), plan(run.pose(2), 1.0)]
        if k >= 55:
            act[2] = [-0.4, 6.0]
        if run.step(act)['done']:
            break
    col, done = run.col('collisions'), run.col('done')
    wall = first(col[:, 2] == 1)
    assert wall is not None and not done[wall] and done[-1] and not done[:-1].any()
    assert col[-1, 1] == 1 and col[-1, 0] == 1 and run.col('collision_idx')[-1, 1] == 0
    zeroed = int((run.col('state')[wall:, 2, 3] == 0).sum())
    seen = sum(int(r['opp_mod'][:2].any()) for r in run.rec[wall:])
    assert zeroed > 5 and seen > 5
    run.save('A', 'car 2 hits the wall at record %d (done False, its state zeroed at %d records), ego rear-ends car 0 at %d'
             % (wall, zeroed, len(run.rec) - 1))


def case_B(be, plan):
    run = Run(be, kwargs(num_agents=4, ego_idx=3, timestep=0.005))
    poses = [plan.at(30, back=b) for b in (0.0, 0.7, 1.4, 3.2)]   # a train on the straight, 0.7 m apart, car 3 well behind
    poses[1][2] += 0.04
    poses[2][2] -= 0.03
    run.reset(poses)
    for k in range(150):
        run.step([[0.0, 0.3], [0.0, 1.5], [0.0, 2.6], [0.0, 0.3]])   # the rear cars drive into (and through) the front one
    col, idx = run.col('collisions'), run.col('collision_idx')
    three = np.nonzero(col[:, :3].sum(axis=1) == 3)[0]
    assert len(three) > 0
    # "first collider": the lowest-numbered body each car overlaps
    differs = None
    for r in three:
        p = run.rec[r]['scan_pose']
        firsts = [min([j for j in range(4) if j != i and be.gjk(p[i], p[j], PARAMS['length'], PARAMS['width'])] or [-1])
                  for i in range(4)]
        if not np.array_equal(firsts, idx[r]):
            differs = (int(r), firsts, idx[r].tolist())
            break
    assert differs is not None
    assert (col[:, 3] == 0).all() and (idx[:, 3] == -1).all() and not run.col('done').any()
    sees = [r for r in three if run.rec[r]['opp_mod'][3].any()]
    assert sees
    run.force.add(differs[0])
    run.save('B', 'three flags from record %d; at %d collision_idx %s, first colliders %s; car 3 clear throughout'
             % (three[0], differs[0], differs[2], differs[1]))


P_C = dict(PARAMS, width=0.27, length=0.51, lf=0.14, lr=0.16, mu=0.85, m=3.1, a_max=7.0)


def case_C(be, plan):
    run = Run(be, kwargs(map='skirk', num_agents=1, timestep=0.02, integrator='Euler', fov=4.7, seed=777, params=P_C))
    run.reset([[0.0, 0.0, 0.3]])
    for k in range(300):
        if run.step([[0.12 * np.sin(k / 9.0), 3.5]])['done']:
            break
    col = run.col('collisions')
    assert run.col('done')[-1] and col[-1, 0] == 1 and len(run.rec) > 40
    assert (run.rec[-1]['state'][0, 3:] == 0).all()
    run.save('C', 'iTTC wall hit at record %d' % (len(run.rec) - 1))


def case_D(be, plan):
    run = Run(be, kwargs(map='berlin', num_agents=3, ego_idx=2, timestep=0.02, seed=777))
    run.reset([[0.0, 0.0, 0.1], [-3.0, -0.5, 0.3], [2.5, 0.2, 6.1]])
    for k in range(300):
        if run.step([[0.4189, 2.4], [-0.4189, 2.0], [-0.4189, 1.7]])['done']:
            break
    tg, lt = run.col('toggles'), run.col('lap_times')
    fin = [first(tg[:, i] >= 4) for i in range(3)]
    assert None not in fin and len(set(fin)) == 3
    assert run.col('done')[-1] and not run.col('collisions').any() and len(run.rec) - 1 == max(fin)
    assert len(set(lt[-1].tolist())) == 3
    # the frame is the EGO's: with agent 0's start angle the toggles would come at other records
    st = run.col('state')
    th = -run.arg[0][0, 2]
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    other = False
    for i in range(3):
        d = rot @ np.stack([st[:, i, 0] - run.arg[0][i, 0], st[:, i, 1] - run.arg[0][i, 1]])
        ty = np.where(d[1] > 2, d[1] - 2, np.where(d[1] < -2, -2 - d[1], 0.0))
        closes = d[0] ** 2 + ty ** 2 <= 0.1
        n = np.cumsum(np.concatenate([[closes[0] != True], closes[1:] != closes[:-1]]))
        other |= not np.array_equal(n, tg[:, i])
    assert other
    run.save('D', 'cars reach toggle 4 at records %s, lap_times %s' % (fin, lt[-1].tolist()))


P2 = dict(PARAMS, length=0.95, width=0.5, m=4.3, mu=0.9)
P3 = dict(PARAMS, length=0.4, width=0.22, a_max=6.0, sv_max=2.0)


def case_E(be, plan, save=True):
    def drive(update):
        run = Run(be, kwargs(num_agents=2))
        run.reset([plan.at(3), plan.at(3, back=0.7)])
        for k in range(150):
            if k == 40 and update:
                run.update_params(P2, index=1)
            if k == 80 and update:
                run.update_params(P3)
            a0 = plan(run.pose(0), 0.2)
            a1 = plan(run.pose(1), 0.2 if k < 80 else 0.5)
            if run.step([a0, a1])['done']:
                break
        return run
    run = drive(True)
    be.clear_statics()
    plain = drive(False)
    n = min(len(run.rec), len(plain.rec))
    st, st0 = run.col('state')[:n], plain.col('state')[:n]
    assert np.array_equal(st[:41], st0[:41]) and not np.array_equal(st[42:n], st0[42:n])
    mod_differs = [r for r in range(n) if not np.array_equal(run.rec[r]['opp_mod'], plain.rec[r]['opp_mod'])]
    assert mod_differs and mod_differs[0] >= 41 and set(mod_differs) & set(run.sampled())
    # GJK keeps the constructor's size: records where the updated size would decide otherwise
    col = run.col('collisions')
    grown = [r for r in range(42, 81) if col[r].sum() == 0
             and be.gjk(run.rec[r]['scan_pose'][0], run.rec[r]['scan_pose'][1], P2['length'], P2['width'])]
    shrunk = [r for r in range(82, len(run.rec)) if col[r].sum() == 2
              and not be.gjk(run.rec[r]['scan_pose'][0], run.rec[r]['scan_pose'][1], P3['length'], P3['width'])]
    assert grown and shrunk and run.col('done')[-1]
    if save:
        run.save('E', 'opponent-modified beams differ from the run without updates at %d records (first %d); no GJK hit at '
                 '%d records where p2-sized quads overlap; GJK hit at %d records where p3-sized quads do not'
                 % (len(mod_differs), mod_differs[0], len(grown), len(shrunk)))


def case_F(be, plan):
    run = Run(be, kwargs(num_agents=2))
    run.reset([START, plan.at(40)])
    while not run.last['done']:
        run.step([[0.4, 6.0], plan(run.pose(1), 0.6)])
    d1 = len(run.rec) - 1
    assert run.last['collisions'][0] == 1 and run.last['collision_idx'][0] == -1
    run.reset([plan.at(200), plan.at(208)])
    assert run.last['current_time'] == 0.01 and not run.last['toggles'].any() and not run.last['done']
    while not run.last['done']:
        run.step([plan(run.pose(0), 1.3), plan(run.pose(1), 0.3)])
    d2 = len(run.rec) - 1
    assert run.last['collision_idx'][0] == 1
    run.reset([plan.at(400), plan.at(420)])
    for k in range(30):
        run.step([plan(run.pose(0), 1.0), plan(run.pose(1), 1.0)])
    assert not run.last['done']
    run.save('F', 'done at record %d (wall), reset, done at %d (GJK), reset, 30 steps' % (d1, d2))


def case_G(be, plan):
    run = Run(be, kwargs(num_agents=2))
    back = [START[0] - 0.9 * np.cos(START[2]), START[1] - 0.9 * np.sin(START[2]), START[2] + 0.05]
    run.reset([START, back])   # free space in both maps
    for k in range(90):
        if k == 30:
            run.update_map('berlin')
        if k == 60:
            run.update_map('example_map')
        run.step([[0.03, 1.5], [0.0, 1.2]])
    s = set(run.sampled())
    assert {30, 31, 60, 61} <= s and not run.col('collisions').any()
    sc = {r: run.rec[r]['scans'] for r in (30, 31, 60, 61)}
    assert np.abs(sc[30] - sc[31]).max() > 1.0 and np.abs(sc[60] - sc[61]).max() > 1.0
    run.save('G', 'maps switched before records 31 and 61')


PA = dict(PARAMS)
PB = dict(PARAMS, width=0.55, lf=0.25, lr=0.27, length=0.8)


def case_H(be, plan):
    def drive():
        run = Run(be, kwargs(num_agents=1, params=PB))
        run.reset([START])
        for k in range(300):
            if run.step([[0.0 if k < 30 else 0.25, 4.0]])['done']:
                break
        assert run.last['done'] and run.last['collisions'][0] == 1
        return run
    be.clear_statics()
    be.make(kwargs(num_agents=1, params=PA))   # env 1: fixes the statics
    side_a = be.bc.RaceCar.side_distances.copy()
    shared = drive()                           # env 2, same process
    assert np.array_equal(be.bc.RaceCar.side_distances, side_a)
    be.clear_statics()
    own = drive()
    assert not np.array_equal(be.bc.RaceCar.side_distances, side_a)
    h1, h2 = len(shared.rec) - 1, len(own.rec) - 1
    assert h1 != h2, (h1, h2)
    shared.kw['statics_params'] = PA
    own.kw['statics_params'] = PB
    shared.save('H_shared', "wall hit at record %d with env 1's side distances" % h1)
    own.save('H_own', 'wall hit at record %d with its own side distances' % h2)


CASES = {'A': case_A, 'B': case_B, 'C': case_C, 'D': case_D, 'E': case_E, 'F': case_F, 'G': case_G, 'H': case_H}


def record(case):
    be = RefBackend()
    be.clear_statics()
    CASES[case](be, Planner())
