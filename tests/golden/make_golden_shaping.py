"""Generates g16_shaping.npz: the reference's OWN reward code -- SACF110Env._calculate_rewards (src/SAL.py:219-250) with
detect_collison (:766-790), distance_from_row_center / centerline_reward (:879-935) and _world_to_pixel (:139-142) -- on the
images and poses of tests/shaping_cases.py.

Run through make_golden.py.  src/SAL.py is loaded by file path (reference.load_sal()) with empty stand-in modules for cv2,
cvxpy, gym (with an Env class) and pyglet / pyglet.gl (GL_LINES); the functions recorded here are plain Python and NumPy
and call none of them.  They run on a bare SACF110Env.__new__ instance whose map_origin, map_scale,
last_obs and prev_position are set by hand.  The fixture holds inputs and recorded results only.

Images: (a) the FILL image (black background, SAL's call at :76-77) of g8's and g10's scans.  cv2 is absent here, so the
reference's own drawer cannot run: they are drawn by oracle.bitmap, the project's restatement of it -- for this fixture an
image is an INPUT, any 0 / 255 picture serves; (b) hand-built images for the edges of the run search; (c) the sizes 75 x 100
and 40 x 300, whose widths are not multiples of 64.  0 / 255 images are stored with np.packbits.

np.linalg.norm of the progress term goes through the BLAS's dot, so g15's guard is kept: the row runs under
reference.BLAS_PIN, and the generator refuses to run if np.dot still fuses its multiply-add.
"""
import os

import numpy as np

import reference
import shaping_cases as sc
from oracle import bitmap as ob

SIZES = {'a': (256, 256), 'b': (75, 100), 'c': (40, 300)}
POSES_PER_IMAGE = {'a': 36, 'b': 36, 'c': 48}   # per drawn image
POSES_PER_HAND_IMAGE = 144


def g16_shaping():
    reference.require_unfused_dot()
    sal = reference.load_sal()
    g8 = np.load(reference.fixture('g8_env.npz'))
    g10 = np.load(reference.fixture('g10_bitmap_calls.npz'))
    scans = {'a': np.concatenate([g8['scans'], g10['scans']]), 'b': g8['scans'], 'c': g8['scans'][::3]}
    env = sal.SACF110Env.__new__(sal.SACF110Env)
    env.map_origin, env.map_scale = (128, 128), 10.0
    store, cases = {}, {k: [] for k in ('group', 'img', 'xy', 'prev', 'px', 'py', 'collided', 'dist', 'collision_term', 'progress_term',
                                        'centering_term', 'total')}
    n_real = 0
    for gi, grp in enumerate(sc.GROUPS):
        rows, cols = SIZES[grp]
        fill = ob.lidar_to_bitmap(scans[grp], output_image_dims=(rows, cols), bg_color='black', draw_mode='FILL')
        imgs = np.concatenate([fill, sc.hand_images(rows, cols)])
        assert set(np.unique(imgs)) <= {0, 255}
        store['img_' + grp] = np.packbits((imgs.reshape(imgs.shape[0], -1) == 255).astype(np.uint8), axis=1)
        store['shape_' + grp] = np.array([rows, cols], dtype=np.int32)
        for k in range(imgs.shape[0]):
            poses = sc.designed_poses(rows, cols, POSES_PER_IMAGE[grp] if k < fill.shape[0] else POSES_PER_HAND_IMAGE, 1600 + 1000 * gi + k)
            if grp == 'a' and k < g8['scans'].shape[0]:
                # real pairs: the image of g8's recorded scan k, the pose of the step after it, the position before as prev_position
                s = int(g8['scan_steps'][k])
                s1 = min(s + 1, g8['x'].shape[0] - 1)
                poses = np.concatenate([[[g8['x'][s1], g8['y'][s1], g8['x'][s], g8['y'][s]]], poses])
                n_real += 1
            for x, y, x0, y0 in poses:
                obs = {'poses_x': np.array([x]), 'poses_y': np.array([y])}
                env.last_obs = {'lidar_bitmap': imgs[k]}
                env.prev_position = np.array([x0, y0])
                r = env._calculate_rewards(obs, False)
                assert list(r) == ['base', 'progress', 'collision', 'centering'] and r['base'] == 0.0
                px, py = env._world_to_pixel(obs['poses_x'][0], obs['poses_y'][0])
                dist = sal.distance_from_row_center(imgs[k], int(obs['poses_x'][0]), int(obs['poses_y'][0]))
                hit = sal.detect_collison(imgs[k], px, py)
                assert (r['collision'] == -100.0) == bool(hit)
                for key, v in (('group', gi), ('img', k), ('xy', (x, y)), ('prev', (x0, y0)), ('px', int(px)), ('py', int(py)),
                               ('collided', int(bool(hit))), ('dist', np.nan if dist is None else dist), ('collision_term', r['collision']),
                               ('progress_term', r['progress']), ('centering_term', r['centering']), ('total', sum(r.values()))):
                    cases[key].append(v)
    c = {k: np.array(v, dtype={'group': np.int8, 'img': np.int16, 'px': np.int32, 'py': np.int32, 'collided': np.uint8}.get(k, np.float64))
         for k, v in cases.items()}
    n = c['group'].shape[0]
    # coverage: the reference alone must demonstrate every branch on at least 5 % of the cases
    car_x, car_y = np.trunc(c['xy'][:, 0]), np.trunc(c['xy'][:, 1])
    dims = np.array([SIZES[g] for g in sc.GROUPS])[c['group']]
    inside = (car_x >= 0) & (car_x < dims[:, 1]) & (car_y >= 0) & (car_y < dims[:, 0])
    reward = c['centering_term'] / 2.0
    cover = {'collided': c['collided'] == 1, 'not collided': c['collided'] == 0,
             'centering -1, outside the image': (reward == -1.0) & ~inside, 'centering -1, no run': (reward == -1.0) & inside,
             'centering inside (0, 1)': (reward > 0.0) & (reward < 1.0), 'centering 0.0 (clamped)': reward == 0.0}
    for name, m in cover.items():
        print('%-34s %5d cases (%.1f %%)' % (name, m.sum(), 100.0 * m.mean()))
        assert m.mean() >= 0.05, name
    size = reference.save('g16_shaping.npz', n_real=np.int64(n_real), **store, **c)
    print('  %d cases (%d real pairs) on %d images' % (n, n_real, sum(store['img_' + g].shape[0] for g in sc.GROUPS)))
    assert size < os.path.getsize(reference.fixture('g6_raycast.npz'))
