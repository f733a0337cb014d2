"""The bits form of the lidar bitmap on the GPU: f110_bitmap_render_bits `==` the packed byte render and the packed oracle
image, the shaper's and the replay push's bits forms `==` their bytes forms and the recorded reference, through the closed loop,
graphs and checkpoints.  Every comparison is `==` / torch.equal."""
import ctypes as C
import os

import numpy as np
import pytest

import bits_cases as bc
import shaping_cases as sc

pytestmark = pytest.mark.gpu

OUT_KEYS = sc.TERMS + ('collided',)
INFO_KEYS = ('reward_collision', 'reward_progress', 'reward_centering', 'bitmap_collided')
RING_KEYS = ('frames', 'actions', 'rewards', 'dones', 'valid', 'count')


def _env(assets, B, A=1, **kw):
    from red_gym_amd import F110VecEnv
    return F110VecEnv(B, map=os.path.join(assets, 'example_map'), map_ext='.png', num_agents=A, **kw)


def _options(mode, dims):
    """Renderer options for an image of `dims`: SAL's 10 pixels per metre, scans sized so that the polygon has an inside."""
    return dict(draw_mode=mode, output_image_dims=dims, target_beam_count=50 if mode == 'RAYS' else 600)


def _reach(dims):
    """The scans' size in metres for an image of `dims`: the reference draws around (x, y) = (rows // 2, cols // 2), which lies
    outside an image that is much wider than high -- the corridor's walls are put at about the distance from there to the
    image's middle (10 pixels per metre), so that every size has edges, filled area and clipped segments."""
    rows, cols = dims
    d = np.hypot(rows // 2 - cols / 2.0, cols // 2 - rows / 2.0)
    return max(d, min(dims) / 4.0, 4.0) / 3.0


def _check_render(r, ob, scans, kw, what):
    """bits(scans) `==` pack(img == draw) for img from the renderer's own byte form and from the oracle, with `out` full of
    ones beforehand: fp64, fp32 and a strided fp32 batch."""
    import torch
    n = scans.shape[0]
    rows, cols = kw['output_image_dims']
    draw = 255 if kw['bg_color'] == 'black' else 0
    wide = torch.zeros((n, 2 * scans.shape[1] + 3), dtype=torch.float32, device='cuda')
    wide[:, :scans.shape[1]] = torch.as_tensor(scans.astype(np.float32))
    forms = {'fp64': (torch.as_tensor(scans, device='cuda'), scans),
             'fp32': (torch.as_tensor(scans.astype(np.float32), device='cuda'), scans.astype(np.float32).astype(np.float64)),
             'strided': (wide[:, :scans.shape[1]], scans.astype(np.float32).astype(np.float64))}
    assert forms['strided'][0].stride(0) != scans.shape[1]
    for form, (dev, host) in forms.items():
        out = torch.full((n, rows, bc.words(cols)), -1, dtype=torch.int64, device='cuda')
        got = r.bits(dev, out=out)
        assert got.data_ptr() == out.data_ptr() and got.shape == (n, rows, bc.words(cols)) and got.dtype == torch.int64
        got = bc.as_u64(got)
        own = bc.pack(r(dev).cpu().numpy() == draw)
        ref = bc.pack(ob.lidar_to_bitmap(host, **kw) == draw)
        bad_own, bad_ref = int((got != own).sum()), int((got != ref).sum())
        print('%s %s: %d words, %d set bits, differing from own bytes %d, from the oracle %d'
              % (what, form, got.size, int(np.unpackbits(got.view(np.uint8)).sum()), bad_own, bad_ref))
        assert bad_own == 0 and bad_ref == 0, (what, form, np.argwhere(got != ref)[:5].tolist())
    return got


@pytest.mark.parametrize('dims', bc.SIZES)
@pytest.mark.parametrize('mode', bc.MODES)
def test_render_bits_equals_packed_bytes_and_oracle(mode, dims):
    """Every mode at every size of bits_cases.SIZES, 5 scans, centre marker on and off, black and white background."""
    from oracle import bitmap as ob
    from red_gym_amd.lidar import LidarBitmap
    scans = bc.scans(5, seed=7 * bc.MODES.index(mode) + dims[1], reach=_reach(dims))
    seen = 0
    for draw_center in (True, False):
        for bg in ('black', 'white'):
            kw = dict(_options(mode, dims), bg_color=bg, draw_center=draw_center)
            r = LidarBitmap(1080, **kw)
            got = _check_render(r, ob, scans, kw, '%s %s center=%d %s' % (mode, dims, draw_center, bg))
            seen += int(got.any())
            r.close()
    assert seen == 4, 'an option set drew nothing'


def test_render_bits_single_scan_and_arguments():
    """The argument handling of __call__: one scan gives [rows, words], a host array is uploaded, a wrong `out` is refused."""
    import torch
    from red_gym_amd import _lib
    from red_gym_amd.lidar import LidarBitmap
    scans = bc.scans(2, seed=3)
    r = LidarBitmap(1080, bg_color='black', draw_mode='FILL', output_image_dims=(75, 100), channels=3)   # channels: no part
    one = r.bits(torch.as_tensor(scans[0], device='cuda'))
    both = r.bits(scans)
    assert one.shape == (75, 2) and both.shape == (2, 75, 2) and torch.equal(one, both[0])
    assert np.array_equal(bc.as_u64(both), bc.pack(r(scans).cpu().numpy()[..., 0] == 255))
    with pytest.raises(AssertionError):
        r.bits(scans, out=torch.zeros((2, 75, 100), dtype=torch.uint8, device='cuda'))
    lib = _lib.load()
    rc_ = lib.f110_bitmap_render_bits(r.h, both.data_ptr(), 1, 1, 1080, both.data_ptr() + 8, None)
    assert rc_ == _lib.E_INVALID and b'aligned' in lib.f110_last_error()
    r.close()


@pytest.mark.parametrize('mode,dims', [('FILL', (256, 256)), ('FILL', (75, 100)), ('POLYGON', (256, 256)), ('FILL', (9, 257))])
def test_one_workgroup_draws_every_image(mode, dims, monkeypatch):
    """F110_BM_GRID=1 and 7 scans: one workgroup runs the fetch-ahead loop over all of them, through both store forms in
    turn -- the planes, the records' place and the prefetched ranges are handed from image to image the same way."""
    from oracle import bitmap as ob
    from red_gym_amd.lidar import LidarBitmap
    scans = bc.scans(7, seed=41 + dims[1], reach=_reach(dims))
    kw = dict(_options(mode, dims), bg_color='black', draw_center=True)
    r = LidarBitmap(1080, **kw)
    monkeypatch.setenv('F110_BM_GRID', '1')
    _check_render(r, ob, scans, kw, 'grid 1 %s %s' % (mode, dims))
    monkeypatch.delenv('F110_BM_GRID')
    _check_render(r, ob, scans, kw, 'full grid %s %s' % (mode, dims))
    r.close()


def _terms_np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    bad = {k: int((~sc.same(got[k], want[k])).sum()) for k in OUT_KEYS}
    print(what, 'differing elements:', bad)
    assert not any(bad.values()), (what, bad)


def test_shaper_bits_equals_the_reference_on_g16(golden):
    """f110_shaping_terms_bits on the packed images of g16, every case (one launch per image size: a launch has one size):
    the four terms and collided `==` what the reference's own _calculate_rewards returned."""
    import torch
    from red_gym_amd import shaping
    g = golden('g16_shaping.npz')
    total = 0
    for gi, grp in enumerate(sc.GROUPS):
        imgs = sc.unpack_images(g, grp)
        m = np.flatnonzero(g['group'] == gi)
        packed = torch.as_tensor(bc.pack(imgs[g['img'][m]] == 255).view(np.int64), device='cuda')
        out = shaping.reward_terms_bits(packed, torch.as_tensor(g['xy'][m], device='cuda'), torch.as_tensor(g['prev'][m], device='cuda'), cols=imgs.shape[2])
        _assert_same(_terms_np(out), {k: g[k][m] for k in OUT_KEYS}, 'g16 group %s as bits (%d x %d, %d cases)' % ((grp,) + imgs.shape[1:] + (m.size,)))
        total += m.size
    assert total == g['group'].shape[0] >= 7000


@pytest.mark.parametrize('rows,cols', [(75, 100), (40, 300), (10, 65), (11, 600)])
def test_shaper_bits_equals_the_checker_on_designed_poses(rows, cols):
    """Hand-built images and designed poses (tests/shaping_cases.py) at two words of which the second is partial, five words,
    one word and a pixel, and ten words (a third pass of the four-word loop): `==` the NumPy checker and the bytes kernel."""
    import torch
    from red_gym_amd import shaping
    cfg = sc.config(rows=rows, cols=cols, clip_max=max(rows, cols) - 1, scale=2.0, origin_x=cols / 2.0, origin_y=rows / 2.0,
                    max_lane_halfwidth=cols / 4.0, neighborhood=1 + rows % 2)
    imgs = sc.hand_images(rows, cols)
    n = 61 * imgs.shape[0]
    poses = sc.designed_poses(rows, cols, n, rows * cols, cfg)
    pick = np.arange(n) % imgs.shape[0]
    want = [sc.reward_terms(imgs[pick[k]], poses[k, 0], poses[k, 1], poses[k, 2], poses[k, 3], cfg) for k in range(n)]
    want = {k: np.array([w[k] for w in want]) for k in OUT_KEYS}
    opts = {k: v for k, v in cfg.items() if k != 'agent'}
    xy, prev = torch.as_tensor(poses[:, :2], device='cuda'), torch.as_tensor(poses[:, 2:], device='cuda')
    packed = torch.as_tensor(bc.pack(imgs[pick] == 255).view(np.int64), device='cuda')
    got = _terms_np(shaping.reward_terms_bits(packed, xy, prev, **opts))
    _assert_same(got, want, '%d x %d as bits' % (rows, cols))
    _assert_same(got, _terms_np(shaping.reward_terms(torch.as_tensor(imgs[pick], device='cuda'), xy, prev, **opts)), '%d x %d bits vs bytes' % (rows, cols))
    reward = want['centering_term'] / cfg['w_centering']
    assert 0.1 < want['collided'].mean() < 0.9 and ((reward > 0) & (reward < 1)).mean() > 0.1 and (reward == -1).mean() > 0.1
    assert n % 4 != 0
    with pytest.raises(ValueError):
        shaping.reward_terms_bits(packed, xy, prev, **dict(opts, cols=cols + 64))
    with pytest.raises(ValueError):
        shaping.reward_terms_bits(packed, xy, prev)


def test_bind_wants_exactly_one_image(assets):
    import torch
    from red_gym_amd import _lib
    env = _env(assets, 2)
    env.shape_rewards(image='bits')
    sh = env.eng.shaper
    assert sh.buf['bitmap'].dtype == torch.int64 and tuple(sh.buf['bitmap'].shape) == (2, 256, 4)
    ptrs = _lib.ShapingBuffers()
    for name in _lib.SHAPING_FIELDS:
        setattr(ptrs, name, sh.buf['bitmap' if name == 'bitmap_bits' else name].data_ptr())
    assert env.eng.lib.f110_shaping_bind(env.eng._h, C.byref(ptrs)) == _lib.E_INVALID               # both
    assert b'exactly one' in env.eng.lib.f110_last_error()
    ptrs.bitmap, ptrs.bitmap_bits = None, None
    assert env.eng.lib.f110_shaping_bind(env.eng._h, C.byref(ptrs)) == _lib.E_INVALID               # neither
    ptrs.bitmap_bits = sh.buf['bitmap'].data_ptr()
    assert env.eng.lib.f110_shaping_bind(env.eng._h, C.byref(ptrs)) == 0
    env.close()


def test_pose_that_is_not_finite_in_bits_mode(assets):
    """As in bytes mode: the four terms are NaN, collided is 0, prev_xy stays; the other envs are paid normally."""
    import torch
    from red_gym_amd import workload
    B = 8
    env = _env(assets, B, autoreset=False)
    env.shape_rewards(image='bits')
    env.reset(workload.spawn_poses(B, 1))
    env.step(torch.zeros((B, 1, 2), dtype=torch.float64, device=env.device))
    prev = env.eng.shaper.buf['prev_xy'].clone()
    env.state[0::4, 0, 0] = float('nan')
    env.state[1::4, 0, 1] = float('inf')
    env.eng.t['current_time'] += 1.0                               # "stepped": the clocks moved
    env.eng.shaper.kernel()
    torch.cuda.synchronize()
    s = env.eng.shaper.buf
    bad = (torch.arange(B, device=env.device) % 4) < 2
    for k in ('collision_term', 'progress_term', 'centering_term', 'total'):
        assert torch.isnan(s[k][bad]).all() and torch.isfinite(s[k][~bad]).all(), k
    assert (s['collided'][bad] == 0).all() and torch.equal(s['prev_xy'][bad], prev[bad])
    assert torch.equal(s['prev_xy'][~bad], env.state[~bad, 0, :2])
    assert env.eng.device_errors() == 0
    env.close()


def _twins(assets, B, T, **kw):
    """Two envs that differ in the image form alone, shaper, follower and replay on."""
    envs = []
    for image in ('bytes', 'bits'):
        env = _env(assets, B, autoreset=True, timestep=0.025)
        env.shape_rewards(image=image, **kw)
        env.follow_paths()
        env.record_replay(steps=T)
        envs.append(env)
    return envs


def _same_step(res_bytes, res_bits, what):
    import torch
    (_, r0, d0, i0), (_, r1, d1, i1) = res_bytes, res_bits
    nan = lambda t: torch.nan_to_num(t.double(), nan=-12345.0)   # noqa: E731
    assert torch.equal(nan(r0), nan(r1)) and torch.equal(d0, d1), what
    for k in INFO_KEYS + ('replay_valid', 'replay_count', 'current_time'):
        assert torch.equal(nan(i0[k]), nan(i1[k])), (what, k)
    assert 'lidar_bitmap_bits' in i1 and 'lidar_bitmap' not in i1 and 'lidar_bitmap' in i0 and 'lidar_bitmap_bits' not in i0
    assert np.array_equal(bc.as_u64(i1['lidar_bitmap_bits']), bc.pack(i0['lidar_bitmap'].cpu().numpy() == 255)), what


@pytest.mark.parametrize('rows,cols', [(256, 256), (75, 100)])
def test_closed_loop_twins(assets, rows, cols):
    """5 envs (a batch that does not fill a workgroup; env 1 spawned across the track and driven at the wall), shaper, follower
    and a ring of 8 steps, 60 steps with autoreset and a masked reset in the middle, random raw actions: after every step the
    reward, its terms, collided and the push's verdict are `==` between the twins and the bits image is the packed byte image;
    at the end the rings are `==` tensor by tensor."""
    import torch
    from red_gym_amd import workload
    B, T, AD = 5, 8, 16
    e0, e1 = _twins(assets, B, T, rows=rows, cols=cols)
    assert e1.eng.shaper.buf['bitmap'].shape == (B, rows, bc.words(cols)) and e0.eng.shaper.buf['bitmap'].shape == (B, rows, cols)
    spawn = workload.spawn_poses(B, 1)
    crash = np.arange(B) % 4 == 1
    spawn[crash, 0, 2] += np.pi / 2
    crash_dev = torch.as_tensor(crash, device=e0.device)
    rng = np.random.default_rng(18)
    _same_step(e0.reset(spawn), e1.reset(spawn), 'reset')
    autoresets, masked = 0, 0
    for k in range(60):
        if k == 30:
            mask = torch.as_tensor((np.arange(B) % 2 == 0).astype(np.uint8))
            res = e0.reset(spawn, mask), e1.reset(spawn, mask)
            _same_step(res[0], res[1], 'masked reset')
            masked += int((res[1][3]['current_time'].cpu().numpy() == e1.timestep).sum())
            continue
        raw = torch.as_tensor(rng.uniform(-1.0, 1.0, (B, AD)), device=e0.device)
        res = []
        for env in (e0, e1):
            acts = env.path_actions(raw)
            acts[:, 0, 0] = torch.where(crash_dev, 0.0, acts[:, 0, 0])
            acts[:, 0, 1] = torch.where(crash_dev, 8.0, acts[:, 0, 1])
            res.append(env.step(acts))
        _same_step(res[0], res[1], 'step %d' % k)
        autoresets += int((res[1][3]['current_time'].cpu().numpy() == e1.timestep).sum())
    print('autoresets: %d, envs reset by the mask: %d, valid transitions held: %d' % (autoresets, masked, len(e1.replay)))
    assert autoresets > 0, 'no autoreset happened'
    assert masked >= 3, 'no masked reset was issued'
    torch.cuda.synchronize()
    assert len(e1.replay) > 0 and int(e1.replay.buf['count']) == 61
    for k in RING_KEYS:
        assert torch.equal(e0.replay.buf[k], e1.replay.buf[k]), k
    assert bool(e1.replay.buf['frames'].any())
    # what the ring gives back is the same too
    idx = torch.arange(T * B, device=e0.device)
    for a, b in zip(e0.replay.sample_at(idx), e1.replay.sample_at(idx)):
        assert torch.equal(a, b)
    assert e0.eng.device_errors() == 0 and e1.eng.device_errors() == 0
    e0.close(); e1.close()


def _run(env, stepper, pool, sd, lo, hi):
    import torch
    env.load_state_dict(sd)
    env.replay.buf['count'].zero_()                               # (load_state_dict leaves the ring alone: start every run alike)
    env.replay.restart()
    outs = []
    for k in range(lo, hi):
        env.replay_action.fill_(float(k))
        _, reward, _, info = stepper(pool[k])
        o = {key: info[key].clone() for key in INFO_KEYS + ('replay_valid',)}
        o['total'] = reward.clone()
        key = 'lidar_bitmap_bits' if 'lidar_bitmap_bits' in info else 'lidar_bitmap'
        o['image'] = info[key].clone() if key == 'lidar_bitmap_bits' else None
        o['bytes'] = info[key].clone() if key == 'lidar_bitmap' else None
        outs.append(o)
    torch.cuda.synchronize()
    return outs, {k: env.replay.buf[k].clone() for k in RING_KEYS}


def _equal_runs(a, b, what, keys=None):
    import torch
    for k, (x, y) in enumerate(zip(a, b)):
        for key in keys or x:
            if x[key] is None or y[key] is None:
                continue
            assert torch.equal(torch.nan_to_num(x[key].double(), nan=-12345.0), torch.nan_to_num(y[key].double(), nan=-12345.0)), (what, k, key)


def test_graphs_and_checkpoints_in_bits_mode(assets):
    """In bits mode step_graph and step_lib_graph `==` eager for 12 steps, ring included; a state_dict() taken in bits mode
    continues `==` in a bytes-mode env and the other way round; installing the shaper again in the other form keeps the replay
    buffer and its ring."""
    import torch
    from red_gym_amd import replay, workload
    B, A, T = 6, 2, 5
    pool = workload.action_pool(20, B, A)
    env = _env(assets, B, A, autoreset=True)
    env.shape_rewards(image='bits')
    env.record_replay(steps=T, action_dim=3)
    env.reset(workload.spawn_poses(B, A))
    for k in range(4):
        env.step(pool[k])
    sd = env.state_dict()
    assert {'prev_xy', 't_seen', 'lidar_bitmap_bits'} <= set(sd) and 'lidar_bitmap' not in sd
    assert sd['lidar_bitmap_bits'].dtype == torch.int64 and tuple(sd['lidar_bitmap_bits'].shape) == (B, 256, 4)
    eager, ring = _run(env, env.step, pool, sd, 4, 16)
    assert float(eager[-1]['reward_progress'].max()) > 0.0 and bool(ring['valid'].any())
    env.capture_step()
    outs, ring_g = _run(env, env.step_graph, pool, sd, 4, 16)
    _equal_runs(eager, outs, 'step_graph')
    env.build_step_graph()
    outs, ring_lg = _run(env, env.step_lib_graph, pool, sd, 4, 16)
    _equal_runs(eager, outs, 'step_lib_graph')
    for k in RING_KEYS:
        assert torch.equal(ring[k], ring_g[k]) and torch.equal(ring[k], ring_lg[k]), k
    # the checkpoint of the bits env in a bytes env ...
    other = _env(assets, B, A, autoreset=True)
    other.shape_rewards()
    other.record_replay(steps=T, action_dim=3)
    other.reset(workload.spawn_poses(B, A))
    outs, ring_b = _run(other, other.step, pool, sd, 4, 16)
    _equal_runs(eager, outs, 'bits checkpoint in a bytes env', INFO_KEYS + ('replay_valid', 'total'))
    for k in RING_KEYS:
        assert torch.equal(ring[k], ring_b[k]), k
    for o, e in zip(outs, eager):
        assert torch.equal(replay.pack_bitmaps(o['bytes']), e['image'])
    # ... and a bytes checkpoint in the bits env
    other.load_state_dict(sd)
    for k in range(4, 8):
        other.step(pool[k])
    mid = other.state_dict()
    assert 'lidar_bitmap' in mid and 'lidar_bitmap_bits' not in mid and mid['lidar_bitmap'].dtype == torch.uint8
    rest_bytes, _ = _run(other, other.step, pool, mid, 8, 16)
    rest_bits, _ = _run(env, env.step, pool, mid, 8, 16)
    _equal_runs(eager[4:], rest_bytes, 'bytes run resumed', INFO_KEYS + ('total',))
    _equal_runs(eager[4:], rest_bits, 'bytes checkpoint in the bits env', INFO_KEYS + ('total', 'image'))
    # the other form at the same size: the shaper restarts, the replay buffer and what it holds stay
    held = {k: env.replay.buf[k].clone() for k in RING_KEYS}
    env.shape_rewards(image='bytes')
    assert env.replay.on and env.eng.shaper.buf['bitmap'].dtype == torch.uint8
    for k in RING_KEYS:
        assert torch.equal(env.replay.buf[k], held[k]), k
    _, _, _, info = env.step(pool[0])
    assert 'lidar_bitmap' in info and 'lidar_bitmap_bits' not in info and int(info['replay_count']) == int(held['count']) + 1
    env.shape_rewards(image='bits')
    assert env.replay.on
    _, _, _, info = env.step(pool[1])
    assert 'lidar_bitmap_bits' in info and int(info['replay_count']) == int(held['count']) + 2
    env.shape_rewards(image='bits', rows=75, cols=100)                 # another size: the ring goes, as before
    assert not env.replay.on
    assert env.eng.device_errors() == 0 and other.eng.device_errors() == 0
    env.close(); other.close()


def test_stem_reads_the_bits(assets):
    """BitConvStem on info['lidar_bitmap_bits'] torch.equal to the same module on the twin's info['lidar_bitmap'], and
    replay.unpack_bitmaps gives the byte image back."""
    import torch
    from red_gym_amd import replay, workload
    from red_gym_amd.bitconv import BitConvStem
    B = 5
    pool = workload.action_pool(4, B, 1)
    infos = []
    for image in ('bytes', 'bits'):
        env = _env(assets, B, autoreset=True)
        env.shape_rewards(image=image)
        env.reset(workload.spawn_poses(B, 1))
        for k in range(4):
            info = env.step(pool[k])[3]
        infos.append({k: v.clone() for k, v in info.items() if k.startswith('lidar_bitmap')})
        env.close()
    torch.manual_seed(4)
    stem = BitConvStem(cols=256, device='cuda')
    with torch.no_grad():
        a, b = stem(infos[0]['lidar_bitmap']), stem(infos[1]['lidar_bitmap_bits'])
    assert a.shape == b.shape and a.shape[0] == B and bool((a != 0).any())
    assert torch.equal(a, b)
    assert torch.equal(replay.unpack_bitmaps(infos[1]['lidar_bitmap_bits'], 256), infos[0]['lidar_bitmap'])


def test_default_is_unmoved(assets):
    import torch
    from red_gym_amd import workload
    B = 3
    env = _env(assets, B, autoreset=True)
    env.shape_rewards()
    _, _, _, info = env.reset(workload.spawn_poses(B, 1))
    assert 'lidar_bitmap_bits' not in info and 'lidar_bitmap_bits' not in env.state_dict()
    assert info['lidar_bitmap'].dtype == torch.uint8 and tuple(info['lidar_bitmap'].shape) == (B, 256, 256)
    assert env.eng.shaper.bits is False
    with pytest.raises(ValueError):
        env.shape_rewards(image='words')
    assert env.eng.shaper.on and 'lidar_bitmap' in env.step(workload.action_pool(1, B, 1)[0])[3]   # a refused install changes nothing
    env.close()
