"""Times the observation path of the SAC wrapper's step with the lidar bitmap held as bytes against held as bits
(shape_rewards(image='bytes' | 'bits')), SAL's 256 x 256 FILL image, two envs of the same size in one process:
    python tools/time_bits.py [launches] [--variant LIB] [envs ...]
(a) the render (f110_bitmap_render against f110_bitmap_render_bits), (b) the shaper's kernel, (c) the replay push, (d) the whole
step with shaper + follower + replay, eager and step_lib_graph, (e) the device memory the observation path holds.
hipEvents around `launches` back-to-back calls after a warm-up; the windows of the two forms alternate, the median of 5 is
reported and the 5 values are printed: their spread is what a difference has to exceed.
--variant LIB: a second build of the library whose bits form stores non-temporally (tools/build_variant.sh stream
-DF110_BM_BITS_STREAM=1), loaded beside the product build; its render joins the alternation of (a).
Results: profiles/r15_bitmap_bits.txt."""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from red_gym_amd import F110VecEnv, _lib, workload
from red_gym_amd.lidar import LidarBitmap
from timing import report

args = sys.argv[1:]
VARIANT = None
if '--variant' in args:
    i = args.index('--variant')
    VARIANT = args[i + 1]
    del args[i:i + 2]
N = int(args[0]) if args else 50
SIZES = [int(a) for a in args[1:]] or [4096, 65536]
T = 3            # step slots of the ring
ROWS = COLS = 256
FORMS = ('bytes', 'bits')


def variant_renderer(path, num_beams, device):
    """A FILL renderer of the shaper's options that runs the library build at `path` instead of the product build."""
    lib = C.CDLL(os.path.abspath(path))
    for name in ('f110_bitmap_create', 'f110_bitmap_render', 'f110_bitmap_render_bits', 'f110_bitmap_destroy'):
        getattr(lib, name).argtypes = _lib.SYMBOLS[name]
        getattr(lib, name).restype = C.c_int
    lib.f110_bitmap_destroy.restype = None
    product, _lib._lib = _lib._lib, lib
    try:
        return LidarBitmap(num_beams, bg_color='black', draw_mode='FILL', output_image_dims=(ROWS, COLS), device=device)
    finally:
        _lib._lib = product


for B in SIZES:
    envs = {}
    for image in FORMS:
        env = F110VecEnv(B, map=workload.EXAMPLE_MAP, num_agents=1, autoreset=True)
        env.shape_rewards(image=image, rows=ROWS, cols=COLS)
        env.follow_paths()
        env.record_replay(steps=T)
        env.reset(torch.as_tensor(workload.spawn_poses(B, 1), device=env.device))
        envs[image] = env
    dev = envs['bytes'].device
    raw = torch.empty((B, 16), dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=torch.Generator(device=dev).manual_seed(5))
    for env in envs.values():
        for _ in range(T + 2):
            env.step(env.path_actions(raw))
    # the two envs are twins: the same rewards and the same ring so far
    torch.cuda.synchronize()
    a, b = envs['bytes'], envs['bits']
    assert torch.equal(a.eng.shaper.buf['total'], b.eng.shaper.buf['total']) and torch.equal(a.replay.buf['frames'], b.replay.buf['frames'])
    print('---- %d envs x 1, %d x %d FILL, T = %d, %d launches per window' % (B, ROWS, COLS, T, N), flush=True)

    def tick(env):
        env.eng.t['current_time'].add_(env.timestep)   # (a clock that stands still marks the env as not stepped; ~2 us)

    def shaper_kernel(env):
        tick(env)
        env.eng.shaper.kernel()

    def push(env):
        tick(env)
        env.replay.kernel()

    renders = {image: envs[image].eng.shaper.render for image in FORMS}
    if VARIANT:
        vr = variant_renderer(VARIANT, a.eng.num_beams, a.eng.device_index)
        spare = torch.empty_like(b.eng.shaper.buf['bitmap'])
        scans = b.eng.t['scans'][:, 0]
        renders['bits, non-temporal stores (variant build)'] = lambda: vr.bits(scans, out=spare)
        renders['bits, product build into the same spare buffer'] = lambda: b.eng.shaper._to_img.bits(scans, out=spare)
    report(renders, N, 10, 5, name='(a) render, ')
    if VARIANT:
        vr.bits(scans, out=spare)
        torch.cuda.synchronize()
        assert torch.equal(spare, b.eng.shaper.buf['bitmap'])
        vr.close()
        del spare
    report({image: (lambda e=envs[image]: shaper_kernel(e)) for image in FORMS}, N, 10, 5, name='(b) shaper kernel (+ clock add), ')
    report(dict({image: (lambda e=envs[image]: push(e)) for image in FORMS},
               **{'clock add alone': lambda: tick(a)}), N, 10, 5, name='(c) replay push (+ clock add), ')

    def eager(env):
        env.step(env.path_actions(raw))

    report({image: (lambda e=envs[image]: eager(e)) for image in FORMS}, max(N // 2, 5), 10, 5, name='(d) step + shaper + follower + replay, eager, ')
    bufs = {image: envs[image].build_step_graph() for image in FORMS}

    def graphed(env, buf):
        env.path_actions(raw, out=buf)
        env.step_lib_graph()

    report({image: (lambda e=envs[image], g=bufs[image]: graphed(e, g)) for image in FORMS}, max(N // 2, 5), 10, 5, name='(d) the same through step_lib_graph, ')
    for image in FORMS:
        env = envs[image]
        bm, fr = env.eng.shaper.buf['bitmap'], env.replay.buf['frames']
        print('(e) %-5s shaper bitmap %s %s = %.1f MB, ring frames (T + 1 = %d slots) %.1f MB, together %.1f MB'
              % (image, tuple(bm.shape), str(bm.dtype).replace('torch.', ''), bm.numel() * bm.element_size() / 1e6, T + 1,
                 fr.numel() * fr.element_size() / 1e6, (bm.numel() * bm.element_size() + fr.numel() * fr.element_size()) / 1e6), flush=True)
        assert env.eng.device_errors() == 0
    for env in envs.values():
        env.close()
    del envs, a, b, env, renders, bufs
    torch.cuda.empty_cache()
