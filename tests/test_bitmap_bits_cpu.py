"""The bits form of the lidar bitmap without a GPU: header, exports and the Python mirror agree on its entry points and on the
struct field appended for it, the argument handling of shape_rewards(image=...), and the NumPy checker gives the reference's
recorded rewards when it is fed images that went through the bit format."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_header
import bits_cases as bc
import replay_cases as rc
import shaping_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('f110_bitmap_render_bits', 'f110_shaping_terms_bits')


@pytest.fixture(scope='module')
def lib():
    from red_gym_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope='module')
def header():
    return abi_header.read(os.path.join(ROOT, 'include', 'f110_hip.h'))


def test_header_exports_and_mirror_agree_on_the_new_entry_points(lib, header):
    from red_gym_amd import _lib
    for name, twin in zip(NEW, ('f110_bitmap_render', 'f110_shaping_terms')):
        # the bits entry takes what its bytes twin takes, but for the image: uint64 words instead of uint8 pixels
        (ret, params), (twin_ret, twin_params) = header[2][name], header[2][twin]
        assert ret == twin_ret and len(params) == len(twin_params)
        assert [(p, q) for p, q in zip(params, twin_params) if p != q] == [('uint64*', 'uint8*')]
        assert list(_lib.SYMBOLS[name]) == list(_lib.SYMBOLS[twin])
    # without a renderer / a config both refuse before any HIP call
    assert lib.f110_bitmap_render_bits(None, None, 0, 1, 1080, None, None) == _lib.E_INVALID
    assert lib.f110_shaping_terms_bits(None, None, None, None, 1, None, None, None, None, None, None) == _lib.E_INVALID


def test_shaping_buffers_field_is_appended(header):
    from red_gym_amd import _lib
    fields = _lib.SHAPING_FIELDS        # (that they are the header's, with its offsets: tests/test_abi_cpu.py)
    assert fields[-1] == 'bitmap_bits' and fields[0] == 'bitmap' and len(fields) == 9      # appended: the first eight keep their offsets
    assert [getattr(_lib.ShapingBuffers, f).offset for f in fields] == [i * C.sizeof(C.c_void_p) for i in range(9)]
    assert header[1]['f110_shaping_buffers'][-1] == ('bitmap_bits', 'uint64*', 0)


def test_image_argument_handling(lib):
    from red_gym_amd import shaping
    shaping.validate(num_agents=1, image='bits')
    shaping.validate(num_agents=1, image='bytes')
    shaping.validate(num_agents=3, image='bits', agent=2, rows=75, cols=100)
    assert shaping.image_form('bits') is True and shaping.image_form('bytes') is False
    for bad in ('bit', 'BITS', '', 'uint8', 'packed'):
        with pytest.raises(ValueError):
            shaping.validate(num_agents=1, image=bad)
        with pytest.raises(ValueError):
            shaping.image_form(bad)
    with pytest.raises(ValueError):
        shaping.image_form(None)
    with pytest.raises(ValueError):                       # the other refusals stay what they were
        shaping.validate(num_agents=1, image='bits', rows=0)
    # `image` is no field of the config
    assert 'image' not in shaping.DEFAULTS and 'image' not in [f for f, _ in shaping.make_config()._fields_]
    with pytest.raises(TypeError):
        shaping.make_config(image='bits')
    # install() checks `image` before it touches the engine
    shaper = shaping.RewardShaper.__new__(shaping.RewardShaper)
    with pytest.raises(ValueError):
        shaping.RewardShaper.install(shaper, image='neither')
    assert shaping.RewardShaper.IMAGE_KEYS == ('lidar_bitmap', 'lidar_bitmap_bits')


def test_pack_is_the_rings_format():
    """bits_cases.pack of (img == 255) is replay_cases.pack(img), tail bits 0, and unpack inverts it -- at every size used."""
    for rows, cols in bc.SIZES:
        imgs = rc.random_images(rows, cols, n=3, seed=1)
        p = bc.pack(imgs == 255)
        assert p.shape == (3, rows, bc.words(cols)) and p.dtype == np.uint64
        assert np.array_equal(p, rc.pack(imgs))
        assert np.array_equal(bc.unpack(p, cols), np.where(imgs == 255, 255, 0).astype(np.uint8))
        if cols % 64:
            assert not (p[:, :, -1] >> np.uint64(cols % 64)).any()
        full = bc.pack(np.ones((1, rows, cols), bool))
        assert int(full[0, 0, -1]) == (1 << (cols % 64 or 64)) - 1


def test_checker_over_the_bit_format_equals_the_reference_on_g16(golden):
    """The reference's recorded rewards of g16 from images that went through pack / unpack: the bit format loses nothing the
    shaper reads (a FILL image holds 0 and 255 only)."""
    g = golden('g16_shaping.npz')
    imgs = {}
    for k, grp in enumerate(sc.GROUPS):
        raw = sc.unpack_images(g, grp)
        imgs[k] = bc.unpack(bc.pack(raw == 255), raw.shape[2])
        assert np.array_equal(imgs[k], raw)
    n = g['group'].shape[0]
    keys = ('collided',) + sc.TERMS
    got = {k: np.zeros(n) for k in keys}
    for i in range(n):
        r = sc.reward_terms(imgs[int(g['group'][i])][int(g['img'][i])], g['xy'][i, 0], g['xy'][i, 1], g['prev'][i, 0], g['prev'][i, 1])
        for k in keys:
            got[k][i] = r[k]
    bad = {k: int((~sc.same(got[k], g[k].astype(np.float64))).sum()) for k in keys}
    print('g16 through the bit format: %d cases, differing:' % n, bad)
    assert n >= 5000 and not any(bad.values()), bad
