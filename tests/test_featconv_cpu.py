"""The dense feature-map convolution without a device: f110_featconv_validate and f110_featconv_workspace limit by limit through the
loaded library, the checkers of tests/featconv_cases.py against naive loops, against fp64 within gamma * mag at every case and
against the reference's own Actor (g22_trunk.npz, g22_trunk_unit.npz) within 2 * gamma * mag, the banding arithmetic (paths) on every case, and what
FeatConv2d and Trunk refuse on the host."""

import numpy as np
import pytest

import bitconv_cases as bc
import featconv_cases as fc

GOOD = dict(in_channels=32, rows=30, cols=30, out_channels=32, kernel=3, stride=1)


def _within(v, ref, mag, terms, factor=1.0):
    err = np.abs(np.asarray(v, np.float64) - ref)
    bound = factor * fc.gamma(terms) * mag
    print('T = %d: worst error / bound %.4f' % (terms, float((err / np.maximum(bound, 1e-300)).max())))
    return bool((err <= bound).all())


def test_validate_each_limit_at_its_edge():
    """Every limit at its last accepted and its first refused value; the symbols do not exist before this feature."""
    from red_gym_amd import _lib, featconv
    lib = _lib.load()
    assert lib.f110_featconv_validate(None) == _lib.E_INVALID
    featconv.validate(**GOOD)
    edges = [(dict(kernel=1), dict(kernel=0)), (dict(kernel=4, out_channels=32), dict(kernel=5, in_channels=16, out_channels=16)),
             (dict(stride=1), dict(stride=0)), (dict(stride=4), dict(stride=5)),
             (dict(in_channels=1), dict(in_channels=0)), (dict(in_channels=32), dict(in_channels=33)),
             (dict(out_channels=1), dict(out_channels=0)), (dict(out_channels=64, kernel=2), dict(out_channels=65, kernel=2)),
             (dict(in_channels=32, kernel=4), dict(in_channels=29, kernel=5, out_channels=8)),        # Ci k^2 = 512 | kernel itself
             (dict(in_channels=32, kernel=4, out_channels=32), dict(in_channels=32, kernel=4, out_channels=33)),   # Co k^2 = 512 | 528
             (dict(in_channels=32, kernel=4, out_channels=8, rows=4, cols=4), dict(in_channels=32, kernel=4, out_channels=8, rows=3, cols=4)),
             (dict(out_channels=56, kernel=3), dict(out_channels=57, kernel=3)),                       # Co k^2 = 504 | 513
             (dict(rows=3), dict(rows=2)), (dict(cols=3), dict(cols=2)), (dict(cols=64), dict(cols=65)),
             (dict(rows=16384), dict(rows=-1))]
    for ok, bad in edges:
        featconv.validate(**dict(GOOD, **ok))
        with pytest.raises(ValueError):
            featconv.validate(**dict(GOOD, **bad))
    # Ci k^2 above 512 with every other limit kept needs k = 4 and Ci = 33, which in_channels refuses first; Co k^2 is reachable alone
    with pytest.raises(ValueError, match='out_channels \\* kernel'):
        featconv.validate(**dict(GOOD, out_channels=57))
    with pytest.raises(ValueError, match='out_channels \\* kernel'):
        featconv.validate(**dict(GOOD, out_channels=64, kernel=4, in_channels=8, rows=8, cols=8))
    for case in fc.CASES + [fc.LOOP_CASE]:
        ci, h, w, co, k, s = case
        cfg = featconv.validate(ci, h, w, co, k, s, True)
        assert (cfg.in_channels, cfg.rows, cfg.cols, cfg.out_channels, cfg.kernel, cfg.stride, cfg.relu, cfg.reserved) == (ci, h, w, co, k, s, 1, 0)
        assert featconv.output_size(h, w, k, s) == fc.out_size(h, w, k, s)


def test_workspace_matches_the_formula():
    from red_gym_amd import _lib, featconv
    lib = _lib.load()
    for case in fc.CASES:
        ci, h, w, co, k, s = case
        cfg = featconv.make_config(ci, h, w, co, k, s)
        for n in (1, 3, 64, 4096):
            assert featconv.workspace_bytes(cfg, n) == n * co * (ci * k * k + 1) * 4
        assert featconv.workspace_bytes(cfg, 0) == 0 and featconv.workspace_bytes(cfg, -5) == 0
    conv3 = featconv.make_config(*fc.CONV3)
    assert featconv.workspace_bytes(conv3, 64) == 2367488 and featconv.workspace_bytes(conv3, 4096) == 151519232
    assert featconv.workspace_bytes(conv3, 1 << 40) == (1 << 40) * 32 * 289 * 4
    most = (2 ** 63 - 1) // (32 * 289 * 4)                         # the last n whose byte count fits int64
    assert featconv.workspace_bytes(conv3, most) == most * 32 * 289 * 4
    assert featconv.workspace_bytes(conv3, most + 1) == 0 and featconv.workspace_bytes(conv3, 1 << 62) == 0 and featconv.workspace_bytes(conv3, 2 ** 63 - 1) == 0
    for bad in (dict(kernel=5), dict(cols=65), dict(in_channels=33), dict(out_channels=0), dict(stride=0), dict(out_channels=57)):
        assert featconv.workspace_bytes(featconv.make_config(**dict(GOOD, **bad)), 8) == 0
    assert lib.f110_featconv_workspace(None, 8) == 0


def test_checkers_equal_naive_chains():
    """grad_x, the partials and the reduction on a tiny strided shape, element by element from the contract's sentences."""
    ci, h, w, co, k, s = 2, 6, 7, 3, 3, 2
    r = fc.reference((ci, h, w, co, k, s), 2, True, seed=5)
    oh, ow = fc.out_size(h, w, k, s)
    x, wt, g = r['x'], r['w'], r['g']
    assert (r['out'] == 0).any() and (g != r['grad_out']).any() and (g != 0).any()
    assert bc.bit_patterns(r['out']).tolist() == bc.bit_patterns(fc.forward(x, wt, r['b'], s, True)).tolist()
    for n in range(2):
        for c in range(ci):
            for iy in range(h):
                for ix in range(w):
                    acc = np.float32(0.0)
                    for o in range(co):
                        for ky in range(k):
                            for kx in range(k):
                                py, px = iy - ky, ix - kx
                                if py >= 0 and px >= 0 and py % s == 0 and px % s == 0 and py // s < oh and px // s < ow:
                                    acc = fc.fma32(wt[o, c, ky, kx], g[n, o, py // s, px // s], acc)
                    assert bc.bit_patterns(acc) == bc.bit_patterns(r['grad_x'][n, c, iy, ix])
        for o in range(co):
            bsum = np.float32(0.0)
            for oy in range(oh):
                for ox in range(ow):
                    bsum = np.float32(bsum + g[n, o, oy, ox])
            assert bc.bit_patterns(bsum) == bc.bit_patterns(r['B'][n, o])
            for c in range(ci):
                for ky in range(k):
                    for kx in range(k):
                        acc = np.float32(0.0)
                        for oy in range(oh):
                            for ox in range(ow):
                                acc = fc.fma32(g[n, o, oy, ox], x[n, c, s * oy + ky, s * ox + kx], acc)
                        assert bc.bit_patterns(acc) == bc.bit_patterns(r['P'][n, o, c, ky, kx])
    assert np.array_equal(r['grad_weight'], r['P'][0] + r['P'][1]) and np.array_equal(r['grad_bias'], r['B'][0] + r['B'][1])
    three = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    assert fc.reduce(three)[0] == np.float32(1.0) and np.float32(three[0] + (three[1] + three[2]))[0] != np.float32(1.0)   # ascending, not a tree
    assert (r['grad_x'][:, :, :, :] != 0).any()


@pytest.mark.parametrize('case', fc.CASES)
def test_checkers_within_gamma_mag_of_fp64(case):
    ci, h, w, co, k, s = case
    n = 2
    r = fc.reference(case, n, True)
    oh, ow = fc.out_size(h, w, k, s)
    ref, mag = fc.forward_fp64(r['x'], r['w'], r['b'], s)
    assert _within(r['out'], np.maximum(ref, 0.0), mag, ci * k * k + 1)
    assert _within(fc.finish2(r['acc'], None, False), *fc.forward_fp64(r['x'], r['w'], None, s), ci * k * k)
    ref, mag = fc.grad_x_fp64(r['g'], r['w'], s, h, w)
    assert _within(r['grad_x'], ref, mag, co * (-(-k // s)) ** 2)
    gw, mw, gb, mb = fc.grad_w_fp64(r['g'], r['x'], k, s)
    assert _within(r['grad_weight'], gw, mw, n * oh * ow) and _within(r['grad_bias'], gb, mb, n * oh * ow)
    if co * oh * ow >= 8:                                          # (one pixel behind a ReLU may be masked in both samples)
        assert (r['out'] == 0).any() and (r['out'] > 0).any() and (r['grad_weight'] != 0).any() and (r['P'][0] != r['P'][1]).any()


@pytest.mark.parametrize('name', fc.GOLDEN)
def test_checkers_within_twice_gamma_mag_of_the_reference(golden, name):
    """Layer by layer on the inputs the reference's Actor recorded (the raw 0 / 255 row and the / 255
    row), its `out` as the mask of the backward: the checker and the reference each stand within gamma * mag of the same fp64 value."""
    g = golden(name)
    rows = g['a1'].shape[0]
    assert g['on'].shape == (rows,) and g['cotangent'].shape == (rows, 32 * 28 * 28) and float(g['on'][0]) == (255.0 if name == fc.GOLDEN[0] else 1.0)
    for name, xin, s, go in fc.golden_layers(g):
        w, b, out = g[name + '_weight'], g[name + '_bias'], g[name + '_out']
        co, ci, k, _ = w.shape
        assert all(v.dtype == np.float32 for v in (w, b, out, go, xin)) and 0.05 < (out > 0).mean() < 0.95
        ref, mag = fc.forward_fp64(xin, w, b, s)
        assert _within(fc.forward(xin, w, b, s, True), out.astype(np.float64), mag, ci * k * k + 1, 2.0)
        gm = fc.masked(out, go, True)
        _, mag = fc.grad_x_fp64(gm, w, s, xin.shape[2], xin.shape[3])
        assert _within(fc.grad_x(gm, w, s, xin.shape[2], xin.shape[3]), g[name + '_grad_input'].astype(np.float64), mag, co * (-(-k // s)) ** 2, 2.0)
        P, B = fc.partials(gm, xin, k, s)
        _, mw, _, mb = fc.grad_w_fp64(gm, xin, k, s)
        pixels = rows * out.shape[2] * out.shape[3]
        assert _within(fc.reduce(P), g[name + '_weight_grad'].astype(np.float64), mw, pixels, 2.0)
        assert _within(fc.reduce(B), g[name + '_bias_grad'].astype(np.float64), mb, pixels, 2.0)


def test_every_case_selects_what_it_claims():
    P = {c: fc.paths(*c) for c in fc.CASES}
    conv3, conv2, odd, one, pixel, three, four, apart, full, gap1, gap2, gap3, gap4 = (P[c] for c in fc.CASES)
    assert fc.GAP_CASES == fc.CASES[9:] == [(3, 9, 11, 5, 1, 2), (4, 10, 13, 6, 2, 3), (2, 12, 14, 4, 3, 4), (5, 8, 9, 3, 1, 4)]
    assert all(c[4] >= c[5] for c in fc.CASES[:9])
    for p in P.values():
        assert max(p['lds'], p['gx_lds'], p['gw_lds']) <= fc.FC_LDS_BYTES and p['xw'] <= 64 and p['gx_xw'] <= 67
    assert (conv3['oh'], conv3['ow'], conv3['ktot'], conv3['chunks'], conv3['NT'], conv3['br'], conv3['bands']) == (28, 28, 288, 9, 2, 14, 2)
    assert not conv3['kpad'] and conv3['partial_m'] and conv3['ragged'] and (conv3['gx_br'], conv3['gx_bands'], conv3['gx_last_rows']) == (13, 3, 4)
    assert (conv3['gw_NT'], conv3['gw_groups'], conv3['gw_idle_waves'], conv3['gw_MT'], conv3['gw_br'], conv3['gw_bands']) == (18, 3, 3, 2, 7, 4)
    assert (conv2['oh'], conv2['ow'], conv2['ktot'], conv2['br'], conv2['bands'], conv2['last_rows'], conv2['lds']) == (30, 30, 256, 7, 5, 2, 64528)
    assert conv2['gx_dilated'] and (conv2['gx_ktot'], conv2['gx_chunks'], conv2['gx_bands']) == (512, 16, 16) and conv2['unused_rows'] == conv2['unused_cols'] == 1
    assert (conv2['gw_groups'], conv2['gw_idle_waves'], conv2['gw_bands'], conv2['gw_last_rows']) == (2, 0, 8, 2)
    # (5, 11, 13, 7, 3, 2): K = 45 padded, partial tiles everywhere, a dilated g; its windows reach every row and column of x -- the
    # rows and columns no window reaches are conv2's (one each) and those of (32, 6, 6, 8, 4, 3) (two each)
    assert (odd['ktot'], odd['chunks']) == (45, 2) and odd['kpad'] and odd['partial_m'] and odd['partial_n'] and odd['gx_kpad'] and odd['gx_dilated']
    assert odd['gw_partial_n'] and odd['gw_partial_m'] and odd['gw_kpad'] and odd['idle'] and (odd['unused_rows'], odd['unused_cols']) == (0, 0)
    assert (one['ktot'], one['chunks'], one['xw'], one['ow'], one['gx_xw']) == (3, 1, 64, 64, 64) and not one['partial_m'] and not one['ragged']
    assert (pixel['oh'], pixel['ow'], pixel['MT'], pixel['gw_br']) == (1, 1, 1, 1) and pixel['gw_kpad'] and pixel['idle']
    assert three['NT'] == 3 and three['partial_n'] and three['gw_MT'] == 3 and three['gx_kpad']
    assert four['NT'] == 4 and four['gw_MT'] == 4 and four['gx_ktot'] == 256 and four['gx_bands'] == 2 and four['gw_bands'] == 2 and four['jobs'] == 20
    assert apart['gx_dilated'] and apart['NT'] == 2 and apart['gx_bands'] == 2 and (apart['unused_rows'], apart['unused_cols']) == (0, 0)
    assert (full['ktot'], full['chunks'], full['gw_NT'], full['gw_groups'], full['gw_idle_waves']) == (512, 16, 32, 4, 0) and (full['unused_rows'], full['unused_cols']) == (2, 2)
    # kernel < stride: grad_x runs over a dilated g whose taps leave pixels between the windows untouched; every one of them is one
    # band, one padded chunk forward and a partial M- and N-tile, so what differs is the stride, the gaps and K
    for c, p in zip(fc.GAP_CASES, (gap1, gap2, gap3, gap4)):
        ci, h, w, co, k, s = c
        assert k < s and p['gx_dilated'] and p['kpad'] and p['gx_kpad'] and p['partial_m'] and p['partial_n'] and p['gx_partial_m'] and p['gx_partial_n']
        assert (p['bands'], p['gx_bands'], p['gw_bands'], p['chunks']) == (1, 1, 1, 1) and p['xw'] == (p['ow'] - 1) * s + k <= w
        reached = np.zeros((h, w), bool)                              # from the windows themselves
        for oy in range(p['oh']):
            for ox in range(p['ow']):
                reached[s * oy:s * oy + k, s * ox:s * ox + k] = True
        unreached, inside = fc.holes(h, w, k, s)
        assert np.array_equal(unreached, ~reached) and inside.sum() > 0 and not (inside & reached).any()
        assert inside.sum() == (h - p['unused_rows']) * (w - p['unused_cols']) - reached.sum()
    assert [(int(fc.holes(c[1], c[2], c[4], c[5])[1].sum()), int(fc.holes(c[1], c[2], c[4], c[5])[0].sum())) for c in fc.GAP_CASES] == [(69, 69), (40, 82), (40, 87), (39, 66)]
    assert all(not fc.holes(c[1], c[2], c[4], c[5])[1].any() for c in fc.CASES[:9])        # k >= s: no pixel between two windows is skipped
    assert (gap1['oh'], gap1['ow'], gap1['ktot'], gap1['gx_ktot'], gap1['unused_rows'], gap1['unused_cols'], gap1['MT']) == (5, 6, 3, 5, 0, 0, 2)
    assert (gap2['oh'], gap2['ow'], gap2['ktot'], gap2['gx_ktot'], gap2['unused_rows'], gap2['unused_cols']) == (3, 4, 16, 24, 2, 2)
    assert (gap2['gw_NT'], gap2['gw_partial_n'], gap2['gw_kpad']) == (1, False, False)
    assert (gap3['oh'], gap3['ow'], gap3['ktot'], gap3['gx_ktot'], gap3['gx_chunks'], gap3['gw_NT'], gap3['unused_rows'], gap3['unused_cols']) == (3, 3, 18, 36, 2, 2, 1, 3)
    assert (gap4['oh'], gap4['ow'], gap4['ktot'], gap4['gx_ktot'], gap4['unused_rows'], gap4['unused_cols'], gap4['gw_kpad']) == (2, 3, 5, 3, 3, 0, True)
    assert {c[5] - c[4] for c in fc.GAP_CASES} == {1, 3} and {c[5] for c in fc.GAP_CASES} == {2, 3, 4} and {c[4] for c in fc.GAP_CASES} == {1, 2, 3}
    # together: one to four N-tiles forward, every instantiation of the partials' kernel, one and several bands with a short last
    # one in all three kernels, padded and whole K in all three, one to four workgroups per sample of partials
    assert {p['NT'] for p in P.values()} == {1, 2, 3, 4} and {p['gw_MT'] for p in P.values()} == {1, 2, 3, 4}
    assert {p['gw_groups'] for p in P.values()} == {1, 2, 3, 4} and {p['gx_NT'] for p in P.values()} == {1, 2}
    for pre in ('', 'gx_', 'gw_'):
        assert any(p[pre + 'bands'] > 1 and p[pre + 'last_rows'] < p[pre + 'br'] for p in P.values()) and any(p[pre + 'bands'] == 1 for p in P.values())
        assert {p[pre + 'kpad'] for p in P.values()} == {True, False}
    loop = fc.paths(*fc.LOOP_CASE, n=fc.LOOP_N)
    assert loop['items'] > loop['grid'] == fc.FC_MAX_GRID and loop['walks'] == 3 and loop['items'] % loop['grid'] != 0
    assert loop['gx_items'] > fc.FC_MAX_GRID and loop['gw_grid'] == fc.FC_MAX_GRID and loop['gw_walks'] == 3


def test_modules_refuse_on_the_host():
    import torch
    from red_gym_amd.featconv import FeatConv2d, Trunk, conv_feat
    nn = torch.nn
    layer = FeatConv2d(16, 32, 4, 2, relu=True)
    assert sorted(layer.state_dict()) == ['bias', 'weight'] and tuple(layer.weight.shape) == (32, 16, 4, 4)
    for args in ((33, 32, 3, 1), (32, 65, 2, 1), (32, 32, 5, 1), (32, 32, 3, 5), (32, 57, 3, 1), (0, 4, 1, 1)):
        with pytest.raises(ValueError):
            FeatConv2d(*args)
    conv = nn.Conv2d(32, 32, 3, 1)
    shared = FeatConv2d.from_conv(conv, relu=True)
    assert shared.weight is conv.weight and shared.bias is conv.bias and shared.relu and (shared.kernel_size, shared.stride) == (3, 1)
    for bad in (nn.Conv2d(32, 32, 3, 1, padding=1), nn.Conv2d(32, 32, 3, 1, dilation=2), nn.Conv2d(32, 32, 3, 1, groups=2), nn.Conv2d(32, 32, (3, 2), 1),
                nn.Conv2d(32, 32, 3, (1, 2)), nn.Conv2d(32, 32, 5, 1), nn.Conv2d(40, 32, 3, 1), nn.Linear(3, 3)):
        with pytest.raises(ValueError):
            FeatConv2d.from_conv(bad)
    trunk = Trunk(on=255.0, cols=256)
    assert list(trunk.state_dict()) == ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias', 'conv3.weight', 'conv3.bias']
    c1, c2, c3 = nn.Conv2d(1, 16, 8, 4), nn.Conv2d(16, 32, 4, 2), nn.Conv2d(32, 32, 3, 1)
    shared = Trunk.from_convs(c1, c2, c3, on=1.0, cols=256)
    assert shared.conv1.weight is c1.weight and shared.conv2.bias is c2.bias and shared.conv3.weight is c3.weight and shared.conv1.on == 1.0
    trunk.load_state_dict({n + '.' + k: v for n, c in (('conv1', c1), ('conv2', c2), ('conv3', c3)) for k, v in c.state_dict().items()})
    assert torch.equal(trunk.conv3.bias, c3.bias)
    for convs in ((nn.Conv2d(3, 16, 8, 4), c2, c3), (c1, nn.Conv2d(8, 32, 4, 2), c3), (c1, c2, nn.Conv2d(16, 32, 3, 1)), (c1, nn.Conv2d(16, 32, 4, 2, padding=1), c3),
                  (c1, c2, nn.Conv2d(32, 32, 3, 1, groups=4)), (c1, nn.Conv2d(16, 32, 5, 2), c3), (nn.Conv2d(1, 32, 8, 4), nn.Conv2d(32, 32, 4, 2), c3)):
        with pytest.raises(ValueError):
            Trunk.from_convs(*convs)
    x, w = torch.zeros(1, 32, 30, 30), torch.zeros(32, 32, 3, 3)
    with pytest.raises(ValueError):
        conv_feat(x, w)                                           # not on a GPU
    with pytest.raises(ValueError):
        conv_feat(x.numpy(), w)
