"""The checker of the fused policy stem (tests/bitconv2_cases.py) checked itself, and what needs no device: the exact fp32 fma
against rational arithmetic, forward2 against an fp64 convolution and a naive loop, f110_bitconv2_validate field by field, and
the kernel's banding arithmetic (paths2) on every case."""
from fractions import Fraction

import numpy as np
import pytest

import bitconv2_cases as b2
import bitconv_cases as bc


def _round32(q):
    """The fp32 nearest to the rational q (ties to even), q within fp32's normal range or 0."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = 0
    while q >= 2:
        q, e = q / 2, e + 1
    while q < 1:
        q, e = q * 2, e - 1
    assert -126 <= e <= 127
    scaled = q * 2 ** 23
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    return np.float32(sign * float(Fraction(m) * Fraction(2) ** (e - 23)))


def _triples(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    c = (rng.normal(size=n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    q = n // 4
    c[:q] = -(a[:q] * b[:q])                                    # c = -fp32(a b): the result is the product's rounding error
    c[q:2 * q] = -(a[q:2 * q] * b[q:2 * q]) * np.float32(1 + 2.0 ** -20)
    return a, b, c


def test_fma32_against_rational_arithmetic():
    a, b, c = _triples(4000, 1)
    got = b2.fma32(a, b, c)
    assert got.dtype == np.float32
    want = np.array([_round32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(bc.bit_patterns(got), bc.bit_patterns(want))
    assert (got[:1000] != 0).any() and (np.abs(got[:1000]) < np.abs(a[:1000] * b[:1000]) * 1e-6).all()   # (the cancelling ones cancelled)


def test_fma32_where_fp64_rounds_twice():
    """A constructed case where plain fp64 arithmetic rounds twice: a = b = 1 + 2^-12, so a b = 1 + 2^-11 + 2^-24 exactly, the
    midpoint of two neighbouring fp32; c = 2^-80 lifts the sum just above it, so the fma rounds up.  fp64 cannot hold 2^-80
    beside 1: its sum is the midpoint itself, and rounding that to fp32 ties to even, down."""
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)   # a b = 1 + 2^-11 + 2^-24: a midpoint of fp32 (24 bits after 1)
    c = np.float32(2.0 ** -80)                                       # pushes it just above the midpoint; fp64 cannot hold 2^-80 beside 1
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    right = _round32(exact)
    naive = np.float32(np.float64(a) * np.float64(b) + np.float64(c))            # fp64 sum = the midpoint, then ties to even
    got = b2.fma32(a, b, c)
    assert naive != right and got == right
    assert right == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and naive == np.float32(1 + 2.0 ** -11)
    # and the mirror image, just below the midpoint of an odd neighbour pair
    got, right = b2.fma32(a, b, -c), _round32(Fraction(float(a)) * Fraction(float(b)) - Fraction(float(c)))
    assert got == right == np.float32(1 + 2.0 ** -11)


def test_forward2_equals_a_naive_chain_and_lies_within_the_bound():
    rows, cols, k1, s1, c1, k2, s2, c2 = 12, 14, 3, 2, 3, 2, 1, 4
    imgs = b2.images2(rows, cols)
    w1, b1, w2, bb = b2.params2(k1, c1, k2, c2)
    out = b2.forward2(imgs, w1, b1, s1, 255.0, True, w2, bb, s2, False)
    a1 = bc.forward(imgs, w1, b1, s1, 255.0, True)
    oh2, ow2 = b2.out_size2(rows, cols, k1, s1, k2, s2)
    assert out.shape == (3, c2, oh2, ow2)
    for n in range(3):
        for co in range(c2):
            for oy in range(oh2):
                for ox in range(ow2):
                    acc = np.float32(0.0)
                    for ci in range(c1):
                        for ky in range(k2):
                            for kx in range(k2):
                                acc = b2.fma32(w2[co, ci, ky, kx], a1[n, ci, s2 * oy + ky, s2 * ox + kx], acc)
                    assert bc.bit_patterns(np.float32(acc + bb[co])) == bc.bit_patterns(out[n, co, oy, ox])
    assert (out < 0).any() and (out > 0).any()


@pytest.mark.parametrize('case', b2.CASES2[1:])
def test_forward2_within_the_bound_of_an_fp32_sum(case):
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    imgs = b2.images2(rows, cols)
    w1, b1, w2, bb = b2.params2(k1, c1, k2, c2)
    a1 = bc.forward(imgs, w1, b1, s1, 1.0, True)
    out = b2.finish2(b2.accumulate2(a1, w2, s2), bb, False)
    want, mag = b2.conv2_fp64(a1, w2, bb, s2)
    K = c1 * k2 * k2
    bound = bc.gamma(K + 1) * mag + np.abs(want) * bc.U
    assert (np.abs(out - want) <= bound).all() and (out[0] != out[2]).any()


@pytest.mark.parametrize('case', b2.CASES2 + [b2.LOOP_CASE])
def test_validate2_accepts_the_cases(case):
    from red_gym_amd import bitconv
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    cfg = bitconv.validate2(rows, cols, k1, s1, c1, k2, s2, c2)
    assert (cfg.kernel2, cfg.stride2, cfg.channels2, cfg.relu, cfg.relu2) == (k2, s2, c2, 1, 1)
    assert bitconv.output_size2(rows, cols, k1, s1, k2, s2) == b2.out_size2(rows, cols, k1, s1, k2, s2)
    assert b2.paths2(*case)['ow1'] <= b2.BC2_MAX_OW1


def test_validate2_refuses_one_field_at_a_time():
    from red_gym_amd import bitconv
    good = dict(rows=256, cols=256, kernel=8, stride=4, channels=16, kernel2=4, stride2=2, channels2=32, on=1.0)
    bitconv.validate2(**good)
    bad = [dict(kernel=0), dict(kernel=9), dict(stride=0), dict(stride=9), dict(channels=0), dict(channels=17), dict(rows=7), dict(cols=7),
           dict(rows=16385), dict(on=float('nan')), dict(on=float('inf')), dict(on=1e39),                    # the first layer's own
           dict(kernel2=0), dict(kernel2=5), dict(stride2=0), dict(stride2=5), dict(stride2=-1), dict(channels2=0), dict(channels2=65),
           dict(rows=16), dict(cols=16),                                                                      # OH1 / OW1 = 3 < kernel2
           dict(cols=264)]                                                                                    # OW1 = 65
    for change in bad:
        with pytest.raises(ValueError):
            bitconv.validate2(**dict(good, **change))
    bitconv.validate2(**dict(good, cols=260))                      # OW1 = 64
    bitconv.validate2(**dict(good, rows=16384))                    # any number of rows
    bitconv.validate2(**dict(good, rows=20, cols=20))              # OH1 = OW1 = 4 = kernel2
    bitconv.validate2(**dict(good, channels2=64, kernel2=1, stride2=1))


def test_every_case_selects_what_it_claims():
    P = {c: b2.paths2(*c) for c in b2.CASES2}
    sal, tall, low, odd, one, four, wide, three, mono, pixel, two = (P[c] for c in b2.CASES2)
    assert all(p['lds'] <= b2.BC2_LDS_BYTES and p['xw'] <= p['ow1'] <= 64 for p in P.values())
    assert (sal['oh2'], sal['ow2'], sal['br'], sal['bands'], sal['last_rows']) == (30, 30, 6, 5, 6)
    assert (sal['ktot'], sal['blocks'], sal['NT'], sal['mw'], sal['per'], sal['runs']) == (256, 4, 2, 2, 6, 1) and not sal['ragged']
    assert sal['vec'] and not sal['scalar'] and sal['straddles'] and sal['partial_m']
    assert (tall['ow1'], tall['oh1'], tall['bands'], tall['last_rows']) == (64, 17, 2, 1) and tall['scalar'] and tall['vec']
    assert (low['ow1'], low['oh2'], low['bands'], low['MT']) == (64, 1, 1, 2) and not low['idle']
    assert odd['unused_rows'] == 1 and odd['unused_cols'] == 1 and odd['kpad'] and odd['u8_bytes'] and odd['partial_m'] and odd['partial_n']
    assert (one['ktot'], one['ksteps'], one['ow2']) == (3, 1, 64) and one['kpad'] and not one['straddles']
    assert (four['NT'], four['mw']) == (2, 2) and four['partial_n'] and four['idle'] and four['unused_cols'] == 3
    assert (wide['NT'], wide['mw'], wide['runs']) == (4, 1, 2) and wide['ragged'] and not wide['partial_n']
    assert three['NT'] == 3 and three['reload'] and three['blocks'] == 3 and three['runs'] == 4
    assert (mono['ktot'], mono['ksteps']) == (4, 1) and not mono['kpad']
    assert (pixel['oh2'], pixel['ow2'], pixel['MT']) == (1, 1, 1) and not pixel['vec']
    assert two['blocks'] == 2
    # together: every kernel size of the first layer, every block count of the multiply, every split of the waves, both
    # stores, one and several bands, a last band that is shorter, one and several runs of accumulators, idle waves
    assert {c[2] for c in b2.CASES2} == set(range(1, 9))
    assert {p['blocks'] for p in P.values()} == {1, 2, 3, 4} and {p['NT'] for p in P.values()} == {1, 2, 3, 4}
    assert {p['mw'] for p in P.values()} == {1, 2, 4}
    assert any(p['bands'] > 1 and p['last_rows'] < p['br'] for p in P.values()) and any(p['bands'] == 1 for p in P.values())
    loop = b2.paths2(*b2.LOOP_CASE, n=b2.LOOP_N)
    assert loop['items'] > loop['grid'] == b2.BC2_MAX_GRID and loop['walks'] == 3 and loop['items'] % loop['grid'] != 0
