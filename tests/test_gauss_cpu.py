"""No-GPU checks of the policy's Gaussian draws (csrc/f110_gauss.h): the Philox block function of csrc/f110_philox.h, compiled for the
host, against numpy.random.Philox's raw words; the checker of tests/gauss_cases.py against a plain Generator and its three base cases
against the minimums every test rests on; the host checks and the launch plan of csrc/f110_gauss_plan.h compiled for the host; the
library's own refusals before any launch; the mirrored state struct against the C compiler."""
import ctypes as C
import re

import numpy as np
import pytest

import gauss_cases as gc
import host_build

M64 = 2 ** 64 - 1
# (key, counter): high bits set in every word, t = 2^64 - 1, a counter word 0 that wraps, and the agent's plain case
PHILOX = [
    ((2025, 0), (0, 0, 0, 0)),
    ((2025, 2), (0, 15, 4095, 2 ** 40 + 3)),
    ((0x8000000000000001, 0xC000000000000003), (0x8000000000000000, 0x8000000000000010, 0xFFFFFFFF00000000, M64)),
    ((M64, M64), (M64 - 1, M64, M64, M64)),
    ((0xDEADBEEFCAFEF00D, 0x8123456789ABCDEF), (0xF000000000000000, 0x800000000000001F, 2 ** 63 + 2 ** 33 + 5, M64)),
    ((1, 0x8000000000000000), (0xFFFFFFFF, 0xFFFFFFFF00000001, 2 ** 62, M64)),
]

SHIM = host_build.FAIL_SHIM + r'''
#include "f110_philox.h"
#include "f110_gauss_plan.h"
using namespace f110;
typedef long long ll;
typedef unsigned long long ull;
// blocks b = 1 .. n of counter [c0 + b, c1, c2, c3] (mod 2^64 in word 0 alone, with the carry NumPy gives it), four words each
extern "C" void shim_philox(const ull *key, const ull *counter, int blocks, ull *out)
{
    uint64_t k[2] = {key[0], key[1]}, c[4] = {counter[0], counter[1], counter[2], counter[3]}, w[4];
    for (int b = 0; b < blocks; b++) {
        if (++c[0] == 0 && ++c[1] == 0 && ++c[2] == 0) ++c[3];
        philox4x64_10(c, k, w);
        for (int i = 0; i < 4; i++) out[4 * b + i] = w[i];
    }
}
extern "C" void shim_mulhilo(ull a, ull b, ull *out) { uint64_t hi, lo; philox_mulhilo(a, b, hi, lo); out[0] = hi; out[1] = lo; }
extern "C" ll shim_constant(int which)
{
    const ll v[] = {GS_THREADS, GS_MAX_BLOCKS, GS_MAX_ELEMENTS, (ll)sizeof(f110_gauss_state), F110_GAUSS_STREAMS, F110_GAUSS_MAX_COLUMNS};
    return v[which];
}
extern "C" int shim_check(int by_state, ll state, int stream, ll n, int A, ll rows, ll out)
{
    if (int rc = gauss_check("check", by_state != 0, (const f110_gauss_state *)(uintptr_t)state, stream, n, A, (const float *)(uintptr_t)out)) return rc;
    return gauss_rows_check("check", (const int64_t *)(uintptr_t)rows);
}
// o: grid x, y, z, block, lds, inst, total, A, vec
extern "C" void shim_plan(ll n, int A, ll out, ll *o)
{
    const GaussPlan p = gauss_plan(n, A, (const float *)(uintptr_t)out);
    o[0] = p.l.gx; o[1] = p.l.gy; o[2] = p.l.gz; o[3] = p.l.block; o[4] = (ll)p.l.lds; o[5] = p.l.inst; o[6] = p.a.total; o[7] = p.a.A; o[8] = p.a.vec;
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('gauss'), 'gauss', SHIM)
    u64p = C.POINTER(C.c_uint64)
    L.shim_philox.argtypes, L.shim_philox.restype = [u64p, u64p, C.c_int, u64p], None
    L.shim_mulhilo.argtypes, L.shim_mulhilo.restype = [C.c_uint64, C.c_uint64, u64p], None
    L.shim_constant.restype = C.c_longlong
    L.shim_message.restype = C.c_char_p
    L.shim_check.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_longlong]
    L.shim_plan.argtypes, L.shim_plan.restype = [C.c_longlong, C.c_int, C.c_longlong, C.POINTER(C.c_longlong)], None
    return L


@pytest.mark.parametrize('case', range(len(PHILOX)))
def test_host_philox_block_is_numpys(shim, case):
    """random_raw(8) of Philox(key, counter): the blocks of counter + 1 and counter + 2, not of counter itself."""
    key, counter = PHILOX[case]
    want = np.random.Philox(key=np.array(key, np.uint64), counter=np.array(counter, np.uint64)).random_raw(8)
    k, c, out = (C.c_uint64 * 2)(*key), (C.c_uint64 * 4)(*counter), (C.c_uint64 * 8)()
    shim.shim_philox(k, c, 2, out)
    assert [int(v) for v in out] == [int(v) for v in want], (key, counter)
    if 0 < counter[0] < M64:    # without the increment the words are others: the offset is part of the contract
        c0 = (C.c_uint64 * 4)((counter[0] - 1) % 2 ** 64, *counter[1:])
        shim.shim_philox(k, c0, 1, out)
        assert [int(v) for v in out[:4]] != [int(v) for v in want[:4]]


def test_host_mulhilo_is_the_128_bit_product(shim):
    rng = np.random.default_rng(7)
    values = [0, 1, M64, 2 ** 63, 2 ** 32 - 1, 2 ** 32, 0xD2E7470EE14C6C93, 0xCA5A826395121157] + [int(v) for v in rng.integers(0, 2 ** 64, 24, dtype=np.uint64)]
    out = (C.c_uint64 * 2)()
    for a in values:
        for b in values:
            shim.shim_mulhilo(a, b, out)
            assert (int(out[0]) << 64) | int(out[1]) == a * b, (a, b)


def test_checker_is_a_plain_generator():
    """gauss_cases.draws element by element == Generator(Philox(key, counter)).standard_normal(1) cast to fp32."""
    rows = [0, 1, 4095, 2 ** 33 + 5, 2 ** 62, M64]
    for seed, stream, t in gc.BASE + [(M64, 3, M64)]:
        got = gc.draws(seed, stream, t, rows, 5)
        assert got.dtype == np.float32 and got.shape == (len(rows), 5)
        for i, r in enumerate(rows):
            for j in range(5):
                bg = np.random.Philox(key=np.array([seed, stream], np.uint64), counter=np.array([0, j, r, t], np.uint64))
                x = np.random.Generator(bg).standard_normal(1)
                assert got[i, j].view(np.uint32) == x.astype(np.float32)[0].view(np.uint32), (seed, stream, t, r, j)
    # a count is rows 0 .. n-1, and a row's draws do not depend on the rows around it
    assert np.array_equal(gc.draws(2025, 0, 0, 3, 5).view(np.uint32), gc.draws(2025, 0, 0, [0, 1, 2], 5).view(np.uint32))
    assert np.array_equal(gc.draws(2025, 0, 0, [2], 5).view(np.uint32), gc.draws(2025, 0, 0, 3, 5).view(np.uint32)[2:])


# what NumPy 2.2.6 gave for the three base cases; the minimums are what the tests need, the counts are these
CENSUS = {(2025, 0, 0): (1009, 4, 12), (2025, 1, 0): (975, 6, 12), (2025, 2, 2 ** 40 + 3): (1027, 3, 24)}


@pytest.mark.parametrize('case', gc.BASE)
def test_base_cases_meet_the_minimums(case):
    census = gc.census(*case)
    print('case %s: %d elements of more than one word, %d of five or more, %d tail draws' % ((case,) + census))
    gc.require(*case)
    assert (gc.MIN_MULTI, gc.MIN_SECOND_BLOCK, gc.MIN_TAIL) == (500, 2, 5)
    assert census == CENSUS[case]
    w = gc.words_used(*case, gc.BASE_ROWS, gc.BASE_A)
    assert w.min() == 1 and w.shape == (gc.BASE_ROWS, gc.BASE_A)
    assert 0.98 < (w == 1).mean() < 0.99        # the header's "98.5 % take one word"


OUT, STATE, ROWS = 4096 * 100, 4096 * 200, 4096 * 300
# (by_state, state, stream, n, A, rows, out) -> the word the message names the culprit with
REFUSED = [
    ((1, 0, 0, 4, 16, 0, OUT), 'null state'),
    ((1, STATE + 4, 0, 4, 16, 0, OUT), 'state is not 8-byte aligned'),
    ((1, STATE, 0, 4, 16, 0, 0), 'null out'),
    ((0, 0, 0, 4, 16, 0, 0), 'null out'),
    ((1, STATE, 0, 4, 16, 0, OUT + 2), 'out is not 4-byte aligned'),
    ((0, 0, 0, 4, 16, 0, OUT + 1), 'out is not 4-byte aligned'),
    ((1, STATE, -1, 4, 16, 0, OUT), 'stream -1'),
    ((1, STATE, 4, 4, 16, 0, OUT), 'stream 4'),
    ((0, 0, 4, 4, 16, 0, OUT), 'stream 4'),
    ((1, STATE, 0, 0, 16, 0, OUT), 'n=0'),
    ((0, 0, 0, -1, 16, 0, OUT), 'n=-1'),
    ((1, STATE, 0, 4, 0, 0, OUT), 'A=0'),
    ((0, 0, 0, 4, -3, 0, OUT), 'A=-3'),
    ((1, STATE, 0, 4, 33, 0, OUT), 'A=33'),
    ((1, STATE, 0, 2 ** 27 + 1, 16, 0, OUT), 'n * A'),
    ((0, 0, 0, 2 ** 31 + 1, 1, 0, OUT), 'n * A'),
    ((0, 0, 0, 2 ** 62, 32, 0, OUT), 'n * A'),
    ((1, STATE, 0, 4, 16, ROWS + 4, OUT), 'rows is not 8-byte aligned'),
]
ACCEPTED = [(1, STATE, 3, 1, 1, 0, OUT + 4), (0, 0, 0, 2 ** 27, 16, ROWS, OUT), (0, 0, 0, 2 ** 31, 1, 0, OUT), (1, STATE + 8, 0, 2 ** 26, 32, ROWS + 8, OUT + 12)]


def test_plan_header_refuses_and_plans(shim):
    from red_gym_amd import _lib
    assert [shim.shim_constant(k) for k in range(6)] == [gc.GS_THREADS, gc.GS_MAX_BLOCKS, 2 ** 31, 64, _lib.F110_GAUSS_STREAMS, _lib.F110_GAUSS_MAX_COLUMNS]
    for args, word in REFUSED:
        assert shim.shim_check(*args) == _lib.E_INVALID, args
        assert word.encode() in shim.shim_message(), (args, shim.shim_message())
    for args in ACCEPTED:
        assert shim.shim_check(*args) == 0, (args, shim.shim_message())
    per_pass = gc.GS_THREADS * gc.GS_MAX_BLOCKS
    for n, A in gc.SHAPES + [(4096, 16), (per_pass // 16, 16), (per_pass // 16 + 1, 16), (2 ** 27, 16), (2 ** 31, 1)]:
        for off in (0, 4, 8, 12, 16):
            o = (C.c_longlong * 9)()
            shim.shim_plan(n, A, OUT + off, o)
            blocks = min(-(-n * A // gc.GS_THREADS), gc.GS_MAX_BLOCKS)
            assert list(o) == [blocks, 1, 1, gc.GS_THREADS, 0, 0, n * A, A, int(off % 16 == 0)], (n, A, off)


def test_library_refuses_before_any_launch():
    """The shipped entry points, without a device: every refusal above arrives before the runtime is asked anything."""
    from red_gym_amd import _lib
    lib = _lib.load()
    for (by_state, state, stream, n, A, rows, out), word in REFUSED:
        if by_state:
            rc = lib.f110_gauss_fill(state or None, stream, n, A, rows or None, out or None, 1, None)
        else:
            rc = lib.f110_gauss_fill_at(2025, stream, 0, n, A, rows or None, out or None, None)
        assert rc == _lib.E_INVALID, (by_state, state, stream, n, A, rows, out)
        assert word.encode() in lib.f110_last_error(), lib.f110_last_error()
    assert lib.f110_gauss_state_bytes() == 64 == C.sizeof(_lib.GaussState)
    with pytest.raises(ValueError, match='null state'):
        _lib.check(lib.f110_gauss_fill(None, 0, 4, 16, None, OUT, 0, None))
    with pytest.raises(ValueError, match='no CPU path'):
        from red_gym_amd.gauss import GaussianSource
        GaussianSource(0, device='cpu')


def test_mirrored_struct_against_the_compiler(tmp_path):
    """_lib.GAUSS_STRUCTS (a tagged typedef, which the flat mirror's reader passes over): size and every offset as strict C99 sees
    them, the field names, order and array lengths as the header spells them, and the fresh state's words."""
    from red_gym_amd import _lib
    from red_gym_amd.gauss import STATE_BYTES, fresh_state_words
    assert list(_lib.GAUSS_STRUCTS) == ['f110_gauss_state']
    cls = _lib.GaussState
    fields = [f for f, _ in cls._fields_]
    assert fields == ['seed', 'calls', 'reserved']
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "f110_hip.h"', 'int main(void)', '{',
             '    printf("size %d\\n", (int)sizeof(f110_gauss_state));',
             '    printf("streams %d\\n", (int)(sizeof(((f110_gauss_state *)0)->calls) / sizeof(uint64_t)));']
    lines += ['    printf("%s %%d\\n", (int)offsetof(f110_gauss_state, %s));' % (f, f) for f in fields]
    got = dict(line.split() for line in host_build.run_c(tmp_path, 'layout', '\n'.join(lines + ['    return 0;', '}', ''])).splitlines())
    assert int(got['size']) == C.sizeof(cls) == STATE_BYTES == 64 and int(got['streams']) == _lib.F110_GAUSS_STREAMS == 4
    for f in fields:
        assert int(got[f]) == getattr(cls, f).offset, f
    text = re.sub(r'/\*.*?\*/', ' ', open(host_build.ROOT + '/include/f110_hip.h').read(), flags=re.S)
    body = re.search(r'typedef struct f110_gauss_state\s*\{(.*?)\}\s*f110_gauss_state\s*;', text, flags=re.S).group(1)
    assert re.findall(r'uint64_t\s+(\w+)(?:\[(\w+)\])?\s*;', body) == [('seed', ''), ('calls', 'F110_GAUSS_STREAMS'), ('reserved', '3')]
    assert fresh_state_words(2025) == [2025, 0, 0, 0, 0, 0, 0, 0]
    assert fresh_state_words(M64, (1, 2 ** 40 + 3, 2 ** 63, M64)) == [-1, 1, 2 ** 40 + 3, -2 ** 63, -1, 0, 0, 0]
