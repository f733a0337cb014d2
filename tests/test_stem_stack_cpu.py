"""The stacked fused stem without a device: bitconv2_forward_stack_plan (csrc/f110_bitconv_plan.h) compiled for the host -- against the
one-frame plan at stack = 1 on every case of bitconv2_cases.CASES2, and the properties every launch must have on the whole valid
configuration space times stack 1 .. 8 -- and the checker of tests/stem_stack_cases.py against fp64."""
import ctypes

import numpy as np
import pytest

import bitconv2_cases as b2
import bitconv_cases as bc
import host_build
import stack_cases as sc
import stem_stack_cases as ss

KEYS = 'br bands nr1 koff_off a1_off xw ktot ksteps oh2 ow2 lds items grid block inst u8 stack index_null l1_index_null n'.split()

SHIM = r'''
#include "f110_bitconv_plan.h"
using namespace f110;
typedef long long ll;

static f110_bitconv2_config cfg_of(const int *s)
{
    f110_bitconv2_config c = {};
    c.rows = s[0]; c.cols = s[1]; c.kernel = s[2]; c.stride = s[3]; c.channels = s[4]; c.on = 1.0f; c.kernel2 = s[5]; c.stride2 = s[6]; c.channels2 = s[7];
    return c;
}

static void flat(const Bitconv2Args &a, const Launch &l, int stack, bool index_null, ll *o)
{
    const ll v[] = {a.BR, a.bands, a.NR1, a.koff_off, a.a1_off, a.XW, a.ktot, a.ksteps, a.OH2, a.OW2, (ll)l.lds, a.items, l.gx, l.block, l.inst, a.u8,
                    stack, index_null, a.l1.index == nullptr, a.l1.n};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
}

// s: (rows, cols, k1, s1, C1, k2, s2, C2); stack = 0: the one-frame plan
extern "C" int shim_stem_plan(const int *s, int stack, ll n, ll *o)
{
    const f110_bitconv2_config c = cfg_of(s);
    if (int rc = bitconv2_check(&c, "shim")) return rc;
    if (stack == 0) {
        const Bitconv2Plan p = bitconv2_forward_plan(c, false, n);
        flat(p.a, p.l, 0, true, o);
        return p.l.gy == 1 && p.l.gz == 1 ? 0 : 100;
    }
    if (int rc = bitconv_stack_check(stack, "shim")) return 10 * rc;
    const Bitconv2StackPlan p = bitconv2_forward_stack_plan(c, stack, n);
    flat(p.s.a, p.l, p.s.stack, p.s.index == nullptr, o);
    return p.l.gy == 1 && p.l.gz == 1 ? 0 : 100;
}

// The valid configuration space of shim_sweep_bitconv2 (tests/test_launch_plans_cpu.py) x stack 1 .. F110_BITCONV_MAX_STACK, at n = 1 and at
// n above the cap.  out: [0] plans checked, [1] offenders, [2] the most LDS bytes, [3] the most a band of one row needs, [4] which
// property the first offender breaks (1 LDS, 2 BR, 3 the bands' cover, 4 grid, 5 a valid stack refused, 6 differs from the one-frame
// plan), [5..] its configuration, stack and n
extern "C" void shim_sweep_stem_stack(ll *out)
{
    for (int i = 0; i < 16; i++) out[i] = 0;
    const ll ns[] = {1, 2 * BC2_MAX_GRID + 5};
    for (int k = 1; k <= BC_MAX_K; k++) for (int s = 1; s <= k; s++) for (int c1 = 1; c1 <= BC2_MAX_C1; c1++)
        for (int k2 = 1; k2 <= BC2_MAX_K2; k2++) for (int s2 = 1; s2 <= k2; s2++) for (int ow1 : {k2, 63, 64}) for (int oh1 : {k2, 64}) {
            const int cfg[] = {(oh1 - 1) * s + k, (ow1 - 1) * s + k, k, s, c1, k2, s2, 32};
            const f110_bitconv2_config c = cfg_of(cfg);
            if (bitconv2_check(&c, "sweep")) continue;
            for (int stack = 1; stack <= F110_BITCONV_MAX_STACK; stack++) for (ll n : ns) {
                int why = 0;
                if (bitconv_stack_check(stack, "sweep")) why = 5;
                else {
                    const Bitconv2StackPlan p = bitconv2_forward_stack_plan(c, stack, n);
                    const Bitconv2Plan one = bitconv2_forward_plan(c, false, n);
                    const Bitconv2Args &a = p.s.a;
                    const size_t least = bitconv2_lds(c, 1, a.XW, a.ksteps, nullptr, nullptr);
                    if ((ll)p.l.lds > out[2]) out[2] = (ll)p.l.lds;
                    if ((ll)least > out[3]) out[3] = (ll)least;
                    if (p.l.lds > (size_t)BC2_LDS_BYTES || p.l.lds != bitconv2_lds(c, a.BR, a.XW, a.ksteps, nullptr, nullptr)) why = 1;
                    else if (a.BR < 1) why = 2;
                    else if (!((ll)a.bands * a.BR >= a.OH2 && a.OH2 > (ll)(a.bands - 1) * a.BR)) why = 3;
                    else if (p.l.gx < 1 || p.l.gx > (unsigned)BC2_MAX_GRID || p.l.block != (unsigned)BC_THREADS || a.items != n * a.bands) why = 4;
                    else if (a.BR != one.a.BR || a.bands != one.a.bands || p.l.lds != one.l.lds || p.l.gx != one.l.gx || p.s.stack != stack) why = 6;
                }
                out[0]++;
                if (why && !out[1]++) { out[4] = why; for (int i = 0; i < 8; i++) out[5 + i] = cfg[i]; out[13] = stack; out[14] = n; }
            }
        }
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('stem_stack'), 'stemstack', host_build.FAIL_SHIM + SHIM)
    ip, lp, ll = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong), ctypes.c_longlong
    L.shim_stem_plan.argtypes = [ip, ctypes.c_int, ll, lp]
    L.shim_sweep_stem_stack.argtypes, L.shim_sweep_stem_stack.restype = [lp], None
    return L


def plan(L, case, stack, n):
    s = (ctypes.c_int * 8)(*case)
    out = (ctypes.c_longlong * len(KEYS))()
    rc = L.shim_stem_plan(s, stack, n, out)
    return rc, dict(zip(KEYS, out))


@pytest.mark.parametrize('case', b2.CASES2 + [b2.LOOP_CASE])
def test_plan_at_stack_one_is_the_one_frame_plan(lib, case):
    """BR, bands, items, grid and LDS bytes (and the offsets in it) of the new plan at stack = 1 are the one-frame plan's, which
    paths2 restates; the args carry the stack, leave both index pointers to the entry point and read packed frames."""
    for n in (3, b2.LOOP_N):
        rc1, one = plan(lib, case, 0, n)
        rcs, new = plan(lib, case, 1, n)
        assert rc1 == 0 and rcs == 0
        same = 'br bands nr1 koff_off a1_off xw ktot ksteps oh2 ow2 lds items grid block inst u8 n'.split()
        assert {k: new[k] for k in same} == {k: one[k] for k in same}, case
        w = b2.paths2(*case, n=n)
        assert (new['br'], new['bands'], new['items'], new['grid'], new['lds']) == (w['br'], w['bands'], w['items'], w['grid'], w['lds']), case
        assert (new['stack'], new['index_null'], new['l1_index_null'], new['u8'], new['n']) == (1, 1, 1, 0, n)


def test_plan_does_not_depend_on_the_stack(lib):
    """The running sums live in a1: SAL's shape keeps BR = 6 and five bands at every stack; stacks outside 1 .. 8 are refused."""
    for stack in range(1, sc.MAX_STACK + 1):
        rc, p = plan(lib, b2.SAL, stack, 64)
        assert rc == 0 and (p['br'], p['bands'], p['items'], p['stack']) == (6, 5, 320, stack) and p['lds'] <= b2.BC2_LDS_BYTES
    for stack in (-1, sc.MAX_STACK + 1, 1 << 20):
        assert plan(lib, b2.SAL, stack, 64)[0] == -10
    assert plan(lib, (256, 264, 8, 4, 16, 4, 2, 32), 2, 64)[0] == -1               # OW1 = 65: what f110_bitconv2_validate refuses


def test_plan_limits_on_every_valid_configuration(lib):
    """Every (kernel, stride, channels <= 16, kernel2, stride2) at first-layer outputs of {kernel2, 63, 64} columns and {kernel2, 64}
    rows, times stack 1 .. 8, at n = 1 and above the grid's cap: LDS <= BC2_LDS_BYTES, BR >= 1, bands BR >= OH2 > (bands - 1) BR, grid
    <= BC2_MAX_GRID, nothing valid refused, and the one-frame plan's geometry throughout."""
    out = (ctypes.c_longlong * 16)()
    lib.shim_sweep_stem_stack(out)
    o = list(out)
    print('%d plans, most LDS bytes %d, a band of one row needs at most %d' % (o[0], o[2], o[3]))
    assert o[1] == 0, '%d offenders; the first breaks property %d: configuration %s, stack %d, n %d' % (o[1], o[4], o[5:13], o[13], o[14])
    assert o[0] == 36 * 16 * 10 * 3 * 2 * 2 * sc.MAX_STACK and o[2] <= b2.BC2_LDS_BYTES and o[3] < 20 * 1024


@pytest.mark.parametrize('case', [c for c in ss.STACK_CASES if c != ss.SAL] + [b2.LOOP_CASE])
def test_checker_against_fp64(case):
    """stack = 3.  (a) Layer 2 alone, on the checker's own a1: within bitconv2_cases' bound of an fp32 sum, gamma(K + 1) sum |w2 a1| +
    |ref| u (test_bitconv2_cpu.py).  (b) The whole stem against F.conv2d in fp64 on the unpacked stack, relu, F.conv2d in fp64: layer
    1 of the checker lies within e1 = gamma(k k1^2 + 2) (|on| sum |w1| + |b1|) of the fp64 one (test_stack_cpu.py; the relu does not
    widen it), which reaches an output through at most sum |w2| e1, so the bound is (a)'s, taken on the fp64 a1 widened by e1, plus
    that."""
    import torch
    rows, cols, k1, s1, c1, k2, s2, c2 = case
    k = 3
    imgs = ss.frames_pool(rows, cols)
    index = sc.stack_index(3, k, len(imgs))
    w1, b1, w2, bb = ss.params_stem_stack(k1, c1, k, k2, c2)
    K = c1 * k2 * k2
    for on in (1.0, 255.0):
        a1 = sc.forward_stack(imgs, index, w1, b1, s1, on, True)
        got = b2.finish2(b2.accumulate2(a1, w2, s2), bb, False)
        assert got.dtype == np.float32 and np.array_equal(bc.bit_patterns(got), bc.bit_patterns(ss.forward_stem_stack(imgs, index, w1, b1, s1, on, True, w2, bb, s2, False)))
        want, mag = b2.conv2_fp64(a1, w2, bb, s2)
        assert (np.abs(got - want) <= bc.gamma(K + 1) * mag + np.abs(want) * bc.U).all()
        on32 = float(np.float32(on))
        x = torch.as_tensor((sc.unpacked_stack(imgs, index) == 255).astype(np.float64))
        a64 = torch.relu(torch.nn.functional.conv2d(x * on32, torch.as_tensor(w1.astype(np.float64)), torch.as_tensor(b1.astype(np.float64)), stride=s1))
        ref = torch.nn.functional.conv2d(a64, torch.as_tensor(w2.astype(np.float64)), torch.as_tensor(bb.astype(np.float64)), stride=s2).numpy()
        e1 = bc.gamma(k * k1 * k1 + 2) * (abs(on32) * np.abs(w1.astype(np.float64)).sum(axis=(1, 2, 3)) + np.abs(b1.astype(np.float64)))
        assert (np.abs(a1.astype(np.float64) - a64.numpy()) <= e1[None, :, None, None]).all()
        _, mag64 = b2.conv2_fp64(a64.numpy() + e1[None, :, None, None], w2, bb, s2)
        through = (np.abs(w2.astype(np.float64)).sum(axis=(2, 3)) * e1[None, :]).sum(axis=1)
        bound = bc.gamma(K + 1) * mag64 + np.abs(ref) * bc.U + through[None, :, None, None]
        err = np.abs(got.astype(np.float64) - ref)
        print(case, on, 'worst error / bound %.4f' % float((err / bound).max()))
        assert got.shape == ref.shape and (err <= bound).all() and (got[0] != got[1]).any()


def test_the_order_of_the_frames_is_part_of_the_checker():
    """Reversing the index's columns changes bits; permuting w1's j axis alike restores them; stack = 1 is the one-frame checker."""
    rows, cols, k1, s1, c1, k2, s2, c2 = ss.ODD
    imgs = ss.frames_pool(rows, cols)
    w1, b1, w2, bb = ss.params_stem_stack(k1, c1, 3, k2, c2)
    index = sc.stack_index(3, 3, len(imgs))
    base = ss.forward_stem_stack(imgs, index, w1, b1, s1, 1.0, True, w2, bb, s2, True)
    turned = ss.forward_stem_stack(imgs, index[:, ::-1], w1, b1, s1, 1.0, True, w2, bb, s2, True)
    both = ss.forward_stem_stack(imgs, index[:, ::-1], w1[:, ::-1], b1, s1, 1.0, True, w2, bb, s2, True)
    assert (bc.bit_patterns(base) != bc.bit_patterns(turned)).any()
    assert (np.abs(base - both) <= 1e-3 * np.abs(base).max()).all()          # the same sum in another order: close, and not asked to be equal
    one = ss.forward_stem_stack(imgs, index[:, :1], w1[:, :1], b1, s1, 255.0, True, w2, bb, s2, False)
    assert np.array_equal(bc.bit_patterns(one), bc.bit_patterns(b2.forward2(bc.pick(imgs, index[:, 0]), w1[:, :1], b1, s1, 255.0, True, w2, bb, s2, False)))
