"""The launch plans of the policy kernels (red_gym_amd/csrc/f110_{bitconv,policyhead,qhead,featconv}_plan.h) on the CPU: the four
headers and a small extern "C" shim are compiled for the host and loaded with ctypes, as tests/test_scan_plan_cpu.py does for the
scan.  paths() / paths2() of tests/*_cases.py restate the host arithmetic independently, and the coverage proofs of the small GPU
shape tables (test_shape_tables_reach_every_path and its siblings) rest on them: here every constant the cases files type again
and every number both sides define is compared with what the library's own C++ computes -- on the GPU tables, on a seeded sample
of what the compiled checks accept, and, for the properties every launch must have, on every accepted configuration."""
import ctypes

import numpy as np
import pytest

import bitconv2_cases as b2
import bitconv_cases as bc
import featconv_cases as fc
import host_build
import policyhead_cases as ph
import qhead_cases as qh

CONSTANTS = ('REPLAY_MAX_DIM BC_THREADS BC_TX BC_TY BC_MAX_K BC_LROWS BC_LWORDS BC_CHUNK BC_MAX_PARTIALS BC_FORWARD_GROUP '
             'BC2_MAX_K2 BC2_MAX_C1 BC2_MAX_C2 BC2_MAX_OW1 BC2_KSTEPS BC2_ACCS BC2_LDS_BYTES BC2_MAX_GRID '
             'PH_THREADS PH_ROWS PH_MAX_K PH_MAX_A PH_MAX_ROWS PH_LDS_BYTES PH_MAX_GRID PH_PREFETCH PH_GH_ROWS PH_SLICE '
             'QH_THREADS QH_RPW QH_ROWS QH_BROWS QH_MAX_H QH_MAX_A QH_MAX_C QH_MAX_ROWS QH_LDS_BYTES QH_MAX_GRID QH_SLICE '
             'FC_MAX_K FC_MAX_S FC_MAX_CI FC_MAX_CO FC_MAX_KTOT FC_MAX_W FC_THREADS FC_CHUNK FC_ACCS FC_STAGE FC_ZERO_BYTES '
             'FC_LDS_BYTES FC_MAX_GRID FCW_TILES FCW_MAX_MT').split()

# the ints of a flattened plan, in the shim's order
BITCONV_KEYS = ('oh ow words tiles_x tiles_y fwd_block fwd_lds fwd_inst launches G chunks bwd_block bwd_inst reduce_blocks nw '
                'workspace').split()
BITCONV2_KEYS = 'oh1 ow1 oh2 ow2 xw ktot ksteps br bands nr1 koff_off a1_off lds items grid block inst u8'.split()
POLICYHEAD_KEYS = ('T kc chunks tiles slices lds grid block inst b_T b_kc b_chunks b_slices gpre_blocks gpre_inst gh_blocks '
                   'gh_kblocks gw_slices gw_kblocks gw_block reduce_blocks gpre_at partial_at workspace').split()
QHEAD_KEYS = ('hc chunks tiles slices lds grid block b_hc b_chunks btiles b_slices b_lds bgrid amax gw_slices gw_blocks C '
              'gw_amax reduce_blocks reduce_C partial_floats partial_at workspace').split()
FEATCONV_KEYS = ('oh ow ktot chunks xw br bands nr planes_off items lds grid block '
                 'gx_ktot gx_chunks gx_xw gx_br gx_bands gx_nr gx_planes_off gx_items gx_lds gx_grid gx_ph gx_pw gx_ms '
                 'gw_xw gw_ktot gw_NT gw_MT gw_br gw_bands gw_nr gw_gp gw_xs_at gw_lds gw_grid gw_groups gw_inst '
                 'reduce_blocks nw workspace').split()

SHIM = r'''
#include "f110_bitconv_plan.h"
#include "f110_policyhead_plan.h"
#include "f110_qhead_plan.h"
#include "f110_featconv_plan.h"
using namespace f110;
typedef long long ll;

#define C(x) {#x, (ll)x}
static const struct { const char *name; ll value; } constants[] = {@CONSTANTS@};
#undef C
extern "C" int shim_constant(const char *name, ll *out)
{
    for (const auto &c : constants) if (!strcmp(c.name, name)) { *out = c.value; return 1; }
    return 0;
}
extern "C" double shim_half_log_2pi() { return PH_HALF_LOG_2PI; }

static f110_bitconv_config bitconv_cfg(const int *s) { f110_bitconv_config c = {}; c.rows = s[0]; c.cols = s[1]; c.kernel = s[2]; c.stride = s[3]; c.channels = s[4]; c.on = 1.0f; return c; }
static f110_bitconv2_config bitconv2_cfg(const int *s)
{
    f110_bitconv2_config c = {};
    c.rows = s[0]; c.cols = s[1]; c.kernel = s[2]; c.stride = s[3]; c.channels = s[4]; c.on = 1.0f; c.kernel2 = s[5]; c.stride2 = s[6]; c.channels2 = s[7];
    return c;
}
static f110_policyhead_config policyhead_cfg(const int *s) { f110_policyhead_config c = {}; c.in_features = s[0]; c.action_dim = s[1]; c.out_fp64 = s[2]; return c; }
static f110_qhead_config qhead_cfg(const int *s) { f110_qhead_config c = {}; c.hidden = s[0]; c.action_dim = s[1]; c.critics = s[2]; c.ld = s[3]; return c; }
static f110_featconv_config featconv_cfg(const int *s) { f110_featconv_config c = {}; c.in_channels = s[0]; c.rows = s[1]; c.cols = s[2]; c.out_channels = s[3]; c.kernel = s[4]; c.stride = s[5]; return c; }

// s: (rows, cols, kernel, stride, channels); groups: (first, grid) of the forward launches, the first `cap` of them
extern "C" int shim_bitconv(const int *s, ll n, int u8, ll *groups, int cap, ll *o)
{
    const f110_bitconv_config c = bitconv_cfg(s);
    if (int rc = bitconv_check(&c, "shim")) return rc;
    const BitconvForwardPlan f = bitconv_forward_plan(c, u8 != 0, n);
    const BitconvBackwardPlan b = bitconv_backward_plan(c, n);
    const ll v[] = {f.a.OH, f.a.OW, f.a.W, f.a.tiles_x, f.a.tiles_y, f.l.block, (ll)f.l.lds, f.l.inst, (ll)f.groups.size(),
                    b.a.G, b.partials.gy, b.partials.block, b.partials.inst, b.reduce.gx, b.nw, bitconv_workspace_bytes(c, n)};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
    for (size_t i = 0; i < f.groups.size() && (int)i < cap; i++) { groups[2 * i] = f.groups[i].first; groups[2 * i + 1] = f.groups[i].grid; }
    // what the two plans must agree on, and what never varies
    return (b.partials.gx == (unsigned)b.a.G && b.a.OH == f.a.OH && b.a.OW == f.a.OW && b.a.tiles_x == f.a.tiles_x && b.a.tiles_y == f.a.tiles_y
            && f.l.gy == 1 && f.l.gz == 1 && b.partials.gz == 1 && b.partials.lds == 0 && b.reduce.lds == 0 && b.reduce.block == (unsigned)BC_THREADS) ? 0 : 100;
}

// s: (rows, cols, k1, s1, C1, k2, s2, C2)
extern "C" int shim_bitconv2(const int *s, ll n, int u8, ll *o)
{
    const f110_bitconv2_config c = bitconv2_cfg(s);
    if (int rc = bitconv2_check(&c, "shim")) return rc;
    const Bitconv2Plan p = bitconv2_forward_plan(c, u8 != 0, n);
    const Bitconv2Args &a = p.a;
    const ll v[] = {a.l1.OH, a.l1.OW, a.OH2, a.OW2, a.XW, a.ktot, a.ksteps, a.BR, a.bands, a.NR1, a.koff_off, a.a1_off, (ll)p.l.lds, a.items,
                    p.l.gx, p.l.block, p.l.inst, a.u8};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
    return p.l.gy == 1 && p.l.gz == 1 && a.l1.n == n ? 0 : 100;
}

// s: (K, A, out_fp64)
extern "C" int shim_policyhead(const int *s, ll n, ll *o)
{
    const f110_policyhead_config c = policyhead_cfg(s);
    if (int rc = policyhead_check(&c, "shim")) return rc;
    const PolicyheadForwardPlan f = policyhead_forward_plan(c, n);
    const PolicyheadBackwardPlan b = policyhead_backward_plan(c, n);
    const ll v[] = {f.a.T, f.a.kc, f.a.chunks, f.a.tiles, f.a.slices, (ll)f.l.lds, f.l.gx, f.l.block, f.l.inst,
                    b.a.T, b.a.kc, b.a.chunks, b.a.slices, b.gpre.gx, b.gpre.inst, b.gradh.gx, b.gradh.gy, b.gradw.gx, b.gradw.gy - 1, b.gradw.block,
                    b.reduce.gx, b.gpre_at, b.partial_at, policyhead_workspace_bytes(c, n)};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
    return f.l.gy == 1 && f.l.gz == 1 && b.gpre.lds + b.gradh.lds + b.gradw.lds + b.reduce.lds == 0 && b.gpre.block == (unsigned)PH_THREADS
           && b.gradh.block == (unsigned)PH_THREADS && b.reduce.block == (unsigned)PH_THREADS ? 0 : 100;
}

// s: (H, A, C, ld)
extern "C" int shim_qhead(const int *s, ll n, ll *o)
{
    const f110_qhead_config c = qhead_cfg(s);
    if (int rc = qhead_check(&c, "shim")) return rc;
    const QheadForwardPlan f = qhead_forward_plan(c, n);
    const QheadBackwardPlan b = qhead_backward_plan(c, n);
    const ll v[] = {f.a.hc, f.a.chunks, f.a.tiles, f.a.slices, (ll)f.l.lds, f.l.gx, f.l.block,
                    b.a.hc, b.a.chunks, b.a.tiles, b.a.slices, (ll)b.rows.lds, b.rows.gx, b.rows.inst, b.gradw.gx, b.gradw.gy, b.gradw.gz, b.gradw.inst,
                    b.reduce.gx, b.reduce.gy, (ll)qhead_partial_floats(c.hidden, c.action_dim), b.partial_at, qhead_workspace_bytes(c, n)};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
    return f.l.gy == 1 && f.l.gz == 1 && f.l.inst == 0 && b.rows.gy == 1 && b.rows.gz == 1 && b.gradw.lds + b.reduce.lds == 0
           && b.rows.block == (unsigned)QH_THREADS && b.gradw.block == (unsigned)QH_THREADS && b.reduce.block == (unsigned)QH_THREADS ? 0 : 100;
}

// s: (Ci, H, W, Co, k, s)
extern "C" int shim_featconv(const int *s, ll n, ll *o)
{
    const f110_featconv_config c = featconv_cfg(s);
    if (int rc = featconv_check(&c, "shim")) return rc;
    const FeatconvForwardPlan f = featconv_forward_plan(c, n);
    const FeatconvBackwardPlan b = featconv_backward_plan(c, n);
    const FeatconvGemm &g = f.a.g, &x = b.a.g;
    const FeatconvArgs &w = b.a;
    const ll v[] = {f.a.OH, f.a.OW, g.ktot, g.chunks, g.XW, g.BR, g.bands, g.NR, g.planes_off, g.items, (ll)f.l.lds, f.l.gx, f.l.block,
                    x.ktot, x.chunks, x.XW, x.BR, x.bands, x.NR, x.planes_off, x.items, (ll)b.gradx.lds, b.gradx.gx, x.PH, x.PW, x.ms,
                    w.wXW, w.wktot, w.wNT, w.wMT, w.wBR, w.wbands, w.wNR, w.wGP, w.xs_at, (ll)b.partials.lds, b.partials.gx, b.partials.gy, b.partials.inst,
                    b.reduce.gx, b.nw, featconv_workspace_bytes(c, n)};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); i++) o[i] = v[i];
    return f.l.gy == 1 && f.l.gz == 1 && f.l.inst == 0 && b.gradx.gy == 1 && b.gradx.block == (unsigned)FC_THREADS && b.partials.block == (unsigned)FC_THREADS
           && b.reduce.block == (unsigned)FC_THREADS && b.reduce.lds == 0 && g.PH == f.a.OH && g.PW == f.a.OW && g.ms == c.stride && f.a.n == n && w.n == n ? 0 : 100;
}

// ---------------------------------------------------------------- sweeps over everything a check accepts
// out: [0] configurations checked, [1] offenders, [2..4] the most LDS bytes per launch kind, [5..7] the most a band of one row
// would need (`least`: what the limits of the check have to keep inside the budget), [8] which property the first offender
// breaks, [9..] the first offender's configuration and n
struct Sweep {
    ll *o;
    Sweep(ll *out) : o(out) { for (int i = 0; i < 24; i++) o[i] = 0; }
    // one launch: dynamic LDS within `budget`; BR >= 1; (bands - 1) BR < rows <= bands BR; 1 <= grid <= cap
    int launch(int kind, size_t lds, size_t least, int budget, int br, int bands, int rows, unsigned grid, int cap)
    {
        if ((ll)lds > o[2 + kind]) o[2 + kind] = (ll)lds;
        if ((ll)least > o[5 + kind]) o[5 + kind] = (ll)least;
        if (lds > (size_t)budget) return 1 + 10 * kind;
        if (br < 1) return 2 + 10 * kind;
        if (!((ll)(bands - 1) * br < rows && rows <= (ll)bands * br)) return 3 + 10 * kind;
        if (grid < 1 || grid > (unsigned)cap) return 4 + 10 * kind;
        return 0;
    }
    // kc / hc: a positive multiple of 64 whose chunks cover `total`
    static int chunked(int per, int chunks, int total) { return per > 0 && per % 64 == 0 && (ll)(chunks - 1) * per < total && total <= (ll)chunks * per ? 0 : 5; }
    void done(int why, const int *s, int ns, ll n)
    {
        o[0]++;
        if (!why) return;
        if (!o[1]++) { o[8] = why; for (int i = 0; i < ns; i++) o[9 + i] = s[i]; o[9 + ns] = n; }
    }
};

extern "C" void shim_sweep_featconv(ll *out)
{
    Sweep sw(out);
    const ll ns[] = {1, 2 * FC_MAX_GRID + 5};
    for (int k = 1; k <= FC_MAX_K; k++) for (int s = 1; s <= FC_MAX_S; s++) for (int ci = 1; ci <= FC_MAX_CI; ci++) for (int co = 1; co <= FC_MAX_CO; co++)
        for (int cols : {k, 63, 64}) for (int rows : {k, 64}) {
            const int cfg[] = {ci, rows, cols, co, k, s};
            const f110_featconv_config c = featconv_cfg(cfg);
            if (featconv_check(&c, "sweep")) continue;
            for (ll n : ns) {
                const FeatconvForwardPlan f = featconv_forward_plan(c, n);
                const FeatconvBackwardPlan b = featconv_backward_plan(c, n);
                int why = sw.launch(0, f.l.lds, featconv_gemm_lds(f.a.g.chunks, ci, k, f.a.g.XW), FC_LDS_BYTES, f.a.g.BR, f.a.g.bands, f.a.OH, f.l.gx, FC_MAX_GRID);
                if (!why) why = sw.launch(1, b.gradx.lds, featconv_gemm_lds(b.a.g.chunks, co, k, b.a.g.XW), FC_LDS_BYTES, b.a.g.BR, b.a.g.bands, b.a.H, b.gradx.gx, FC_MAX_GRID);
                if (!why) why = sw.launch(2, b.partials.lds, featconv_gradw_gs(c, 1, b.a.OW) + (size_t)ci * k * b.a.wXW * sizeof(float), FC_LDS_BYTES, b.a.wBR, b.a.wbands, b.a.OH, b.partials.gx, FC_MAX_GRID);
                sw.done(why, cfg, 6, n);
            }
        }
}

extern "C" void shim_sweep_bitconv2(ll *out)
{
    Sweep sw(out);
    const ll ns[] = {1, 2 * BC2_MAX_GRID + 5};
    for (int k = 1; k <= BC_MAX_K; k++) for (int s = 1; s <= k; s++) for (int c1 = 1; c1 <= BC2_MAX_C1; c1++)
        for (int k2 = 1; k2 <= BC2_MAX_K2; k2++) for (int s2 = 1; s2 <= k2; s2++) for (int ow1 : {k2, 63, 64}) for (int oh1 : {k2, 64}) {
            const int cfg[] = {(oh1 - 1) * s + k, (ow1 - 1) * s + k, k, s, c1, k2, s2, 32};
            const f110_bitconv2_config c = bitconv2_cfg(cfg);
            if (bitconv2_check(&c, "sweep")) continue;
            for (ll n : ns) {
                const Bitconv2Plan p = bitconv2_forward_plan(c, false, n);
                sw.done(sw.launch(0, p.l.lds, bitconv2_lds(c, 1, p.a.XW, p.a.ksteps, nullptr, nullptr), BC2_LDS_BYTES, p.a.BR, p.a.bands, p.a.OH2, p.l.gx, BC2_MAX_GRID), cfg, 8, n);
            }
        }
}

extern "C" void shim_sweep_policyhead(ll *out)
{
    Sweep sw(out);
    const ll ns[] = {1, (2 * PH_MAX_GRID + 5) * (ll)PH_ROWS};
    for (int K = 0; K <= PH_MAX_K + 1; K++) for (int A = 0; A <= PH_MAX_A + 1; A++) {
        const int cfg[] = {K, A, A & 1};
        const f110_policyhead_config c = policyhead_cfg(cfg);
        if (policyhead_check(&c, "sweep")) continue;
        for (ll n : ns) {
            const PolicyheadForwardPlan f = policyhead_forward_plan(c, n);
            int why = sw.launch(0, f.l.lds, f.l.lds, PH_LDS_BYTES, 1, 1, 1, f.l.gx, PH_MAX_GRID);
            if (!why) why = Sweep::chunked(f.a.kc, f.a.chunks, K);
            sw.done(why, cfg, 3, n);
        }
    }
}

extern "C" void shim_sweep_qhead(ll *out)
{
    Sweep sw(out);
    const ll ns[] = {1, (2 * QH_MAX_GRID + 5) * (ll)QH_ROWS};
    for (int H = 0; H <= QH_MAX_H + 1; H++) for (int A = 0; A <= QH_MAX_A + 1; A++) {
        const int cfg[] = {H, A, 1 + (H & 1), A};
        const f110_qhead_config c = qhead_cfg(cfg);
        if (qhead_check(&c, "sweep")) continue;
        for (ll n : ns) {
            const QheadForwardPlan f = qhead_forward_plan(c, n);
            const QheadBackwardPlan b = qhead_backward_plan(c, n);
            int why = sw.launch(0, f.l.lds, f.l.lds, QH_LDS_BYTES, 1, 1, 1, f.l.gx, QH_MAX_GRID);
            if (!why) why = sw.launch(1, b.rows.lds, b.rows.lds, QH_LDS_BYTES, 1, 1, 1, b.rows.gx, QH_MAX_GRID);
            if (!why) why = Sweep::chunked(f.a.hc, f.a.chunks, H);
            if (!why) why = Sweep::chunked(b.a.hc, b.a.chunks, H);
            sw.done(why, cfg, 4, n);
        }
    }
}
'''


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    L = host_build.build_shim(tmp_path_factory.mktemp('launch_plans'), 'launchplans',
                              host_build.FAIL_SHIM + SHIM.replace('@CONSTANTS@', ', '.join('C(%s)' % c for c in CONSTANTS)))
    L.shim_message.restype = ctypes.c_char_p
    L.shim_half_log_2pi.restype = ctypes.c_double
    ip, lp, ll = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong), ctypes.c_longlong
    L.shim_constant.argtypes = [ctypes.c_char_p, lp]
    L.shim_bitconv.argtypes = [ip, ll, ctypes.c_int, lp, ctypes.c_int, lp]
    L.shim_bitconv2.argtypes = [ip, ll, ctypes.c_int, lp]
    for name in ('shim_policyhead', 'shim_qhead', 'shim_featconv'):
        getattr(L, name).argtypes = [ip, ll, lp]
    for name in ('shim_sweep_featconv', 'shim_sweep_bitconv2', 'shim_sweep_policyhead', 'shim_sweep_qhead'):
        getattr(L, name).argtypes, getattr(L, name).restype = [lp], None
    return L


@pytest.fixture(scope='module')
def hip():
    """The library itself, for the exported f110_*_workspace (host code: no GPU)."""
    from red_gym_amd import _lib
    return _lib, _lib.load()


def constant(L, name):
    v = ctypes.c_longlong()
    assert L.shim_constant(name.encode(), ctypes.byref(v)), name
    return v.value


def flat(fn, keys, shape, *args):
    """A compiled plan as a dict, or None where the compiled check refuses the configuration."""
    s = (ctypes.c_int * len(shape))(*shape)
    out = (ctypes.c_longlong * len(keys))()
    rc = fn(s, *args, out)
    assert rc in (0, -1), 'the plans of %r disagree among themselves' % (shape,)
    return dict(zip(keys, out)) if rc == 0 else None


def same(plan, want, must, inside, where):
    """Every key both sides define is ==; `must` are among them; paths() defines nothing else but `inside`, the keys that describe
    what happens inside a kernel and have no counterpart in a launch plan."""
    both = set(plan) & set(want)
    assert set(must) <= both and set(want) - set(plan) == set(inside), (sorted(set(must) - both), sorted(set(want) - set(plan) ^ set(inside)))
    bad = {k: (plan[k], want[k]) for k in sorted(both) if plan[k] != want[k]}
    assert not bad, (where, bad)


# ---------------------------------------------------------------- the five families: plan against paths()
# keys of paths() / paths2() without a counterpart in a plan
BITCONV_INSIDE = 'nrows nwords wbase off straddles partial_x partial_y last_word tail_word u8_bytes rem passes uneven group'.split()
BITCONV2_INSIDE = ('unused_cols unused_rows kpad blocks last_rows straddles u8_bytes NT partial_n nwn mw reload MT partial_m per runs '
                   'ragged idle vec scalar walks').split()
POLICYHEAD_INSIDE = ('last_chunk pad_cols restage vec_stage scalar_stage idle_lanes live_rows walks last_tile_rows idle_waves '
                     'partial_wave last_slice_rows gh_last_rows gh_partial_k gw_partial_k chains').split()
QHEAD_INSIDE = ('last_chunk restage passes partial_pass_lanes walks last_tile_rows idle_waves odd_row bwalks b_last_tile_rows '
                'last_slice_rows gw_partial').split()
FEATCONV_INSIDE = ('unused_rows unused_cols kpad last_rows NT partial_n MT partial_m jobs ragged idle walks gx_kpad gx_last_rows gx_NT '
                   'gx_partial_n gx_partial_m gx_dilated gw_partial_n gw_idle_waves gw_partial_m gw_last_rows gw_kpad gw_walks').split()


def check_bitconv(L, hip, s, n, u8):
    rows, cols, kernel, stride, channels = s
    cap = 4096
    groups = (ctypes.c_longlong * (2 * cap))()
    p = flat(L.shim_bitconv, BITCONV_KEYS, s, n, int(u8), groups, cap)
    if p is None:
        return None
    w = bc.paths(rows, cols, kernel, stride, channels, n)
    same(p, w, 'oh ow words tiles_x tiles_y G chunks launches'.split(), BITCONV_INSIDE, (s, n))
    # `group` is the images of a forward launch: the list of (first, grid) is its counterpart
    assert p['launches'] <= cap
    per = w['tiles_x'] * w['tiles_y']
    assert list(groups[:2 * p['launches']]) == [v for f in range(0, n, w['group']) for v in (f, min(w['group'], n - f) * per)], (s, n)
    assert (p['fwd_inst'], p['bwd_inst'], p['fwd_lds']) == (2 * kernel + int(u8), kernel, 0), (s, n)
    assert (p['nw'], p['reduce_blocks']) == (channels * kernel * kernel, -(-(channels * (kernel * kernel + 1)) // p['bwd_block'])), (s, n)
    assert p['workspace'] == w['G'] * channels * (kernel * kernel + 1) * 4, (s, n)
    if hip:
        _lib, lib = hip
        cfg = _lib.BitconvConfig(rows, cols, kernel, stride, channels, 0, 1.0)
        assert lib.f110_bitconv_workspace(ctypes.byref(cfg), n) == p['workspace'], (s, n)
    return p


def check_bitconv2(L, s, n, u8):
    rows, cols, k1, s1, c1, k2, s2, c2 = s
    p = flat(L.shim_bitconv2, BITCONV2_KEYS, s, n, int(u8))
    if p is None:
        return None
    w = b2.paths2(*s, n=n)
    same(p, w, 'oh1 ow1 oh2 ow2 xw ktot ksteps br bands lds items grid'.split(), BITCONV2_INSIDE, (s, n))
    # staged rows and the two offsets, from br and the layout tests/bitconv2_cases.py lds_bytes states
    nr1 = (w['br'] - 1) * s2 + k2
    words = ((nr1 - 1) * s1 + k1) * bc.BC_LWORDS * 8
    assert (p['nr1'], p['koff_off'], p['a1_off']) == (nr1, words, words + b2.BC2_KSTEPS * 16), (s, n)
    assert (p['inst'], p['u8']) == (0, int(u8))
    return p


def check_policyhead(L, hip, s, n):
    K, A, f64 = s
    p = flat(L.shim_policyhead, POLICYHEAD_KEYS, s, n)
    if p is None:
        return None
    w = ph.paths(n, K, A)
    same(p, w, 'T kc chunks lds tiles grid slices gh_blocks gh_kblocks gw_kblocks'.split(), POLICYHEAD_INSIDE, (s, n))
    assert (p['b_T'], p['b_kc'], p['b_chunks'], p['b_slices'], p['gw_slices']) == (w['T'], w['kc'], w['chunks'], w['slices'], w['slices']), (s, n)
    assert (p['inst'], p['gpre_inst'], p['gw_block']) == (2 * w['T'] + f64, f64, 64), (s, n)
    assert p['gpre_blocks'] == -(-(n * A) // ph.PH_THREADS) and p['reduce_blocks'] == -(-(2 * A * (K + 1)) // ph.PH_THREADS), (s, n)
    assert (p['gpre_at'], p['partial_at'], p['workspace']) == (0, -(-(n * 2 * A) // 4) * 4, ph.workspace_bytes(n, K, A)), (s, n)
    if hip:
        _lib, lib = hip
        assert lib.f110_policyhead_workspace(ctypes.byref(_lib.PolicyheadConfig(K, A, f64)), n) == p['workspace'], (s, n)
    return p


def check_qhead(L, hip, s, n):
    H, A, C, ld = s
    p = flat(L.shim_qhead, QHEAD_KEYS, s, n)
    if p is None:
        return None
    w = qh.paths(n, H, A, C)
    same(p, w, 'hc chunks lds tiles grid btiles bgrid amax slices gw_blocks partial_floats reduce_blocks C'.split(), QHEAD_INSIDE, (s, n))
    assert (p['b_hc'], p['b_chunks'], p['b_slices'], p['b_lds'], p['gw_slices']) == (w['hc'], w['chunks'], w['slices'], w['lds'], w['slices']), (s, n)
    assert (p['reduce_C'], p['gw_amax'], p['partial_at']) == (C, w['amax'], 0), (s, n)
    assert p['workspace'] == qh.workspace_bytes(n, H, A, C), (s, n)
    if hip:
        _lib, lib = hip
        assert lib.f110_qhead_workspace(ctypes.byref(_lib.QheadConfig(H, A, C, ld, 0)), n) == p['workspace'], (s, n)
    return p


def check_featconv(L, hip, s, n):
    ci, h, wd, co, k, st = s
    p = flat(L.shim_featconv, FEATCONV_KEYS, s, n)
    if p is None:
        return None
    w = fc.paths(*s, n=n)
    same(p, w, ('oh ow ktot chunks xw br bands lds items grid gx_ktot gx_chunks gx_xw gx_br gx_bands gx_lds gx_items '
                'gw_NT gw_MT gw_br gw_bands gw_lds gw_grid gw_groups').split(), FEATCONV_INSIDE, (s, n))
    # staged rows, the planes' offsets and the rest of the GEMMs' fields, from br and the layout gemm_lds / gradw_lds state
    assert (p['nr'], p['gx_nr'], p['gw_nr']) == ((w['br'] - 1) * st + k, w['gx_br'] + k - 1, (w['gw_br'] - 1) * st + k), (s, n)
    assert (p['planes_off'], p['gx_planes_off']) == (w['chunks'] * 4 * fc.FC_CHUNK * 4 + fc.FC_ZERO_BYTES, w['gx_chunks'] * 4 * fc.FC_CHUNK * 4 + fc.FC_ZERO_BYTES), (s, n)
    assert (p['gx_ph'], p['gx_pw'], p['gx_ms'], p['gx_grid']) == (h, wd, 1, min(w['gx_items'], fc.FC_MAX_GRID)), (s, n)
    assert (p['gw_xw'], p['gw_ktot'], p['gw_gp'], p['gw_inst']) == (w['xw'], w['ktot'], w['gw_br'] * w['ow'], w['gw_MT']), (s, n)
    assert p['gw_xs_at'] * 4 == fc.FC_ZERO_BYTES + -(-co * w['gw_br'] * w['ow'] * 4 // 16) * 16, (s, n)
    assert (p['nw'], p['reduce_blocks']) == (co * w['ktot'], -(-(co * (w['ktot'] + 1)) // p['block'])), (s, n)
    assert p['workspace'] == n * co * (w['ktot'] + 1) * 4, (s, n)        # csrc/f110_featconv.h: P is n Co (Ci k^2 + 1) floats
    if hip:
        _lib, lib = hip
        assert lib.f110_featconv_workspace(ctypes.byref(_lib.FeatconvConfig(ci, h, wd, co, k, st, 0, 0)), n) == p['workspace'], (s, n)
    return p


# ---------------------------------------------------------------- constants
def test_constants_the_cases_files_type_again(lib):
    c = {name: constant(lib, name) for name in CONSTANTS}
    want = dict(BC_TX=bc.BC_TX, BC_TY=bc.BC_TY, BC_MAX_K=bc.BC_MAX_K, BC_LROWS=bc.BC_LROWS, BC_LWORDS=bc.BC_LWORDS, BC_CHUNK=bc.BC_CHUNK,
                BC_MAX_PARTIALS=bc.BC_MAX_PARTIALS, BC_FORWARD_GROUP=bc.FORWARD_GROUP,
                BC2_KSTEPS=b2.BC2_KSTEPS, BC2_ACCS=b2.BC2_ACCS, BC2_LDS_BYTES=b2.BC2_LDS_BYTES, BC2_MAX_GRID=b2.BC2_MAX_GRID, BC2_MAX_OW1=b2.BC2_MAX_OW1,
                PH_ROWS=ph.PH_ROWS, PH_LDS_BYTES=ph.PH_LDS_BYTES, PH_MAX_GRID=ph.PH_MAX_GRID, PH_PREFETCH=ph.PH_PREFETCH, PH_GH_ROWS=ph.PH_GH_ROWS,
                PH_THREADS=ph.PH_THREADS, PH_SLICE=ph.R, PH_MAX_K=ph.MAX_K, PH_MAX_A=ph.MAX_A,
                QH_THREADS=qh.QH_THREADS, QH_RPW=qh.QH_RPW, QH_ROWS=qh.QH_ROWS, QH_BROWS=qh.QH_BROWS, QH_LDS_BYTES=qh.QH_LDS_BYTES, QH_MAX_GRID=qh.QH_MAX_GRID,
                QH_SLICE=qh.R, QH_MAX_H=qh.MAX_H, QH_MAX_A=qh.MAX_A, QH_MAX_C=qh.MAX_C, QH_MAX_ROWS=qh.MAX_ROWS,
                FC_CHUNK=fc.FC_CHUNK, FC_ACCS=fc.FC_ACCS, FC_ZERO_BYTES=fc.FC_ZERO_BYTES, FC_LDS_BYTES=fc.FC_LDS_BYTES, FC_MAX_GRID=fc.FC_MAX_GRID,
                FCW_TILES=fc.FCW_TILES)
    assert {k: c[k] for k in want} == want
    # (not typed but computed there, as 0.5 * log(2 pi) rounded twice: one ulp below the header's correctly rounded literal)
    assert lib.shim_half_log_2pi() == float('0.91893853320467274178') and abs(lib.shim_half_log_2pi() - ph.HALF_LOG_2PI) <= np.spacing(ph.HALF_LOG_2PI)
    from red_gym_amd import _lib
    assert (c['PH_SLICE'], c['QH_SLICE']) == (_lib.F110_POLICYHEAD_SLICE_ROWS, _lib.F110_QHEAD_SLICE_ROWS)


# ---------------------------------------------------------------- the shapes the GPU tests run
def test_bitconv_tables(lib, hip):
    for s in bc.SHAPES + bc.CASES:
        for n in (3,) + bc.BACKWARD_N:
            for u8 in (False, True):
                assert check_bitconv(lib, hip, s, n, u8)
    for s in bc.BACKWARD_SHAPES:
        assert check_bitconv(lib, hip, s[:5], s[5], False)
    # the split launch (test_forward_in_two_launches)
    one, two = check_bitconv(lib, hip, (8, 8, 8, 8, 1), 1 << 23, False), check_bitconv(lib, hip, (8, 8, 8, 8, 1), (1 << 23) + 3, True)
    assert (one['launches'], two['launches']) == (1, 2)


def test_bitconv2_tables(lib):
    for s in b2.CASES2:
        for u8 in (False, True):
            assert check_bitconv2(lib, s, 3, u8)
    p = check_bitconv2(lib, b2.LOOP_CASE, b2.LOOP_N, False)
    assert p['items'] > p['grid'] == b2.BC2_MAX_GRID


def test_policyhead_tables(lib, hip):
    for n, K, A in ph.FORWARD_SHAPES + ph.BACKWARD_SHAPES:
        for f64 in (0, 1):
            assert check_policyhead(lib, hip, (K, A, f64), n)
    assert any(-(-n // ph.PH_ROWS) > ph.PH_MAX_GRID for n, K, A in ph.FORWARD_SHAPES)


def test_qhead_tables(lib, hip):
    for n, H, A in qh.FORWARD_SHAPES + qh.BACKWARD_SHAPES:
        for C in (1, 2):
            assert check_qhead(lib, hip, (H, A, C, A + C - 1), n)
    assert any(-(-n // qh.QH_ROWS) > qh.QH_MAX_GRID for n, H, A in qh.FORWARD_SHAPES)


def test_featconv_tables(lib, hip):
    for s in fc.CASES:
        assert check_featconv(lib, hip, s, 3)
    # kernel < stride: the staged width is what the windows span (it skips the gap behind the last one), grad_x stages all of x's
    # columns plus k - 1, and each is one band in all three kernels
    assert len(fc.GAP_CASES) == 4 and all(s in fc.CASES for s in fc.GAP_CASES)
    for s in fc.GAP_CASES:
        ci, h, wd, co, k, st = s
        p = check_featconv(lib, hip, s, 3)
        assert k < st and (p['xw'], p['gw_xw'], p['gx_xw']) == ((p['ow'] - 1) * st + k, (p['ow'] - 1) * st + k, wd + k - 1), s
        assert (p['bands'], p['gx_bands'], p['gw_bands'], p['gx_ph'], p['gx_pw']) == (1, 1, 1, h, wd), s
        assert (p['nr'], p['gx_nr'], p['gw_nr']) == ((p['oh'] - 1) * st + k, h + k - 1, (p['oh'] - 1) * st + k), s
    p = check_featconv(lib, hip, fc.LOOP_CASE, fc.LOOP_N)
    assert p['items'] > p['grid'] == fc.FC_MAX_GRID and p['gx_items'] > p['gx_grid'] and fc.LOOP_N > p['gw_grid'] == fc.FC_MAX_GRID


# ---------------------------------------------------------------- a seeded sample of what the compiled checks accept
SAMPLE = 2000


def batches(rng, cap, rows=1):
    """A batch count of {1, 3, 67, cap, 2 cap + 5}; for a kernel that walks tiles of `rows` rows also the counts that put cap and
    2 cap + 5 tiles in front of cap workgroups."""
    return int(rng.choice(sorted({1, 3, 67, cap, 2 * cap + 5, cap * rows, (2 * cap + 5) * rows})))


def sample(draw, check, rng):
    """SAMPLE configurations the compiled check accepts out of draw()'s (which reach a little past every limit)."""
    ok = tried = 0
    while ok < SAMPLE:
        tried += 1
        assert tried < 20 * SAMPLE
        ok += check(*draw(rng)) is not None
    return tried - ok


def test_bitconv_sample(lib, hip):
    def draw(rng):
        kernel = int(rng.integers(1, bc.BC_MAX_K + 2))
        # mostly images of a few tiles; some as large as the frame format allows
        top = constant(lib, 'REPLAY_MAX_DIM') + 1 if rng.random() < 0.1 else 600
        return ((int(rng.integers(kernel, top + 1)), int(rng.integers(kernel, top + 1)), kernel, int(rng.integers(1, kernel + 2)),
                 int(rng.integers(1, 66))), batches(rng, bc.BC_MAX_PARTIALS), bool(rng.integers(2)))
    refused = sample(draw, lambda s, n, u8: check_bitconv(lib, hip, s, n, u8), np.random.default_rng(23))
    assert refused > 0


def test_bitconv2_sample(lib):
    def draw(rng):
        k1, k2 = int(rng.integers(1, bc.BC_MAX_K + 1)), int(rng.integers(1, 6))
        s1, s2 = int(rng.integers(1, k1 + 1)), int(rng.integers(1, k2 + 2))
        # first-layer outputs of up to 40 rows (paths2 walks every output pixel) and up to one column past the limit
        oh1, ow1 = int(rng.integers(1, 41)), int(rng.integers(1, b2.BC2_MAX_OW1 + 2))
        rows, cols = (oh1 - 1) * s1 + k1 + int(rng.integers(s1)), (ow1 - 1) * s1 + k1 + int(rng.integers(s1))
        return (rows, cols, k1, s1, int(rng.integers(1, 18)), k2, s2, int(rng.integers(1, 66))), batches(rng, b2.BC2_MAX_GRID), bool(rng.integers(2))
    refused = sample(draw, lambda s, n, u8: check_bitconv2(lib, s, n, u8), np.random.default_rng(29))
    assert refused > 0


def test_policyhead_sample(lib, hip):
    def draw(rng):
        K = int(rng.integers(1, ph.MAX_K + 2)) if rng.random() < 0.5 else int(rng.integers(1, 700))
        return (K, int(rng.integers(1, ph.MAX_A + 2)), int(rng.integers(2))), batches(rng, ph.PH_MAX_GRID, ph.PH_ROWS)
    refused = sample(draw, lambda s, n: check_policyhead(lib, hip, s, n), np.random.default_rng(31))
    assert refused > 0


def test_qhead_sample(lib, hip):
    def draw(rng):
        H = int(rng.integers(1, qh.MAX_H + 2)) if rng.random() < 0.5 else int(rng.integers(1, 700))
        A = int(rng.integers(1, qh.MAX_A + 2))
        return (H, A, int(rng.integers(1, 4)), A + int(rng.integers(-1, 3))), batches(rng, qh.QH_MAX_GRID, qh.QH_ROWS)
    refused = sample(draw, lambda s, n: check_qhead(lib, hip, s, n), np.random.default_rng(37))
    assert refused > 0


def test_featconv_sample(lib, hip):
    def draw(rng):
        k = int(rng.integers(1, 6))
        return ((int(rng.integers(1, 34)), int(rng.integers(k, 130)), int(rng.integers(k, 67)), int(rng.integers(1, 66)), k, int(rng.integers(1, 6))),
                batches(rng, fc.FC_MAX_GRID))
    refused = sample(draw, lambda s, n: check_featconv(lib, hip, s, n), np.random.default_rng(41))
    assert refused > 0


# ---------------------------------------------------------------- sweeps: what every launch of every accepted configuration must satisfy
# Dynamic LDS within the family's *_LDS_BYTES; band rows >= 1; (bands - 1) BR < the plane's rows <= bands BR; kc / hc a positive
# multiple of 64 whose chunks cover K / H; 1 <= grid x <= the family's cap, at n = 1 and at n above the cap.  These are caps, not
# measurements; the bytes printed are the worst the sweep met, and the worst a band of one row
# would need.
def sweep(lib, name, n_cfg):
    out = (ctypes.c_longlong * 24)()
    getattr(lib, 'shim_sweep_' + name)(out)
    o = list(out)
    print('%s: %d plans, most LDS bytes per launch %s, that a band of one row would need %s' % (name, o[0], o[2:5], o[5:8]))
    assert o[1] == 0, '%d offenders; the first breaks property %d: configuration and n %s' % (o[1], o[8], o[9:9 + n_cfg + 1])
    return o


def test_featconv_sweep(lib):
    """Every (kernel, stride, in_channels, out_channels) the check accepts at cols in {kernel, 63, 64}, rows in {kernel, 64}."""
    o = sweep(lib, 'featconv', 6)
    pairs = sum(min(32, 512 // (k * k)) * min(64, 512 // (k * k)) for k in range(1, 5))     # (Ci, Co) under the limits on K, per kernel
    assert o[0] == pairs * 4 * 3 * 2 * 2                                # strides, cols, rows, n
    assert max(o[2:5]) <= fc.FC_LDS_BYTES
    assert o[5:8] == [34832, 46416, 40592]          # forward, grad_x, partials: worked out by hand from the limits


def test_bitconv2_sweep(lib):
    """Every (kernel, stride, channels <= 16, kernel2, stride2) at first-layer outputs of {kernel2, 63, 64} columns, {kernel2, 64} rows."""
    o = sweep(lib, 'bitconv2', 8)
    assert o[0] == 36 * 16 * 10 * 3 * 2 * 2 and o[2] <= b2.BC2_LDS_BYTES and o[5] < 20 * 1024


def test_policyhead_sweep(lib):
    """Every (in_features, action_dim)."""
    o = sweep(lib, 'policyhead', 3)
    assert o[0] == ph.MAX_K * ph.MAX_A * 2 and o[2] <= ph.PH_LDS_BYTES


def test_qhead_sweep(lib):
    """Every (hidden, action_dim); the forward's and the backward rows kernel's chunk."""
    o = sweep(lib, 'qhead', 4)
    assert o[0] == qh.MAX_H * qh.MAX_A * 2 and max(o[2:4]) <= qh.QH_LDS_BYTES
    assert o[2] == o[3] and check_qhead(lib, None, (qh.MAX_H, 32, 2, 32), 1)['lds'] == 4 * (32 * (448 + 1) + 2 * 448) == 61056     # A = 32: chunks of 448 units
