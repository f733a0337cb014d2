"""The checker of the critic head (csrc/f110_qhead.h), NumPy only: the numerics contract of include/f110_hip.h restated exactly --
every fused step through bitconv2_cases.fma32, the 64 partial sums and the tree, the slices of the two-stage sums -- so that every
output of the GPU, forward and backward, can be compared with `==`; the kernels' geometry restated, so that every shape can be shown
to select what its comment claims; and the bounds that tie the checker to the recording of the reference's own SACAgent.update
(tests/golden/g21_critic.npz), worked out from the formulas and the recording's own fc1 error, never from the kernel's output."""
import numpy as np

import bitconv2_cases as b2
import bitconv_cases as bc

# csrc/f110_qhead.h and include/f110_hip.h
QH_THREADS, QH_RPW, QH_ROWS, QH_BROWS, QH_LDS_BYTES, QH_MAX_GRID = 256, 2, 8, 4, 64 * 1024, 1024
R = 256                                   # F110_QHEAD_SLICE_ROWS
MAX_H, MAX_A, MAX_C, MAX_ROWS = 4096, 32, 2, 1 << 24
U32, U64 = bc.U, 2.0 ** -53
f32 = np.float32

# (n, H, A); what each selects is asserted from paths() in test_qhead_cpu.py
FORWARD_SHAPES = [
    (1, 1, 1),          # one row, one unit, one action column: one live lane, one live row of one wave
    (1, 64, 1),         # one full pass of 64 lanes
    (3, 65, 2),         # a second pass with one live lane; the second wave holds one row
    (17, 63, 15),       # three tiles, the last of one row; one idle lane
    (64, 512, 16),      # SAL at the batch of an update: every unit of a critic staged once (36.1 KB), 8 full tiles
    (65, 515, 17),      # 576 units staged (the 515 padded), the last pair of passes holds 3 live units; a ninth tile of one row
    (5, 4096, 32),      # the limits: chunks of 448 units, 10 of them, the last of 64; every tile stages its chunks
    (QH_MAX_GRID * QH_ROWS + 1, 8, 2),   # 1025 tiles on 1024 workgroups: one walks a second tile, of one row
]
# (n, H, A) of the backward cases: n in {1, R - 1, R, R + 1, 2R + 3}
BACKWARD_SHAPES = [
    (1, 70, 3),         # one row: a slice of one; a second pass of 6 lanes
    (R - 1, 5, 1),      # a slice one short
    (R, 512, 16),       # SAL: exactly one slice, two stage-1 unit blocks
    (R + 1, 300, 32),   # two slices, the second of one row; A = 32: the wide instantiation; a partial second unit block
    (2 * R + 3, 33, 17),  # three slices, the last of three rows; 17 of 32 accumulators
    (6, 4096, 32),      # chunked staging in the backward rows kernel: two tiles, the second of two rows
]


def paths(n, H, A, C=2):
    """What csrc/f110_qhead.h does with n rows, restated from its arithmetic (qhead_geometry on the host, the kernels' indexing).
    hc: hidden units in LDS at a time; chunks, last_chunk: its live units; restage: every tile stages its chunks; lds: bytes;
    passes: pairs of 64-unit passes per chunk; partial_pass_lanes: live lanes of the last 64-unit pass that has any (64: full);
    stage_passes: staging rounds of a critic; tiles, grid, walks, last_tile_rows, idle_waves: of the forward launch (a wave with no
    row); odd_row: a wave whose second row is past n; btiles, bgrid, bwalks, b_last_tile_rows: of the backward rows kernel; amax:
    the instantiation (accumulators held); slices, last_slice_rows; gw_blocks, gw_partial: stage 1's unit blocks; partial_floats: of
    one (critic, slice); reduce_blocks."""
    hc = min((QH_LDS_BYTES // 4 - A) // (A + 2) // 64 * 64, -(-H // 64) * 64)
    chunks = -(-H // hc)
    last_chunk = H - (chunks - 1) * hc
    tiles = -(-n // QH_ROWS)
    grid = min(tiles, QH_MAX_GRID)
    last_tile_rows = n - (tiles - 1) * QH_ROWS
    btiles = -(-n // QH_BROWS)
    slices = -(-n // R)
    P = H * (A + 2) + 1
    return dict(hc=hc, chunks=chunks, last_chunk=last_chunk, restage=chunks > 1, lds=4 * (A * (hc + 1) + 2 * hc), passes=-(-hc // 128),
                partial_pass_lanes=(H - 1) % 64 + 1, tiles=tiles, grid=grid, walks=-(-tiles // grid), last_tile_rows=last_tile_rows,
                idle_waves=4 - -(-last_tile_rows // QH_RPW), odd_row=n % QH_RPW != 0, btiles=btiles, bgrid=min(btiles, QH_MAX_GRID),
                bwalks=-(-btiles // min(btiles, QH_MAX_GRID)), b_last_tile_rows=n - (btiles - 1) * QH_BROWS, amax=16 if A <= 16 else 32,
                slices=slices, last_slice_rows=n - (slices - 1) * R, gw_blocks=-(-H // QH_THREADS), gw_partial=H % QH_THREADS != 0,
                partial_floats=P, reduce_blocks=-(-P // QH_THREADS), C=C)


def workspace_bytes(n, H, A, C):
    """What f110_qhead_backward writes: [C][slices][H (A + 2) + 1] floats, rounded up to 4."""
    p = paths(n, H, A, C)
    return 4 * (-(-(C * p['slices'] * p['partial_floats']) // 4) * 4)


# ---------------------------------------------------------------------------------------------- inputs
TIE_Q = 1.25                              # q of both critics on a tie row (with biases: pre = TIE_Q - b2, both exact)
SIDE = 8.0                                # what unit 0 adds to one critic's q on the other rows, so that the min's side is known


def special_rows(n, H):
    """(tie rows, the all-zero action row or None, the row of the z == 0 unit or None) of inputs(n, H, ...)."""
    ties = [n // 4, n // 4 + 1] if n >= 8 and H >= 4 else []
    return ties, (n // 3 if n >= 3 else None), (n // 2 if H >= 4 else None)


def inputs(n, H, A, C=2, seed=0):
    """dict of pre (C arrays [n, H] fp32), w_act (C arrays [H, A] fp32, dense), b1 (C x [H]), w2 (C x [H]), b2 (C x [1]), action [n, A]
    fp64 (not fp32 values: the one rounding on load matters), reward [n] fp64, done [n] uint8, nlp [n] fp64; every critic has its own
    parameters.  Built in (H >= 4): unit 0 of every critic has w_act = 0, b1 = 0, w2 = 1, so it adds relu(pre[:, 0]) to q exactly: on
    the tie rows (special_rows; n >= 8) every other unit is dead (pre = -1e6) and pre[:, 0] = TIE_Q - b2, so both q are TIE_Q whatever
    the other parameters, with an active unit to carry the halves; on the other rows pre[:, 0] = SIDE for critic 0 on even rows and for
    critic 1 on odd rows and -1 for the other, which puts each side of the min on half of them.  Unit H // 2 has w_act = 0 and b1 = 0
    and pre = 0 on row n // 2: z == 0 exactly.  Row n // 3 of the action is zeros (n >= 3).  done holds both values (n >= 2).  (With
    b2 passed as NULL the tie rows are no ties.)"""
    rng = np.random.default_rng([n, H, A, C, seed])
    pre = [rng.normal(size=(n, H)).astype(f32) for _ in range(C)]
    scale = 10.0 ** rng.integers(-2, 1, (C, H, A))
    w_act = [(rng.normal(size=(H, A)) * scale[c]).astype(f32) for c in range(C)]
    b1 = [(0.5 * rng.normal(size=H)).astype(f32) for _ in range(C)]
    w2 = [(rng.normal(size=H) / np.sqrt(H)).astype(f32) for _ in range(C)]
    b2 = [np.array([0.25, -0.5][c:c + 1], f32) for c in range(C)]
    action = np.tanh(rng.normal(size=(n, A)))
    ties, zero_row, z0_row = special_rows(n, H)
    if zero_row is not None:
        action[zero_row] = 0.0
    if H >= 4:
        for c in range(C):
            w_act[c][0] = 0.0
            b1[c][0] = 0.0
            w2[c][0] = 1.0
            pre[c][:, 0] = np.where(np.arange(n) % 2 == c, SIDE, -1.0)
            for r in ties:
                pre[c][r] = -1.0e6
                pre[c][r, 0] = f32(TIE_Q) - b2[c][0]
            j0 = H // 2
            w_act[c][j0] = 0.0
            b1[c][j0] = 0.0
            pre[c][z0_row, j0] = 0.0
    done = (rng.random(n) < 0.5).astype(np.uint8)
    if n >= 2:
        done[0], done[-1] = 0, 1
    return dict(pre=pre, w_act=w_act, b1=b1, w2=w2, b2=b2, action=action, reward=rng.normal(size=n), done=done,
                nlp=rng.normal(size=n) * 10.0 - 5.0)


# ---------------------------------------------------------------------------------------------- the contract
def tree64(s):
    """s [..., 64] float32 -> [...]: for m = 32 .. 1: s_l = s_l + s_{l + m} for l < m."""
    s = np.array(s, f32)
    for m in (32, 16, 8, 4, 2, 1):
        s[..., :m] = s[..., :m] + s[..., m:2 * m]
    assert s.dtype == f32
    return s[..., 0]


def hidden(pre, w_act, b1, action32):
    """(z, h) [n, H] float32 of one critic: acc = 0; for a ascending: acc = fma(w_act[j][a], action[b][a], acc); z = (pre + acc) + b1
    (+ 0.0f for None); h = z > 0 ? z : 0."""
    pre, w_act = np.asarray(pre, f32), np.asarray(w_act, f32)
    acc = np.zeros(pre.shape, f32)
    for a in range(w_act.shape[1]):
        acc = b2.fma32(w_act[None, :, a], action32[:, a, None], acc)
    z = (pre + acc) + (np.zeros(pre.shape[1], f32) if b1 is None else np.asarray(b1, f32))[None, :]
    assert z.dtype == f32
    return z, np.where(z > 0, z, f32(0.0))


def q_of(h, w2, b2_):
    """q [n] float32: the 64 partial fma chains over j = l, l + 64, ..., the tree, + b2 (+ 0.0f for None)."""
    n, H = h.shape
    w2 = np.asarray(w2, f32).reshape(-1)
    s = np.zeros((n, 64), f32)
    for i in range(-(-H // 64)):
        cols = slice(64 * i, min(H, 64 * i + 64))
        m = cols.stop - cols.start
        s[:, :m] = b2.fma32(w2[None, cols], h[:, cols], s[:, :m])
    q = tree64(s) + (f32(0.0) if b2_ is None else np.asarray(b2_, f32).reshape(-1)[0])
    assert q.dtype == f32
    return q


def forward(inp, C=None, fp32_action=False, bias=True, target=True, gamma=0.99, alpha=0.2):
    """The forward contract on inputs(): dict of q [C, n], qmin [n], target [n] (None without `target`), z and h (lists), act32 (the
    action as the kernel uses it).  fp32_action: the action (and nlp) are first stored as fp32, as the ring does; bias=False: b1 and
    b2 are NULL."""
    C = len(inp['pre']) if C is None else C
    act = np.asarray(inp['action'], np.float64)
    nlp = np.asarray(inp['nlp'], np.float64)
    if fp32_action:
        act, nlp = act.astype(f32).astype(np.float64), nlp.astype(f32).astype(np.float64)
    act32 = act.astype(f32)
    zs, hs, qs = [], [], []
    for c in range(C):
        z, h = hidden(inp['pre'][c], inp['w_act'][c], inp['b1'][c] if bias else None, act32)
        zs.append(z)
        hs.append(h)
        qs.append(q_of(h, inp['w2'][c], inp['b2'][c] if bias else None))
    q = np.stack(qs)
    qmin = np.where(q[0] < q[1], q[0], q[1]) if C == 2 else q[0].copy()
    tv = None
    if target:
        tq = qmin.astype(np.float64) - alpha * nlp
        tv = (np.asarray(inp['reward'], np.float64) + ((1.0 - inp['done'].astype(np.float64)) * gamma) * tq).astype(f32)
    return dict(q=q, qmin=qmin, target=tv, z=zs, h=hs, act32=act32)


def min_masks(q):
    """m [C, n] float32: 1 where q_c < q_other, 0.5 where equal, 0 where greater; C = 1: ones."""
    if q.shape[0] == 1:
        return np.ones(q.shape, f32)
    m0 = np.where(q[0] < q[1], f32(1.0), np.where(q[0] == q[1], f32(0.5), f32(0.0))).astype(f32)
    m1 = np.where(q[1] < q[0], f32(1.0), np.where(q[0] == q[1], f32(0.5), f32(0.0))).astype(f32)
    return np.stack([m0, m1])


def backward(inp, fwd, grad_q=None, grad_qmin=None, bias=True):
    """The backward contract: dict of G [C, n], grad_pre (C x [n, H]), grad_w_act (C x [H, A]), grad_b1, grad_w2 (C x [H]), grad_b2 (C
    x [1]) and grad_action [n, A] (float32 values; the kernel widens them for an fp64 action), from fwd = forward(...)."""
    q, act32 = fwd['q'], fwd['act32']
    C, n = q.shape
    A = act32.shape[1]
    m = min_masks(q)
    gq = np.zeros((C, n), f32) if grad_q is None else np.asarray(grad_q, f32)
    gm = np.zeros(n, f32) if grad_qmin is None else np.asarray(grad_qmin, f32)
    out = dict(G=[], grad_pre=[], grad_w_act=[], grad_b1=[], grad_w2=[], grad_b2=[])
    ga = np.zeros((n, A), f32)
    for c in range(C):
        G = gq[c] + gm * m[c]
        assert G.dtype == f32
        w2, w_act = np.asarray(inp['w2'][c], f32).reshape(-1), np.asarray(inp['w_act'][c], f32)
        H = w2.shape[0]
        z, h = fwd['z'][c], fwd['h'][c]
        gz = np.where(z > 0, G[:, None] * w2[None, :], f32(0.0)).astype(f32)
        tot = [np.zeros((H, A), f32), np.zeros(H, f32), np.zeros(H, f32), np.zeros(1, f32)]
        for b0 in range(0, n, R):
            acc = [np.zeros((H, A), f32), np.zeros(H, f32), np.zeros(H, f32), np.zeros(1, f32)]
            for b in range(b0, min(n, b0 + R)):
                acc[0] = b2.fma32(gz[b][:, None], act32[b][None, :], acc[0])
                acc[1] = acc[1] + gz[b]
                acc[2] = b2.fma32(G[b], h[b], acc[2])
                acc[3] = acc[3] + G[b]
            tot = [t + a for t, a in zip(tot, acc)]
        assert all(t.dtype == f32 for t in tot)
        s = np.zeros((n, A, 64), f32)
        for i in range(-(-H // 64)):
            cols = slice(64 * i, min(H, 64 * i + 64))
            k = cols.stop - cols.start
            s[:, :, :k] = b2.fma32(gz[:, None, cols], w_act[cols].T[None, :, :], s[:, :, :k])
        ga = ga + tree64(s)
        out['G'].append(G)
        out['grad_pre'].append(gz)
        for key, t in zip(('grad_w_act', 'grad_b1', 'grad_w2', 'grad_b2'), tot):
            out[key].append(t)
    assert ga.dtype == f32
    out['grad_action'] = ga
    out['G'] = np.stack(out['G'])
    return out


# ---------------------------------------------------------------------------------------------- the recording of the reference (g21)
GROUPS = ('01_balanced', '255_balanced', '255_default')
GROUP_ROWS = 16
G21_CRITICS = ('critic1_target', 'critic2_target', 'critic1', 'critic2')   # the order of the fixture's per-critic axes


# ---------------------------------------------------------------------------------------------- bounds against a reference in fp32
def dz_bound(mag, rel, A, gemm_sides=1):
    """Bound on |z of the contract - z of an fp32 reference| per (row, unit).  mag = sum |w| |x| + |b1| over all F + A inputs.  The
    reference's fc1 is one fp32 GEMM whose error against fp64 was MEASURED on the reference side as at most rel * mag over the
    recording's samples; 4 * rel * mag is taken for it, since a maximum over some thousand samples underestimates the tail.
    gemm_sides = 2 when the contract's `pre` comes from the same kind of GEMM (the module on the GPU); 1 when it is the fp64 product
    rounded once (u32 * mag).  The contract's own part by derivation: A fused steps and two additions, gamma_{A + 2} * mag."""
    return (4.0 * rel * gemm_sides + (U32 if gemm_sides == 1 else 0.0) + bc.gamma(A + 2)) * np.asarray(mag, np.float64)


def q_bound(dz, h, w2, b2_):
    """Bound on |q - q_ref| [n] from dz [n, H]: relu is 1-Lipschitz, so h moves by at most dz whatever the sign of z; either side sums
    H products and a bias in fp32 in some order: gamma_{H + 1} (sum |w2| (|h| + dz) + |b2|) each."""
    w2 = np.abs(np.asarray(w2, np.float64).reshape(-1))
    H = w2.shape[0]
    mag = (np.abs(np.asarray(h, np.float64)) + dz) @ w2 + abs(float(b2_))
    return dz @ w2 + 2.0 * bc.gamma(H + 1) * mag


def target_bound(dqmin, qmin, nlp, reward, done, gamma, alpha):
    """Bound on |tv - tv_ref| [n].  The reference works in fp32 (src/SAL.py:540-549): nlp and r rounded to fp32, alpha and gamma used
    as fp32 scalars, every operation rounded: tq = fl(qmin - fl(alpha nlp)): 3 u alpha |nlp| + u |tq|; tv = fl(r + fl(fl((1 - d)
    gamma) tq)): keep * dtq + 3 u |keep tq| + u |r| + u |tv|; the contract is exact up to fp64 and rounds tv once: u |tv|.  First
    order, the roundings doubled for the second."""
    nlp, reward, qmin = (np.asarray(v, np.float64) for v in (nlp, reward, qmin))
    keep = (1.0 - np.asarray(done, np.float64)) * gamma
    tq = qmin - alpha * nlp
    tv = reward + keep * tq
    dtq = dqmin + 2.0 * U32 * (3.0 * alpha * np.abs(nlp) + np.abs(tq))
    return keep * dtq + 2.0 * U32 * (3.0 * np.abs(keep * tq) + np.abs(reward) + 2.0 * np.abs(tv))


def loss_bounds(cq, tv, dq, dtv):
    """F.mse_loss(cq, tv) over n rows and its gradient G = 2 (cq - tv) / n: (loss in fp64, bound on |loss - loss_ref|, G float32 [n],
    bound on |G - G_ref| [n]).  e = cq - tv moves by de = dq + dtv; |e'^2 - e^2| <= 2 |e| de + de^2; the reference subtracts, squares
    and sums n terms in fp32: gamma_{n + 3} of the loss; G: de * 2 / n and four roundings of its own value per side."""
    cq, tv = np.asarray(cq, f32), np.asarray(tv, f32)
    n = cq.shape[0]
    e = cq.astype(np.float64) - tv.astype(np.float64)
    de = dq + dtv
    loss = float((e * e).mean())
    dloss = float((2.0 * np.abs(e) * de + de * de).mean() + 2.0 * bc.gamma(n + 3) * loss)
    G = (f32(2.0 / n) * (cq - tv)).astype(f32)
    return loss, dloss, G, 2.0 * de / n + 8.0 * U32 * np.abs(G)


def grad_bounds(fwd, c, G, dG, dz, w2, act32):
    """Bounds on the four parameter gradients of critic c against an fp32 reference, from G and dG [n] and dz [n, H]: dict of grad_w2
    [H], grad_b2 [1], grad_b1 [H], grad_w_act [H, A].  g_z = [z > 0] G w2: where the sign of z is known on both sides (|z| > dz) it
    moves by dG |w2| and the product's rounding on either side; where it is not, by its full size (|G| + dG) |w2|.  h moves by at most
    dz.  Every sum over the n rows is made in fp32 on either side in some order: gamma_{n + 1} of the absolute sum, each."""
    z, h = fwd['z'][c].astype(np.float64), fwd['h'][c].astype(np.float64)
    n = z.shape[0]
    w2 = np.abs(np.asarray(w2, np.float64).reshape(-1))
    Ga, act = np.abs(np.asarray(G, np.float64)) + dG, np.abs(act32.astype(np.float64))
    full = Ga[:, None] * w2[None, :]
    unknown = np.abs(z) <= dz
    dgz = np.where(unknown, full, dG[:, None] * w2[None, :] + 2.0 * U32 * full)
    gz = np.where((z > 0) | unknown, full, 0.0)
    gam = 2.0 * bc.gamma(n + 1)
    return dict(grad_w2=(dG[:, None] * (h + dz) + Ga[:, None] * dz).sum(0) + gam * (Ga[:, None] * (h + dz)).sum(0),
                grad_b2=np.array([dG.sum() + gam * Ga.sum()]), grad_b1=dgz.sum(0) + gam * gz.sum(0),
                grad_w_act=dgz.T @ act + gam * (gz.T @ act), unknown=unknown)


def g21_pass(g, gi, which):
    """inputs() of one pass of group gi of g21: which = 'target' (the two target critics on (ns, next_a), with the target's inputs) or
    'online' (the two critics on (s, a)) -> (inp, mags [2][n, H] fp64, the recorded q [2, n])."""
    k = 0 if which == 'target' else 2
    inp = dict(pre=[g['pre'][gi, k], g['pre'][gi, k + 1]], w_act=[g['w_act'][0], g['w_act'][1]], b1=[g['b1'][0], g['b1'][1]],
               w2=[g['w2'][0], g['w2'][1]], b2=[g['b2'][gi, k:k + 1], g['b2'][gi, k + 1:k + 2]], action=g['action'][gi, k].astype(np.float64),
               reward=g['reward'][gi], done=g['done'][gi], nlp=g['next_logp'][gi].astype(np.float64))
    assert np.array_equal(g['action'][gi, k], g['action'][gi, k + 1])
    return inp, [g['mag'][gi, k].astype(np.float64), g['mag'][gi, k + 1].astype(np.float64)], (g['ret'][gi, :2] if which == 'target' else g['cq'][gi])


GAMMA, ALPHA = 0.99, 0.2                  # SACAgent's defaults (src/SAL.py:478-479), with which g21 was recorded


def g21_check(g, run_forward, run_backward, report=print):
    """Group by group: q of the four critics, tv, both critic losses and the four recorded gradients per critic within the bounds.
    run_forward(inp, target) -> dict with q [2, n], qmin and target (of the implementation under test, fed fp32 actions);
    run_backward(inp, q, G [2, n]) -> dict of grad_w2, grad_b2, grad_b1, grad_w_act (lists of 2).  The bounds are built on the checker's
    own forward (z, h), which the kernel reproduces bit for bit."""
    A = g['w_act'].shape[2]
    for gi, name in enumerate(GROUPS):
        rel = float(g['fc1_rel_err'][gi])
        inp, mags, rec_q = g21_pass(g, gi, 'target')
        ref = forward(inp, fp32_action=True, gamma=GAMMA, alpha=ALPHA)
        got = run_forward(inp, True)
        dz = [dz_bound(m, rel, A) for m in mags]
        dq = [q_bound(dz[c], ref['h'][c], inp['w2'][c], inp['b2'][c][0]) for c in range(2)]
        for c in range(2):
            err = np.abs(np.asarray(got['q'][c], np.float64) - rec_q[c])
            report('%-13s %s: worst q error %.3g, bound there %.3g' % (name, G21_CRITICS[c], err.max(), dq[c][err.argmax()]))
            assert (err <= dq[c]).all() and dq[c].max() < 1e-2 * max(1.0, np.abs(rec_q[c]).max())
        dtv = target_bound(np.maximum(dq[0], dq[1]), ref['qmin'], inp['nlp'], inp['reward'], inp['done'], GAMMA, ALPHA)
        err = np.abs(np.asarray(got['target'], np.float64) - g['tv'][gi])
        report('%-13s tv: worst error %.3g, bound there %.3g' % (name, err.max(), dtv[err.argmax()]))
        assert (err <= dtv).all()
        assert (np.asarray(got['target'])[inp['done'] == 1] == inp['reward'].astype(f32)[inp['done'] == 1]).all()
        tv = np.asarray(got['target'], f32)
        inp, mags, rec_q = g21_pass(g, gi, 'online')
        ref = forward(inp, fp32_action=True, target=False)
        got = run_forward(inp, False)
        dz = [dz_bound(m, rel, A) for m in mags]
        Gs, dGs = [], []
        for c in range(2):
            dq = q_bound(dz[c], ref['h'][c], inp['w2'][c], inp['b2'][c][0])
            err = np.abs(np.asarray(got['q'][c], np.float64) - rec_q[c])
            report('%-13s %s: worst q error %.3g, bound there %.3g' % (name, G21_CRITICS[2 + c], err.max(), dq[err.argmax()]))
            assert (err <= dq).all()
            loss, dloss, G, dG = loss_bounds(got['q'][c], tv, dq, dtv)
            report('%-13s %s: loss %.9g, recorded %.9g, bound %.3g' % (name, G21_CRITICS[2 + c], loss, g['losses'][gi, c], dloss))
            assert abs(loss - g["losses"][gi, c]) <= dloss and dloss <= 1e-2 * loss
            Gs.append(G)
            dGs.append(dG)
        grads = run_backward(inp, np.asarray(got['q'], f32), np.stack(Gs))
        for c in range(2):
            b = grad_bounds(ref, c, Gs[c], dGs[c], dz[c], inp['w2'][c], ref['act32'])
            for key in ('grad_w2', 'grad_b2', 'grad_b1', 'grad_w_act'):
                rec = g[key][gi, c].astype(np.float64)
                err = np.abs(np.asarray(grads[key][c], np.float64).reshape(rec.shape) - rec)
                scale = np.abs(rec).max()
                report('%-13s %s %s: worst error %.3g (bound there %.3g, largest entry %.3g); %d of %d units of unknown sign'
                       % (name, G21_CRITICS[2 + c], key, err.max(), b[key].reshape(rec.shape).flat[err.argmax()], scale, int(b['unknown'].sum()), b['unknown'].size))
                assert (err <= b[key].reshape(rec.shape)).all()
                # the bounds pin digits: all but the entries that a unit of unknown sign reaches are bounded below a hundredth of the largest entry
                tight = b[key].reshape(rec.shape) <= 1e-2 * scale
                assert tight.mean() >= 0.9, (name, key, float(tight.mean()))
