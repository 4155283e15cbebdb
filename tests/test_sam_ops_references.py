"""CPU: the plain references of tests/sam_ops_cases.py for the Segment Anything kernels (csrc/sam.hip).  There is no C oracle for these ops,
so this file (a) pins every numpy reference to the independent torch statement of tests/sam_restatement.py where one exists (Model._attention
with its decomposed bias, the window partition lines of Model.encoder, _xattn, box_tokens, preprocess, full_logits) to float64 round-off,
(b) asserts that every case has the property it exists for, (c) plants the faults of DESIGN.md 6.6 into the REFERENCE and asserts that each
lands at least 10 bounds away (exact ops: unequal; postprocess: at least 1 % of the compared pixels flip) on the cases meant to catch it.
The one-op program builders here are shared with tests/test_gpu_sam_ops.py.  Runs without a GPU."""
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_ops_cases as C  # noqa: E402
import sam_restatement as R  # noqa: E402
from test_tokens_references import _nchw, _nhwc, _source, _target  # noqa: E402,F401

from cartoonsegmentation_amd import program as P  # noqa: E402

PIN = 1e-12                            # relative, float64 round-off between two statements of one formula


def _pin(mine, theirs):
    mine, theirs = np.asarray(mine, np.float64), np.asarray(theirs, np.float64)
    assert mine.shape == theirs.shape, (mine.shape, theirs.shape)
    assert np.abs(mine - theirs).max() <= PIN * np.abs(theirs).max()


def _model(sd=None, **cfg):
    return R.Model(sd or {}, types.SimpleNamespace(**cfg))


# ---- one-op programs ---------------------------------------------------------------------------------------------------------------------
def raw_rp(p, x, out, heads, d, grid, tab):
    """CSM_OP_ATTENTION_RELPOS as Program.attention_relpos emits it, into a given output view and without that method's checks (tab: the
    packed (Rh ; Rw) sqrt(d) table, or None for none)"""
    a_h = a_n = -1
    if tab is not None:
        a_h, a_n = p._w(tab, tab)
    return p._emit(P.OP_ATTENTION_RELPOS, x, None, out, groups=heads, cin_g=d, kh=grid[0], kw=grid[1], aux_off=a_h, nat=dict(aux_off=a_n))


def packed_table(case):
    return np.concatenate([case['rh'], case['rw']]) * np.sqrt(np.float32(case['d']))


def rp_program(case):
    """-> (program, [input NCHW], output shape NCHW, (wide output buffer, output view) or (None, None))"""
    n, heads, d, (gh, gw) = case['n'], case['heads'], case['d'], case['grid']
    p = P.Program(case['name'])
    x_ext, y_ext = p.ext_nchw(n, 3 * heads * d, gh, gw), p.ext_nchw(n, heads * d, gh, gw)
    if case['sliced']:
        x, _ = _source(p, x_ext, 4, 8)
        out, wide = _target(p, n, gh, gw, heads * d, 8, 4)
        assert x.buf.c != x.c and x.coff == 4 and out.buf.c != out.c                                # ld != c on both sides
        y = raw_rp(p, x, out, heads, d, (gh, gw), packed_table(case))
    else:
        out = wide = None
        y = p.attention_relpos(p.to_nhwc(x_ext), heads, (gh, gw), case['rh'], case['rw'])
    p.to_nchw(y, y_ext)
    return p, [_nchw(case['qkv'].reshape(n, gh, gw, -1))], (n, heads * d, gh, gw), (wide, out)


def xa_program(case):
    n, heads, d, Nq, Nk = case['n'], case['heads'], case['d'], case['Nq'], case['Nk']
    c = heads * d
    p = P.Program(case['name'])
    q_ext, k_ext, y_ext = p.ext_nchw(n, c, Nq, 1), p.ext_nchw(n, 2 * c, Nk, 1), p.ext_nchw(n, c, Nq, 1)
    if case['sliced']:
        q, _ = _source(p, q_ext, 4, 8)
        kv, _ = _source(p, k_ext, 8, 4)
        out, wide = _target(p, n, Nq, 1, c, 8, 4)
        y = p._emit(P.OP_CROSS_ATTENTION, q, kv, out, groups=heads, cin_g=d)
    else:
        out = wide = None
        y = p.cross_attention(p.to_nhwc(q_ext, c_pad=c), p.to_nhwc(k_ext, c_pad=2 * c), heads)
    p.to_nchw(y, y_ext)
    return p, [_nchw(case['q'][:, :, None, :]), _nchw(case['kv'][:, :, None, :])], (n, c, Nq, 1), (wide, out)


def window_program(unpart, gh, gw, ws, n, c, res, sliced):
    wy, wx = -(-gh // ws), -(-gw // ws)
    map_shape, win_shape = (n, gh, gw, c), (n * wy * wx, ws * ws, 1, c)
    in_shape, out_shape = (win_shape, map_shape) if unpart else (map_shape, win_shape)
    p = P.Program("window%d" % unpart)
    x_ext = p.ext_nchw(in_shape[0], c, in_shape[1], in_shape[2])
    r_ext = p.ext_nchw(n, c, gh, gw) if unpart and res else None
    y_ext = p.ext_nchw(out_shape[0], c, out_shape[1], out_shape[2])
    x, _ = _source(p, x_ext, 4, 8) if sliced else _source(p, x_ext, 0, 0)
    r = None
    if r_ext is not None:
        r, _ = _source(p, r_ext, 8, 4) if sliced else _source(p, r_ext, 0, 0)
    out, wide = _target(p, *out_shape, 8, 4) if sliced else (p.buffer(*out_shape), None)
    y = p._emit(P.OP_TOKENS, x, r, out, flags=4 if unpart else 3, kh=ws)
    p.to_nchw(y, y_ext)
    return p, tuple(out_shape[i] for i in (0, 3, 1, 2)), (wide, out)


def bcast_program(n, a, b, k, const, sliced):
    an, h, w, c = a.shape
    p = P.Program("bcast")
    a_ext = p.ext_nchw(an, c, h, w)
    b_ext = p.ext_nchw(b.shape[0], c, h, w) if b is not None else None
    y_ext = p.ext_nchw(n, c, h, w)
    av, _ = _source(p, a_ext, 4, 8) if sliced else _source(p, a_ext, 0, 0)
    bv = None
    if b_ext is not None:
        bv, _ = _source(p, b_ext, 8, 4) if sliced else _source(p, b_ext, 0, 0)
    if not sliced:
        y, out, wide = p.broadcast_add(av, bv, k, per_position=const == 'position', n=n), None, None
    else:
        out, wide = _target(p, n, h, w, c, 8, 4)
        y = raw_bcast(p, av, bv, out, k, const == 'position')
    p.to_nchw(y, y_ext)
    return p, (n, c, h, w), (wide, out)


def raw_bcast(p, a, b, out, k, per_position):
    a_h = a_n = -1
    if k is not None:
        k = np.asarray(k, np.float32).reshape(-1)
        a_h, a_n = p._w(k, k)
    return p._emit(P.OP_TOKENS, a, b, out, flags=6 if per_position else 5, aux_off=a_h, nat=dict(aux_off=a_n))


def dot_program(c, positions, n):
    """-> (program, output shape, (the 4-channel buffer the result is channel 0 of, the result view))"""
    p = P.Program("channel_dot")
    x_ext, h_ext, y_ext = p.ext_nchw(n, c, 1, positions), p.ext_nchw(n, c, 1, 1), p.ext_nchw(n, 1, 1, positions)
    y = p.channel_dot(p.to_nhwc(x_ext), p.to_nhwc(h_ext))
    p.to_nchw(y, y_ext)
    return p, (n, 1, 1, positions), (P.T(p, y.buf, 0, y.buf.c), y)


# ---- attention with the decomposed bias -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(5, 13), (14, 14), (3, 21), (1, 2)])
def test_rp_reference_equals_the_restatement(grid):
    gh, gw = grid
    heads, d, B = 2, 8, 2
    E = heads * d
    rng = np.random.default_rng(gh * 100 + gw)
    sd = {'a.qkv.weight': rng.standard_normal((3 * E, E)) / 4, 'a.qkv.bias': 0.1 * rng.standard_normal(3 * E), 'a.proj.weight': np.eye(E),
          'a.proj.bias': np.zeros(E), 'a.rel_pos_h': rng.standard_normal((2 * gh - 1, d)) / 3, 'a.rel_pos_w': rng.standard_normal((2 * gw - 1, d)) / 3}
    x = rng.standard_normal((B, gh, gw, E))
    theirs = _model(sd, heads=heads)._attention(torch.as_tensor(x), 'a.').numpy().reshape(B, gh * gw, E)
    qkv = (x @ sd['a.qkv.weight'].T + sd['a.qkv.bias']).reshape(B, gh * gw, 3 * E)
    qkv[:, :, :E] *= d ** -0.5                                             # the op receives the scaled q
    _pin(C.rp_reference(qkv, heads, d, grid, sd['a.rel_pos_h'], sd['a.rel_pos_w']), theirs)


@pytest.mark.parametrize("grid", C.RP_GRIDS, ids=['%dx%d' % g for g in C.RP_GRIDS])
def test_rp_sweep_cases_have_their_properties(grid):
    gh, gw = grid
    N, TT = gh * gw, 2 * gh - 1 + 2 * gw - 1
    NT = (N + 31) // 32
    assert N == C.RP_NS[C.RP_GRIDS.index(grid)]
    # what the sizes are for
    assert {1: NT == 1, 2: NT == 1, 31: NT == 1, 32: NT == 1 and N % 32 == 0, 33: NT == 2 and N % 32 == 1, 63: NT == 2, 64: NT == 2 and N % 64 == 0,
            65: NT == 3 and N % 64 == 1, 72: NT == 3, 81: NT == 3, 96: NT == 3 and N % 32 == 0, 98: NT == 4, 196: NT == 7, 272: NT == 9,
            289: NT == 10 and N % 32 == 1, 372: NT == 12}[N]
    assert {(8, 9): 32, (9, 9): 34, (16, 17): 64, (17, 17): 66}.get(grid, TT) == TT
    seen = set()
    for name in C.rp_sweep_names(grid):
        case = C.rp_case(name)
        seen.add((case['d'], case['heads'], case['n']))
        assert case['sliced'] == (case['n'] == 2) and case['rh'].shape[0] != 0
        assert case['n'] == 1 or not np.array_equal(case['qkv'][0], case['qkv'][1])
        assert gh != gw or not np.array_equal(case['rh'], case['rw'])
        e32 = C.rp_e32(case)
        print("%-28s e32 %.3g" % (name, e32))
        assert e32 <= C.bound(e32)
        rp_program(case)[0].plan()
    assert seen == {(d, h, b) for d in C.RP_DS for h in (1, 3) for b in (1, 2)}                    # every instantiation, <128> included


def test_rp_sweep_covers_the_tile_boundaries():
    tts = {2 * gh - 1 + 2 * gw - 1 for gh, gw in C.RP_GRIDS}
    assert {32, 34, 64, 66} <= tts                                           # the padded row tile of the prologue and the waves' split of row tiles
    nts = {(gh * gw + 31) // 32 for gh, gw in C.RP_GRIDS}
    assert {1, 2, 3, 4} <= nts and any(t % 2 == 0 for t in nts) and any(t % 2 == 1 for t in nts)
    assert any((gh * gw) % 32 == 0 for gh, gw in C.RP_GRIDS) and any(gh * gw <= 32 for gh, gw in C.RP_GRIDS)
    assert sum(gh != gw for gh, gw in C.RP_GRIDS) >= 8 and any(gh > gw for gh, gw in C.RP_GRIDS)
    assert any(0 < (gh * gw) % 64 <= 32 for gh, gw in C.RP_GRIDS)            # a second query tile without a real query


@pytest.mark.parametrize("grid", C.RP_BIAS_GRIDS, ids=['%dx%d' % g for g in C.RP_BIAS_GRIDS])
def test_rp_bias_only_and_every_planted_index_fault_shows(grid):
    case = C.rp_case('bias_%dx%d' % grid)
    heads, d = case['heads'], case['d']
    assert not case['qkv'][:, :, heads * d:2 * heads * d].any()
    s = C.rp_logits(case['qkv'], heads, d, grid, case['rh'], case['rw'])
    assert 2.0 < s.std() < 6.0                                               # the bias alone, spread over several units
    e32 = C.rp_e32(case)
    lim = C.bound(e32)
    ref = C.rp_ref64(case)
    for fault in C.RP_FAULTS:
        wrong = C.rp_reference(case['qkv'], heads, d, grid, case['rh'], case['rw'], fault=fault)
        moved = C.rp_err(wrong, ref, case)
        print("bias_%dx%d %-12s moves the output by %.3g = %.0f bounds (e32 %.3g)" % (grid + (fault, moved, moved / lim, e32)))
        if fault == 'gh_for_gw' and grid[0] == grid[1]:
            assert moved == 0.0                                              # on a square grid this is no fault
        else:
            assert moved >= 10 * lim, (grid, fault, moved, lim)


@pytest.mark.parametrize("name", C.RP_PEAK_NAMES)
def test_rp_peaked_and_the_leading_key_leads_by_40(name):
    case = C.rp_case(name)
    s = C.rp_logits(case['qkv'], 1, case['d'], case['grid'], case['rh'], case['rw'])[0, 0]
    N = case['N']
    tgt = C.rp_peak_target(name)
    lead = s[np.arange(N), tgt]
    rest = s.copy()
    rest[np.arange(N), tgt] = -np.inf
    assert (lead - rest.max(1) >= C.PEAK_LEAD).all(), (lead - rest.max(1)).min()
    NT, half = 5, 3
    K = C.RP_PEAK_KEYS
    assert N == 150 and K['key0'] == 0 and half * 32 <= K['half1'] < (half + 1) * 32 and (NT - 1) * 32 <= K['last_tile'] < N - 1 == K['last']
    if name == 'peak_mixed':
        assert sorted(tgt.tolist()) == list(range(N))
    bias = s - C.rp_logits(case['qkv'], 1, case['d'], case['grid'], 0 * case['rh'], 0 * case['rw'])[0, 0]
    assert 0.3 < bias.std() < 3.0                                            # a real bias under the peak
    v = case['qkv'][0, :, 2 * case['d']:]
    assert np.abs(C.rp_ref64(case)[0] - v[tgt]).max() <= C.ULP * C.attn_vmax(case)


@pytest.mark.parametrize("name", C.RP_MOTION_NAMES)
def test_rp_running_max_motion_and_every_tile_moves_it(name):
    case = C.rp_case(name)
    s = C.rp_logits(case['qkv'], case['heads'], case['d'], case['grid'], case['rh'], case['rw'])[0]
    tmax = np.stack([s[:, :, t:t + 32].max(-1) for t in range(0, case['N'], 32)], -1)
    step = np.diff(tmax, axis=-1)
    assert (step > 2.0).all() if name == 'max_rising' else (step < -2.0).all(), (step.min(), step.max())
    assert C.rp_e32(case) <= C.bound(C.rp_e32(case))


def test_rp_offset_logits_sit_at_1000():
    case = C.rp_case('offset')
    s = C.rp_logits(case['qkv'], case['heads'], case['d'], case['grid'], case['rh'], case['rw'])
    assert s.min() > 985.0 and s.max() < 1015.0 and (s.max(-1) - s.min(-1)).min() > 2.0
    e32 = C.rp_e32(case)
    print("offset e32 %.3g" % e32)
    assert 1e-6 < e32 <= C.bound(e32)                                         # the rounding of q k + 1000 at an ulp of 6e-5 is the yardstick


@pytest.mark.parametrize("name", C.RP_ISOLATION_NAMES)
def test_rp_isolation_cases(name):
    case = C.rp_case(name)
    fin = np.broadcast_to(case['finite'], (case['n'], case['N'], case['heads'] * case['d']))
    ref = C.rp_ref64(case)
    assert np.isfinite(ref[fin]).all() and np.isnan(ref[~fin]).all() and (~fin).any()
    if name != 'isolation_head':
        assert np.isnan(case['qkv'][1]).all() and case['N'] in (33, 98)
        assert np.array_equal(ref[:1], C.rp_ref64(C.rp_single_sample(case)))
    assert C.rp_e32(case) <= C.bound(C.rp_e32(case))


def test_rp_real_geometries_and_zero_tables():
    a, b = C.rp_case('real_64x64'), C.rp_case('real_windows')
    assert a['grid'] == (64, 64) and a['d'] == 80 and a['n'] == a['heads'] == 1 and 2 * 64 - 1 + 2 * 64 - 1 == 254
    assert b['grid'] == (14, 14) and b['d'] == 80 and b['n'] == 25
    # the LDS request of the largest geometry that ships, and of the refused one (launch_attention_rp_t)
    lds = lambda d, gh, gw: 4 * (4 * 32 * (d + 4) + 128 + 2 * ((2 * gh + 2 * gw - 2 + 31) // 32 * 32) * 32)      # noqa: E731
    assert lds(80, 64, 64) <= 160 * 1024 < lds(32, 150, 150) == 4 * 32 * 36 * 4 + 512 + 2 * 608 * 32 * 4
    for name in C.RP_ZERO_NAMES:
        z = C.rp_case(name)
        assert not z['rh'].any() and not z['rw'].any() and z['d'] in (32, 64, 128)


# ---- cross-attention ------------------------------------------------------------------------------------------------------------------------
def test_xa_reference_equals_the_restatement():
    for heads, d, nq, nk in ((1, 4, 3, 17), (3, 8, 7, 5), (2, 16, 65, 64)):
        c = heads * d
        rng = np.random.default_rng(nq + nk)
        sd = {}
        for nm in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            sd['x.%s.weight' % nm], sd['x.%s.bias' % nm] = np.eye(c), np.zeros(c)
        q, k, v = rng.standard_normal((2, nq, c)), rng.standard_normal((2, nk, c)), rng.standard_normal((2, nk, c))
        theirs = _model(sd, dec_heads=heads)._xattn(torch.as_tensor(q), torch.as_tensor(k), torch.as_tensor(v), 'x').numpy()
        _pin(C.xa_reference(q * d ** -0.5, np.concatenate([k, v], 2), heads, d), theirs)


def test_xa_sweep_covers_every_instantiation_and_both_kernels():
    names = C.xa_sweep_names()
    cases = [C.xa_case(nm) for nm in names]
    assert len(names) == len(set(names)) and 100 <= len(cases) <= 300
    assert {(c['d'], c['Nk']) for c in cases} == {(d, nk) for d in C.XA_DS for nk in C.XA_NKS}       # every d with every Nk
    for d in C.XA_DS:                                                        # both kernels at every head dimension, <2|4|8|64> included
        assert {C.xa_kernel(c['Nk']) for c in cases if c['d'] == d} == {'lane', 'wave'}
    # the switch as launch_xattn_t states it: Nk = 16 is the last length of the lane kernel, 17 the first of the wave kernel
    assert C.xa_kernel(16) == 'lane' and C.xa_kernel(17) == 'wave' and 16 in C.XA_NKS and 17 in C.XA_NKS
    assert {c['Nq'] for c in cases} == set(C.XA_NQS) and {c['heads'] for c in cases} == {1, 3} and {c['n'] for c in cases} == {1, 2}
    # partly idle last blocks: 4 waves per block in the wave kernel, 256 lanes in the lane kernel
    idle = [(c['n'] * c['heads'] * c['Nq']) % (256 if C.xa_kernel(c['Nk']) == 'lane' else 4) != 0 for c in cases]
    assert 2 * sum(idle) >= len(cases)
    assert all(c['sliced'] == (c['n'] == 2) for c in cases)
    worst = 0.0
    for c in cases:
        e32 = C.xa_e32(c)
        worst = max(worst, e32)
        assert e32 <= C.bound(e32)
        xa_program(c)[0].plan()
    print("cross-attention sweep: e32 <= %.3g" % worst)


@pytest.mark.parametrize("name", C.XA_PEAK_NAMES)
def test_xa_peaked(name):
    case = C.xa_case(name)
    s = C.xa_logits(case['q'], case['kv'], 1, case['d'])[0, 0]
    t = C.xa_peak_target(name)
    rest = np.delete(s, t, 1)
    assert (s[:, t] - rest.max(1) >= C.PEAK_LEAD).all() and case['Nk'] == 130 and C.xa_kernel(130) == 'wave'
    K = C.XA_PEAK_KEYS
    assert K['key0'] == 0 and K['key63'] == 63 and K['key64'] == 64 and K['last'] == case['Nk'] - 1       # lane 63's first key, lane 0's second, the last
    assert np.abs(C.xa_ref64(case)[0] - case['kv'][0, t, case['d']:]).max() <= C.ULP * C.attn_vmax(case)


@pytest.mark.parametrize("name", C.XA_MOTION_NAMES)
def test_xa_running_max_motion(name):
    case = C.xa_case(name)
    s = C.xa_logits(case['q'], case['kv'], case['heads'], case['d'])[0]                    # [heads, Nq, Nk]
    sign = 1.0 if name.endswith('rising') else -1.0
    if name.startswith('stride'):
        # a lane's successive keys j, j + 64, j + 128, ...: each raises (lowers) its running maximum by more than 2
        assert case['Nk'] == 200 and (sign * (s[..., 64:] - s[..., :-64]) > 2.0).all()
    elif name.startswith('lanes'):
        # neighbouring lanes end at different maxima: the merge's exp(m_lane - M) is far from 1 for most lanes
        assert case['Nk'] == 200 and (sign * np.diff(s, axis=-1) > 0.25).all() and np.ptp(s, -1).min() > 100.0
    else:
        assert case['Nk'] == 16 and C.xa_kernel(16) == 'lane' and (sign * np.diff(s, axis=-1) > 2.0).all()
    assert C.xa_e32(case) <= C.bound(C.xa_e32(case))


def test_xa_planted_faults_show_and_the_lane_kernel_is_no_fault():
    sweep = [C.xa_case(nm) for nm in C.xa_sweep_names()]
    pick = lambda **kw: next(c for c in sweep if all(c[k] == v for k, v in kw.items()))      # noqa: E731
    first_wave = pick(d=16, Nk=17, heads=3)
    cases = {c['name']: c for c in (first_wave, pick(d=64, Nk=1000, heads=3), pick(d=2, Nk=63, heads=3))}
    cases.update({nm: C.xa_case(nm) for nm in ('lanes_rising', 'lanes_falling', 'stride_rising', 'peak_key63', 'peak_key64', 'peak_last')})
    for fault in C.XA_FAULTS:
        hit = 0
        for nm, c in cases.items():
            if (fault == 'v_head_stride' and c['heads'] == 1) or (fault == 'l_unscaled' and c is first_wave):
                continue                                                     # one head: the two strides are equal
            lim = C.bound(C.xa_e32(c))
            moved = C.xa_err(C.xa_reference(c['q'], c['kv'], c['heads'], c['d'], fault=fault), C.xa_ref64(c), c)
            print("%-28s %-14s %.3g = %.0f bounds" % (nm, fault, moved, moved / lim))
            assert moved >= 10 * lim, (nm, fault, moved, lim)
            hit += 1
        assert hit >= 5
    # the lane kernel's arithmetic beyond 16 keys (one running max / sum over all keys in order) is the reference itself: no fault
    c = first_wave
    s = C.xa_logits(c['q'], c['kv'], c['heads'], c['d'])
    m, l, o = np.full(s.shape[:-1], -3.0e38), 0.0, 0.0
    v = c['kv'].astype(np.float64)[:, :, c['heads'] * c['d']:].reshape(c['n'], 17, 3, 16).transpose(0, 2, 1, 3)
    for j in range(17):
        mn = np.maximum(m, s[..., j])
        alpha, pj = np.exp(m - mn), np.exp(s[..., j] - mn)
        l, o, m = l * alpha + pj, o * alpha[..., None] + pj[..., None] * v[:, :, j][:, :, None, :], mn
    _pin((o / l[..., None]).transpose(0, 2, 1, 3).reshape(c['n'], c['Nq'], 48), C.xa_ref64(c))


def test_xa_isolation_cases():
    for name in C.XA_ISOLATION_NAMES:
        case = C.xa_case(name)
        ref = C.xa_ref64(case)
        assert np.isfinite(ref[0]).all() and np.isnan(ref[1]).all() and C.xa_kernel(case['Nk']) == name.split('_')[1]
        assert np.array_equal(ref[:1], C.xa_ref64(C.xa_single_sample(case)))


# ---- window partition / un-partition ------------------------------------------------------------------------------------------------------
def _torch_partition(x, ws):
    """the lines of sam_restatement.Model.encoder, with a height and a width of their own"""
    B, gh, gw, E = x.shape
    ph, pw = (-gh) % ws, (-gw) % ws
    y = torch.nn.functional.pad(torch.as_tensor(x), (0, 0, 0, pw, 0, ph))
    return y.reshape(B, (gh + ph) // ws, ws, (gw + pw) // ws, ws, E).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, E).numpy()


def _torch_unpartition(xw, ws, n, gh, gw):
    ghp, gwp = gh + (-gh) % ws, gw + (-gw) % ws
    y = torch.as_tensor(xw).reshape(n, ghp // ws, gwp // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(n, ghp, gwp, -1)
    return y[:, :gh, :gw].numpy()


def test_window_references_equal_the_restatement_and_the_planted_faults_show():
    counts = {0: set(), 1: set()}
    shapes = set()
    for gh, gw, ws, n, c, res, sliced in C.window_cases():
        x, xw, r = C.window_input(gh, gw, ws, n, c)
        wy, wx = -(-gh // ws), -(-gw // ws)
        part = C.window_partition_reference(x, ws)
        assert np.array_equal(part, _torch_partition(x, ws).reshape(part.shape))
        un = C.window_unpartition_reference(xw, ws, (n, gh, gw), r if res else None)
        assert np.array_equal(un, _torch_unpartition(xw, ws, n, gh, gw) + (r if res else 0)) and un.dtype == np.float32
        # padded positions are exactly +0.0, and partition followed by un-partition is the identity (plus the residual)
        pad = np.ones((n, wy * ws, wx * ws), bool)
        pad[:, :gh, :gw] = False
        padw = _torch_partition(pad[..., None].astype(np.float32), ws).reshape(part.shape[0], ws * ws) > 0
        assert not part[padw].any() and not np.signbit(part[padw]).any() and padw.sum() == n * (wy * ws * wx * ws - gh * gw)
        assert np.array_equal(C.window_unpartition_reference(part, ws, (n, gh, gw), r if res else None), x + r if res else x)
        for unpart in (0, 1):
            window_program(unpart, gh, gw, ws, n, c, res, sliced)[0].plan()
        counts[0].add(part.size // 4)
        counts[1].add(un.size // 4)
        shapes.add((gh, gw, ws))
        # planted faults: each shows wherever it can (more than one window row and column of different counts; ws > 1; padding)
        for fault in C.WINDOW_FAULTS:
            p2 = C.window_partition_reference(x, ws, fault=fault)
            u2 = C.window_unpartition_reference(xw, ws, (n, gh, gw), r if res else None, fault=fault)
            can = {'wy_wx': wy != wx, 't_div_mod': ws > 1 and gh * gw > 1, 'crop_padded': gw % ws != 0 and gh > 1}[fault]
            if fault != 'crop_padded':
                assert np.array_equal(p2, part) != can, (fault, gh, gw, ws)
            assert np.array_equal(u2, un) != (can and (fault != 'wy_wx' or wy > 1)), (fault, gh, gw, ws)
    assert shapes >= set(C.WINDOW_SHAPES) and set(C.TAIL_COUNTS) <= counts[0] and set(C.TAIL_COUNTS) <= counts[1]
    cs = C.window_cases()
    assert 0.4 <= np.mean([k[-1] for k in cs]) <= 0.6                        # half of them through slices
    for fault, need in (('wy_wx', 2), ('t_div_mod', 6), ('crop_padded', 3)):
        assert sum({'wy_wx': -(-g[0] // g[2]) != -(-g[1] // g[2]), 't_div_mod': g[2] > 1 and g[0] * g[1] > 1,
                    'crop_padded': g[1] % g[2] != 0 and g[0] > 1}[fault] for g in C.WINDOW_SHAPES) >= need


# ---- broadcast add --------------------------------------------------------------------------------------------------------------------------
def test_bcast_cases_cover_the_operand_forms():
    cs = C.bcast_cases()
    assert {(k[0], k[1]) for k in cs} == {(1, 1), (3, 1), (3, 3)} and {(k[0], k[2]) for k in cs} == {(1, 0), (1, 1), (3, 0), (3, 1), (3, 3)}
    assert {k[3] for k in cs} == {None, 'channel', 'position'} and {k[4][0] * k[4][1] for k in cs} == {1, 5, 49} and {k[5] for k in cs} == {4, 68}
    assert {k[6] for k in cs} == {False, True}
    for n, an, bn, const, hw, c, sliced in cs:
        a, b, k = C.bcast_input(n, an, bn, const, hw, c)
        ref = C.bcast_reference(n, a, b, k)
        t = torch.as_tensor(a).expand(n, -1, -1, -1)
        t = t if b is None else t + torch.as_tensor(b)
        t = t if k is None else t + torch.as_tensor(k)
        assert np.array_equal(ref, t.numpy()) and ref.shape == (n, hw[0], hw[1], c)
        assert n == 1 or an == 1 or not np.array_equal(a[0], a[1])
        bcast_program(n, a, b, k, const, sliced)[0].plan()


# ---- channel dot ----------------------------------------------------------------------------------------------------------------------------
def test_dot_reference_and_planted_faults():
    lo, hi = 1.0, 0.0
    for c in C.DOT_CS:
        for positions in C.DOT_POSITIONS:
            for n in (1, 3):
                x, h = C.dot_input(c, positions, n)
                ref = C.dot_reference(x, h)
                _pin(ref[..., 0], np.einsum('bypc,bc->byp', x.astype(np.float64), h[:, 0, 0].astype(np.float64)))
                scale = np.abs(ref).max()
                e32 = C._err(C.dot_reference(x, h, np.float32), ref, scale)
                lo, hi = min(lo, e32), max(hi, e32)
                assert e32 <= C.bound(e32) and (n == 1 or not np.array_equal(h[0], h[1]))
                for fault in C.DOT_FAULTS:
                    if fault == 'h_of_sample_0' and n == 1:
                        continue
                    moved = C._err(C.dot_reference(x, h, fault=fault), ref, scale)
                    assert moved >= 10 * C.bound(e32), (c, positions, n, fault, moved)
                dot_program(c, positions, n)[0].plan()
    print("channel_dot e32 %.3g .. %.3g of max|ref|" % (lo, hi))


# ---- preprocess -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.PRE_SHAPES, ids=['%dx%d_S%d' % s for s in C.PRE_SHAPES])
def test_preprocess_reference_equals_the_restatement_and_planted_faults_show(shape):
    H, W, S = shape
    m = _model(image=S)
    nh, nw = C.preprocess_shape(H, W, S)
    assert (nh, nw) == m.preprocess_shape(H, W) and max(nh, nw) == S
    for kind in ('noise', 'constant'):
        img = C.pre_image(H, W, kind)
        ref = C.preprocess_reference(img, S)
        _pin(ref, m.preprocess(img).numpy()[0])
        assert not ref[:, nh:].any() and not ref[:, :, nw:].any()
        scale = np.abs(ref).max()
        e32 = C._err(C.preprocess_reference(img, S, np.float32), ref, scale)
        print("preprocess %s %s: e32 %.3g of max|ref|, bound %.3g" % (shape, kind, e32, C.bound(e32)))
        assert e32 <= C.bound(e32)
        if kind == 'constant' or (H == S and W == S):
            plain = (np.broadcast_to(img[..., ::-1].astype(np.float64).transpose(2, 0, 1)[:, :1, :1], (3, nh, nw)) if kind == 'constant' else
                     img[..., ::-1].astype(np.float64).transpose(2, 0, 1))
            want = (plain - np.asarray(C.PRE_MEAN)[:, None, None]) / np.asarray(C.PRE_STD)[:, None, None]
            _pin(ref[:, :nh, :nw], want)
    # planted faults, on the noise image
    img = C.pre_image(H, W, 'noise')
    ref = C.preprocess_reference(img, S)
    lim = C.bound(C._err(C.preprocess_reference(img, S, np.float32), ref, np.abs(ref).max()))
    for fault in C.PRE_FAULTS:
        identity = {'align_corners': (H == nh or H == 1) and (W == nw or W == 1), 'scale_from_S': (nh == S or H == 1) and (nw == S or W == 1)}.get(fault, False)
        moved = C._err(C.preprocess_reference(img, S, fault=fault), ref, np.abs(ref).max())
        print("preprocess %s %-13s %.3g = %.0f bounds" % (shape, fault, moved, moved / lim))
        assert moved == 0.0 if identity else moved >= 10 * lim, (shape, fault, moved)
    assert (H, W, S) != (200, 120, 32) or H / nh > 6.0                       # 6 x down: no antialiasing in the definition


# ---- postprocess ----------------------------------------------------------------------------------------------------------------------------
POST_FAULT_CASES = {'xy': (0, 1, 2, 4, 6), 'no_crop': (0, 1, 2, 4, 6, 7), 'scale_from_S': (0, 1, 2, 4, 6, 7)}


@pytest.mark.parametrize("i", range(len(C.POST_SHAPES)))
def test_postprocess_reference_premise_and_planted_faults(i):
    L, S, nh, nw, H, W = C.POST_SHAPES[i]
    low = C.post_logits(i)
    assert low.shape == (3, L, L)
    ref = C.postprocess_reference(low, S, nh, nw, H, W)
    F = torch.nn.functional
    t = F.interpolate(torch.as_tensor(low.astype(np.float64))[:, None], (S, S), mode='bilinear', align_corners=False)[..., :nh, :nw]
    _pin(ref, F.interpolate(t, (H, W), mode='bilinear', align_corners=False)[:, 0].numpy())
    if C.preprocess_shape(H, W, S) == (nh, nw):
        _pin(ref, _model(image=S).full_logits(torch.as_tensor(low.astype(np.float64)), H, W).numpy())
    # the premise of the comparison, on the reference alone
    sure = C.post_sure(ref)
    left_out = 1.0 - sure.mean((1, 2))
    assert (left_out <= C.POST_LEFT_OUT).all(), left_out
    # the float32 restatement of the formula is wrong on no compared pixel and 60 x inside the margin
    r32 = C.postprocess_reference(low, S, nh, nw, H, W, np.float32)
    assert np.array_equal((r32 > 0)[sure], (ref > 0)[sure])
    d32 = (np.abs(r32 - ref).max((1, 2)) / np.abs(ref).max((1, 2))).max()
    assert d32 <= C.POST_MARGIN / 50
    print("postprocess %d: left out <= %.5f, float32 restatement within %.3g of max|ref|" % (i, left_out.max(), d32))
    for fault, where in POST_FAULT_CASES.items():
        wrong = C.postprocess_reference(low, S, nh, nw, H, W, fault=fault)
        flips = min(float(((wrong[k] > 0) != (ref[k] > 0))[sure[k]].mean()) for k in range(3))
        print("postprocess %d %-13s flips %.4f of the compared pixels" % (i, fault, flips))
        if i in where:
            assert flips >= C.POST_FLIP, (i, fault, flips)


def test_postprocess_fault_cases_are_the_ones_that_can_show_them():
    for i, (L, S, nh, nw, H, W) in enumerate(C.POST_SHAPES):
        square = nh == nw == S and H == W
        assert (i in POST_FAULT_CASES['xy']) <= (not square) and (i in POST_FAULT_CASES['no_crop']) <= (nh < S or nw < S)
    assert all(len(v) >= 5 for v in POST_FAULT_CASES.values())


# ---- box tokens -----------------------------------------------------------------------------------------------------------------------------
def test_box_reference_equals_the_restatement_and_planted_faults_show():
    assert {k[0] for k in C.box_cases()} == set(C.BOX_NS) and {k[1] for k in C.box_cases()} == set(C.BOX_CS)
    assert {k[2] for k in C.box_cases()} == set(C.BOX_STATIC) and {k[3] for k in C.box_cases()} == {64, 1024}
    for n, Cc, ns, S, sx, sy in C.box_cases():
        assert sx != sy
        boxes, consts = C.box_input(n, Cc, ns, S)
        assert boxes[0, 0] == boxes[0, 2] and boxes[0, 1] == boxes[0, 3]                          # degenerate
        assert n < 3 or ((boxes[1] < 0).any() and (boxes[2] > S).any())
        ref = C.box_reference(boxes, sx, sy, S, consts, Cc, ns)
        assert ref.shape == (n, Cc, ns + 2, 1)
        sd = {'prompt_encoder.pe_layer.positional_encoding_gaussian_matrix': consts[(ns + 2) * Cc:].reshape(2, Cc // 2),
              'prompt_encoder.point_embeddings.2.weight': consts[ns * Cc:(ns + 1) * Cc][None],
              'prompt_encoder.point_embeddings.3.weight': consts[(ns + 1) * Cc:(ns + 2) * Cc][None]}
        theirs = _model(sd, image=S).box_tokens(boxes.astype(np.float64) * np.asarray([sx, sy, sx, sy])).numpy()          # [n, 2, C]
        mine = ref[:, :, ns:, 0].transpose(0, 2, 1)
        assert np.abs(mine - theirs).max() <= 1e-12 * max(1.0, np.abs(theirs).max()) * 50      # (arguments up to 2 pi * 50: 1e-12 of the argument)
        assert np.array_equal(ref[:, :, :ns, 0], np.broadcast_to(consts[:ns * Cc].reshape(ns, Cc).T.astype(np.float64), (n, Cc, ns)))
        lim = C.ULP * np.maximum(np.abs(ref), 1.0)
        for fault in C.BOX_FAULTS:
            wrong = C.box_reference(boxes, sx, sy, S, consts, Cc, ns, fault=fault)
            if fault == 'corners' and n == 1:
                # one degenerate box: its two corners coincide, only the embeddings tell them apart
                assert np.array_equal(wrong, ref)
                continue
            assert (np.abs(wrong - ref) >= 10 * lim).any(), (n, Cc, ns, S, fault)
            assert np.array_equal(wrong[:, :, :ns], ref[:, :, :ns])
