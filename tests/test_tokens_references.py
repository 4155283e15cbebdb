"""CPU: the oracle's transformer ops (oracle/nets_oracle.c: orc_attention, orc_layernorm, orc_tokens, orc_depth_to_space and the GELU of
orc_act) against the plain float64 references of tests/tokens_cases.py, on every case the GPU tests use -- and, for every case, the
property the case exists for (the leading key leads by 40, every tile raises the maximum, the one-pass variance is 10 x outside the
bound, a wrong table entry moves the bias-only output by more than the bound, the plain float32 evaluation stays inside its own
bound).  Each op is reached through a one-op Program (ext NCHW -> NHWC -> op -> NCHW); the builders here are shared with
tests/test_gpu_tokens.py.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tokens_cases as C  # noqa: E402

from cartoonsegmentation_amd import program as P  # noqa: E402
from oracle import nets as onets  # noqa: E402

ORACLE_ATTENTION = 2.0 ** -24          # double accumulation: one output rounding, in units of max|v|
ORACLE_LAYERNORM = 2.0 ** -23          # in units of max|ref|


# ---- one-op programs ---------------------------------------------------------------------------------------------------------------
def _nchw(x):
    """[n, h, w, c] -> contiguous [n, c, h, w]"""
    return np.ascontiguousarray(np.asarray(x, np.float32).transpose(0, 3, 1, 2))


def _nhwc(y):
    return y.transpose(0, 2, 3, 1)


def _source(p, x_ext, lead, tail):
    """the NHWC copy of an ext tensor: a buffer of its own, or channels lead .. lead + c of one `lead + tail` channels wider"""
    if not lead and not tail:
        return p.to_nhwc(x_ext), None
    wide = p.buffer(x_ext.n, x_ext.h, x_ext.w, x_ext.c + lead + tail)
    x = wide.slice(lead, lead + x_ext.c)
    p.to_nhwc_into(x_ext, x)
    return x, wide


def _target(p, n, h, w, c, lead, tail):
    if not lead and not tail:
        return None, None
    wide = p.buffer(n, h, w, c + lead + tail)
    return wide.slice(lead, lead + c), wide


def raw_attention(p, x, out, heads, d, grid=None, table=None):
    """CSM_OP_ATTENTION as Program.attention emits it, without that method's checks (the refusal tests hand the library shapes the
    lowering never produces)"""
    a_h = a_n = -1
    if table is not None:
        table = np.asarray(table, np.float32)
        a_h, a_n = p._w(np.ascontiguousarray(table.T), table)
    gh, gw = grid if grid is not None else (0, 0)
    return p._emit(P.OP_ATTENTION, x, None, out, groups=heads, cin_g=d, kh=gh, kw=gw, aux_off=a_h, nat=dict(aux_off=a_n))


def attention_program(case):
    """-> (program, [input NCHW], output shape NCHW, wide input buffer or None)"""
    n, N, heads, d = case['n'], case['N'], case['heads'], case['d']
    p = P.Program(case['name'])
    x_ext, y_ext = p.ext_nchw(n, 3 * heads * d, N, 1), p.ext_nchw(n, heads * d, N, 1)
    x, wide = _source(p, x_ext, 4, 8) if case['in_slice'] else _source(p, x_ext, 0, 0)
    assert (x.buf.c != x.c) == case['in_slice']                                                  # ld != c
    p.to_nchw(p.attention(x, heads, case['grid'], case['table']), y_ext)
    return p, [_nchw(case['qkv'][:, :, None, :])], (n, heads * d, N, 1), wide


def layernorm_program(k):
    c, rows = k['c'], k['rows']
    p = P.Program("layernorm")
    x_ext, y_ext = p.ext_nchw(1, c, rows, 1), p.ext_nchw(1, c, rows, 1)
    x, _ = _source(p, x_ext, 4, 4) if k['sliced'] else _source(p, x_ext, 0, 0)
    out, wide = _target(p, 1, rows, 1, c, 8, 4) if k['sliced'] else (None, None)
    p.to_nchw(p.layernorm(x, k['gamma'], k['beta'], k['eps'], out=out), y_ext)
    return p, [_nchw(k['x'][None, :, None, :])], (1, c, rows, 1), (wide, out)


def tokens_program(mode, n, c, grid, sliced, cls=None):
    """the token op with both operands as channel slices of wider buffers when `sliced`"""
    gh, gw = grid
    p = P.Program("tokens%d" % mode)
    in_shape = (n, gh, gw, c) if mode == 0 else (n, gh * gw + 1, 1, c)
    out_shape = (n, gh * gw + 1, 1, c) if mode == 0 else (n, gh, gw, c * (2 if mode == 1 else 1))
    x_ext = p.ext_nchw(in_shape[0], in_shape[3], in_shape[1], in_shape[2])
    y_ext = p.ext_nchw(out_shape[0], out_shape[3], out_shape[1], out_shape[2])
    x, _ = _source(p, x_ext, 4, 8) if sliced else _source(p, x_ext, 0, 0)
    if not sliced:
        y, wide = (p.tokens_assemble(x, cls) if mode == 0 else p.tokens_readout(x, grid, project=mode == 1)), None
    else:
        out, wide = _target(p, *out_shape, 8, 4)
        if mode == 0:
            a_h, a_n = p._w(cls, cls)
            y = p._emit(P.OP_TOKENS, x, None, out, flags=0, aux_off=a_h, nat=dict(aux_off=a_n))
        else:
            y = p._emit(P.OP_TOKENS, x, None, out, flags=mode, kh=gh, kw=gw)
    p.to_nchw(y, y_ext)
    return p, tuple(out_shape[i] for i in (0, 3, 1, 2)), (wide, y)


def depth_to_space_program(n, h, w, k, c, sliced):
    p = P.Program("d2s")
    x_ext, y_ext = p.ext_nchw(n, k * k * c, h, w), p.ext_nchw(n, c, h * k, w * k)
    x, _ = _source(p, x_ext, 4, 8) if sliced else _source(p, x_ext, 0, 0)
    if not sliced:
        y, wide = p.depth_to_space(x, k), None
    else:
        out, wide = _target(p, n, h * k, w * k, c, 8, 4)
        y = p._emit(P.OP_DEPTH_TO_SPACE, x, None, out, stride=k)
    p.to_nchw(y, y_ext)
    return p, (n, c, h * k, w * k), (wide, y)


def gelu_program(rows, act='gelu'):
    """a 1x1 convolution with identity weights and zero bias: the pre-activation is the input itself"""
    p = P.Program("gelu")
    x_ext, y_ext = p.ext_nchw(1, C.GELU_C, rows, 1), p.ext_nchw(1, C.GELU_C, rows, 1)
    y = p.conv(p.to_nhwc(x_ext), np.eye(C.GELU_C, dtype=np.float32).reshape(C.GELU_C, C.GELU_C, 1, 1), np.zeros(C.GELU_C, np.float32), act=act)
    p.to_nchw(y, y_ext)
    return p


def oracle_run(prog, ext_in, out_shape, want=()):
    out = np.zeros(out_shape, np.float32)
    views = onets.run_program(prog, list(ext_in) + [out], [v for v in want if v is not None])
    return out, views


def check_guard(full, view, inside, is_guard):
    """a [n, h, w, C] buffer whose channels view.coff .. + view.c are the op's output: those equal `inside`, the others are untouched"""
    lo, hi = view.coff, view.coff + view.c
    assert np.array_equal(full[..., lo:hi], inside)
    assert is_guard(full[..., :lo]).all() and is_guard(full[..., hi:]).all()


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def oracle_attention(case):
    p, ext_in, shape, _ = attention_program(case)
    y, _ = oracle_run(p, ext_in, shape)
    return np.ascontiguousarray(_nhwc(y)[:, :, 0, :])


def check_attention_result(got, case, what):
    """finite where the inputs are, NaN where they are not, and inside the case's bound against float64; returns (error, e32)"""
    ref, e32 = C.attention_ref64(case), C.attention_e32(case)
    fin = case.get('finite_samples')
    if fin is not None:
        assert np.isfinite(got[fin]).all(), (what, case['name'])
        assert np.isnan(got[fin.stop:]).all(), (what, case['name'])
    else:
        assert np.isfinite(got).all(), (what, case['name'])
    err = C.attention_err(got, ref, case, fin)
    print("%s %-22s err %.3g  e32 %.3g  bound %.3g (of max|v|)" % (what, case['name'], err, e32, C.bound(e32)))
    assert err <= C.bound(e32), (what, case['name'], err, e32)
    return err, e32


def _oracle_attention_case(name):
    case = C.attention_case(name)
    got = oracle_attention(case)
    check_attention_result(got, case, 'oracle')
    assert C.attention_err(got, C.attention_ref64(case), case, case.get('finite_samples')) <= ORACLE_ATTENTION, name
    assert C.attention_e32(case) <= C.bound(C.attention_e32(case))                          # the plain evaluation inside its own bound
    return case, got


@pytest.mark.parametrize("N", C.SWEEP_NS)
def test_attention_oracle_shape_sweep(N):
    for name in C.sweep_names(N):
        case, _ = _oracle_attention_case(name)
        assert case['N'] == N and case['table'] is None
    NT = (N + 31) // 32
    # what the sizes are for: one key tile / two / an odd count / a partial last tile / a partial last query block
    assert {1: NT == 1, 2: NT == 1, 31: NT == 1, 32: NT == 1 and N % 32 == 0, 33: NT == 2 and N % 32 == 1, 63: NT == 2, 64: NT == 2 and N % 64 == 0,
            65: NT == 3 and N % 64 == 1, 96: NT == 3 and N % 32 == 0, 97: NT == 4, 129: NT == 5 and N % 64 == 1}[N]


@pytest.mark.parametrize("name", C.GRID_NAMES)
def test_attention_oracle_grids_with_a_table(name):
    case, _ = _oracle_attention_case(name)
    gh, gw = case['grid']
    # the index statement here against the arithmetic form of include/csm355.h
    idx = C.relative_position_index(gh, gw)
    i, j = np.meshgrid(np.arange(gh * gw), np.arange(gh * gw), indexing='ij')
    assert np.array_equal(idx[1:, 1:], (i // gw - j // gw + gh - 1) * (2 * gw - 1) + (i % gw - j % gw + gw - 1))
    T = case['table'].shape[0]
    assert (idx[0, 1:] == T - 3).all() and (idx[1:, 0] == T - 2).all() and idx[0, 0] == T - 1 and idx.min() == 0 and idx[1:, 1:].max() == T - 4


@pytest.mark.parametrize("name", C.BIAS_NAMES)
def test_attention_oracle_bias_only_and_every_wrong_entry_shows(name):
    case, _ = _oracle_attention_case(name)
    heads, d, grid = case['heads'], case['d'], case['grid']
    assert not case['qkv'][:, :, :heads * d].any()
    assert np.array_equal(case['table'][-3:, 0], np.asarray(C.CLS_BIAS, np.float32))
    lim = C.bound(C.attention_e32(case))
    ref = C.attention_ref64(case)
    true_idx = C.relative_position_index(*grid)
    maps = C.shifted_indices(*grid)
    assert len(maps) >= (3 if grid == (1, 1) else 5)
    for lab, m in maps.items():
        wrong = C.attention_reference(case['qkv'], heads, d, case['table'], grid, index=m)
        rows = (m != true_idx).any(1)                                        # the queries whose bias row the wrong map changes
        assert rows.any()
        moved = np.abs(wrong - ref).reshape(case['n'], case['N'], heads, d).max(-1) / C.attention_vmax(case)      # [n, N, heads]
        assert moved[:, rows].min() > 10 * lim, (name, lab, moved[:, rows].min(), lim)


@pytest.mark.parametrize("name", C.PEAK_NAMES)
def test_attention_oracle_peaked_and_the_leading_key_leads_by_40(name):
    case, got = _oracle_attention_case(name)
    s = C.attention_logits(case['qkv'], case['heads'], case['d'])[0, 0]
    tgt = C.peak_target(name)
    lead = s[np.arange(case['N']), tgt]
    rest = s.copy()
    rest[np.arange(case['N']), tgt] = -np.inf
    assert (lead - rest.max(1) >= C.PEAK_LEAD).all(), (lead - rest.max(1)).min()
    NT, half = 5, 3
    assert case['N'] == 150 and (case['N'] + 31) // 32 == NT
    K = C.PEAK_KEYS
    assert K['key0'] == 0 and 0 < K['tile0'] < 32 and half * 32 <= K['half1'] < (NT - 1) * 32 <= K['last_tile'] < case['N'] - 1 == K['last']
    if name == 'peak_mixed':
        assert sorted(tgt.tolist()) == list(range(case['N']))
    # the output is the leading key's v row
    v = case['qkv'][0, :, 2 * case['d']:]
    assert np.abs(got[0] - v[tgt]).max() <= C.FLOOR * C.attention_vmax(case)


@pytest.mark.parametrize("name", C.MOTION_NAMES)
def test_attention_oracle_running_max_motion_and_every_tile_moves_it(name):
    case, _ = _oracle_attention_case(name)
    s = C.attention_logits(case['qkv'], case['heads'], case['d'])[0]                      # [heads, N, N]
    N = case['N']
    tmax = np.stack([s[:, :, t:t + 32].max(-1) for t in range(0, N, 32)], -1)             # [heads, N, tiles]
    step = np.diff(tmax, axis=-1)
    if name == 'max_rising':
        assert (step > 2.0).all(), step.min()                                             # a rescale by < e^-2 at every tile, in both halves
    else:
        assert (step < -2.0).all(), step.max()                                            # a half's first tile holds its maximum


@pytest.mark.parametrize("name", C.OFFSET_NAMES + C.OTHER_NAMES)
def test_attention_oracle_offsets_and_wide_spread(name):
    case, _ = _oracle_attention_case(name)
    s = C.attention_logits(case['qkv'], case['heads'], case['d'], case['table'], case['grid'])
    if name.startswith('offset_table'):
        assert s.min() > 990.0 and case['table'].min() > 990.0
        if name.endswith('q0'):
            # exact logits: the plain float32 evaluation has nothing to round before the exp, the bound is at its floor
            assert np.array_equal(s, C.attention_logits(case['qkv'], case['heads'], case['d'], case['table'], case['grid'], dtype=np.float32))
            assert C.bound(C.attention_e32(case)) == C.FLOOR
    elif name == 'offset_qk':
        assert s.min() > 2900.0 and np.array_equal(s, np.rint(s))
        assert np.array_equal(s, C.attention_logits(case['qkv'], case['heads'], case['d'], dtype=np.float32))
        assert C.attention_e32(case) < 1e-6                                               # (two separately rounded products: ~ 3000 * 2^-24 * 1.44 = 2.6e-4)
        top2 = np.sort(s, -1)[..., -2:]
        assert ((top2[..., 1] - top2[..., 0]) <= 3).mean() > 0.9                          # several keys compete: the softmax is not one-hot
    else:
        assert ((s.max(-1) - s.min(-1)) > 200.0).all()
        p = np.exp(s - s.max(-1, keepdims=True))
        assert (p < 2.0 ** -149).mean() > 0.5                                             # most probabilities underflow in fp32


@pytest.mark.parametrize("name", C.ISOLATION_NAMES)
def test_attention_oracle_isolation_of_a_nan_sample(name):
    case, got = _oracle_attention_case(name)
    assert np.isnan(case['qkv'][1]).all() and np.isfinite(case['qkv'][0]).all() and case['N'] % 32 == 1
    alone = oracle_attention(C.single_sample(case))
    assert np.array_equal(got[:1], alone)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
def oracle_layernorm(k):
    p, ext_in, shape, (wide, view) = layernorm_program(k)
    y, views = oracle_run(p, ext_in, shape, (wide,))
    got = _nhwc(y)[0, :, 0, :]
    if wide is not None:
        check_guard(views[wide], view, got[None, :, None, :], lambda a: a == 0)
    return got


def check_layernorm_result(got, k, what):
    ref = C.layernorm_reference(k['x'], k['gamma'], k['beta'], k['eps'])
    e32 = C.layernorm_err(C.layernorm_reference(k['x'], k['gamma'], k['beta'], k['eps'], np.float32), ref)
    err = C.layernorm_err(got, ref)
    print("%s layernorm c %d rows %d eps %g: err %.3g  e32 %.3g  bound %.3g (of max|ref|)" % (what, k['c'], k['rows'], k['eps'], err, e32, C.bound(e32)))
    assert err <= C.bound(e32), (what, k['c'], k['rows'], k['eps'], err, e32)
    return err, e32


@pytest.mark.parametrize("c", C.LN_CS)
def test_layernorm_oracle_shapes(c):
    for rows in C.LN_ROWS:
        for eps in C.LN_EPS:
            k = C.layernorm_case(c, rows, eps)
            assert (k['gamma'] == 0).any() and (k['gamma'] < 0).any() and k['sliced'] == (rows % 2 == 1)
            got = oracle_layernorm(k)
            err, e32 = check_layernorm_result(got, k, 'oracle')
            assert err <= ORACLE_LAYERNORM and e32 <= C.bound(e32)
    k = C.layernorm_constant_case(c)
    assert np.array_equal(oracle_layernorm(k), np.broadcast_to(k['beta'], (k['rows'], c)))


def test_layernorm_oracle_large_mean_and_the_one_pass_variance_fails_it():
    """64 rows of mean 1000, sigma 0.9, c = 1028.  Measured: two-pass float32 3.3e-5 of max|ref| (bound 1.3e-4), one-pass 6.8e-2: 520 x
    outside, asserted >= 10 x.  (The two-pass evaluation cannot be "10 x inside" a bound that is 4 x its own error; it is inside.)"""
    k = C.layernorm_offset_case()
    assert abs(k['x'].mean()) / k['x'].std(1).max() >= 1e3 and k['c'] == 1028
    err, e32 = check_layernorm_result(oracle_layernorm(k), k, 'oracle')
    assert err <= ORACLE_LAYERNORM
    ref = C.layernorm_reference(k['x'], k['gamma'], k['beta'], k['eps'])
    one = C.layernorm_err(C.layernorm_reference(k['x'], k['gamma'], k['beta'], k['eps'], np.float32, one_pass=True), ref)
    print("one-pass %.3g, two-pass %.3g, bound %.3g" % (one, e32, C.bound(e32)))
    assert one >= 10 * C.bound(e32)


# ---- token plumbing, depth to space ------------------------------------------------------------------------------------------------
def token_cases():
    """(mode, n, c, grid, sliced): the issue's cross product, then the 255 / 256 / 257-float4 launches"""
    out = [(mode, n, c, grid, (i + mode + n) % 2 == 1) for mode in (0, 1, 2) for n in C.TOKEN_NS for c in C.TOKEN_CS
           for i, grid in enumerate(C.TOKEN_GRIDS)]
    for cnt in C.TAIL_COUNTS:
        out += [(0, 1, 4, (1, cnt - 1), False), (1, 1, 4, (1, cnt), False), (2, 1, 4, (1, cnt), False), (2, 2, 4, (1, cnt), True)]
    return out


def token_float4s(mode, n, c, grid):
    return (n * (grid[0] * grid[1] + 1) if mode == 0 else n * grid[0] * grid[1]) * (2 if mode == 1 else 1) * (c // 4)


def d2s_cases():
    out = [(n, h, w, k, c, (n + k) % 2 == 0) for n in (1, 2) for (h, w) in C.D2S_MAPS for k in C.D2S_KS for c in (4, 68)]
    return out + [(1, 1, cnt, 1, 4, False) for cnt in C.TAIL_COUNTS] + [(2, 1, 257, 2, 4, True)]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tokens_oracle_equals_the_index_expressions(mode):
    counts = set()
    for m, n, c, grid, sliced in token_cases():
        if m != mode:
            continue
        x, cls = C.token_input(mode, n, c, grid)
        assert n == 1 or not np.array_equal(x[0], x[1])
        p, shape, (wide, view) = tokens_program(mode, n, c, grid, sliced, cls)
        y, views = oracle_run(p, [_nchw(x)], shape, (wide,))
        ref = C.tokens_reference(mode, x, grid, cls)
        assert np.array_equal(_nhwc(y), ref), (mode, n, c, grid, sliced)
        if sliced:
            check_guard(views[wide], view, ref, lambda a: a == 0)
        counts.add(token_float4s(mode, n, c, grid))
    assert (set(C.TAIL_COUNTS) <= counts) if mode != 1 else ({2 * t for t in C.TAIL_COUNTS} <= counts)


def test_depth_to_space_oracle_equals_the_index_expression():
    counts = set()
    for n, h, w, k, c, sliced in d2s_cases():
        x = C.depth_to_space_input(n, h, w, k, c)
        p, shape, (wide, view) = depth_to_space_program(n, h, w, k, c, sliced)
        y, views = oracle_run(p, [_nchw(x)], shape, (wide,))
        ref = C.depth_to_space_reference(x, k)
        assert np.array_equal(_nhwc(y), ref), (n, h, w, k, c, sliced)
        if sliced:
            check_guard(views[wide], view, ref, lambda a: a == 0)
        counts.add(n * h * k * w * k * (c // 4))
    assert set(C.TAIL_COUNTS) <= counts
    # the reference itself, element by element on one case
    x = C.depth_to_space_input(1, 3, 5, 2, 4)
    ref = C.depth_to_space_reference(x, 2)
    for y_ in range(3):
        for x_ in range(5):
            for ky in range(2):
                for kx in range(2):
                    assert np.array_equal(ref[0, 2 * y_ + ky, 2 * x_ + kx], x[0, y_, x_, (ky * 2 + kx) * 4:(ky * 2 + kx) * 4 + 4])


# ---- GELU ------------------------------------------------------------------------------------------------------------------------------
def check_gelu_result(got, x, what):
    ref = C.gelu_reference(x)
    g = got.astype(np.float64)
    assert np.isfinite(got).all()
    ratio = np.abs(g - ref) / C.gelu_bound(x)
    print("%s gelu: largest |error| %.3g at x = %.6g, largest error / max(|x|, 1) %.3g" % (what, np.abs(g - ref).max(), x.reshape(-1)[np.abs(g - ref).argmax()],
                                                                                        ratio.max() * C.GELU_REL))
    assert (ratio <= 1.0).all(), (what, x.reshape(-1)[ratio.argmax()], ratio.max())
    lo, hi = x <= -6.0, x >= 6.0
    assert lo.sum() > 3000 and hi.sum() > 3000
    assert (got[lo] <= 0.0).all() and (np.abs(g[lo]) <= C.GELU_REL * np.abs(x[lo].astype(np.float64))).all()
    assert (np.abs(g[hi] - x[hi].astype(np.float64)) <= C.gelu_bound(x[hi])).all()


def oracle_gelu(x, act='gelu'):
    y, _ = oracle_run(gelu_program(x.shape[0], act), [_nchw(x[None, :, None, :])], (1, C.GELU_C, x.shape[0], 1))
    return _nhwc(y)[0, :, 0, :]


def test_gelu_oracle_against_erf_in_float64():
    x = C.gelu_points()
    assert x.size >= 12000 + 16 and x.min() == np.float32(-3e38) and x.max() == np.float32(3e38)
    for v in (1e-30, 1e-40, 20.0, 87.0, 100.0, 1e4):
        assert (x == np.float32(v)).any() and (x == np.float32(-v)).any()
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny                                # a float32 denormal
    # the identity convolution hands the activation the input itself (a -0 arrives as +0: the chain starts from the bias + 0)
    assert np.array_equal(oracle_gelu(x, None), x)
    check_gelu_result(oracle_gelu(x), x, 'oracle')
