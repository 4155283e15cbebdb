"""GPU: the Segment Anything kernels of csrc/sam.hip one by one (k_attention_rp<32|64|80|128>, k_xattn_lane / k_xattn_wave<2..64>, k_window,
k_bcast_add, k_channel_dot, k_sam_preprocess, k_sam_postprocess, k_sam_box_tokens) against the plain float64 references of
tests/sam_ops_cases.py, at the edge shapes listed there.  tests/test_sam_ops_references.py pins the same references to the torch
restatement, proves the property each case exists for and the distance of every planted fault, on the CPU.

Every program op runs as a one-op program (ext NCHW -> NHWC -> op -> NCHW) with the workspace and the output NaN-filled beforehand:
whatever the kernel reads outside its view is NaN, whatever it leaves unwritten stays NaN.  The csm_sam_* calls run directly, into
NaN- / sentinel-filled outputs.  Bounds: DESIGN.md 6.6; nothing in one comes from the kernel."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_ops_cases as C  # noqa: E402
import test_sam_ops_references as R  # noqa: E402
from test_tokens_references import _nchw, _nhwc, check_guard  # noqa: E402

from cartoonsegmentation_amd import program as P  # noqa: E402

CSM_OK, CSM_ERR_ARG = 0, 1


def _L():
    from cartoonsegmentation_amd import _lib
    return _lib.load()


def hip_run(prog, ext_in, out_shape, want=()):
    """-> (output NCHW, {view: [n, h, w, C] copy of its whole buffer})"""
    from cartoonsegmentation_amd.runtime import CompiledProgram
    prog.plan()
    cp = CompiledProgram(prog, 'cuda')
    cp.workspace.fill_(float('nan'))
    out = torch.full(out_shape, float('nan'), device='cuda')
    cp.run(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in ext_in], out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), {v: cp.read_view(v).cpu().numpy() for v in want if v is not None}


def refused(prog, what, word):
    """the program's only op is refused with CSM_ERR_ARG before any launch: the workspace is untouched"""
    from cartoonsegmentation_amd._lib import stream_ptr
    from cartoonsegmentation_amd.runtime import CompiledProgram
    L = _L()
    prog.plan()
    cp = CompiledProgram(prog, 'cuda')
    cp.workspace.fill_(float('nan'))
    rc = L.csm_run_program(cp.ops, ctypes.c_int(len(cp.ops)), cp.tensors, ctypes.c_int(len(cp.tensors)), ctypes.c_void_p(cp.weights.data_ptr()),
                           ctypes.c_void_p(cp.workspace.data_ptr()), cp._ext, ctypes.c_int(0), stream_ptr())
    assert rc == CSM_ERR_ARG, (what, rc)
    assert word in L.csm_last_error(), (what, L.csm_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(cp.workspace).all()), what


# ---- attention with the decomposed relative position bias --------------------------------------------------------------------------------
def hip_rp(case):
    p, ext_in, shape, (wide, view) = R.rp_program(case)
    y, views = hip_run(p, ext_in, shape, (wide,))
    if wide is not None:
        check_guard(views[wide], view, _nhwc(y), np.isnan)                # the other channels of the output buffer stay NaN
    return np.ascontiguousarray(_nhwc(y)).reshape(case['n'], case['N'], -1)


def check_rp(case, what='hip'):
    got = hip_rp(case)
    fin = case.get('finite')
    if fin is None:
        assert np.isfinite(got).all(), case['name']
    else:
        full = np.broadcast_to(fin, got.shape)
        assert np.isfinite(got[full]).all() and np.isnan(got[~full]).all(), case['name']
    err, e32 = C.rp_err(got, C.rp_ref64(case), case), C.rp_e32(case)
    print("%s %-28s err %.3g  e32 %.3g  bound %.3g  err / bound %.2f" % (what, case['name'], err, e32, C.bound(e32), err / C.bound(e32)))
    assert err <= C.bound(e32), (case['name'], err, e32)
    return got


@pytest.mark.parametrize("grid", C.RP_GRIDS, ids=['%dx%d' % g for g in C.RP_GRIDS])
def test_attention_relpos_shape_sweep(grid):
    """16 grids (N = 1 .. 372: one key tile with the second half empty, even and odd tile counts, full and partial last tile, a second
    query tile without a real query; TT = 32, 34, 64, 66 around the prologue's row tiles; 11 of them not square) x d 32 / 64 / 80 / 128 x
    1 / 3 heads x batch 1 / 2, Rh and Rw drawn separately; batch 2 reads qkv as channels 4.. of a wider buffer and writes a slice of a
    wider output whose other channels stay NaN"""
    for name in C.rp_sweep_names(grid):
        check_rp(C.rp_case(name))


@pytest.mark.parametrize("name", C.RP_REAL_NAMES)
def test_attention_relpos_real_geometries(name):
    """64 x 64 tokens at d = 80 (TT = 254, the largest LDS request that ships) and one image's 25 windows of 14 x 14 in gridDim.z"""
    check_rp(C.rp_case(name))


@pytest.mark.parametrize("grid", C.RP_BIAS_GRIDS, ids=['%dx%d' % g for g in C.RP_BIAS_GRIDS])
def test_attention_relpos_bias_only(grid):
    """k = 0, tables N(0, 3 / sqrt d): the logits are the bias alone.  Rh <-> Rw, yi - yj -> yj - yi (and x), the query's row / column
    taken with gh for gw and a table row off by one each move the output by > 10^5 bounds (CPU test)"""
    check_rp(C.rp_case('bias_%dx%d' % grid))


@pytest.mark.parametrize("name", C.RP_PEAK_NAMES + C.RP_MOTION_NAMES + ['offset'])
def test_attention_relpos_peaked_moving_maximum_and_offset(name):
    """peak_*: one key leads every query by >= 40 (key 0, the second half's first tile, the partial last tile, N - 1, a permutation):
    the output is that key's v row to 8 ulp.  max_rising / max_falling: every tile moves / the first tile of a half holds the maximum.
    offset: every logit at 1000 +- a few"""
    case = C.rp_case(name)
    got = check_rp(case)
    if name.startswith('peak_'):
        v = case['qkv'][0, :, 2 * case['d']:]
        assert np.abs(got[0] - v[C.rp_peak_target(name)]).max() <= C.FLOOR * C.attn_vmax(case)


@pytest.mark.parametrize("name", C.RP_ISOLATION_NAMES)
def test_attention_relpos_isolates_nan(name):
    """batch 2 with sample 1 NaN at N = 33 and N = 98: sample 0 finite, inside the bound and within it of its single-sample run, sample
    1 NaN; one head NaN out of three: the two others finite and inside the bound"""
    case = C.rp_case(name)
    got = check_rp(case)
    if name != 'isolation_head':
        alone = hip_rp(C.rp_single_sample(case))
        assert np.isfinite(alone).all()
        assert C.rp_err(got[:1], alone.astype(np.float64), C.rp_single_sample(case)) <= C.bound(C.rp_e32(case))


@pytest.mark.parametrize("name", C.RP_ZERO_NAMES)
def test_attention_relpos_with_zero_tables_agrees_with_plain_attention(name):
    case = C.rp_case(name)
    got = check_rp(case)
    n, N, c = got.shape
    p = P.Program("attention")
    x, y = p.ext_nchw(n, 3 * c, N, 1), p.ext_nchw(n, c, N, 1)
    p.to_nchw(p.attention(p.to_nhwc(x), case['heads']), y)
    plain, _ = hip_run(p, [_nchw(case['qkv'][:, :, None, :])], (n, c, N, 1))
    plain = _nhwc(plain)[:, :, 0, :]
    diff = C.rp_err(got, plain.astype(np.float64), case)
    print("%s: relpos with zero tables - plain attention %.3g of max|v|, bit-equal: %s" % (name, diff, np.array_equal(got, plain)))
    assert diff <= C.bound(C.rp_e32(case))


def test_attention_relpos_refuses_what_it_cannot_run_without_a_launch():
    """d = 48, gh gw != N, no table, an unaligned ld, and a grid whose LDS request exceeds 160 KB (150 x 150 at d = 32): CSM_ERR_ARG from
    csm_run_program, the NaN-filled workspace (qkv and the output) untouched"""
    rng = np.random.default_rng(3)
    tab = lambda gh, gw, d: rng.normal(0, 1, (2 * gh - 1 + 2 * gw - 1, d)).astype(np.float32)      # noqa: E731
    for what, (gh, gw), grid, heads, d, table, pad in (('d48', (2, 4), (2, 4), 2, 48, tab(2, 4, 48), 0), ('grid', (3, 4), (3, 5), 1, 32, tab(3, 5, 32), 0),
                                                        ('table', (3, 4), (3, 4), 1, 32, None, 0), ('ld', (3, 4), (3, 4), 1, 32, tab(3, 4, 32), 2),
                                                        ('lds', (150, 150), (150, 150), 1, 32, tab(150, 150, 32), 0)):
        p = P.Program(what)
        x = p.buffer(1, gh, gw, 3 * heads * d + pad).slice(0, 3 * heads * d)
        R.raw_rp(p, x, p.buffer(1, gh, gw, heads * d), heads, d, grid, table)
        refused(p, what, b'attention_relpos')


# ---- cross-attention ------------------------------------------------------------------------------------------------------------------------
def hip_xa(case):
    p, ext_in, shape, (wide, view) = R.xa_program(case)
    y, views = hip_run(p, ext_in, shape, (wide,))
    if wide is not None:
        check_guard(views[wide], view, _nhwc(y), np.isnan)
    return np.ascontiguousarray(_nhwc(y)[:, :, 0, :])


def check_xa(case):
    got = hip_xa(case)
    fin = case.get('finite')
    if fin is None:
        assert np.isfinite(got).all(), case['name']
    else:
        full = np.broadcast_to(fin, got.shape)
        assert np.isfinite(got[full]).all() and np.isnan(got[~full]).all(), case['name']
    err, e32 = C.xa_err(got, C.xa_ref64(case), case), C.xa_e32(case)
    print("hip %-28s %s err %.3g  e32 %.3g  bound %.3g  err / bound %.2f" % (case['name'], C.xa_kernel(case['Nk']), err, e32, C.bound(e32), err / C.bound(e32)))
    assert err <= C.bound(e32), (case['name'], err, e32)
    return got


@pytest.mark.parametrize("d", C.XA_DS)
def test_cross_attention_sweep(d):
    """d x Nk 1 / 2 / 7 / 16 (k_xattn_lane) and 17 / 63 / 64 / 65 / 129 / 1000 (k_xattn_wave; below 64 keys some lanes have none), Nq and the
    head count cycling through 1 / 3 / 7 / 65 and 1 / 3 (a partly idle last block everywhere), batch 1 plain and batch 2 with q, kv and the
    output as slices of wider buffers"""
    names = [nm for nm in C.xa_sweep_names() if nm.startswith('sweep_d%d_' % d)]
    assert len(names) == 2 * len(C.XA_NKS)
    for name in names:
        check_xa(C.xa_case(name))


@pytest.mark.parametrize("name", C.XA_PEAK_NAMES + C.XA_MOTION_NAMES)
def test_cross_attention_peaked_and_moving_maximum(name):
    """peak_*: key 0, 63, 64 or Nk - 1 = 129 leads every query by >= 40: the output is its v row to 8 ulp.  stride_*: a lane's successive
    keys raise (lower) its maximum by 6 each; lanes_*: the logits climb along the key index, the lanes end at different maxima;
    lane_kernel_*: the same inside k_xattn_lane"""
    case = C.xa_case(name)
    got = check_xa(case)
    if name.startswith('peak_'):
        assert np.abs(got[0] - case['kv'][0, C.xa_peak_target(name), case['d']:]).max() <= C.FLOOR * C.attn_vmax(case)


@pytest.mark.parametrize("name", C.XA_ISOLATION_NAMES)
def test_cross_attention_isolates_a_nan_sample(name):
    case = C.xa_case(name)
    got = check_xa(case)
    alone = hip_xa(C.xa_single_sample(case))
    assert np.isfinite(alone).all()
    assert C.xa_err(got[:1], alone.astype(np.float64), C.xa_single_sample(case)) <= C.bound(C.xa_e32(case))


def test_cross_attention_refuses_d3_and_an_empty_operand():
    for what, heads, d, nk in (('d3', 4, 3, 5), ('empty', 1, 16, 0)):
        p = P.Program(what)
        q, kv, out = p.buffer(1, 3, 1, heads * d), p.buffer(1, nk, 1, 2 * heads * d), p.buffer(1, 3, 1, heads * d)
        p._emit(P.OP_CROSS_ATTENTION, q, kv, out, groups=heads, cin_g=d)
        refused(p, what, b'cross_attention')


# ---- window partition / un-partition, broadcast add (exact) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("unpart", [0, 1], ids=['partition', 'unpartition'])
def test_window_ops_equal_the_index_expressions(unpart):
    """(gh, gw, ws) from 1x1/1 to 23x23/14 with 5x13, 13x5, 3x5/7 and 15x1 between, n 1 / 2, c 4 / 68, with and without the residual,
    launches of exactly 255 / 256 / 257 float4s, half of the cases through slices of wider buffers whose other channels stay NaN: exact;
    padded positions exactly +0.0"""
    for gh, gw, ws, n, c, res, sliced in C.window_cases():
        if res and not unpart:
            continue
        x, xw, r = C.window_input(gh, gw, ws, n, c)
        p, shape, (wide, view) = R.window_program(unpart, gh, gw, ws, n, c, res, sliced)
        y, views = hip_run(p, [_nchw(xw), _nchw(r)] if unpart and res else [_nchw(xw if unpart else x)], shape, (wide,))
        ref = C.window_unpartition_reference(xw, ws, (n, gh, gw), r if res else None) if unpart else C.window_partition_reference(x, ws)
        got = _nhwc(y)
        assert np.array_equal(got, ref), (unpart, gh, gw, ws, n, c, res, sliced)
        assert not np.signbit(got[got == 0]).any()
        if sliced:
            check_guard(views[wide], view, ref, np.isnan)


def test_window_partition_then_unpartition_is_the_identity_plus_the_residual():
    for gh, gw, ws in C.WINDOW_SHAPES:
        x, _, r = C.window_input(gh, gw, ws, 2, 68)
        p = P.Program("roundtrip")
        x_ext, r_ext, y_ext = p.ext_nchw(2, 68, gh, gw), p.ext_nchw(2, 68, gh, gw), p.ext_nchw(2, 68, gh, gw)
        xx, rr = p.to_nhwc(x_ext), p.to_nhwc(r_ext)
        p.to_nchw(p.window_unpartition(p.window_partition(xx, ws), ws, xx, res=rr), y_ext)
        y, _ = hip_run(p, [_nchw(x), _nchw(r)], (2, 68, gh, gw))
        assert np.array_equal(_nhwc(y), x + r), (gh, gw, ws)


def test_broadcast_add_equals_float32_numpy():
    """a.n in {1, n}, b absent / batch 1 / batch n, const absent / per channel / per position and channel, n 1 / 3, 1 / 5 / 49 positions,
    c 4 / 68, half through slices: bit-equal to (a + b) + const in float32; an operand batch that is neither 1 nor n is refused"""
    for n, an, bn, const, hw, c, sliced in C.bcast_cases():
        a, b, k = C.bcast_input(n, an, bn, const, hw, c)
        p, shape, (wide, view) = R.bcast_program(n, a, b, k, const, sliced)
        y, views = hip_run(p, [_nchw(a)] + ([_nchw(b)] if b is not None else []), shape, (wide,))
        ref = C.bcast_reference(n, a, b, k)
        assert np.array_equal(_nhwc(y), ref), (n, an, bn, const, hw, c, sliced)
        if sliced:
            check_guard(views[wide], view, ref, np.isnan)
    for an, bn in ((2, 0), (3, 2)):
        p = P.Program("refused")
        a, b, out = p.buffer(an, 1, 5, 4), (p.buffer(bn, 1, 5, 4) if bn else None), p.buffer(3, 1, 5, 4)
        R.raw_bcast(p, a, b, out, None, False)
        refused(p, (an, bn), b'broadcast add')


# ---- channel dot ----------------------------------------------------------------------------------------------------------------------------
def test_channel_dot_vs_float64():
    """c 4 / 8 / 32 / 68 x 1 / 255 / 256 / 257 positions x n 1 / 3 with a different h per sample; channels 1..3 of the output buffer stay NaN"""
    worst = 0.0
    for c in C.DOT_CS:
        for positions in C.DOT_POSITIONS:
            for n in (1, 3):
                x, h = C.dot_input(c, positions, n)
                p, shape, (wide, view) = R.dot_program(c, positions, n)
                y, views = hip_run(p, [_nchw(x), _nchw(h)], shape, (wide,))
                got = _nhwc(y)
                check_guard(views[wide], view, got, np.isnan)
                ref = C.dot_reference(x, h)
                scale = np.abs(ref).max()
                e32, err = C._err(C.dot_reference(x, h, np.float32), ref, scale), C._err(got, ref, scale)
                print("hip channel_dot c %d positions %d n %d: err %.3g  e32 %.3g  bound %.3g" % (c, positions, n, err, e32, C.bound(e32)))
                assert err <= C.bound(e32), (c, positions, n, err, e32)
                worst = max(worst, err / C.bound(e32))
    print("channel_dot: worst err / bound %.2f" % worst)


# ---- csm_sam_preprocess / postprocess / box_tokens ---------------------------------------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def hip_preprocess(img, S):
    from cartoonsegmentation_amd._lib import stream_ptr
    H, W = img.shape[:2]
    nh, nw = C.preprocess_shape(H, W, S)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    out = torch.full((3, S, S), float('nan'), device='cuda')
    rc = _L().csm_sam_preprocess(_ptr(t), ctypes.c_int(H), ctypes.c_int(W), ctypes.c_int(S), ctypes.c_int(nh), ctypes.c_int(nw), _ptr(out), stream_ptr())
    assert rc == CSM_OK
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", C.PRE_SHAPES, ids=['%dx%d_S%d' % s for s in C.PRE_SHAPES])
def test_preprocess_vs_float64(shape):
    """landscape, portrait, 6 x down (no antialiasing), one row, one column, identity and 10 x up, on uint8 white noise and on a constant
    255 image (the Sam class's own nh, nw): inside max(4 e32, 8 ulp) of max|ref| with the float32 source coordinate part of e32; exactly 0
    beyond (nh, nw); at H = W = S and on the constant image (v - mean) / std to 2 ulp"""
    from cartoonsegmentation_amd.sam import Sam
    H, W, S = shape
    nh, nw = C.preprocess_shape(H, W, S)
    assert Sam.preprocess_shape(types.SimpleNamespace(cfg=types.SimpleNamespace(image=S)), H, W) == (nh, nw)
    for kind in ('noise', 'constant'):
        img = C.pre_image(H, W, kind)
        got = hip_preprocess(img, S)
        assert np.isfinite(got).all()
        assert not got[:, nh:].any() and not got[:, :, nw:].any() and not np.signbit(got[:, nh:]).any()
        ref = C.preprocess_reference(img, S)
        scale = np.abs(ref).max()
        e32, err = C._err(C.preprocess_reference(img, S, np.float32), ref, scale), C._err(got, ref, scale)
        print("hip preprocess %s %s: err %.3g  e32 %.3g  bound %.3g  err / bound %.2f" % (shape, kind, err, e32, C.bound(e32), err / C.bound(e32)))
        assert err <= C.bound(e32), (shape, kind, err, e32)
        if kind == 'constant' or (H == S and W == S):
            inside = np.abs(got[:, :nh, :nw] - ref[:, :nh, :nw])
            print("   plain (v - mean) / std: %.2f ulp of max(|ref|, 1)" % (inside / (C.ULP * np.maximum(np.abs(ref[:, :nh, :nw]), 1.0))).max())
            assert (inside <= 2 * C.ULP * np.maximum(np.abs(ref[:, :nh, :nw]), 1.0)).all()


def hip_postprocess(low, S, nh, nw, H, W, fill=7):
    from cartoonsegmentation_amd._lib import stream_ptr
    n, L = low.shape[0], low.shape[-1]
    t = torch.from_numpy(np.ascontiguousarray(low)).cuda()
    out = torch.full((max(n, 1), H, W), fill, dtype=torch.uint8, device='cuda')
    rc = _L().csm_sam_postprocess(_ptr(t), ctypes.c_int(n), ctypes.c_int(L), ctypes.c_int(S), ctypes.c_int(nh), ctypes.c_int(nw), ctypes.c_int(H),
                                  ctypes.c_int(W), _ptr(out), stream_ptr())
    assert rc == CSM_OK
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("i", range(len(C.POST_SHAPES)))
def test_postprocess_vs_float64(i):
    """(L, S, nh, nw, H, W) landscape, portrait, 3 x up, identity, one row, square, narrow and L = 2; three masks of standard normal
    logits: uint8 0 / 1, equal to (float64 resize -> crop -> resize) > 0 wherever |ref| > 1e-4 max|ref| of the mask (premise: at most
    0.005 of a mask left out); all-positive logits give ones, all-negative and all-zero logits zeros; n = 0 writes nothing"""
    L, S, nh, nw, H, W = C.POST_SHAPES[i]
    low = C.post_logits(i)
    ref = C.postprocess_reference(low, S, nh, nw, H, W)
    sure = C.post_sure(ref)
    assert (1.0 - sure.mean((1, 2)) <= C.POST_LEFT_OUT).all()             # the premise, on the reference alone
    got = hip_postprocess(low, S, nh, nw, H, W)
    assert got.dtype == np.uint8 and got.shape == ref.shape and np.isin(got, (0, 1)).all()
    wrong = (got != (ref > 0)) & sure
    print("hip postprocess %d: %d of %d compared pixels differ, %d left out" % (i, wrong.sum(), sure.sum(), (~sure).sum()))
    assert not wrong.any(), (i, int(wrong.sum()))
    assert (hip_postprocess(np.abs(low) + np.float32(1e-3), S, nh, nw, H, W) == 1).all()
    assert (hip_postprocess(-np.abs(low) - np.float32(1e-3), S, nh, nw, H, W) == 0).all()
    assert (hip_postprocess(np.zeros_like(low), S, nh, nw, H, W) == 0).all()      # > 0 is strict
    assert (hip_postprocess(low[:0], S, nh, nw, H, W) == 7).all()


def hip_box_tokens(boxes, sx, sy, S, consts, Cc, ns, expect=CSM_OK):
    from cartoonsegmentation_amd._lib import stream_ptr
    n = boxes.shape[0]
    b = torch.from_numpy(np.ascontiguousarray(boxes.reshape(-1, 4))).cuda() if n else torch.zeros(4, device='cuda')
    k = torch.from_numpy(consts).cuda()
    out = torch.full((max(n, 1), Cc, ns + 2, 1), float('nan'), device='cuda')
    rc = _L().csm_sam_box_tokens(_ptr(b), ctypes.c_int(n), ctypes.c_double(sx), ctypes.c_double(sy), ctypes.c_int(S), _ptr(k), ctypes.c_int(Cc),
                                 ctypes.c_int(ns), _ptr(out), stream_ptr())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_box_tokens_vs_float64():
    """n 1 / 3 / 300 x C 2 / 32 / 256 x 0 / 5 static rows, S 64 / 1024, sx != sy, a degenerate box, negative coordinates and coordinates
    beyond the frame: static rows exact, corner rows within 2^-23 max(|ref|, 1); n = 0 writes nothing; an odd C is refused"""
    worst = 0.0
    for n, Cc, ns, S, sx, sy in C.box_cases():
        boxes, consts = C.box_input(n, Cc, ns, S)
        got = hip_box_tokens(boxes, sx, sy, S, consts, Cc, ns)
        ref = C.box_reference(boxes, sx, sy, S, consts, Cc, ns)
        assert np.isfinite(got).all()
        assert np.array_equal(got[:, :, :ns], ref[:, :, :ns].astype(np.float32))
        ratio = (np.abs(got[:, :, ns:] - ref[:, :, ns:]) / (C.ULP * np.maximum(np.abs(ref[:, :, ns:]), 1.0))).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (n, Cc, ns, S, ratio)
    print("box_tokens: worst corner error %.3f of 2^-23 max(|ref|, 1)" % worst)
    boxes, consts = C.box_input(3, 32, 5, 64)
    assert np.isnan(hip_box_tokens(boxes[:0], 1.0, 1.0, 64, consts, 32, 5)).all()
    assert np.isnan(hip_box_tokens(boxes, 1.0, 1.0, 64, consts[:7 * 31 + 31], 31, 5, expect=CSM_ERR_ARG)).all()
