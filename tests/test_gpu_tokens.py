"""GPU: the transformer kernels of csrc/tokens.hip one by one (k_attention on both bias paths, k_layernorm, k_tokens, k_depth_to_space)
and the GELU epilogue of the convolution engine, against the plain float64 references of tests/tokens_cases.py and against the oracle,
at the edge shapes listed there.  tests/test_tokens_references.py proves the same cases (and the property each exists for) on the CPU.

Every op runs as a one-op program with the workspace and the output NaN-filled beforehand: whatever the kernel reads outside its view is
NaN, whatever it leaves unwritten stays NaN."""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tokens_cases as C  # noqa: E402
import test_tokens_references as R  # noqa: E402

from cartoonsegmentation_amd import program as P  # noqa: E402

CSM_ERR_ARG = 1
WINDOW_VS_GATHER = 1e-6                 # of max|out| (tests/test_gpu_dpt_beit.py)


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


class bias_path:
    """0: the LDS window of the table, 1: the gather from global memory (csm_debug_attention_options), restored on exit"""
    def __init__(self, option):
        self.option = option

    def __enter__(self):
        _L().csm_debug_attention_options(ctypes.c_int(self.option))

    def __exit__(self, *exc):
        _L().csm_debug_attention_options(ctypes.c_int(0))


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def hip_attention(case):
    p, ext_in, shape, _ = R.attention_program(case)
    y, _ = hip_run(p, ext_in, shape)
    return np.ascontiguousarray(R._nhwc(y)[:, :, 0, :])


def _check(case, what='hip'):
    """the kernel on one case: inside the bound against float64, and against the oracle (itself within one output rounding of float64)"""
    got = hip_attention(case)
    err, e32 = R.check_attention_result(got, case, what)
    fin = case.get('finite_samples')
    assert C.attention_err(got, R.oracle_attention(case).astype(np.float64), case, fin) <= C.bound(e32) + R.ORACLE_ATTENTION
    return got


@pytest.mark.parametrize("N", C.SWEEP_NS)
def test_attention_shape_sweep(N):
    """N = 1 .. 129 x d 32 / 64 / 128 x 1 / 3 heads x batch 1 / 2 without a table: one key tile (the second key half empty), two, an odd
    count, a partial last tile, a partial last query block; batch 2 reads qkv as a channel slice of a wider buffer (ld != c)"""
    for name in C.sweep_names(N):
        _check(C.attention_case(name))


@pytest.mark.parametrize("name", C.TABLE_NAMES)
def test_attention_with_a_table_on_both_bias_paths(name):
    """every case with a relative position table through the LDS window AND through the global gather: each inside the case's bound
    against float64, the two within 1e-6 of each other.  grid_*: unit logits; bias_*: q = 0, the logits are the table entries (N(0, 3),
    class-token entries +5 / -5 / +3), so one wrong (i, j) -> table index moves the output by > 10 x the bound (asserted on the CPU);
    offset_table*: table + 1000; isolation_table: sample 1 is NaN"""
    case = C.attention_case(name)
    res = []
    for option in (0, 1):
        with bias_path(option):
            res.append(_check(case, 'hip %s' % ('window' if option == 0 else 'gather')))
    fin = case.get('finite_samples') or slice(None)
    print("window - gather %-22s %.3g of max|out|" % (name, np.abs(res[0][fin] - res[1][fin]).max() / np.abs(res[1][fin]).max()))
    assert np.abs(res[0][fin] - res[1][fin]).max() <= WINDOW_VS_GATHER * np.abs(res[1][fin]).max()


@pytest.mark.parametrize("name", C.PEAK_NAMES + C.MOTION_NAMES + ['offset_qk'] + C.OTHER_NAMES)
def test_attention_peaked_moving_maximum_offset_and_spread(name):
    """peak_*: one key leads every query by >= 40 (key 0, first tile, second key half, last partial tile, N - 1, and a permutation):
    the output is that key's v row -- the half merge and the key <-> register-row map.  max_rising / max_falling: every tile raises
    every query's maximum (a rescale per tile) / the first tile of a half holds it (never again).  offset_qk: exact integer logits near
    3000 (the subtraction before the log2 e product).  wide_spread: logit range > 200, most probabilities underflow."""
    case = C.attention_case(name)
    got = _check(case)
    if name.startswith('peak_'):
        v = case['qkv'][0, :, 2 * case['d']:]
        assert np.abs(got[0] - v[C.peak_target(name)]).max() <= C.FLOOR * C.attention_vmax(case)


@pytest.mark.parametrize("name", C.ISOLATION_NAMES)
def test_attention_isolates_a_nan_sample(name):
    """batch 2, sample 1 entirely NaN, N = 33: sample 0 is finite, inside the bound, and within it of the same sample run alone (a
    key row read past N without the clamp lies in sample 1: 0 x NaN in the P V product); sample 1 is NaN"""
    case = C.attention_case(name)
    got = _check(case)
    alone = hip_attention(C.single_sample(case))
    assert np.isfinite(alone).all()
    assert C.attention_err(got[:1], alone.astype(np.float64), case) <= C.bound(C.attention_e32(case))


def test_attention_refuses_what_it_cannot_run_without_a_launch():
    """d = 48, N = 0 and a table whose grid does not match N: an argument error from csm_run_program, the workspace (qkv and the output)
    untouched"""
    from cartoonsegmentation_amd._lib import stream_ptr
    from cartoonsegmentation_amd.runtime import CompiledProgram
    L = _L()
    table = np.random.default_rng(3).normal(0, 1, ((2 * 3 - 1) * (2 * 4 - 1) + 3, 1)).astype(np.float32)
    for what, N, heads, d, grid, tab in (('d48', 8, 2, 48, None, None), ('N0', 0, 1, 32, None, None), ('grid', 12, 1, 32, (3, 4), table)):
        p = P.Program(what)
        x, out = p.buffer(1, N, 1, 3 * heads * d), p.buffer(1, N, 1, heads * d)
        R.raw_attention(p, x, out, heads, d, grid, tab)
        p.plan()
        cp = CompiledProgram(p, 'cuda')
        before = torch.arange(cp.workspace.numel(), dtype=torch.float32, device='cuda') * 0.01 - 1.0
        cp.workspace.copy_(before)
        for option in (0, 1):
            with bias_path(option):
                rc = L.csm_run_program(cp.ops, ctypes.c_int(len(cp.ops)), cp.tensors, ctypes.c_int(len(cp.tensors)),
                                       ctypes.c_void_p(cp.weights.data_ptr()), ctypes.c_void_p(cp.workspace.data_ptr()), cp._ext, ctypes.c_int(0),
                                       stream_ptr())
            assert rc == CSM_ERR_ARG, (what, rc)
            assert b'attention' in L.csm_last_error(), what
        torch.cuda.synchronize()
        assert torch.equal(cp.workspace, before), what


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------
def hip_layernorm(k):
    p, ext_in, shape, (wide, view) = R.layernorm_program(k)
    y, views = hip_run(p, ext_in, shape, (wide,))
    got = R._nhwc(y)[0, :, 0, :]
    if wide is not None:
        R.check_guard(views[wide], view, got[None, :, None, :], np.isnan)
    return got


def _check_layernorm(k):
    got = hip_layernorm(k)
    assert np.isfinite(got).all()
    err, e32 = R.check_layernorm_result(got, k, 'hip')
    assert C.layernorm_err(got, R.oracle_layernorm(k).astype(np.float64)) <= C.bound(e32) + R.ORACLE_LAYERNORM
    return got


@pytest.mark.parametrize("c", C.LN_CS)
def test_layernorm_shapes(c):
    """c = 4 .. 1028 (below / at / above one 256-channel sweep of a wave, and four of them) x rows 1 .. 257 (the 4-row blocks' tail) x eps
    1e-6 / 1e-5 / 1e-12, gamma with zero and negative entries; odd row counts read and write channel slices of wider buffers whose other
    channels stay NaN.  A constant row of 3.0 gives exactly beta."""
    for rows in C.LN_ROWS:
        for eps in C.LN_EPS:
            _check_layernorm(C.layernorm_case(c, rows, eps))
    k = C.layernorm_constant_case(c)
    assert np.array_equal(hip_layernorm(k), np.broadcast_to(k['beta'], (k['rows'], c)))


def test_layernorm_large_mean():
    """mean 1000, sigma 0.9, c = 1028: inside the two-pass bound, which a one-pass E[x^2] - mean^2 misses by a factor > 100 (CPU test)"""
    _check_layernorm(C.layernorm_offset_case())


# ---- token plumbing, depth to space ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tokens_equal_the_index_expressions(mode):
    """assemble / readout project / readout slice, n 1 / 2 (distinct samples), c 4 / 68, grids 1x1 / 3x5 / 7x2, launches of 255 / 256 / 257
    float4s, both operands as slices of wider buffers (the other channels of the output buffer stay NaN): exact"""
    for m, n, c, grid, sliced in R.token_cases():
        if m != mode:
            continue
        x, cls = C.token_input(mode, n, c, grid)
        p, shape, (wide, view) = R.tokens_program(mode, n, c, grid, sliced, cls)
        y, views = hip_run(p, [R._nchw(x)], shape, (wide,))
        ref = C.tokens_reference(mode, x, grid, cls)
        assert np.array_equal(R._nhwc(y), ref), (mode, n, c, grid, sliced)
        if sliced:
            R.check_guard(views[wide], view, ref, np.isnan)


def test_depth_to_space_equals_the_index_expression():
    """k 1 / 2 / 4 on 1x1 and 3x5 maps, n 1 / 2, c 4 / 68, launches of 255 / 256 / 257 float4s, slices on both sides: exact"""
    for n, h, w, k, c, sliced in R.d2s_cases():
        x = C.depth_to_space_input(n, h, w, k, c)
        p, shape, (wide, view) = R.depth_to_space_program(n, h, w, k, c, sliced)
        y, views = hip_run(p, [R._nchw(x)], shape, (wide,))
        ref = C.depth_to_space_reference(x, k)
        assert np.array_equal(R._nhwc(y), ref), (n, h, w, k, c, sliced)
        if sliced:
            R.check_guard(views[wide], view, ref, np.isnan)


# ---- GELU ------------------------------------------------------------------------------------------------------------------------------
def test_gelu_epilogue_equals_the_oracle_and_erf_in_float64():
    """the conv engine's GELU (Abramowitz-Stegun erf on the polynomial expf) behind an identity 1x1 convolution, 12 000 points on
    [-12, 12] and +-0, 1e-30, 1e-40, 20, 87, 100, 1e4, 3e38: bit-equal to the oracle (fmaf-chain contract), within 3.2e-7 max(|x|, 1) of
    float64, finite, <= 0 below -6, x above 6"""
    x = C.gelu_points()
    y, _ = hip_run(R.gelu_program(x.shape[0]), [R._nchw(x[None, :, None, :])], (1, C.GELU_C, x.shape[0], 1))
    got = R._nhwc(y)[0, :, 0, :]
    R.check_gelu_result(got, x, 'hip')
    ref = R.oracle_gelu(x)
    assert np.array_equal(got, ref), "differs from the oracle at x = %r" % x[got != ref][:8]
