"""GPU parity of the convolution epilogues' residual paths against the CPU oracle (oracle.nets.run_program): BIT-EXACT.

The epilogues request a lane's residual values ahead of its stores (csrc/wino4.hip: all of a block's before the first exchange round;
csrc/csm_conv.h::conv_tail: an accumulator's sixteen first) instead of one load next to each store.  The arithmetic per element is
untouched -- bias, res_mode 1 add, activation, res_mode 2 add -- so every case must give the oracle's bits.  Shapes are the smallest at
which the new order can go wrong: ragged and empty squares, a second square in the next sample, views with different pitches, a residual
view that IS the output view, M and cout tails, and every epilogue path a launcher can take (plain, serial and parallel split-K,
persistent, weights-stationary) through the force switches of include/csm355.h."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cartoonsegmentation_amd import program as P  # noqa: E402
from oracle import nets as onets  # noqa: E402
from test_oracle_winograd4 import forced  # noqa: E402

MODE_ACT = [(m, a) for m in (1, 2) for a in ('relu', 'silu', 'prelu')]
IDS = ["res%d-%s" % ma for ma in MODE_ACT]


def _run_both(prog, ext):
    """ext: the program's external tensors in creation order, outputs as shapes (tuples) -> (oracle outputs, device outputs)"""
    from cartoonsegmentation_amd.runtime import CompiledProgram
    host = [np.zeros(e, np.float32) if isinstance(e, tuple) else np.ascontiguousarray(e) for e in ext]
    onets.run_program(prog, host)
    cp = CompiledProgram(prog, 'cuda')
    dev = [torch.full(e, float('nan'), device='cuda') if isinstance(e, tuple) else torch.from_numpy(np.ascontiguousarray(e)).cuda() for e in ext]
    cp.run(*dev)
    torch.cuda.synchronize()
    outs = [i for i, e in enumerate(ext) if isinstance(e, tuple)]
    return [host[i] for i in outs], [dev[i].cpu().numpy() for i in outs], (cp, dev, outs)


def _params(rng, cin, cout, k, act, groups=1):
    wt = (rng.standard_normal((cout, cin // groups, k, k)) / np.sqrt(k * k * cin // groups)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    slope = rng.uniform(0.05, 0.3, cout).astype(np.float32) if act == 'prelu' else None
    return wt, b, slope


def _same(yo, yd):
    assert np.isfinite(yd).all() and np.array_equal(yd, yo), "max abs diff %g in %d values" % (np.abs(yd - yo).max(), (yd != yo).sum())


# ---- F(4x4), fused form and row-split forms -------------------------------------------------------------------------------------------

def _f4_plain(res_mode, act, n, h, w, cin, cout, seed):
    rng = np.random.default_rng(seed)
    with forced('f4'):
        p = P.Program("res_f4")
        x_ext = p.ext_nchw(n, cin, h, w); y_ext = p.ext_nchw(n, cout, h, w); r_ext = p.ext_nchw(n, cout, h, w)
        wt, b, slope = _params(rng, cin, cout, 3, act)
        y = p.conv(p.to_nhwc(x_ext), wt, b, pad=1, act=act, slope=slope, res=p.to_nhwc(r_ext), res_mode=res_mode)
        p.to_nchw(y, y_ext)
    assert [o['flags'] for o in p.ops if o['kind'] == P.OP_CONV] == [P.CONV_FLAG_WINOGRAD4]
    return p, [rng.standard_normal((n, cin, h, w)).astype(np.float32), (n, cout, h, w), rng.standard_normal((n, cout, h, w)).astype(np.float32)]


@pytest.mark.parametrize("res_mode,act", MODE_ACT, ids=IDS)
def test_f4_fused_ragged_squares_odd_square_count(res_mode, act):
    """3 x 17 x 19: four squares of 16 x 16 pixels per sample, three of them ragged.  Twelve squares are an even count, so the case with
    an empty second square in the last block is the second shape: 3 x 33 x 16 has three squares per sample, nine in all, and blocks
    1 and 3 hold the last square of one sample and the first of the next"""
    p, ext = _f4_plain(res_mode, act, 3, 17, 19, 32, 64, 100 + res_mode)
    (yo,), (yd,), _ = _run_both(p, ext)
    _same(yo, yd)
    p, ext = _f4_plain(res_mode, act, 3, 33, 16, 32, 64, 200 + res_mode)      # nine squares: the last block's second square is empty
    (yo,), (yd,), _ = _run_both(p, ext)
    _same(yo, yd)


@pytest.mark.parametrize("res_mode,act", MODE_ACT, ids=IDS)
def test_f4_fused_residual_and_output_are_slices_with_different_pitches(res_mode, act):
    """2 x 13 x 37, 64 -> 128: the residual is channels [32, 160) of a 160-channel tensor, the output channels [64, 192) of a 192-channel
    buffer whose first 64 channels a 1x1 conv fills (ldr = 160, ldo = 192)"""
    rng = np.random.default_rng(300 + res_mode)
    n, h, w, cin, cout = 2, 13, 37, 64, 128
    with forced('f4'):
        p = P.Program("res_f4_slices")
        x_ext = p.ext_nchw(n, cin, h, w); y_ext = p.ext_nchw(n, cout + 64, h, w); r_ext = p.ext_nchw(n, cout + 32, h, w)
        x = p.to_nhwc(x_ext); rw = p.to_nhwc(r_ext)
        cat = p.buffer(n, h, w, cout + 64)
        wt, b, slope = _params(rng, cin, cout, 3, act)
        p.conv(x, wt, b, pad=1, act=act, slope=slope, res=rw.slice(32, 32 + cout), res_mode=res_mode, out=cat.slice(64, 64 + cout))
        p.conv(x, (rng.standard_normal((64, cin, 1, 1)) / 8).astype(np.float32), None, out=cat.slice(0, 64))
        p.to_nchw(cat, y_ext)
    assert sum(1 for o in p.ops if o['flags'] & P.CONV_FLAG_WINOGRAD4) == 1
    (yo,), (yd,), _ = _run_both(p, [rng.standard_normal((n, cin, h, w)).astype(np.float32), (n, cout + 64, h, w),
                                    rng.standard_normal((n, cout + 32, h, w)).astype(np.float32)])
    _same(yo, yd)


@pytest.mark.parametrize("kind", ["f4", "direct"])
@pytest.mark.parametrize("res_mode,act", MODE_ACT, ids=IDS)
def test_residual_view_that_is_the_output_view(kind, res_mode, act):
    """out = res (the same view): a lane reads exactly the elements it writes, so the early loads see the values the late ones saw"""
    rng = np.random.default_rng(400 + res_mode)
    n, h, w, cin, cout = 2, 21, 18, 32, 64
    with forced(kind):
        p = P.Program("res_inplace")
        x_ext = p.ext_nchw(n, cin, h, w); y_ext = p.ext_nchw(n, cout, h, w); r_ext = p.ext_nchw(n, cout, h, w)
        r = p.to_nhwc(r_ext)
        wt, b, slope = _params(rng, cin, cout, 3, act)
        p.conv(p.to_nhwc(x_ext), wt, b, pad=1, act=act, slope=slope, res=r, res_mode=res_mode, out=r)
        p.to_nchw(r, y_ext)
    assert [bool(o['flags'] & P.CONV_FLAG_WINOGRAD4) for o in p.ops if o['kind'] == P.OP_CONV] == [kind == 'f4']
    (yo,), (yd,), _ = _run_both(p, [rng.standard_normal((n, cin, h, w)).astype(np.float32), (n, cout, h, w),
                                    rng.standard_normal((n, cout, h, w)).astype(np.float32)])
    _same(yo, yd)


@pytest.mark.parametrize("res_mode,act", MODE_ACT, ids=IDS)
def test_f4_small_map_layer(res_mode, act):
    """1 x 9 x 9, 32 -> 64: one block tile, so the lowering gives the op the row-split forms' scratch and the launcher may run
    k_wino4_rowpass (whatever form it picks here; test_f4_row_split_forms forces forms 2 and 3 on this test)"""
    p, ext = _f4_plain(res_mode, act, 1, 9, 9, 32, 64, 500 + res_mode)
    assert [o['scratch'] >= 0 for o in p.ops if o['kind'] == P.OP_CONV] == [True]
    (yo,), (yd,), _ = _run_both(p, ext)
    _same(yo, yd)


@pytest.mark.parametrize("form", ["2", "3"])
def test_f4_row_split_forms(form):
    """CSM_WINO4_FORM is read once per process: the small-map cases above in a child per form"""
    e = dict(os.environ, CSM_WINO4_FORM=form)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_f4_small_map_layer"], env=e,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "%d passed" % len(MODE_ACT) in r.stdout and "failed" not in r.stdout


# ---- direct kernels: every tile configuration x every split-K execution ---------------------------------------------------------------

DIRECT_LAYERS = [
    # n, h, w, cin, cout, k
    (1, 7, 9, 64, 96, 1),          # M = 63: a tail in every M tile; 96 channels: a tail in every 64- and 128-wide N tile
    (2, 5, 6, 32, 32, 3),          # 9 chunks: ksplit 4 cuts them into runs of 2, 2, 2 and 3
    # two channel blocks (the patch kernels switch patch stages inside a tile; 18 chunks: the run boundary of ksplit 2 falls on the block
    # boundary, those of ksplit 4 at chunks 4, 9 and 13 -- inside a block and on the boundary); 17 wide: a ragged 16- and 8-pixel tile
    # column; 96 channels: a tail in every 64- and 128-wide N tile
    (1, 9, 17, 64, 96, 3),
]
DIRECT_IDS = ["1x1_64to96", "3x3_32to32", "3x3_64to96"]
# (with ksplit 1 and 2 the serial fold only ever takes its first-run branch; the 1x1 layer has two chunks, so no ksplit 4 there)
DIRECT_CASES = [(layer, ks) for layer in DIRECT_LAYERS for ks in (1, 2, 4) if ks <= layer[5] * layer[5] * (layer[3] // 32)]
DIRECT_CASE_IDS = ["%s-%d" % (DIRECT_IDS[DIRECT_LAYERS.index(layer)], ks) for layer, ks in DIRECT_CASES]


@pytest.mark.parametrize("layer,ksplit", DIRECT_CASES, ids=DIRECT_CASE_IDS)
@pytest.mark.parametrize("res_mode,act", MODE_ACT, ids=IDS)
def test_direct_kernels_every_epilogue_path(res_mode, act, layer, ksplit):
    """every configuration of the tile table (families MFMA, DMA, PATCH, DMA_P, PATCH_P, WS, NARROW; one that cannot run the layer falls
    back) with K in one run (plain epilogue), cut in two and cut in four (blocks + k_splitk_reduce, and the serial walk of one block:
    only with more than two runs does its fold add to a running total)"""
    from cartoonsegmentation_amd import _lib
    from cartoonsegmentation_amd.runtime import conv_cfg_table
    n, h, w, cin, cout, k = layer
    rng = np.random.default_rng(600 + 10 * k + res_mode)
    p = P.Program("res_direct")
    p.winograd = False
    p.choose_ksplit = lambda M, N, T, groups: ksplit
    x_ext = p.ext_nchw(n, cin, h, w); y_ext = p.ext_nchw(n, cout, h, w); r_ext = p.ext_nchw(n, cout, h, w)
    wt, b, slope = _params(rng, cin, cout, k, act)
    y = p.conv(p.to_nhwc(x_ext), wt, b, pad=k // 2, act=act, slope=slope, res=p.to_nhwc(r_ext), res_mode=res_mode)
    p.to_nchw(y, y_ext)
    assert [(o['flags'], o['ksplit']) for o in p.ops if o['kind'] == P.OP_CONV] == [(0, ksplit)]
    L = _lib.load()
    try:
        L.csm_debug_force_conv_cfg(0)
        L.csm_debug_force_splitk_serial(0)
        (yo,), (yd,), (cp, dev, outs) = _run_both(p, [rng.standard_normal((n, cin, h, w)).astype(np.float32), (n, cout, h, w),
                                                      rng.standard_normal((n, cout, h, w)).astype(np.float32)])
        _same(yo, yd)
        ref = torch.from_numpy(yo).cuda()
        wrong = []
        for cfg in [c['id'] for c in conv_cfg_table()]:
            L.csm_debug_force_conv_cfg(cfg)
            for ser in ((0, 1) if ksplit > 1 else (0,)):
                L.csm_debug_force_splitk_serial(ser)
                dev[outs[0]].fill_(float('nan'))
                cp.run(*dev)
                if not torch.equal(dev[outs[0]], ref):
                    wrong.append((cfg, ser))
        assert not wrong, "(tile configuration, serial split-K) that differ from the oracle: %s" % wrong
    finally:
        L.csm_debug_force_conv_cfg(-1)
        L.csm_debug_force_splitk_serial(-1)


@pytest.mark.parametrize("res_mode,act", MODE_ACT, ids=IDS)
def test_grouped_vector_kernel(res_mode, act):
    """1 x 6 x 7, four groups of 8 channels on k_conv_grouped: ragged tile, the rolled general epilogue with its one-pixel-ahead fetch"""
    rng = np.random.default_rng(700 + res_mode)
    n, h, w, cg, groups = 1, 6, 7, 8, 4
    c = cg * groups
    old = P.Program.grouped_valu
    P.Program.grouped_valu = True
    try:
        p = P.Program("res_grouped")
        x_ext = p.ext_nchw(n, c, h, w); y_ext = p.ext_nchw(n, c, h, w); r_ext = p.ext_nchw(n, c, h, w)
        wt, b, slope = _params(rng, c, c, 3, act, groups=groups)
        y = p.conv(p.to_nhwc(x_ext), wt, b, pad=1, groups=groups, act=act, slope=slope, res=p.to_nhwc(r_ext), res_mode=res_mode)
        p.to_nchw(y, y_ext)
    finally:
        P.Program.grouped_valu = old
    assert [bool(o['flags'] & P.CONV_FLAG_GROUPED) for o in p.ops if o['kind'] == P.OP_CONV] == [True]
    (yo,), (yd,), _ = _run_both(p, [rng.standard_normal((n, c, h, w)).astype(np.float32), (n, c, h, w), rng.standard_normal((n, c, h, w)).astype(np.float32)])
    _same(yo, yd)
