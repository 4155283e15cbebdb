"""GPU: the convolution kernels one layer at a time -- the tile families of csrc/conv_mfma.hip / conv_dma.hip / conv_patch.hip with
k_splitk_reduce, k_conv_stem, k_conv_narrow / k_conv_narrow_cb, k_conv_grouped, k_conv_wino and k_conv_wino4 with k_wino4_rowpass --
against the plain float64 references of tests/conv_cases.py: the same bound (max(4 e32, 8 * 2^-23) of max|ref|), the same equality on
the one-hot cases and the same guards as tests/test_conv_references.py holds the oracle to on the CPU.  The oracle is not involved here
(device == oracle bit for bit is tests/test_gpu_nets.py, test_gpu_winograd*.py, test_gpu_grouped.py, test_gpu_residual_epilogue.py).

Every layer runs as a one-layer program with the workspace and the output NaN-filled beforehand: whatever a kernel reads outside its
views is NaN, whatever it leaves unwritten stays NaN, and the other channels of a buffer whose slice it writes must still be NaN.
The tile kernels run once under the built-in rule (no autotuning) and once per family with one forced configuration
(csm_debug_force_conv_cfg; one that cannot run a layer falls back inside the library), the split-K cases with the runs as separate
blocks and walked by one block.  CSM_WINO4_FORM is read once per process: the F(4x4) cases run in whatever form the launcher picks
here and under forms 2, 3 and 6 in one child pytest process each.  Both tile widths of k_conv_grouped are reached through the map widths
(7 and 37); CSM_WINO_VARIANT exists in development builds only."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as C  # noqa: E402
import test_conv_references as R  # noqa: E402

TILE_FAMILIES_OF_CASES = ('direct', 'splitk', 'narrow', 'grouped_bd', 'lowerings')


@pytest.fixture(autouse=True)
def _built_in_rule(monkeypatch):
    """a program's first run would time every tile configuration of every conv: these tests choose the configurations themselves"""
    monkeypatch.setenv("CSM_AUTOTUNE", "0")


def hip_run(b):
    """-> (output NCHW, {whole-buffer view: [n, h, w, C]})"""
    from cartoonsegmentation_amd.runtime import CompiledProgram
    b.prog.plan()
    cp = CompiledProgram(b.prog, 'cuda')
    cp.workspace.fill_(float('nan'))
    out = torch.full(b.out_shape, float('nan'), device='cuda')
    cp.run(*[torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in b.ext_in], out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ({b.guard[0]: cp.read_view(b.guard[0]).cpu().numpy()} if b.guard else {})


def _run_cases(cases, label, cfg=None):
    """every case inside its bound against float64 (or equal), the guard channels still NaN; a failure names the case, the kernel and the
    error in units of the bound"""
    got, worst = [], 0.0
    for k in cases:
        g = R.result_of(k, hip_run, np.isnan)
        worst = max(worst, R.check_case(k, g, 'hip', "%s%s" % (C.variant(k, cfg), '' if cfg is None else ' <- ' + cfg)))
        got.append(g)
    R.summary('hip', label, cases, got)
    print("hip %s: worst error %.3g of its bound" % (label, worst))


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_family_is_inside_the_bound_or_equal(family):
    """direct: M = 63, 9 / 18 chunks, stride 2, dilation 2 / 8, valid, K tails 36 / 40, cout tails 8 / 48 / 169, cin 512; splitk: ksplit 2
    / 4 / 16 by the rule and forced; narrow: cout 1 .. 4; stem: 7x7 s2, 3x3 s2 / s1, the 16x16 s16 patch embedding on odd frames;
    grouped_bd / grouped_valu: cin_g 4 .. 64, both tile widths, ragged and one-pixel maps, the views the vector kernel refuses; f2 / f4:
    one pixel .. 45 x 45 forced, 23 x 23 and 80 x 80 by the rule; lowerings: linear, conv_transpose k 2 / 4; epilogue: every activation x
    res_mode on every class; onehot: the shifted input to the bit.  Views: input / output / residual slices, out is res"""
    _run_cases(C.FAMILIES[family](), family)


def _forced(cfg, serial):
    from cartoonsegmentation_amd import _lib
    L = _lib.load()
    L.csm_debug_force_conv_cfg(C.cfg_table()[cfg]['id'] if cfg is not None else -1)
    L.csm_debug_force_splitk_serial(serial)


@pytest.mark.parametrize("cfg", C.FORCED_CFGS)
def test_tile_kernels_under_one_forced_configuration_per_family(cfg):
    """MFMA, DMA, PATCH, DMA_P, PATCH_P, WS and NARROW: the direct, split-K (parallel and serial), narrow, block-diagonal grouped and
    1x1-lowering cases, their one-hot cases and their rows of the epilogue cross under that family's configuration"""
    cases = [k for f in TILE_FAMILIES_OF_CASES for k in C.FAMILIES[f]()]
    cases += [k for k in C.onehot_cases() if C.variant(k) == 'tile'] + [k for k in C.epilogue_cases() if k['cls'] in ('direct', 'splitk', 'narrow', 'grouped_bd')]
    assert all(C.variant(k) == 'tile' for k in cases)
    names = {k['name'] for k in cases if C.conv_op(C.program(k))['ksplit'] > 1}
    split = [k for k in cases if k['name'] in names]
    assert len(split) >= 30
    try:
        _forced(cfg, -1)
        _run_cases([k for k in cases if k['name'] not in names], cfg, cfg)
        for serial in (0, 1):
            _forced(cfg, serial)
            _run_cases(split, "%s split-K %s" % (cfg, ('parallel', 'serial')[serial]), cfg)
    finally:
        _forced(None, -1)


@pytest.mark.parametrize("serial", [0, 1])
def test_split_k_parallel_and_serial_under_the_built_in_rule(serial):
    split = C.splitk_cases() + [k for k in C.epilogue_cases() if k['cls'] == 'splitk'] + [k for k in C.onehot_cases() if k['name'].startswith('1hot_sk')]
    try:
        _forced(None, serial)
        _run_cases(split, "split-K %s" % ('parallel', 'serial')[serial])
    finally:
        _forced(None, -1)


def test_f4_cases_in_this_process():
    """the F(4x4) cases and the F(4x4) rows of the epilogue cross in the form this process runs them in (the children of
    test_f4_row_split_and_fused_forms: the form CSM_WINO4_FORM names wherever the lowering planned the scratch for it)"""
    cases = C.f4_cases() + [k for k in C.epilogue_cases() if k['cls'] == 'f4']
    assert sum(1 for k in cases if C.program(k).aux is not None) >= 30
    _run_cases(cases, "f4 (CSM_WINO4_FORM=%s)" % os.environ.get("CSM_WINO4_FORM", "unset"))


@pytest.mark.parametrize("form", ["2", "3", "6"])
def test_f4_row_split_and_fused_forms(form):
    """CSM_WINO4_FORM is read once per process: a fresh child pytest per form"""
    e = dict(os.environ, CSM_WINO4_FORM=form)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_f4_cases_in_this_process"], env=e,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "1 passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("S,arith", [(96, 'f4'), (192, 'rule')], ids=["l-96-f4", "l-192-rule"])
def test_rtmdet_with_f4_layers_matches_the_independent_torch_modules(S, arith):
    """the device twin of tests/test_oracle_rtmdet_graph.py's F(4x4) cases: RTMDet-Ins-L with every eligible layer forced to F(4x4) at
    S = 96, and under the shipped rule at S = 192 (the 24 x 24 neck and head layers), against the independent nn.Modules: < 1e-4"""
    import test_oracle_rtmdet_graph as G
    from cartoonsegmentation_amd import synth
    from cartoonsegmentation_amd.nets.rtmdet import RTMDetConfig
    from cartoonsegmentation_amd.runtime import CompiledProgram
    from oracle import segment as oseg
    cfg = RTMDetConfig()
    if arith == 'f4':
        with G.forced('f4'):
            model, rp, _ = G._build(cfg, S)
    else:
        model, rp, _ = G._build(cfg, S)
    assert len(G._f4_maps(rp)) >= (40 if arith == 'f4' else 10)
    x = oseg.det_preprocess(synth.image_u8(S, S, 77), S, cfg, S, S)
    cp = CompiledProgram(rp.prog, 'cuda')
    cp.workspace.fill_(float('nan'))
    cp.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    with torch.no_grad():
        cls_t, reg_t, kern_t, mf_t = model(torch.from_numpy(x))
    got = lambda v: cp.read_view(v).cpu().numpy()[0]                                  # noqa: E731
    nhwc = lambda t: t[0].permute(1, 2, 0).numpy()                                    # noqa: E731
    worst = 0.0
    for lvl, stride in enumerate(cfg.strides):
        worst = max(worst, G._rel(got(rp.cls[lvl]), nhwc(cls_t[lvl].sigmoid())), G._rel(got(rp.reg[lvl]) * np.float32(stride), nhwc(reg_t[lvl])),
                    G._rel(got(rp.kern[lvl]), nhwc(kern_t[lvl])))
    worst = max(worst, G._rel(got(rp.mask_feat)[..., :cfg.num_prototypes], nhwc(mf_t)))
    print("hip rtmdet-l S = %d %s: %d F(4x4) layers, worst relative error %.3g" % (S, arith, len(G._f4_maps(rp)), worst))
    assert worst < 1e-4
