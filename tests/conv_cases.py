"""Case generators, plain references and one-layer programs for the convolutions on the matrix pipe and their vector-pipe relatives
(Program.conv / linear / conv_transpose_nonoverlap -> csrc/conv_mfma.hip, conv_dma.hip, conv_patch.hip, k_conv_stem, k_conv_narrow,
k_splitk_reduce, csrc/grouped.hip, csrc/wino.hip, csrc/wino4.hip), one layer at a time.  The conventions are those of
tests/netops_cases.py, whose helpers (act64, act32, bound, rel_err, the slice builders) are imported, not restated.

Reference: CPU torch F.conv2d (F.conv_transpose2d) in float64 on the NATURAL weights with stride, pad, dilation and groups, then in
float64 bias, the res_mode 1 add, the activation, the res_mode 2 add.  Nothing comes from the oracle, from Program or from the library.

Yardstick: |got - f64| <= max(4 e32, 8 * 2^-23) * max|ref|, e32 = the error against float64 of the PLAIN
FLOAT32 EVALUATION of the same formula in the straightforward order:
  * direct-chain classes (direct, split-K, stem, narrow, grouped, the 1x1 lowerings): an im2col accumulation, taps row-major, channels
    ascending, one rounded multiply and one rounded add per term (direct32) -- not torch's float32 conv, whose order depends on the
    backend and the thread count;
  * F(2x2) and F(4x4): the Winograd formula itself, V = B^T d B, M = sum_c U * V (channels ascending), Y = A^T M A, every operation
    rounded to float32, U from program.wino_transform / wino4_transform (wino32): the contract's own arithmetic is the yardstick there.
One-hot weights (one (ci, ky, kx) per output channel, no bias, an exact activation) must reproduce the shifted, zero-padded input
EXACTLY on the direct-chain classes: every tap, pad, stride phase, dilation step and group assignment with no tolerance at all.

program(case) lowers a case to ext NCHW -> NHWC [a channel slice of a wider buffer] -> conv -> NCHW; variant(case, cfg) names the kernel
it selects (the op's flags; for the tile families the host-only csm_debug_conv_resolve_cfg).  tests/test_conv_references.py holds the
oracle to the references on a machine without a GPU and proves what each family exists for; tests/test_gpu_conv.py runs the HIP kernels
on the same cases.  All generators are seeded."""
import contextlib
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

from cartoonsegmentation_amd import program as P

import netops_cases as N
from netops_cases import EXACT_ACTS, Built, act32, act64, bound, f32, f64, nchw, nhwc, rel_err  # noqa: F401  (re-exported to the tests)

ACTS = (None, 'relu', 'silu', 'prelu', 'hsigmoid', 'sigmoid', 'softplus', 'gelu')            # every activation of program.ACT
assert {P.ACT[a] for a in ACTS} == set(P.ACT.values())
TILE_FAMILIES = ('MFMA', 'DMA', 'PATCH', 'DMA_P', 'PATCH_P', 'WS', 'NARROW')
# one configuration per tile family that the GPU test forces on every direct case (names of csrc/csm_convcfg.h; one that cannot run a
# layer falls back inside the library, resolve_cfg says where to)
FORCED_CFGS = ('64x64', 'D64x64', 'P64x64', 'Q64x64', 'R64x64', 'W256x32', 'NARROW')


# ---- activations: netops_cases' plus gelu ----------------------------------------------------------------------------------------------
def _act(y, act, slope, dtype):
    if act == 'gelu':                                                      # torch's exact (erf) gelu on the CPU in `dtype`
        return F.gelu(torch.from_numpy(np.ascontiguousarray(y, dtype))).numpy()
    return (act64 if dtype is f64 else act32)(y, act, slope)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def out_size(i, k, stride, pad, dil):
    return (i + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _case(family, name, n, hw, cin, cout, k=3, stride=1, pad=None, dil=1, groups=1, act=None, res_mode=0, bias=True, values='normal',
          in_slice=None, out_slice=None, res_slice=None, inplace=False, lower='direct', ksplit=None, valu=None, max_cg=None, onehot=None,
          op='conv'):
    """values: 'normal' N(0, 1) inputs, weights N(0, 1 / K); 'relu' non-negative inputs max(N(0, 1), 0) + 0.5 (post-ReLU with a DC
    offset); 'spread' weights times 10^U(-2, 2).  lower: 'direct' / 'f2' / 'f4' forced, 'rule' the shipped rule.  ksplit: None = what
    choose_ksplit gives.  valu / max_cg: Program.grouped_valu and GROUPED_VALU_MAX_CG for this lowering.  op: 'conv', 'linear', 'convT'"""
    rng = N._rng('conv', name)
    h, w = hw
    pad = dil * (k // 2) if pad is None else pad
    cin_g = cin // groups
    x = rng.normal(0.0, 1.0, (n, h, w, cin))
    if values == 'relu':
        x = np.maximum(x, 0.0) + 0.5
    if op == 'convT':                                                      # w [cin, cout, k, k], stride k
        wt = rng.normal(0.0, 1.0, (cin, cout, k, k)) / np.sqrt(cin)
        ho, wo = h * k, w * k
    else:
        wt = rng.normal(0.0, 1.0, (cout, cin_g, k, k)) / np.sqrt(k * k * cin_g)
        ho, wo = out_size(h, k, stride, pad, dil), out_size(w, k, stride, pad, dil)
    if values == 'spread':
        wt = wt * 10.0 ** rng.uniform(-2.0, 2.0, wt.shape)
    if onehot is not None:                                                 # output channel co reads tap (co + off) % taps of one channel
        taps = k * k
        co = np.arange(cout)
        tap, ci = (co + onehot) % taps, (5 * co + co // taps + onehot // taps) % cin_g
        wt = np.zeros((cout, cin_g, k, k))
        wt[co, ci, tap // k, tap % k] = 1.0
        bias, res_mode = False, 0
        assert act in EXACT_ACTS
    assert ho >= 1 and wo >= 1
    return dict(kind='conv', family=family, name=name, x=x.astype(f32), w=wt.astype(f32), b=rng.normal(0.0, 1.0, cout).astype(f32) if bias else None,
                k=k, stride=stride, pad=pad, dil=dil, groups=groups, act=act, slope=rng.uniform(0.05, 0.5, cout).astype(f32) if act == 'prelu' else None,
                res=rng.normal(0.0, 1.0, (n, ho, wo, cout)).astype(f32) if res_mode else None, res_mode=res_mode, in_slice=in_slice,
                out_slice=out_slice, res_slice=res_slice, inplace=inplace, lower=lower, ksplit=ksplit, valu=valu, max_cg=max_cg, onehot=onehot, op=op,
                exact=onehot is not None)


def _cycle(i):
    """(act, res_mode, bias) that change from case to case"""
    return dict(act=ACTS[i % 4], res_mode=(i // 2) % 3, bias=i % 3 != 2)


VIEWS = dict(in_sl=dict(in_slice=(4, 8)), out_sl=dict(out_slice=(8, 4)), res_sl=dict(res_slice=(4, 12), res_mode=1),
             inplace=dict(inplace=True, res_mode=2), inplace_sl=dict(inplace=True, res_mode=1, res_slice=(8, 4)))
# output views that are not 16-byte aligned at every pixel: channel offset 2, and a buffer of c + 6 channels (32 + 6 = 38)
ODD_VIEWS = dict(off2=dict(out_slice=(2, 6)), ld6=dict(out_slice=(4, 2)), off2_res=dict(out_slice=(2, 6), res_slice=(2, 6), res_mode=1))
VALUES = ('relu', 'spread')


@functools.lru_cache(maxsize=None)
def direct_cases():
    """K in one run (ksplit forced to 1) on the tile kernels.  The three shapes of test_gpu_residual_epilogue.py::DIRECT_LAYERS: M = 63
    (a tail in every M tile), 9 and 18 chunks, 17 wide, cout 96 (a tail in every 64- and 128-wide N tile)"""
    c = lambda name, *a, **kw: _case('direct', name, *a, **dict(dict(ksplit=1), **kw))
    out = [c('d_1x1_m63', 1, (7, 9), 64, 96, k=1, act='relu'),
           c('d_3x3_9', 2, (5, 6), 32, 32, act='silu', res_mode=2),
           c('d_3x3_18', 1, (9, 17), 64, 96),
           c('d_s2', 2, (9, 17), 32, 48, stride=2, act='relu', res_mode=1),                # cout tail 48
           c('d_1x1_s2', 1, (9, 17), 32, 64, k=1, stride=2),
           c('d_dil2', 1, (11, 13), 32, 64, dil=2, act='relu'),                            # ISNet: pad = dilation
           c('d_dil8', 1, (19, 17), 32, 32, dil=8, act='prelu'),
           c('d_valid', 1, (9, 17), 32, 64, pad=0, act='silu'),
           c('d_cin36', 1, (7, 9), 36, 64, act='relu'),                                    # a K tail inside a 32-chunk
           c('d_cin40', 2, (7, 9), 40, 8, res_mode=1),                                     # and the cout tail 8
           c('d_cout169', 1, (5, 6), 32, 169, k=1, act='relu'),
           c('d_cin512', 1, (5, 6), 512, 64, act='relu', bias=False),
           c('d_5x5', 1, (9, 11), 32, 32, k=5, act='relu'),
           c('d_n3', 3, (5, 7), 64, 96, act='relu', res_mode=2)]
    for lab, v in VIEWS.items():
        out.append(c('d_view_%s' % lab, 2, (9, 17), 64, 96, **dict(dict(act='relu'), **v)))
    out.append(c('d_view_off2', 1, (9, 17), 64, 96, act='relu', **ODD_VIEWS['off2_res']))       # conv_tail stores single floats
    for v in VALUES:
        out.append(c('d_%s' % v, 1, (9, 17), 64, 96, values=v))
    return out


@functools.lru_cache(maxsize=None)
def splitk_cases():
    """ksplit as choose_ksplit gives it (9 chunks -> 2, 18 chunks -> 4, the K = 2048 1x1 -> 16) and forced to 2 and 4 (forced to 1: the
    direct family)"""
    c = lambda name, *a, **kw: _case('splitk', name, *a, **kw)
    out = [c('sk_rule_9', 2, (5, 6), 32, 32, act='relu'), c('sk_rule_18', 1, (9, 17), 64, 96, act='silu', res_mode=1),
           c('sk_rule_k2048', 1, (8, 8), 2048, 256, k=1, act='relu')]
    for i, ks in enumerate((2, 4)):
        out.append(c('sk%d_9' % ks, 2, (5, 6), 32, 32, ksplit=ks, **_cycle(i + 1)))
        out.append(c('sk%d_18' % ks, 1, (9, 17), 64, 96, ksplit=ks, **_cycle(i + 3)))
        out.append(c('sk%d_cin40' % ks, 1, (7, 9), 40, 48, ksplit=ks, **_cycle(i + 5)))        # 18 chunks, half of them 8 channels wide
    for lab, v in VIEWS.items():
        out.append(c('sk_view_%s' % lab, 2, (9, 17), 64, 96, ksplit=4, **dict(dict(act='relu'), **v)))
    for v in VALUES:
        out.append(c('sk_%s' % v, 1, (9, 17), 64, 96, ksplit=4, values=v))
    return out


@functools.lru_cache(maxsize=None)
def narrow_cases():
    """cout <= 4 (k_conv_narrow / k_conv_narrow_cb when its configuration is forced, the 64x16 MFMA tile under the built-in rule)"""
    out = []
    for cout in (1, 2, 3, 4):
        for res in (0, 1):
            out.append(_case('narrow', 'nr_c%d_r%d' % (cout, res), 1 + res, (9, 33), (64, 32)[cout % 2], cout, act=(None, 'sigmoid')[res],
                             res_mode=(0, 2, 1)[res * (1 + cout % 2)]))
    out += [_case('narrow', 'nr_cin3', 2, (9, 11), 3, 3, act='relu'), _case('narrow', 'nr_s2', 1, (9, 33), 32, 1, stride=2),
            _case('narrow', 'nr_dil2', 1, (9, 33), 32, 4, dil=2), _case('narrow', 'nr_1x1', 1, (9, 33), 64, 1, k=1),
            _case('narrow', 'nr_view_in', 1, (9, 33), 32, 4, in_slice=(4, 8)), _case('narrow', 'nr_view_out', 1, (9, 33), 32, 1, out_slice=(8, 3)),
            _case('narrow', 'nr_view_res', 1, (9, 33), 32, 3, res_slice=(1, 4), res_mode=1),
            _case('narrow', 'nr_relu', 1, (9, 33), 64, 1, values='relu'), _case('narrow', 'nr_spread', 1, (9, 33), 64, 4, values='spread')]
    return out


@functools.lru_cache(maxsize=None)
def stem_cases():
    """cin_g == 4 (3 padded to 4, or 4), cout > 4: k_conv_stem from pack_stem_weights' (tap, channel) image, on odd frame sizes"""
    c = lambda name, *a, **kw: _case('stem', name, *a, **kw)
    return [c('st_7x7s2', 1, (33, 31), 3, 64, k=7, stride=2, act='relu'), c('st_3x3s2', 2, (33, 31), 3, 32, stride=2, act='silu'),
            c('st_3x3s1', 1, (9, 11), 3, 24, act='relu', res_mode=1), c('st_patch16', 2, (48, 35), 3, 96, k=16, stride=16, pad=0),
            c('st_cout169', 1, (9, 11), 3, 169, res_mode=2, act='relu'), c('st_cin4', 1, (9, 11), 4, 64, act='prelu'),
            c('st_view_in', 1, (9, 11), 4, 64, in_slice=(4, 8)), c('st_view_out', 2, (9, 11), 3, 24, out_slice=(8, 4)),
            c('st_view_res', 1, (9, 11), 3, 24, res_slice=(4, 12), res_mode=1), c('st_inplace', 1, (9, 11), 3, 24, inplace=True, res_mode=2),
            c('st_relu', 1, (33, 31), 3, 64, k=7, stride=2, values='relu'), c('st_spread', 1, (33, 31), 3, 64, k=7, stride=2, values='spread')]


@functools.lru_cache(maxsize=None)
def grouped_bd_cases():
    """the block-diagonal form on the tile kernels (Program.grouped_valu off, or a layer the vector kernel refuses)"""
    c = lambda name, *a, **kw: _case('grouped_bd', name, *a, **dict(dict(valu=False), **kw))
    out = [c('gb_cg4', 1, (6, 7), 32, 32, groups=8, act='relu'), c('gb_cg8', 2, (6, 7), 32, 32, groups=4, act='silu', res_mode=1),
           c('gb_cg64', 1, (5, 6), 128, 128, groups=2), c('gb_s2', 1, (6, 7), 32, 32, groups=4, stride=2, act='relu'),
           c('gb_cg4_s2', 1, (9, 7), 64, 64, groups=16, stride=2), c('gb_cout16', 1, (6, 7), 32, 64, groups=4, res_mode=2),
           c('gb_1x1px', 2, (1, 1), 32, 32, groups=4), c('gb_k1', 1, (6, 7), 64, 64, groups=8, k=1)]
    for lab, v in VIEWS.items():
        out.append(c('gb_view_%s' % lab, 1, (6, 7), 64, 64, groups=8, **dict(dict(act='relu'), **v)))
    for v in VALUES:
        out.append(c('gb_%s' % v, 1, (6, 7), 64, 64, groups=8, values=v))
    return out


@functools.lru_cache(maxsize=None)
def grouped_valu_cases():
    """k_conv_grouped: cin_g 8 and 16 under the shipped switches, 32 with GROUPED_VALU_MAX_CG raised; 7 wide takes the 32-pixel tile, 37
    wide the 40-pixel one (launch_conv_grouped); ragged 6 x 7 and 1 x 1 tiles.  The *_off2 / *_ld6 views are the ones grouped_eligible
    refuses (csrc/grouped.hip: float4 stores): they must lower to the block-diagonal form"""
    c = lambda name, *a, **kw: _case('grouped_valu', name, *a, **dict(dict(valu=True), **kw))
    out = [c('gv_cg8', 1, (6, 7), 32, 32, groups=4, act='relu'), c('gv_cg16', 2, (6, 7), 64, 64, groups=4, act='silu', res_mode=1),
           c('gv_cg32', 1, (6, 7), 64, 64, groups=2, max_cg=32, act='relu', res_mode=2), c('gv_1x1px', 2, (1, 1), 32, 32, groups=4),
           c('gv_w37_cg8', 1, (9, 37), 32, 32, groups=4, act='relu'), c('gv_w37_cg16', 1, (5, 37), 32, 32, groups=2, res_mode=1, act='prelu'),
           c('gv_w41', 1, (3, 41), 32, 32, groups=4)]
    for lab, v in dict(VIEWS, **ODD_VIEWS).items():
        out.append(c('gv_view_%s' % lab, 1, (6, 7), 32, 32, groups=4, **dict(dict(act='relu'), **v)))
    for v in VALUES:
        out.append(c('gv_%s' % v, 1, (6, 7), 64, 64, groups=8, values=v))
    return out


WINO_SHAPES = ((2, (1, 1), 32, 64), (1, (2, 67), 64, 128), (2, (13, 37), 64, 64), (1, (7, 5), 256, 64), (1, (45, 45), 96, 128))


def _wino_cases(mode):
    c = lambda name, *a, **kw: _case(mode, name, *a, **dict(dict(lower=mode), **kw))
    out = [c('%s_%dx%d_%d' % ((mode,) + hw + (cin,)), n, hw, cin, cout, **_cycle(i)) for i, (n, hw, cin, cout) in enumerate(WINO_SHAPES)]
    for lab, v in dict(VIEWS, **ODD_VIEWS).items():
        out.append(c('%s_view_%s' % (mode, lab), 2, (13, 21), 32, 64, **dict(dict(act='relu'), **v)))
    for v in VALUES:
        out.append(c('%s_%s' % (mode, v), 1, (13, 21), 64, 64, values=v))
    return out


@functools.lru_cache(maxsize=None)
def f2_cases():
    """F(2x2, 3x3), forced on the shapes of test_oracle_winograd4.py"""
    return _wino_cases('f2')


@functools.lru_cache(maxsize=None)
def f4_cases():
    """F(4x4, 3x3): forced on the shapes of test_oracle_winograd4.py, and BY THE SHIPPED RULE at 23 x 23 (128 -> 128, 512 -> 128: the
    small-map rule) and 80 x 80 (64 -> 64: WINO4_MIN_PIXELS)"""
    rule = lambda name, *a, **kw: _case('f4', name, *a, **dict(dict(lower='rule'), **kw))
    return _wino_cases('f4') + [rule('f4_rule_23_128', 1, (23, 23), 128, 128, act='relu'), rule('f4_rule_23_512', 1, (23, 23), 512, 128, act='silu', res_mode=1),
                                rule('f4_rule_80', 1, (80, 80), 64, 64, act='relu', res_mode=2)]


@functools.lru_cache(maxsize=None)
def lowering_cases():
    """Program.linear with a residual (tokens [n, T, 1, c]) and conv_transpose_nonoverlap with k = 2 and 4 (a 1x1 conv to k k cout channels
    and the depth-to-space scatter; reference F.conv_transpose2d)"""
    return [_case('lowerings', 'lin_res', 2, (17, 1), 64, 96, k=1, res_mode=1, op='linear'), _case('lowerings', 'lin_gelu', 1, (17, 1), 96, 64, k=1, act='gelu', op='linear'),
            _case('lowerings', 'lin_res_sl', 2, (17, 1), 64, 96, k=1, res_mode=1, res_slice=(4, 12), out_slice=(8, 4), op='linear'),
            _case('lowerings', 'convT_k2', 1, (5, 6), 32, 16, k=2, op='convT'), _case('lowerings', 'convT_k4', 2, (3, 5), 32, 8, k=4, op='convT'),
            _case('lowerings', 'convT_k2_nobias', 1, (5, 6), 64, 4, k=2, op='convT', bias=False)]


# one small layer per class for the epilogue cross (every activation of program.ACT x res_mode 0, 1, 2)
EPILOGUE_LAYERS = dict(direct=dict(n=1, hw=(5, 6), cin=32, cout=48, ksplit=1), splitk=dict(n=1, hw=(5, 6), cin=32, cout=48, ksplit=4),
                       narrow=dict(n=1, hw=(9, 33), cin=32, cout=3), stem=dict(n=1, hw=(5, 6), cin=3, cout=24),
                       grouped_bd=dict(n=1, hw=(5, 6), cin=32, cout=32, groups=4, valu=False), grouped_valu=dict(n=1, hw=(5, 6), cin=32, cout=32, groups=4, valu=True),
                       f2=dict(n=1, hw=(5, 6), cin=32, cout=64, lower='f2'), f4=dict(n=1, hw=(5, 6), cin=32, cout=64, lower='f4'))


@functools.lru_cache(maxsize=None)
def epilogue_cases():
    out = []
    for cls, kw in EPILOGUE_LAYERS.items():
        kw = dict(kw)
        n, hw, cin, cout = kw.pop('n'), kw.pop('hw'), kw.pop('cin'), kw.pop('cout')
        for act in ACTS:
            for rm in (0, 1, 2):
                k = _case('epilogue', 'ep_%s_%s_r%d' % (cls, act, rm), n, hw, cin, cout, act=act, res_mode=rm, **kw)
                k['cls'] = cls
                out.append(k)
    return out


@functools.lru_cache(maxsize=None)
def onehot_cases():
    """one-hot weights on every direct-chain class; the offsets give every tap of every kernel size its turn"""
    out = []

    def add(name, n, hw, cin, cout, **kw):
        k = kw.get('k', 3)
        for j, off in enumerate(range(0, k * k, cout)):
            out.append(_case('onehot', '1hot_%s_o%d' % (name, off), n, hw, cin, cout, onehot=off, act=EXACT_ACTS[(len(out) + j) % 3], **kw))
    add('d_1x1', 1, (7, 9), 64, 96, k=1, ksplit=1)
    add('d_3x3', 1, (9, 17), 64, 96, ksplit=1)
    add('d_s2', 2, (9, 17), 32, 48, stride=2, ksplit=1)
    add('d_dil2', 1, (11, 13), 32, 64, dil=2, ksplit=1)
    add('d_dil8', 1, (19, 17), 32, 32, dil=8, ksplit=1)
    add('d_valid', 1, (9, 17), 32, 64, pad=0, ksplit=1)
    add('d_cin40', 1, (7, 9), 40, 48, ksplit=1)
    add('d_5x5', 1, (9, 11), 32, 32, k=5, ksplit=1)
    add('d_view', 2, (9, 17), 64, 96, ksplit=1, in_slice=(4, 8), out_slice=(8, 4))
    add('sk_rule', 1, (9, 17), 64, 96)
    add('sk2', 2, (5, 6), 32, 32, ksplit=2)
    add('sk4_s2', 1, (9, 17), 64, 96, ksplit=4, stride=2)
    add('nr_c1', 1, (9, 33), 32, 1)
    add('nr_c4', 1, (9, 33), 64, 4)
    add('nr_c3_s2', 1, (9, 33), 32, 3, stride=2)
    add('nr_cin3', 1, (9, 11), 3, 3)
    add('st_7x7s2', 1, (33, 31), 3, 64, k=7, stride=2)
    add('st_3x3s2', 2, (33, 31), 3, 32, stride=2)
    add('st_3x3s1', 1, (9, 11), 3, 24)
    add('st_patch16', 1, (48, 35), 3, 256, k=16, stride=16, pad=0)
    add('gb_cg4', 1, (6, 7), 32, 32, groups=8, valu=False)
    add('gb_cg8_s2', 1, (6, 7), 32, 32, groups=4, stride=2, valu=False)
    add('gb_cg64', 1, (5, 6), 128, 128, groups=2, valu=False)
    add('gv_cg8', 1, (6, 7), 32, 32, groups=4, valu=True)
    add('gv_cg16', 2, (6, 7), 64, 64, groups=4, valu=True)
    add('gv_cg32_w37', 1, (5, 37), 64, 64, groups=2, valu=True, max_cg=32)
    add('gv_off2', 1, (6, 7), 32, 32, groups=4, valu=True, out_slice=(2, 6))
    return out


FAMILIES = dict(direct=direct_cases, splitk=splitk_cases, narrow=narrow_cases, stem=stem_cases, grouped_bd=grouped_bd_cases,
                grouped_valu=grouped_valu_cases, f2=f2_cases, f4=f4_cases, lowerings=lowering_cases, epilogue=epilogue_cases, onehot=onehot_cases)


def all_cases():
    return [k for f in FAMILIES.values() for k in f()]


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------
def conv64(k, w=None, x=None, stride=None, pad=None, dil=None):
    """F.conv2d / F.conv_transpose2d on the CPU in float64, natural weights, no bias -> NHWC.  The keyword overrides are for the mutants"""
    w = k['w'] if w is None else w
    x = k['x'] if x is None else x
    xt = torch.from_numpy(np.ascontiguousarray(x, f64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w, f64))
    if k['op'] == 'convT':
        y = F.conv_transpose2d(xt, wt, None, stride=k['k'])
    else:
        y = F.conv2d(xt, wt, None, k['stride'] if stride is None else stride, k['pad'] if pad is None else pad, k['dil'] if dil is None else dil, k['groups'])
    return y.permute(0, 2, 3, 1).numpy()


def epilogue(k, y, dtype=f64, order='bias,res1,act,res2'):
    """bias, the res_mode 1 add, the activation, the res_mode 2 add, in `dtype`; `order` only for the mutants"""
    y = np.asarray(y, dtype)
    r = None if k['res'] is None else k['res'].astype(dtype)
    for step in order.split(','):
        if step == 'bias' and k['b'] is not None:
            y = y + k['b'].astype(dtype)
        elif step == 'res1' and k['res_mode'] == 1:
            y = y + r
        elif step == 'act':
            y = _act(y, k['act'], k['slope'], dtype)
        elif step == 'res2' and k['res_mode'] == 2:
            y = y + r
    assert y.dtype == dtype
    return y


def onehot_expected(k):
    """the shifted, zero-padded input: output channel co is the strided window of its tap in its input channel (no arithmetic at all)"""
    x, kk, s, d, pad, g = k['x'], k['k'], k['stride'], k['dil'], k['pad'], k['groups']
    n, h, w, cin = x.shape
    cout, cin_g = k['w'].shape[:2]
    ho, wo = out_size(h, kk, s, pad, d), out_size(w, kk, s, pad, d)
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, cin), f32)
    xp[:, pad:pad + h, pad:pad + w] = x
    out = np.empty((n, ho, wo, cout), f32)
    for co in range(cout):
        (ci,), (ky,), (kx,) = np.nonzero(k['w'][co])
        out[..., co] = xp[:, ky * d:ky * d + (ho - 1) * s + 1:s, kx * d:kx * d + (wo - 1) * s + 1:s, (co // (cout // g)) * cin_g + ci]
    return out


_REF, _E32 = {}, {}


def reference(k):
    """float64 NHWC, computed once per case"""
    if k['name'] not in _REF:
        r = _act(onehot_expected(k).astype(f64), k['act'], k['slope'], f64) if k['exact'] else epilogue(k, conv64(k))
        r.setflags(write=False)
        _REF[k['name']] = r
    return _REF[k['name']]


# ---- the plain float32 evaluations -----------------------------------------------------------------------------------------------------
def direct32(k):
    """im2col accumulation in float32: taps row-major, channels ascending, one rounded multiply and one rounded add per term"""
    x, wt, kk, s, d, pad, g = k['x'], k['w'], k['k'], k['stride'], k['dil'], k['pad'], k['groups']
    n, h, w, cin = x.shape
    if k['op'] == 'convT':                                                 # output pixel (y kk + ky, x kk + kx) = the 1x1 conv with w[:, :, ky, kx]
        cout = wt.shape[1]
        out = np.zeros((n, h * kk, w * kk, cout), f32)
        for ky in range(kk):
            for kx in range(kk):
                acc = np.zeros((n, h, w, cout), f32)
                for c in range(cin):
                    acc = acc + x[..., c:c + 1] * wt[c, :, ky, kx]
                out[:, ky::kk, kx::kk] = acc
        return out
    cout, cin_g = wt.shape[:2]
    cout_g = cout // g
    ho, wo = out_size(h, kk, s, pad, d), out_size(w, kk, s, pad, d)
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, cin), f32)
    xp[:, pad:pad + h, pad:pad + w] = x
    out = np.zeros((n, ho, wo, cout), f32)
    for gi in range(g):
        acc = np.zeros((n, ho, wo, cout_g), f32)
        wg = wt[gi * cout_g:(gi + 1) * cout_g]
        for ky in range(kk):
            for kx in range(kk):
                win = xp[:, ky * d:ky * d + (ho - 1) * s + 1:s, kx * d:kx * d + (wo - 1) * s + 1:s, gi * cin_g:(gi + 1) * cin_g]
                for c in range(cin_g):
                    acc = acc + win[..., c:c + 1] * wg[:, c, ky, kx]
        out[..., gi * cout_g:(gi + 1) * cout_g] = acc
    assert out.dtype == f32
    return out


# the transform matrices of the two Winograd contracts (include/csm355.h; F(4x4): Lavin & Gray, points 0, +-1, +-2, inf -- the matrices
# of tests/test_oracle_winograd4.py::test_the_transform_matrices_are_a_convolution)
WINO = {2: dict(BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], AT=[[1, 1, 1, 0], [0, 1, -1, -1]],
                G=[[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
        4: dict(BT=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
                AT=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]],
                G=[[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])}


def _apply32(M, a, axis):
    """sum_k M[i][k] a[k] along `axis` in float32, k ascending, zero entries skipped, every product and every sum rounded"""
    a = np.moveaxis(a, axis, 0)
    rows = []
    for row in M:
        acc = None
        for kk, m in enumerate(row):
            if m:
                t = a[kk] * f32(m)
                acc = t if acc is None else acc + t
        rows.append(acc)
    r = np.moveaxis(np.stack(rows), 0, axis)
    assert r.dtype == f32
    return r


def wino32(k, m):
    """the Winograd formula F(m x m, 3x3) in plain float32 on tiles of m x m outputs: V = B^T d B, M = sum_c U * V (c ascending), Y = A^T M A"""
    x, wt = k['x'], k['w']
    n, h, w, cin = x.shape
    cout = wt.shape[0]
    t = m + 2
    U = (P.wino_transform if m == 2 else P.wino4_transform)(wt).reshape(t, t, cout, cin)
    th, tw = -(-h // m), -(-w // m)
    xp = np.zeros((n, th * m + 2, tw * m + 2, cin), f32)
    xp[:, 1:h + 1, 1:w + 1] = x
    # d [n, th, tw, t, t, cin]
    dtile = np.stack([np.stack([xp[:, i:i + th * m:m, j:j + tw * m:m] for j in range(t)], 3) for i in range(t)], 3)
    V = _apply32(WINO[m]['BT'], _apply32(WINO[m]['BT'], dtile, 3), 4)
    M = np.zeros((n, th, tw, t, t, cout), f32)
    for c in range(cin):
        M = M + V[..., c:c + 1] * U[:, :, :, c]
    Y = _apply32(WINO[m]['AT'], _apply32(WINO[m]['AT'], M, 3), 4)                              # [n, th, tw, m, m, cout]
    y = Y.transpose(0, 1, 3, 2, 4, 5).reshape(n, th * m, tw * m, cout)[:, :h, :w]
    assert y.dtype == f32
    return np.ascontiguousarray(y)


def arithmetic(k):
    """'direct', 'f2' or 'f4': the arithmetic the lowered case runs (its op's flags)"""
    fl = conv_op(program(k))['flags']
    return 'f4' if fl & P.CONV_FLAG_WINOGRAD4 else 'f2' if fl & P.CONV_FLAG_WINOGRAD else 'direct'


def plain32(k):
    a = arithmetic(k)
    return epilogue(k, direct32(k) if a == 'direct' else wino32(k, 2 if a == 'f2' else 4), f32)


def scale(k):
    return float(np.abs(reference(k)).max())


def error(k, got):
    """the distance of a result from the reference in units of max|ref|"""
    return rel_err(got, reference(k), scale(k))


def e32(k):
    if k['name'] not in _E32:
        _E32[k['name']] = error(k, plain32(k))
    return _E32[k['name']]


# ---- one-layer programs ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def lowering(k):
    """the switches of the lowering a case asks for, restored afterwards"""
    old = (P.Program.winograd, P.Program.winograd4, P.WINO_MIN_PIXELS, P.WINO4_MIN_PIXELS, P.Program.grouped_valu, P.GROUPED_VALU_MAX_CG)
    try:
        if k['lower'] != 'rule':
            P.Program.winograd, P.Program.winograd4 = k['lower'] != 'direct', k['lower'] == 'f4'
            P.WINO_MIN_PIXELS = P.WINO4_MIN_PIXELS = 0
        if k['valu'] is not None:
            P.Program.grouped_valu = k['valu']
        if k['max_cg'] is not None:
            P.GROUPED_VALU_MAX_CG = k['max_cg']
        yield
    finally:
        P.Program.winograd, P.Program.winograd4, P.WINO_MIN_PIXELS, P.WINO4_MIN_PIXELS, P.Program.grouped_valu, P.GROUPED_VALU_MAX_CG = old


def _src(p, x, sl):
    """netops_cases._source; a tensor whose channel count is no multiple of 4 gets a buffer of exactly its channels (ld = c)"""
    n, h, w, c = x.shape
    if sl is not None or c % 4 == 0:
        return N._source(p, x, sl)
    v = p.buffer(n, h, w, c)
    p.to_nhwc_into(p.ext_nchw(n, c, h, w), v)
    return v


def program(k):
    """ext NCHW -> NHWC (a buffer of its own, or a channel slice of a wider one) -> the layer -> NCHW.  Built.views = (input, residual,
    output), Built.guard = (the whole buffer, the slice) where the layer writes a channel slice, Built.aux = the scratch view or None"""
    with lowering(k):
        p = P.Program(k['name'])
        if k['ksplit'] is not None:
            p.choose_ksplit = lambda M, N_, T, groups, ks=k['ksplit']: ks
        n, h, w, cin = k['x'].shape
        xv = p.to_nhwc(p.ext_nchw(n, cin, h, w)) if cin % 4 else N._source(p, k['x'], k['in_slice'])
        ext_in = [nchw(k['x'])]
        rv = None
        if k['res_mode']:
            rv = _src(p, k['res'], k['res_slice'])
            ext_in.append(nchw(k['res']))
        ref_shape = reference(k).shape
        if k['inplace']:
            out, wide = rv, (P.T(p, rv.buf, 0, rv.buf.c) if rv.buf.c != rv.c else None)
        else:
            out, wide = N._target(p, ref_shape, k['out_slice'])
        if k['op'] == 'linear':
            r = p.linear(xv, k['w'][:, :, 0, 0], k['b'], act=k['act'], res=rv, out=out)
        elif k['op'] == 'convT':
            r = p.conv_transpose_nonoverlap(xv, k['w'], k['b'], k['k'])
        else:
            r = p.conv(xv, k['w'], k['b'], k['stride'], k['pad'], k['dil'], k['groups'], k['act'], k['slope'], res=rv, res_mode=k['res_mode'], out=out)
        assert r.shape == ref_shape, (k['name'], r.shape, ref_shape)
        for v, sl in ((xv, k['in_slice']), (rv, k['res_slice']), (None if k['inplace'] else r, k['out_slice'])):
            assert v is None or (v.buf.c != v.c) == (sl is not None), k['name']            # ld != c exactly where the case says so
        y_ext = p.ext_nchw(r.n, r.c, r.h, r.w)
        p.to_nchw(r, y_ext)
    op = conv_op(p)
    scr = p.views[op['scratch']] if op['scratch'] >= 0 else None
    return Built(p, ext_in, (r.n, r.c, r.h, r.w), (xv, rv, r), (wide, r) if wide is not None else None, scr)


def conv_op(b):
    """the one CONV op of a lowered case (a Built or its Program)"""
    ops = [o for o in getattr(b, 'prog', b).ops if o['kind'] == P.OP_CONV]
    assert len(ops) == 1
    return ops[0]


# ---- which kernel a case selects -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cfg_table():
    """{name: row} of the library's tile configurations (host only)"""
    from cartoonsegmentation_amd.runtime import conv_cfg_table
    return {c['name']: c for c in conv_cfg_table()}


def resolve_cfg(k, cfg_name):
    """the configuration csm_run_program launches for a direct case that carries `cfg_name` (csm_debug_conv_resolve_cfg, host only) -> row"""
    from cartoonsegmentation_amd import _lib
    b = program(k)
    ops, tens, _ = b.prog.serialise()
    i = [j for j, o in enumerate(b.prog.ops) if o['kind'] == P.OP_CONV][0]
    got = _lib.load().csm_debug_conv_resolve_cfg(ctypes.c_int(cfg_table()[cfg_name]['id']), ctypes.byref(ops[i]), ctypes.byref(tens[ops[i].in0]),
                                                 ctypes.byref(tens[ops[i].out]))
    return [c for c in cfg_table().values() if c['id'] == got][0]


def variant(k, cfg_name=None):
    """the kernel family the case's conv op runs: by its flags, or -- a plain op -- the tile family `cfg_name` resolves to (no name: 'tile')"""
    fl = conv_op(program(k))['flags']
    for bit, name in ((P.CONV_FLAG_STEM, 'k_conv_stem'), (P.CONV_FLAG_GROUPED, 'k_conv_grouped'), (P.CONV_FLAG_WINOGRAD4, 'k_conv_wino4'),
                      (P.CONV_FLAG_WINOGRAD, 'k_conv_wino')):
        if fl & bit:
            return name
    return 'tile' if cfg_name is None else resolve_cfg(k, cfg_name)['family']


# ---- planted faults: float64 references of what a wrong kernel would compute -----------------------------------------------------------
MUTANTS = ('tap', 'pad', 'phase', 'dil', 'groups', 'lastchunk', 'run_dropped', 'run_doubled', 'tail', 'bias_after', 'res_swapped', 'stem_transposed')


def chunks(k):
    """(32-channel blocks, taps): the K chunks of a dense layer in chain order are (block, tap), block outer"""
    return -(-k['w'].shape[1] // 32), k['k'] * k['k']


def mutant(k, kind, ksplit=None):
    """the reference with one fault planted, or None where the case cannot show that fault.  tap: the centre tap's weights and its
    neighbour's exchanged; pad: the left padding one short (the right one longer: same output size); phase: every window starts one pixel
    late (stride > 1); dil: the dilation ignored; groups: the weights of groups 0 and 1 exchanged; lastchunk: the last K chunk (last
    32-channel block, last tap) dropped; run_dropped / run_doubled: the first chunk of split-K run 1 (chunk T // ksplit) dropped / counted
    twice; tail: the last output channel zeroed; bias_after: the bias added after the activation; res_swapped: res_mode 1 and 2
    exchanged; stem_transposed: the stem's (tap, channel) packing read as (channel, tap)"""
    w, kk, pad, op = k['w'].astype(f64), k['k'], k['pad'], k['op']
    x = k['x'].astype(f64)
    conv = op != 'convT'
    if kind == 'tap' and kk >= 2 and conv:
        c, w2 = kk // 2, w.copy()
        w2[..., c, c], w2[..., c, c - 1] = w[..., c, c - 1], w[..., c, c]
        return epilogue(k, conv64(k, w=w2))
    if kind == 'pad' and pad >= 1 and conv:
        return epilogue(k, conv64(k, x=np.pad(x, ((0, 0), (pad, pad), (pad - 1, pad + 1), (0, 0))), pad=0))
    if kind == 'phase' and k['stride'] > 1 and conv:
        return epilogue(k, conv64(k, x=np.pad(x, ((0, 0), (pad, pad + 1), (pad, pad + 1), (0, 0)))[:, 1:, 1:], pad=0))
    if kind == 'dil' and k['dil'] > 1:
        return epilogue(k, conv64(k, dil=1, pad=pad - (k['dil'] - 1) * (kk - 1) // 2))
    if kind == 'groups' and k['groups'] > 1:
        cg = w.shape[0] // k['groups']
        return epilogue(k, conv64(k, w=np.concatenate([w[cg:2 * cg], w[:cg], w[2 * cg:]])))
    if kind in ('lastchunk', 'run_dropped', 'run_doubled') and k['groups'] == 1 and conv:
        ncb, taps = chunks(k)
        if kind == 'lastchunk':
            t, f = ncb * taps - 1, 0.0
        elif ksplit is None or ksplit < 2:
            return None
        else:
            t, f = ncb * taps // ksplit, (0.0 if kind == 'run_dropped' else 2.0)
        cb, tap = divmod(t, taps)
        w2 = w.copy()
        w2[:, 32 * cb:32 * cb + 32, tap // kk, tap % kk] *= f
        return epilogue(k, conv64(k, w=w2))
    if kind == 'tail':
        r = np.array(reference(k))
        r[..., -1] = 0.0
        return r
    if kind == 'bias_after' and k['b'] is not None and k['act'] is not None:
        return epilogue(k, conv64(k), order='res1,act,bias,res2')
    if kind == 'res_swapped' and k['res_mode'] and k['act'] is not None:
        return epilogue(dict(k, res_mode=3 - k['res_mode']), conv64(k))
    if kind == 'stem_transposed' and k['family'] == 'stem':
        cout, cin = w.shape[:2]
        return epilogue(k, conv64(k, w=w.reshape(cout, kk * kk, cin).transpose(0, 2, 1).reshape(w.shape)))
    return None
