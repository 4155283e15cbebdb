"""CPU: the oracle's layer ops that are not matrix-pipe convolutions (oracle/nets_oracle.c: orc_dwconv, orc_maxpool, orc_bilinear,
orc_nearest, orc_eltwise with orc_act, orc_attractor, orc_logbinom, orc_gavgpool and the two transposes) against the plain float64
references of tests/netops_cases.py, on every case the GPU tests use -- and, for every case family, the property it exists for: the
kernel variant its shapes select, the edge it sits on, and a planted fault that the reference rejects (by more than ten times the bound,
or by plain inequality where the op is exact).  Each op is reached through a one-op Program (ext NCHW -> NHWC -> op -> NCHW); the runner
and the checks here are shared with tests/test_gpu_netops.py.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netops_cases as C  # noqa: E402

from oracle import nets as onets  # noqa: E402

f32, f64 = np.float32, np.float64


# ---- running a case ------------------------------------------------------------------------------------------------------------------
def oracle_run(b):
    """-> (output NCHW, {whole-buffer view: [n, h, w, C]}); the oracle's workspace starts as zeros"""
    out = np.zeros(b.out_shape, f32)
    want = [b.guard[0]] if b.guard else []
    return out, onets.run_program(b.prog, [np.ascontiguousarray(a, f32) for a in b.ext_in] + [out], want)


def result_of(k, run, is_guard):
    """the case's result in the reference's layout; where the op writes a channel slice of a wider buffer, the slice holds the result
    and every other channel of the buffer still holds what it was filled with"""
    b = C.program(k)
    y, views = run(b)
    got = y if k['kind'] == 'layout' else C.nhwc(y)
    if b.guard:
        wide, view = b.guard
        full, inside = views[wide], C.nhwc(got) if k['kind'] == 'layout' else got
        lo, hi = view.coff, view.coff + view.c
        assert np.array_equal(full[..., lo:hi], inside, equal_nan=True), k['name']
        assert is_guard(full[..., :lo]).all() and is_guard(full[..., hi:]).all(), k['name']
    return np.ascontiguousarray(got)


def oracle_result(k):
    return result_of(k, oracle_run, lambda a: a == 0)


def check_case(k, got, what):
    """finite where the inputs are, NaN where they are not; equal to the float32 rounding of the reference where the op is exact, inside
    max(4 e32, 8 * 2^-23) of the case's scale otherwise.  -> the error in units of the bound (0 for an exact case)"""
    ref = C.reference(k)
    assert got.shape == ref.shape, (what, k['name'], got.shape, ref.shape)
    fin = k.get('finite_samples')
    if fin is not None:
        assert np.isfinite(got[fin]).all() and np.isnan(got[fin.stop:]).all(), (what, k['name'])
    else:
        assert np.isfinite(got).all(), (what, k['name'])
    if k['exact']:
        want = C.compared(k, ref).astype(f32)
        bad = C.compared(k, got) != want
        assert not bad.any(), (what, k['name'], int(bad.sum()), C.compared(k, got)[bad][:4], want[bad][:4])
        return 0.0
    e32, err = C.e32(k), C.error(k, got)
    lim = C.bound(e32)
    print("%s %-34s err %.3g  e32 %.3g  bound %.3g" % (what, k['name'], err, e32, lim))
    assert e32 <= lim                                                      # the plain float32 evaluation inside its own bound
    assert err <= lim, (what, k['name'], err, e32, lim)
    return err / lim


def summary(what, family, cases, errs):
    """one line per family: the range of e32, of the error and the worst error in units of its bound"""
    inexact = [(k, e) for k, e in zip(cases, errs) if not k['exact']]
    if not inexact:
        print("%s %s: %d cases, all exact" % (what, family, len(cases)))
        return
    e32s = [C.e32(k) for k, _ in inexact]
    es = [C.error(k, g) for k, g in inexact]
    print("%s %s: %d cases (%d exact); e32 %.2g .. %.2g; error %.2g .. %.2g; worst error / bound %.3g" % (
        what, family, len(cases), len(cases) - len(inexact), min(e32s), max(e32s), min(es), max(es), max(e / C.bound(s) for e, s in zip(es, e32s))))


# ---- every case against its reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_oracle_is_inside_the_bound_or_equal(family):
    cases = C.FAMILIES[family]()
    assert len({k['name'] for k in cases}) == len(cases)
    got = [oracle_result(k) for k in cases]
    for k, g in zip(cases, got):
        check_case(k, g, 'oracle')
    summary('oracle', family, cases, got)


def test_every_kernel_of_the_table_has_a_case():
    """the union of variant(case) over all cases is the kernel list of csmconv::launch_netop, and the cases meant for a variant select it"""
    by = {}
    for k in C.all_cases():
        for v in C.variant(k):
            by.setdefault(v, []).append(k['name'])
    for v in C.KERNELS:
        print("%-22s %d cases" % (v, len(by.get(v, []))))
    assert set(by) == set(C.KERNELS), set(by) ^ set(C.KERNELS)
    one = {k['name']: C.variant(k) for k in C.all_cases()}
    # depthwise: 9 x 9 is the largest kernel of the LDS form, 11 x 11 falls back; a channel count off 32, a stride, a dilation do too
    assert C.dw_lds_bytes(9) == 59520 <= 65536 < C.dw_lds_bytes(11) == 75392
    for k in C.dwconv_cases() + C.dwconv_onehot_cases():
        lds = k['k'] <= 9 and k['c'] % 32 == 0 and k['stride'] == 1 and k['dil'] == 1
        assert one[k['name']] == ('k_dwconv_lds' if lds else 'k_dwconv',), k['name']
    for K in (3, 5, 7, 9):
        assert one['dw_k%d_9x17' % K] == ('k_dwconv_lds',) and one['dw1hot_k%d_9x17_o0' % K] == ('k_dwconv_lds',)
    assert one['dw_k11_9x17'] == ('k_dwconv',) and one['dw1hot_k11_9x17_o0'] == ('k_dwconv',)
    assert one['dw_isolation_lds'] == ('k_dwconv_lds',) and one['dw_isolation_generic'] == ('k_dwconv',)
    # bilinear: the two grid limits reach k_bilinear<4>, the odd-offset 1- and 2-channel slices k_bilinear<1>, everything else the rows
    for k in C.bilinear_cases():
        want = 'k_bilinear<4>' if k['name'].startswith(('bil_tall', 'bil_batch')) else 'k_bilinear<1>' if k['name'].startswith(('bil_c1', 'bil_c2')) else 'k_bilinear_rows'
        assert one[k['name']] == (want,), k['name']
    for k in C.eltwise_cases() + C.activation_cases():
        v = one[k['name']][0]
        narrow = k['x'].shape[-1] == 2
        if k.get('crop'):
            assert v == 'k_eltwise/3'
        elif k['op'] == 'scale':
            assert v == 'k_eltwise/2'
        else:
            assert v == ('k_eltwise' if narrow else 'k_eltwise4') + ('/1' if k['op'] == 'add' else '/0'), (k['name'], v)
    for k in C.gavgpool_cases():
        assert one[k['name']] == ('k_gavgpool32' if k['x'].shape[-1] % 32 == 0 else 'k_gavgpool',), k['name']
    assert one['gap_25x40_c32_sl'] == ('k_gavgpool32',)
    for k in C.layout_cases():
        c = k['c'] if k['mode'] == 'slice' else (k['c'] + 3) // 4 * 4
        tile = 8 <= c <= 240
        assert one[k['name']] == ('k_nchw_to_nhwc_tile' if tile else 'k_nchw_to_nhwc', 'k_nhwc_to_nchw_tile' if tile else 'k_nhwc_to_nchw'), k['name']
    for c, tile in ((7, False), (8, True), (240, True), (241, False)):
        assert ('tile' in one['layout_c%d_8x8_slice' % c][0]) == tile


# ---- depthwise conv ------------------------------------------------------------------------------------------------------------------
def test_dwconv_cases_sit_on_the_tile_edges_and_cover_every_option():
    TH, TW = 8, 16
    h, w = zip(*C.DW_FRAMES)
    assert (1, 1) in C.DW_FRAMES and (TH - 1, TW - 1) in C.DW_FRAMES and (TH, TW) in C.DW_FRAMES and (TH + 1, TW + 1) in C.DW_FRAMES
    assert any(1 < b_ < 5 for a, b_ in C.DW_FRAMES) and max(h) > 2 * TH and max(w) > 2 * TW
    for lds in (True, False):
        cs = [k for k in C.dwconv_cases() if (C.variant(k) == ('k_dwconv_lds',)) == lds]
        assert {k['act'] for k in cs} == set(C.DW_ACTS) and {k['b'] is None for k in cs} == {True, False}, lds
        assert {k['in_slice'] is None for k in cs} == {True, False} and {k['n'] for k in cs} == {1, 2}
        assert {k['c'] for k in cs} >= ({32, 64} if lds else {4, 36})
    gen = [k for k in C.dwconv_cases() if C.variant(k) == ('k_dwconv',)]
    assert {k['stride'] for k in gen} == {1, 2} and {k['dil'] for k in gen} == {1, 2}
    pads = {(k['k'], k['pad']) for k in C.dwconv_cases()}
    assert pads >= {(3, 0), (3, 1), (3, 2), (5, 0), (5, 2), (5, 4), (7, 3), (9, 4), (11, 5)}
    for k in C.dwconv_cases():
        if k['c'] == 64:
            assert not np.array_equal(k['w'][:32], k['w'][32:])
    # every tap of every kernel size has its one-hot turn
    for K in C.DW_KS:
        for hw in C.DW_FRAMES:
            taps = set()
            for k in C.dwconv_onehot_cases():
                if k['name'].startswith('dw1hot_k%d_%dx%d_o' % (K, hw[0], hw[1])):
                    assert (k['w'].sum((1, 2, 3)) == 1).all() and set(np.unique(k['w'])) == {0.0, 1.0}
                    taps |= set(k['w'].reshape(k['c'], -1).argmax(1).tolist())
            assert taps == set(range(K * K)), (K, hw)
    for k in C.dwconv_cases():
        if k['finite_samples'] is not None:
            assert np.isnan(k['x'][1]).all() and np.isfinite(k['x'][0]).all() and np.isfinite(C.reference(k)[0]).all()


def test_dwconv_reference_rejects_a_shifted_tap_and_swapped_channel_blocks():
    worst = np.inf
    for k in C.dwconv_cases():
        if k['finite_samples'] is not None:
            continue
        lim = C.bound(C.e32(k))
        faults = [('tap', C.dw_shift_centre_tap(k['w']))] + ([('blocks', C.dw_swap_blocks(k['w']))] if k['c'] == 64 else [])
        for lab, wt in faults:
            moved = C.error(k, C.dwconv_reference(k, wt))
            worst = min(worst, moved / lim)
            assert moved > 10 * lim, (k['name'], lab, moved, lim)
    print("a planted depthwise fault moves the reference by at least %.3g x the bound" % worst)
    # the one-hot cases: another tap is another window of the input (plain inequality)
    for k in C.dwconv_onehot_cases():
        if k['x'].shape[1:3] == (1, 1):
            continue                                                       # one pixel: only the centre tap sees it, any other gives zeros
        k2 = dict(k, onehot=k['onehot'] + 1)
        assert not np.array_equal(C.dwconv_onehot_expected(k2), C.reference(k)), k['name']


# ---- max pool ------------------------------------------------------------------------------------------------------------------------
def test_maxpool_cases_and_zero_padding_shows():
    names = {k['name'] for k in C.maxpool_cases()}
    assert len(names) == 2 * (len(C.POOL_CFGS) * len(C.POOL_SIZES) - 2)     # 1 x 1 has no output under (2, 2, 0, floor) and (3, 2, 0, ceil): torch refuses both
    drop = [k for k in C.maxpool_cases() if k['name'].startswith('pool_k2s2p1ceil_3x3')]
    assert len(drop) == 2 and all(C.reference(k).shape[1:3] == (2, 2) for k in drop)       # torch drops the window that starts in the right padding
    assert C.pool_out_size(3, 2, 2, 1, True) == 2 and -(-(3 + 2 - 2) // 2) + 1 == 3
    shown = 0
    for k in C.maxpool_cases():
        assert (k['x'] < 0).all()
        h, w = k['x'].shape[1:3]
        ho, wo = C.reference(k).shape[1:3]
        assert (ho, wo) == tuple(C.pool_out_size(i, k['k'], k['stride'], k['pad'], k['ceil']) for i in (h, w))
        outside = k['pad'] > 0 or (ho - 1) * k['stride'] + k['k'] - k['pad'] > h or (wo - 1) * k['stride'] + k['k'] - k['pad'] > w
        wrong = C.maxpool_reference(k, zero_pad=True)
        assert np.array_equal(wrong, C.reference(k)) == (not outside), k['name']
        shown += outside
    assert shown >= 30


# ---- bilinear ------------------------------------------------------------------------------------------------------------------------
def test_bilinear_cases_and_a_flipped_align_corners_shows():
    rows = [k for k in C.bilinear_cases() if C.variant(k) == ('k_bilinear_rows',)]
    assert {k['x'].shape[-1] // 4 for k in rows} == {1, 3, 5, 7, 9, 25}
    per_row = {k['size'][1] * k['x'].shape[-1] // 4 for k in rows}
    assert min(per_row) < 256 and {256, 257} <= per_row and any(v > 512 and v % 256 for v in per_row), sorted(per_row)
    pairs = {(k['x'].shape[1:3], k['size']) for k in rows}
    for ih, oh in ((23, 45), (45, 90), (12, 23), (45, 23), (7, 1)):
        assert ((ih, ih), (oh, oh)) in pairs
    assert ((1, 1), (5, 7)) in pairs and ((5, 7), (1, 1)) in pairs
    assert any(i[0] == o[0] and i[1] != o[1] for i, o in pairs) and any(i[0] != o[0] and i[1] == o[1] for i, o in pairs) and any(i == o for i, o in pairs)
    assert {k['align'] for k in rows} == {False, True} and any(k['act'] == 'prelu' for k in rows)
    for name in ('bil_tall_a0', 'bil_batch_a0', 'bil_c1_a1', 'bil_c2_a0'):
        assert any(k['name'] == name for k in C.bilinear_cases())
    worst = np.inf
    for k in C.bilinear_cases():
        lim = C.bound(C.e32(k))
        moved = C.error(k, C.bilinear_reference(k, align=not k['align']))
        if k['align_matters']:
            worst = min(worst, moved / lim)
            assert moved > 10 * lim, (k['name'], moved, lim)
        else:
            assert moved <= lim, k['name']                                 # equal sizes, or a single source pixel: the flag changes nothing
    print("a flipped align_corners moves the reference by at least %.3g x the bound" % worst)


# ---- element-wise and activations ----------------------------------------------------------------------------------------------------
def test_eltwise_cases_and_wrong_pitch_or_scale_vector_shows():
    crops = set()
    for k in C.eltwise_cases():
        assert k['x'].shape[0] == 2 and not np.array_equal(k['x'][0], k['x'][1])
        if k.get('crop'):
            crops.add(k['crop'])
            assert not np.array_equal(C.eltwise_reference(k, 'pitch').astype(f32), C.reference(k).astype(f32)), k['name']
            if k['crop'] == (1, 0):                                        # one more row: only the sample pitch differs
                assert np.array_equal(C.eltwise_reference(k, 'pitch')[0], C.reference(k)[0])
        if k['op'] == 'scale':
            assert not np.array_equal(k['y'][0], k['y'][1])
            wrong = C.eltwise_reference(k, 'sample0').astype(f32)
            assert np.array_equal(wrong[0], C.reference(k)[0].astype(f32)) and (wrong[1] != C.reference(k)[1].astype(f32)).mean() > 0.99
    assert crops == {(1, 0), (0, 1), (1, 1)}
    assert {k['x'].shape[1] * k['x'].shape[2] for k in C.eltwise_cases() if not k.get('crop')} == {15, 259}


def test_activation_points_and_softplus_without_its_switch_fails_at_100():
    x = C.activation_points()
    assert x.size % 4 == 0 and x.size >= 4096
    for v in [0.0, 1e-40, 2.0 ** -20, 0.5, 16.0, 3.0, 87.0, 88.0, 89.0, 100.0, 1e4]:
        assert (x == f32(v)).any() and ((x == f32(-v)) & (np.signbit(x))).any(), v
    assert 0 < f32(1e-40) < np.finfo(f32).tiny
    for v in (3.0, -3.0, 20.0):
        assert (x == np.nextafter(f32(v), f32(np.inf))).any() and (x == np.nextafter(f32(v), f32(-np.inf))).any()
    sp = [k for k in C.activation_cases() if k['act'] == 'softplus'][0]
    lim = C.bound(C.e32(sp))
    at100 = (sp['x'] == f32(100.0))
    wrong = np.where(at100, C.softplus_without_switch(sp['x']), C.reference(sp))
    moved = C.error(sp, wrong)
    print("softplus without the v > 20 switch: %.3g of max(|x|, 1) at x = 100, bound %.3g" % (moved, lim))
    assert at100.sum() == 1 and moved > 10 * lim
    assert {k['act'] for k in C.activation_cases() if k['exact']} == {'relu', 'prelu'}


# ---- attractor, log-binomial ---------------------------------------------------------------------------------------------------------
def test_attractor_cases_hold_exact_hits_and_far_attractors():
    combos = set()
    for k in C.attractor_cases():
        A, b = k['x'].astype(f64), k['y'].astype(f64)
        dx = A[..., :, None] - b[..., None, :]
        assert (dx == 0).any() and (k['alpha'] * dx * dx > 100).any(), k['name']
        assert A.shape[1] * A.shape[2] == 257
        combos.add((A.shape[-1], b.shape[-1], k['typ'], k['agg'], k['alpha']))
    assert len(combos) == 3 * 3 * 2 * 2 * 2
    assert any(k['in_slice'] and k['in1_slice'] for k in C.attractor_cases()) and any(not k['in_slice'] and not k['in1_slice'] for k in C.attractor_cases())


def test_logbinom_cases_hit_both_clamps_and_both_temperatures_and_the_clamps_show():
    from cartoonsegmentation_amd.nets import zoedepth_head
    tmin, tmax = C.shipped_temperatures()
    assert (tmin, tmax) == (0.0212, 50.0)
    for K in C.LOGBINOM_KS:
        assert np.array_equal(C.log_binom_table(K), zoedepth_head.log_binom_table(K))
    for k in C.logbinom_cases():
        q = k['x'].astype(f64) + k['p_eps']
        p = q[..., 0] / (q[..., 0] + q[..., 1])
        t = q[..., 2] / (q[..., 2] + q[..., 3])
        assert (p < 1e-4).sum() > 30 and (1 - p < 1e-4).sum() > 30 and (t < 1e-2).sum() > 30 and (t > 1 - 1e-4).sum() > 30
        assert ((p < 1e-4) & (t < 1e-2)).any() and ((p < 1e-4) & (t > 1 - 1e-4)).any() and ((1 - p < 1e-4) & (t > 1 - 1e-4)).any()
        assert k['x'].shape[2] == 257 and k['in_slice'] == (0, 4) and k['min_temp'] == (tmin if k['family'] == 'shipped' else 1.0) and k['max_temp'] == tmax
        lim = C.bound(C.e32(k))
        moved = C.error(k, C.logbinom_reference(k, clamps=False))
        print("%s: without the clamps %.3g of max|ref|, bound %.3g" % (k['name'], moved, lim))
        if k['K'] > 1:
            assert moved > 10 * lim, (k['name'], moved, lim)
        else:
            assert moved == 0                                              # one bin: the output is its centre


# ---- global average pool, layout -----------------------------------------------------------------------------------------------------
def test_gavgpool_cases():
    assert {k['x'].shape[1] * k['x'].shape[2] for k in C.gavgpool_cases()} == {1, 7, 255, 256, 257, 1000}
    assert all(k['x'].shape[0] == 2 for k in C.gavgpool_cases())
    off = [k for k in C.gavgpool_cases() if k['name'].endswith('_off')]
    assert len(off) >= 4 and all(k['x'].min() > 990 for k in off)
    sl = [k for k in C.gavgpool_cases() if k['in_slice']]
    assert all(k['x'].shape[-1] == 32 and k['in_slice'] == (4, 4) for k in sl) and len(sl) >= 6


def test_layout_cases_and_a_transposed_pair_shows():
    assert {k['c'] for k in C.layout_cases()} == {1, 3, 4, 7, 8, 9, 64, 69, 240, 241}
    assert {k['x'].shape[2] * k['x'].shape[3] for k in C.layout_cases()} == {1, 63, 64, 65, 130}
    for k in C.layout_cases():
        x = k['x']
        assert x.shape[0] == 2 and np.unique(x).size == x.size and x.max() < 2 ** 24
        n, c, h, w = x.shape
        same = np.array_equal(C.layout_reference(k, transposed=True), C.reference(k))
        assert same == (c == 1 or h * w == 1), k['name']
        if k['mode'] == 'pad':
            assert C.reference(k).shape[1] == (c + 3) // 4 * 4 and not C.reference(k)[:, c:].any()
