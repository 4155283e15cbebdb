"""CPU: the oracle's convolutions (oracle/nets_oracle.c: orc_conv, orc_conv_fast, orc_conv_wino, orc_conv_wino4 behind one-layer
programs) against the plain float64 references of tests/conv_cases.py, on every case the GPU tests use -- and, for every case family,
what it exists for: the kernel class its shapes select (flags, ksplit, scratch, a tile configuration of each of the seven families that
does not fall back), and the planted faults its reference rejects by at least sixteen bounds.  The runner and the checks here are shared
with tests/test_gpu_conv.py.  Runs without a GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as C  # noqa: E402

from cartoonsegmentation_amd import program as P  # noqa: E402
from oracle import nets as onets  # noqa: E402

f32, f64 = np.float32, np.float64
MUTANT_DISTANCE = 16.0                                                     # bounds between a planted fault and the true reference


# ---- running a case ------------------------------------------------------------------------------------------------------------------
def oracle_run(b):
    """-> (output NCHW, {whole-buffer view: [n, h, w, C]}); the oracle's workspace starts as zeros"""
    out = np.zeros(b.out_shape, f32)
    want = [b.guard[0]] if b.guard else []
    return out, onets.run_program(b.prog, [np.ascontiguousarray(a, f32) for a in b.ext_in] + [out], want)


def result_of(k, run, is_guard, built=None):
    """the case's result as NHWC; where the layer writes a channel slice of a wider buffer, the slice holds the result and every other
    channel still holds what it was filled with (`is_guard`), or -- a residual slice written in place -- the residual tensor's neighbours"""
    b = C.program(k) if built is None else built
    y, views = run(b)
    got = np.ascontiguousarray(C.nhwc(y))
    if b.guard:
        wide, view = b.guard
        full = views[wide]
        lo, hi = view.coff, view.coff + view.c
        assert np.array_equal(full[..., lo:hi], got, equal_nan=True), k['name']
        assert is_guard(full[..., :lo]).all() and is_guard(full[..., hi:]).all(), "%s: a channel outside the output slice was written" % k['name']
    return got


def oracle_result(k):
    return result_of(k, oracle_run, lambda a: a == 0)


def check_case(k, got, what, variant=''):
    """finite; equal to the float32 rounding of the reference where the case is exact, inside max(4 e32, 8 * 2^-23) of max|ref|
    otherwise.  -> the error in units of the bound (0 for an exact case).  A failure names the case, the variant and that ratio"""
    ref = C.reference(k)
    assert got.shape == ref.shape, (what, k['name'], variant, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, k['name'], variant, "%d values are not finite" % int((~np.isfinite(got)).sum()))
    if k['exact']:
        want = ref.astype(f32)
        bad = got != want
        assert not bad.any(), (what, k['name'], variant, int(bad.sum()), got[bad][:4], want[bad][:4])
        return 0.0
    e32, err = C.e32(k), C.error(k, got)
    lim = C.bound(e32)
    print("%s %-28s %-14s err %.3g  e32 %.3g  bound %.3g  err / bound %.3g" % (what, k['name'], variant, err, e32, lim, err / lim))
    assert e32 <= lim
    assert err <= lim, "%s %s (%s): error %.3g = %.3g x the bound %.3g (e32 %.3g)" % (what, k['name'], variant, err, err / lim, lim, e32)
    return err / lim


def summary(what, family, cases, got):
    """one line per family: the range of e32, of the error and the worst error in units of its bound"""
    inexact = [(k, g) for k, g in zip(cases, got) if not k['exact']]
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
        check_case(k, g, 'oracle', C.variant(k))
    summary('oracle', family, cases, got)


def test_case_names_are_unique_and_shapes_stay_small():
    names = [k['name'] for k in C.all_cases()]
    assert len(set(names)) == len(names)
    for k in C.all_cases():
        n, h, w, cin = k['x'].shape
        big = k['name'] in ('f4_rule_80', 'sk_rule_k2048')                 # the two exceptions: an F(4x4)-by-rule 80 x 80 map, a 1x1 layer with K = 2048
        assert n <= 3 and (h * w <= 48 * 48 or big) and (cin <= 512 or big) and k['w'].shape[0] <= 512, k['name']


# ---- every class has a case that really selects it -----------------------------------------------------------------------------------
def test_flags_ksplit_and_scratch_of_every_family():
    op = {k['name']: C.conv_op(C.program(k)) for k in C.all_cases()}
    for k in C.direct_cases() + C.narrow_cases():
        assert (op[k['name']]['flags'], op[k['name']]['ksplit'], op[k['name']]['scratch']) == (0, 1, -1), k['name']
    assert all(k['w'].shape[0] <= 4 for k in C.narrow_cases()) and {k['w'].shape[0] for k in C.narrow_cases()} == {1, 2, 3, 4}
    # split-K: the rule's own choice (2, 4, and 16 for the K = 2048 1x1 layer) and the forced ones, each with its scratch view
    assert [op[n]['ksplit'] for n in ('sk_rule_9', 'sk_rule_18', 'sk_rule_k2048')] == [2, 4, 16]
    for k in C.splitk_cases():
        o = op[k['name']]
        assert o['flags'] == 0 and o['ksplit'] >= 2 and o['ksplit'] == (k['ksplit'] or o['ksplit']) and o['scratch'] >= 0, k['name']
        assert C.program(k).aux.c == o['ksplit'] * k['w'].shape[0]
    assert {op[k['name']]['ksplit'] for k in C.splitk_cases()} == {2, 4, 16}
    for k in C.stem_cases():
        assert op[k['name']]['flags'] == P.CONV_FLAG_STEM and op[k['name']]['cin_g'] == 4 and op[k['name']]['ksplit'] == 1, k['name']
    assert {k['x'].shape[-1] for k in C.stem_cases()} == {3, 4} and {(k['k'], k['stride']) for k in C.stem_cases()} >= {(7, 2), (3, 2), (3, 1), (16, 16)}
    # grouped: the block-diagonal form packs narrow groups into 32-channel super-groups; the vector kernel keeps the real groups
    for k in C.grouped_bd_cases():
        o = op[k['name']]
        assert o['flags'] == 0 and o['groups'] <= k['groups'] and o['cin_g'] == max(k['w'].shape[1], min(32, k['x'].shape[-1])), k['name']
    assert {k['w'].shape[1] for k in C.grouped_bd_cases()} >= {4, 8, 64} and any(k['stride'] == 2 for k in C.grouped_bd_cases())
    for k in C.grouped_valu_cases():
        o = op[k['name']]
        refused = k['out_slice'] is not None and (k['out_slice'][0] % 4 != 0 or sum(k['out_slice']) % 4 != 0)
        assert bool(o['flags'] & P.CONV_FLAG_GROUPED) == (not refused), k['name']
        assert (o['groups'], o['cin_g']) == ((k['groups'], k['w'].shape[1]) if not refused else (1, 32)), k['name']
    assert P.GROUPED_VALU_MAX_CG == 16 and {k['w'].shape[1] for k in C.grouped_valu_cases()} == {8, 16, 32}
    assert all((k['w'].shape[1] == 32) == (k['max_cg'] == 32) for k in C.grouped_valu_cases())
    widths = {k['x'].shape[2] for k in C.grouped_valu_cases()}                                 # launch_conv_grouped: the 40-pixel tile when it pads the row no more
    assert any(-(-w // 40) * 40 <= -(-w // 32) * 32 for w in widths) and any(-(-w // 40) * 40 > -(-w // 32) * 32 for w in widths)
    assert {k['x'].shape[1:3] for k in C.grouped_valu_cases()} >= {(6, 7), (1, 1)}
    for k in C.f2_cases():
        assert op[k['name']]['flags'] == P.CONV_FLAG_WINOGRAD and op[k['name']]['ksplit'] == 1, k['name']
    for k in C.f4_cases():
        assert op[k['name']]['flags'] == P.CONV_FLAG_WINOGRAD4 and op[k['name']]['ksplit'] == 1, k['name']
    rule = [k for k in C.f4_cases() if k['lower'] == 'rule']                                   # the shipped rule, nothing forced
    assert {(k['x'].shape[1], k['x'].shape[3], k['w'].shape[0]) for k in rule} == {(23, 128, 128), (23, 512, 128), (80, 64, 64)}
    assert any(op[k['name']]['scratch'] >= 0 for k in C.f4_cases()) and op['f4_rule_80']['scratch'] >= 0
    for name in ('f2', 'f4'):
        shapes = {(k['x'].shape[0], k['x'].shape[1:3], k['x'].shape[3], k['w'].shape[0]) for k in C.FAMILIES[name]()}
        assert shapes >= set(C.WINO_SHAPES)
    # the epilogue cross: every activation x res_mode on one layer per class, and the class is the one its name says
    want = dict(direct=(0, 1), splitk=(0, 4), narrow=(0, 1), stem=(P.CONV_FLAG_STEM, 1), grouped_bd=(0, 1), grouped_valu=(P.CONV_FLAG_GROUPED, 1),
                f2=(P.CONV_FLAG_WINOGRAD, 1), f4=(P.CONV_FLAG_WINOGRAD4, 1))
    seen = set()
    for k in C.epilogue_cases():
        assert (op[k['name']]['flags'], op[k['name']]['ksplit']) == want[k['cls']], k['name']
        assert op[k['name']]['act'] == P.ACT[k['act']] and op[k['name']]['res_mode'] == k['res_mode']
        seen.add((k['cls'], k['act'], k['res_mode']))
    assert len(seen) == len(want) * len(C.ACTS) * 3
    # views: every class that accepts them has an input slice (ld > c), an output slice at a multiple of 4, a residual slice of another
    # pitch and out is res; the grouped and Winograd classes also an output at channel offset 2 and one of pitch c + 6
    for fam in ('direct', 'splitk', 'grouped_bd', 'grouped_valu', 'f2', 'f4'):
        cs = C.FAMILIES[fam]()
        assert any(k['in_slice'] for k in cs) and any(k['out_slice'] and k['out_slice'][0] % 4 == 0 for k in cs) and any(k['inplace'] for k in cs), fam
        assert any(k['res_slice'] and k['out_slice'] is None and not k['inplace'] for k in cs), fam
        assert {v for k in cs for v in C.VALUES if k['name'].endswith(v)} == set(C.VALUES), fam
    for fam in ('grouped_valu', 'f2', 'f4'):
        cs = C.FAMILIES[fam]()
        assert any(k['out_slice'] == (2, 6) for k in cs) and any(k['out_slice'] == (4, 2) for k in cs), fam
    assert any(k['out_slice'] == (4, 2) and k['w'].shape[0] == 32 for k in C.grouped_valu_cases())      # a 38-channel buffer


def test_each_tile_family_has_a_case_and_a_configuration_that_does_not_fall_back():
    """csm_debug_conv_resolve_cfg (host only): for each of the seven families a direct case on which its forced configuration is the
    one that runs; and where a forced configuration cannot run a case, another family's does (the GPU test runs both)"""
    table = C.cfg_table()
    assert {c['family'] for c in table.values()} == set(C.TILE_FAMILIES)
    assert [table[n]['family'] for n in C.FORCED_CFGS] == list(C.TILE_FAMILIES)
    runs = {fam: [] for fam in C.TILE_FAMILIES}
    for k in C.direct_cases() + C.splitk_cases() + C.narrow_cases():
        for name in C.FORCED_CFGS:
            got = C.resolve_cfg(k, name)
            assert C.variant(k, name) == got['family']
            if got['name'] == name:
                runs[table[name]['family']].append(k['name'])
    for fam, names in runs.items():
        print("%-8s %d cases without fall-back, e.g. %s" % (fam, len(names), names[:3]))
        assert names, fam
    assert 'd_3x3_18' in runs['WS'] and 'd_3x3_18' in runs['PATCH'] and 'd_1x1_m63' in runs['DMA_P'] and 'd_dil2' not in runs['PATCH']
    assert set(runs['NARROW']) <= {k['name'] for k in C.narrow_cases()} and len(runs['NARROW']) >= 8


# ---- the references themselves -------------------------------------------------------------------------------------------------------
def test_transform_matrices_are_a_convolution():
    """A^T [(G g) * (B^T d)] = the 1-D correlation of d with g for both Winograd sizes, in exact rational arithmetic: the matrices wino32
    evaluates are the contract's"""
    rng = np.random.default_rng(0)
    for m, W in C.WINO.items():
        t = m + 2
        BT, AT = W['BT'], W['AT']
        G = [[Fraction(v).limit_denominator(24) for v in row] for row in W['G']]
        d = [Fraction(int(v)) for v in rng.integers(-9, 9, t)]
        g = [Fraction(int(v)) for v in rng.integers(-9, 9, 3)]
        v = [sum(BT[i][j] * d[j] for j in range(t)) for i in range(t)]
        u = [sum(G[i][j] * g[j] for j in range(3)) for i in range(t)]
        assert [sum(AT[a][i] * u[i] * v[i] for i in range(t)) for a in range(m)] == [sum(d[a + j] * g[j] for j in range(3)) for a in range(m)]
        # and program.py's weight transform is G g G^T
        w = rng.standard_normal((1, 1, 3, 3)).astype(f32)
        U = (P.wino_transform if m == 2 else P.wino4_transform)(w).reshape(t, t)
        assert np.allclose(U, np.array(W['G']) @ w[0, 0].astype(f64) @ np.array(W['G']).T, rtol=1e-6, atol=1e-7)


def test_one_hot_cases_are_the_shifted_input_and_give_every_tap_its_turn():
    taps = {}
    for k in C.onehot_cases():
        w = k['w']
        assert set(np.unique(w)) == {0.0, 1.0} and (w.reshape(w.shape[0], -1).sum(1) == 1).all() and k['b'] is None and k['act'] in C.EXACT_ACTS
        # the window picked by hand is what F.conv2d gives in float64 (a sum of one term and zeros)
        assert np.array_equal(C.onehot_expected(k).astype(f64), C.conv64(k)), k['name']
        key = k['name'].rsplit('_o', 1)[0]
        taps.setdefault(key, (k['k'], set()))[1].update(w.reshape(w.shape[0], w.shape[1], -1).sum(1).argmax(1).tolist())
        if k['x'].shape[1] * k['x'].shape[2] > 1 and k['k'] > 1:           # another tap is another window: a shifted tap shows as plain inequality
            k2 = dict(k, w=np.roll(w.reshape(w.shape[0], w.shape[1], -1), 1, 2).reshape(w.shape))
            assert not np.array_equal(C.onehot_expected(k2), C.onehot_expected(k)), k['name']
    for key, (kk, seen) in taps.items():
        assert seen == set(range(kk * kk)), (key, sorted(seen))
    fams = {k['name'].split('_')[1].rstrip('0123456789') for k in C.onehot_cases()}
    assert fams == {'d', 'sk', 'nr', 'st', 'gb', 'gv'}


# ---- each family's cases show the mistakes they exist for ---------------------------------------------------------------------------
# fault -> the families whose cases are meant for it (every case of the family that can show the fault must)
MEANT_FOR = dict(tap=('direct', 'splitk', 'narrow', 'stem', 'grouped_bd', 'grouped_valu', 'f2', 'f4'),
                 pad=('direct', 'splitk', 'narrow', 'stem', 'grouped_bd', 'grouped_valu', 'f2', 'f4'),
                 phase=('direct', 'narrow', 'stem', 'grouped_bd'), dil=('direct', 'narrow'), groups=('grouped_bd', 'grouped_valu'),
                 lastchunk=('direct', 'splitk'), run_dropped=('splitk',), run_doubled=('splitk',),
                 tail=('direct', 'splitk', 'narrow', 'stem', 'grouped_bd', 'grouped_valu', 'f2', 'f4', 'lowerings', 'epilogue'),
                 bias_after=('direct', 'splitk', 'stem', 'f2', 'f4', 'epilogue'), res_swapped=('direct', 'splitk', 'f2', 'f4', 'epilogue'),
                 stem_transposed=('stem',))


def mutant_distances(scale_bound=1.0):
    """{fault: (cases that show it, the smallest distance from the true reference in units of the case's bound)}"""
    out = {}
    for kind, fams in MEANT_FOR.items():
        n, worst = 0, np.inf
        for fam in fams:
            for k in C.FAMILIES[fam]():
                m = C.mutant(k, kind, C.conv_op(C.program(k))['ksplit'])
                if m is None:
                    continue
                d = C.error(k, m) / (scale_bound * C.bound(C.e32(k)))
                assert d >= MUTANT_DISTANCE, "%s: the fault '%s' moves the reference by %.3g bounds only" % (k['name'], kind, d)
                n, worst = n + 1, min(worst, d)
        out[kind] = (n, worst)
    return out


def test_planted_faults_lie_sixteen_bounds_from_the_reference():
    assert set(MEANT_FOR) == set(C.MUTANTS)
    for kind, (n, worst) in mutant_distances().items():
        print("fault %-16s %3d cases, at least %.3g bounds away" % (kind, n, worst))
        assert n >= 2, kind
