"""No GPU: the numpy restatement of the autozoom coverage count (tests/autozoom_restatement.py) against the C oracle (oracle/warp.py)
on every case of tests/autozoom_cases.py, the hand-placed cases against the counts written down by hand, deliberately wrong
variants of the restatement against the cases that have to notice them, and the derivations the cases rest on (band_geom's width
classes, the entry cache, the segment capacity) against the kernel's source text."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import autozoom_cases as K  # noqa: E402
import autozoom_restatement as A  # noqa: E402
import warptile_restatement as R  # noqa: E402
from oracle import warp as orc  # noqa: E402

F, D = np.float32, np.float64
SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cartoonsegmentation_amd", "csrc", "autozoom.hip")


def _s32(shifts):
    return np.asarray(shifts, D).reshape(-1, 3).astype(F)


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.CASES)
def test_restatement_against_the_oracle(name):
    c = K.case(name)
    H, W, pts = c['H'], c['W'], c['pts']
    ones = np.ones((1, 1, pts.shape[1]), F)
    for k, s in enumerate(_s32(c['shifts'])):
        mask = A.coverage_mask(pts, s, H, W, c['focal'], c['baseline'])
        moved = np.stack(R.process_shift(pts, s))[None]
        existing = orc.render_pointcloud(moved, ones, W, H, c['focal'], c['baseline'], degrid_mode=1)[1][0, 0]
        bad = mask != (existing > 0)
        assert not bad.any(), "%s candidate %d: %d pixels differ, first (y, x) = %s; restated count %d, oracle %d" % (
            name, k, int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)), int(mask.sum()), int((existing > 0).sum()))
    assert len(K.restated(name)) == len(c['shifts'])


def test_nonfinite_points_count_for_nothing():
    c = K.case('nonfinite')
    fin = np.isfinite(c['pts']).all(0)
    assert 0 < (~fin).sum() < fin.size
    assert K.restated('nonfinite') == tuple(A.coverage_counts(c['pts'][:, fin], c['shifts'], c['H'], c['W'], c['focal'], c['baseline']))


def test_cases_leave_holes_and_cover_something():
    """the sparse clouds neither cover the frame nor leave it empty, so a count says something"""
    for name in tuple(K.GEOMETRY) + K.GROUPING + ('recache', 'near_zero', 'tiny_err', 'nonfinite'):
        c = K.case(name)
        for n in K.restated(name):
            assert 0 < n <= c['H'] * c['W'], name
        if name != 'recache' and K.restated(name):
            assert max(K.restated(name)) < c['H'] * c['W'], name
    assert set(K.restated('empty')) == {0} and K.restated('k0') == ()
    assert len(set(K.restated('group_16x16'))) > 16                    # the candidates of the full batch are told apart


# ---- the hand-placed cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.HAND)
def test_hand_placed_counts_are_the_literals(name):
    c = K.case(name)
    assert c['br'] == 8 and (c['H'], c['W']) == (16, 64)
    assert list(K.restated(name)) == c['literal'], name


def test_place_is_exact():
    x, y, z = K.place(20.0, 6.0, K.E0 + 0.5)
    ok, fx, fy, err = R.project(*R.process_shift(K._pts((x, y, z)), K.ZERO), K.HH, K.HW, K.FOCAL, K.BASELINE)
    assert ok[0] and fx[0] == F(20.0) and fy[0] == F(6.0) and err[0] == F(K.E0 + 0.5)


# ---- wrong variants of the restatement ---------------------------------------------------------------------------------------------

def degrid_loop(zee, both_ends=True, in_place=False):
    """updateDegrid pixel by pixel.  both_ends=False: a line counts when one of its ends is inside (the other one reads 0);
    in_place=True: raster order on the buffer itself (models/utils.py:152-212 taken literally, one interleaving of its race)"""
    H, W = zee.shape
    src = zee.astype(F).copy()
    out = src if in_place else src.copy()
    for y in range(H):
        for x in range(W):
            c = src[y, x]
            cnt, s = 0, F(0.0)
            for ox, oy in ((1, 0), (0, 1), (1, 1), (1, -1)):
                ends = []
                for xx, yy in ((x + ox, y + oy), (x - ox, y - oy)):
                    inside = 0 <= xx < W and 0 <= yy < H
                    ends.append((inside, src[yy, xx] if inside else F(0.0)))
                (ia, a), (ib, d) = ends
                if not ((ia and ib) if both_ends else (ia or ib)):
                    continue
                if D(c) >= D(a) + 1.0 and D(c) >= D(d) + 1.0:
                    cnt += 2
                    s = F(F(s + a) + d)
            if cnt > 0:
                out[y, x] = min(c, F(s / F(cnt)))
    return out


def degrid_without_halo(br):
    def f(zee):
        zd = R.degrid(zee).copy()
        for r0 in range(br, zee.shape[0], br):                           # the first row of a band sees 1e6 in the row above
            cut = zee.copy()
            cut[r0 - 1] = F(1000000.0)
            zd[r0] = R.degrid(cut)[r0]
        return zd
    return f


def count_band_windows(br):
    def f(mask):                                                         # every band counts its halo rows too
        return sum(int(mask[max(r0 - 1, 0):r0 + br + 1].sum()) for r0 in range(0, mask.shape[0], br))
    return f


def argmax_reversed(w):
    nw, ne, sw, se = w
    conds = [(se >= nw) & (se >= ne) & (se >= sw), (sw >= nw) & (sw >= ne) & (sw >= se),
             (ne >= nw) & (ne >= sw) & (ne >= se), (nw >= ne) & (nw >= sw) & (nw >= se)]
    return np.select(conds, [3, 2, 1, 0], default=-1)


def mutants(br):
    return {
        'z-test strict <': dict(ztest=lambda e, z: e.astype(D) < z.astype(D) + 1.0),
        'z-test + 0.0': dict(ztest=lambda e, z: e.astype(D) <= z.astype(D) + 0.0),
        'degrid in place (raster)': dict(degrid=lambda z: degrid_loop(z, in_place=True)),
        'degrid line with one end inside': dict(degrid=lambda z: degrid_loop(z, both_ends=False)),
        'mark on w >= 0': dict(positive=lambda w: F(1.0) * w >= F(0.0)),
        'arg-max ties in the opposite order': dict(argmax=argmax_reversed),
        'halo dropped': dict(degrid=degrid_without_halo(br)),
        'shared rows counted twice': dict(count=count_band_windows(br)),
        'fy < 0 discarded': dict(keep=lambda fx, fy: fy >= F(0.0)),
    }


# mutant -> the named cases that have to notice it: a hand-placed one built for it and, where one does, a generated cloud
CAUGHT_BY = {
    'z-test strict <': ('hand_degrid_line',),
    'z-test + 0.0': ('hand_degrid_line',),
    'degrid in place (raster)': ('hand_degrid_order',),
    'degrid line with one end inside': ('hand_edge_line',),
    'mark on w >= 0': ('hand_centre',),
    'arg-max ties in the opposite order': ('hand_argmax_tie',),
    'halo dropped': ('hand_degrid_line', 'group_17x1'),
    'shared rows counted twice': ('hand_seam', 'group_17x1'),
    'fy < 0 discarded': ('hand_north', 'exact'),
}


def test_degrid_loop_is_the_restated_degrid():
    """the scalar loop the degrid mutants are made from is, unmutated, the restatement's degrid"""
    c = K.case('short')
    g = np.random.default_rng(3)
    zee = np.where(g.random((c['H'], c['W'])) < 0.5, F(1000000.0), g.uniform(999940, 999990, (c['H'], c['W'])).astype(F)).astype(F)
    assert np.array_equal(degrid_loop(zee), R.degrid(zee))
    assert not np.array_equal(degrid_loop(zee, in_place=True), R.degrid(zee))


@pytest.mark.parametrize("mutant", list(CAUGHT_BY))
def test_every_mutant_is_caught_by_a_named_case(mutant):
    assert set(CAUGHT_BY) == set(mutants(8))
    for name in CAUGHT_BY[mutant]:
        c = K.case(name)
        got = A.coverage_counts(c['pts'], c['shifts'], c['H'], c['W'], c['focal'], c['baseline'], **mutants(c['br'])[mutant])
        assert tuple(got) != K.restated(name), "mutant '%s' gives the restated counts %s on %s" % (mutant, got, name)


# ---- the derivations the cases rest on -------------------------------------------------------------------------------------------

def test_band_geom_classes_are_those_of_the_kernel_source():
    text = open(SRC).read()
    found = re.findall(r"\(2 \* (\d+) \+ 2\) \* W \* 4 <= (\d+) \* 1024\) bg\.br = (\d+);", text)
    assert [(int(a), int(b)) for a, b, _ in found] == list(K.BAND_CLASSES) and all(a == c for a, _, c in found), found
    assert "if (W % 2) return bg;" in text
    assert re.search(r"kBandLds = (\d+) \* 1024;", text).group(1) == str(K.LDS_KIB)
    assert re.search(r"kGroupMax = (\d+), kPerGroup = (\d+);", text).groups() == (str(K.GROUP_MAX), str(K.PER_GROUP))
    assert re.search(r"kMaxChunk = (\d+);", text).group(1) == str(K.MAX_CHUNK)
    assert "(int64_t)(per_band * 3.0) + 1023" in text and "(double)N * (bg.br + 3) / (double)H" in text
    assert "cap < 4096 ? 4096" in text and "(kBandLds - window) / 16" in text
    # the thresholds, recomputed: 18 W 4 <= 40 KiB, 10 W 4 <= 48 KiB, 6 W 4 <= 72 KiB
    assert (K.last_width(8), K.last_width(4), K.last_width(2)) == (568, 1228, 3072)
    for br in (8, 4, 2):
        assert K.band_rows(K.last_width(br)) == br and K.band_rows(K.last_width(br) + 2) == {8: 4, 4: 2, 2: 0}[br]
    for name, (H, W, br, _) in K.GEOMETRY.items():
        c = K.case(name)
        assert (c['H'], c['W'], c['br'], c['band']) == (H, W, br, int(br > 0)), name
    g = K.GEOMETRY
    assert g['br8_max'][1] == K.last_width(8) and g['br4_min'][1] == K.last_width(8) + 2
    assert g['br4_max'][1] == K.last_width(4) and g['br2_min'][1] == K.last_width(4) + 2
    assert g['br2_max'][1] == K.last_width(2) and g['unsupported'][1] == K.last_width(2) + 2
    assert g['one_px_rows'][0] < 8 and g['short'][0] < 8 and g['exact'][0] == 8 and g['ragged8'][0] % 8 == 1 and g['ragged8'][1] % 4 == 2
    assert g['br4_min'][0] % 4 == 1 and g['br2_min'][0] % 2 == 1 and g['pitch4'][1] % 4 == 2
    H, W = g['odd'][:2]
    assert W % 2 == 1 and (H * W) % 4 != 0
    assert g['pitch4'][1] < g['br4_max'][1] and g['unsupported'][0] * g['unsupported'][1] % 4 != 0


def test_grouping_cases_select_their_paths():
    def groups(shifts):
        """the launch batches of csm_autozoom_coverage_bands: candidates sorted by sy, <= PER_GROUP per group, <= GROUP_MAX groups"""
        sy = sorted(float(F(s[1])) for s in shifts)
        out, i = [], 0
        while i < len(sy):
            n = 1
            while i + n < len(sy) and n < K.PER_GROUP and sy[i + n] == sy[i]:
                n += 1
            out.append(n); i += n
        return [out[j:j + K.GROUP_MAX] for j in range(0, len(out), K.GROUP_MAX)]
    sh = {n: K.case(n)['shifts'] for n in K.GROUPING}
    assert groups(sh['group_17x1']) == [[16, 1]]
    assert groups(sh['group_1x17']) == [[1] * 16, [1]]
    assert groups(sh['group_16x16']) == [[16] * 16]
    assert groups(sh['group_257']) == [[16] * 5 + [16, 1] + [16] * 9, [16]]
    assert groups(sh['group_shuffled']) in ([[16, 1, 16, 2]], [[16, 2, 16, 1]]) and len(sh['group_shuffled']) == 35
    assert len(set(sh['group_shuffled'])) == 34 and sh['group_shuffled'] != sorted(sh['group_shuffled'], key=lambda s: s[1])
    assert groups(sh['k1']) == [[1]] and sh['k0'] == []
    assert len(sh['planes_k33']) == K.MAX_CHUNK + 1 and K.case('planes_k33')['chunks'] == (None, 32, 5, 1)
    for n in K.CASES:
        assert len({s[2] for s in K.case(n)['shifts']}) <= 1 and len(K.case(n)['shifts']) <= 40 or n in ('group_16x16', 'group_257')


def test_load_cases_reach_the_cache_and_the_capacity():
    c = K.case('recache')
    g = K.band_geom(c['H'], c['W'], c['pts'].shape[1])
    assert g == dict(br=8, nbands=2, cap=41984, ncache=(150 * 1024 - 18 * 64 * 4) // 16)
    for sy in {s[1] for s in c['shifts']}:
        n = K.band_entries(c, sy)
        assert n.min() > g['ncache'] and n.max() <= g['cap'], (sy, n, g)
    c = K.case('pileup')
    g = K.band_geom(c['H'], c['W'], c['pts'].shape[1])
    assert g['cap'] == 4096 and c['overflow']
    for sy in {s[1] for s in c['shifts']}:
        assert K.band_entries(c, sy).max() > g['cap']
    for name in K.CASES:                                                # no other case overflows: the band path answers them itself
        c = K.case(name)
        if name != 'pileup' and c['band'] and c['pts'].shape[1]:
            g = K.band_geom(c['H'], c['W'], c['pts'].shape[1])
            for sy in {s[1] for s in c['shifts']}:
                assert K.band_entries(c, sy).max() <= g['cap'], name


def test_tiny_case_has_tiny_z_buffer_values_beside_degridded_pixels():
    c = K.case('tiny_err')
    for s in _s32(c['shifts']):
        zee, _ = A.zbuffer(c['pts'], s, c['H'], c['W'], c['focal'], c['baseline'])
        tiny = K.is_tiny(zee)
        near = np.zeros_like(tiny)                                       # the pixels that read a tiny value: itself and its 8 neighbours
        pad = np.pad(tiny, 1)
        for dy in range(3):
            for dx in range(3):
                near |= pad[dy:dy + tiny.shape[0], dx:dx + tiny.shape[1]]
        changed = R.degrid(zee) != zee
        assert tiny.sum() >= 20 and (changed & near).sum() >= 10 and (changed & tiny).sum() >= 1, (int(tiny.sum()), int((changed & near).sum()))
        seen = zee[zee < 1e6]
        assert np.abs(seen).max() < 4.0 and (seen < 0).sum() >= 100 and (seen > 0).sum() >= 100
    zee, _ = A.zbuffer(K.case('near_zero')['pts'], _s32(K.case('near_zero')['shifts'])[0], 64, 96, K.FOCAL, K.BASELINE)
    assert 60.0 < zee.min() and zee[zee < 1e6].max() < 80.0              # 'near_zero' keeps the other test's cloud: see autozoom_cases


def test_search_case_has_ties_at_the_top():
    """the cloud of the search case covers the whole frame for several candidates, and not for the first one"""
    s = K.search_case()
    cands, shifts = K.search_candidates(s)
    counts = A.coverage_counts(s['pts'], shifts, s['H'], s['W'], K.FOCAL, K.BASELINE)
    best = max(counts)
    assert best == s['H'] * s['W'] and counts.count(best) >= 4 and counts[0] < best and len(set(counts)) >= 3
    assert 16 <= len(cands) < 256
