"""CPU: the oracle of the depth-of-field frame tail (oracle/kenburns.py: _percentile, colorize_gray_r, the bokeh depth of bokeh_blur)
against the plain references of tests/frametail_cases.py on every case of tests/test_gpu_frametail.py, and the property each case
exists for: which counting path of the radix select it reaches (by the restated traversal), which route an alignment takes, the rank
structure a value kind claims.  A case that does not reach its path fails here, not silently on the GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import frametail_cases as C  # noqa: E402
from oracle import kenburns as okb  # noqa: E402

F32, F64 = np.float32, np.float64
PCT_CASES = C.percentile_cases()


# =====================================================================================================================================
# 1. percentiles
# =====================================================================================================================================
def test_percentile_case_list_is_what_the_suite_claims():
    """about 150 calls; every length with 'depth' and 'signed'; every kind at two lengths with every pair; t == 0.5 exactly"""
    assert 140 <= len(PCT_CASES) <= 160 and len(set(PCT_CASES)) == len(PCT_CASES)
    for kind in ('depth', 'signed'):
        assert {c[1] for c in PCT_CASES if c[0] == kind and c[2]} >= set(C.PCT_LENGTHS)
        assert {c[1] for c in PCT_CASES if c[0] == kind and not c[2]} >= set(C.PCT_OFFSET_LENGTHS)
    for kind in C.PCT_KINDS:
        for n in C.PCT_KIND_LENGTHS:
            assert {(c[3], c[4]) for c in PCT_CASES if c[0] == kind and c[1] == n and c[2]} >= set(C.PCT_PAIRS)
    assert F64(3 - 1) * (F64(25.0) / F64(100.0)) == 0.5 and ('depth', 3, True, 25.0, 25.0) in PCT_CASES
    assert C.four_ranks(3, 25.0, 75.0) == [0, 1, 1, 2]
    a = np.array([1.0, 4.0, 2.0], F32)
    assert C.percentile_ref(a, 25.0) == F32(1.5) and C.percentile_ref(a, 75.0) == F32(3.0)


@pytest.mark.parametrize("case", PCT_CASES, ids=C.percentile_id)
def test_oracle_percentile_equals_the_reference(case):
    """oracle/kenburns.py _percentile == percentile_ref (a sort of its own) == the shared sorted array's value, NaN equal to NaN"""
    kind, n, _, q_lo, q_hi = case
    a = C.percentile_values(kind, n)
    want = C.percentile_want(case)
    with np.errstate(invalid='ignore', over='ignore'):
        got = np.array([okb._percentile(a, q_lo), okb._percentile(a, q_hi)], F32)
    assert C.same(got, want), (got, want)
    if n <= 65539:
        assert C.same(np.array([C.percentile_ref(a, q_lo), C.percentile_ref(a, q_hi)]), want)
        if np.isfinite(a).all():                            # numpy's own percentile (>= 2 differs in the last digits: one ulp)
            ref = np.percentile(a.astype(F64), [q_lo, q_hi])
            assert np.all(np.abs(want.astype(F64) - ref) <= 2.0 * np.spacing(np.abs(want)).astype(F64)), (want, ref)


def test_percentile_values_hold_the_special_values():
    a = C.percentile_values('wide', 65539)
    u = a.view(np.uint32)
    for s in C.WIDE_SPECIAL:
        assert (u == np.array([s], F32).view(np.uint32)[0]).any(), s          # +0 and -0, denormals, +-FLT_MAX, +-inf by their bits
    assert not np.isnan(a).any() and (a > 0).any() and (a < 0).any()
    assert np.abs(a[np.isfinite(a) & (a != 0)]).min() < 1e-29 and np.abs(a[np.isfinite(a)]).max() == C.FLT_MAX
    for kind in C.PCT_KINDS:
        for n in C.PCT_KIND_LENGTHS:
            assert not np.isnan(C.percentile_values(kind, n)).any()          # NaN is outside the contract: no test feeds it
    assert np.unique(C.percentile_values('constant', 257)).size == 1
    assert np.unique(C.percentile_values('ties', 65539)).size == 9


def _rank_keys(kind, n, q_lo, q_hi):
    keys = np.sort(C.ordered_key(C.percentile_values(kind, n)))
    return keys[C.four_ranks(n, q_lo, q_hi)]


@pytest.mark.parametrize("n", C.PCT_KIND_LENGTHS)
def test_rank_structure_of_the_prefix_kinds(n):
    """computed from the sorted keys: 'one_prefix' -- the four ranks of (2, 85) share their 16-bit prefix but not their 24-bit one (one
    shared table in pass 2, several in pass 3); 'one_key24' -- they share 24 bits (one table in both passes); 'four_prefixes' -- four
    different 16-bit prefixes (no sharing), and three at (0, 100) where the upper ranks coincide"""
    k = _rank_keys('one_prefix', n, 2.0, 85.0)
    assert np.unique(k >> 16).size == 1 and np.unique(k >> 8).size > 1
    assert np.unique(C.ordered_key(C.percentile_values('one_prefix', n)) >> 16).size == 1
    k = _rank_keys('one_key24', n, 2.0, 85.0)
    assert np.unique(k >> 8).size == 1 and np.unique(C.ordered_key(C.percentile_values('one_key24', n)) >> 8).size == 1
    assert np.unique(C.percentile_values('one_key24', n)).size > 100
    for pair in ((2.0, 85.0), (50.0, 99.9)):
        assert len(set(C.four_ranks(n, *pair))) == 4 and np.unique(_rank_keys('four_prefixes', n, *pair) >> 16).size == 4
    assert np.unique(_rank_keys('four_prefixes', n, 0.0, 100.0) >> 16).size == 3
    assert np.unique(_rank_keys('four_prefixes', n, 100.0, 100.0) >> 16).size == 1
    # 'depth' (the frame loop's plane): a few prefixes, each shared by many elements
    assert 1 < np.unique(C.ordered_key(C.percentile_values('depth', n)) >> 16).size < 300


def test_traversal_visits_every_element_once_and_splits_as_the_kernel_does():
    for n in C.PCT_LENGTHS[:13]:
        for aligned in (True, False):
            tr = C.traversal(n, aligned)
            live = tr['calls'][tr['calls'] >= 0]
            assert np.array_equal(np.sort(live), np.arange(n)), (n, aligned)
            assert tr['grid'] == min(256, -(-n // 4096)) and tr['n4'] == (n // 4 if aligned else 0)
            tail = tr['calls'][tr['trip'] < 0]
            assert (tail[tail >= 0] >= tr['n4'] * 4).all() and tail[tail >= 0].size == n - tr['n4'] * 4
    assert C.traversal(3, True)['n4'] == 0 and C.traversal(4, True)['n4'] == 1 and C.traversal(7, True)['n4'] == 1
    assert C.traversal(4096, True)['grid'] == 1 and C.traversal(4097, True)['grid'] == 2          # the 4097 case runs two blocks
    t = C.traversal(4097, True)
    assert set(t['block']) == {0, 1} and (t['calls'][t['block'] == 1] >= 0).any()
    for n in C.PCT_OFFSET_LENGTHS:                                                                # the offset views: the scalar route
        tr = C.traversal(n, False)
        assert tr['n4'] == 0 and (tr['trip'] == -1).all()
    # one million: every block makes exactly one outer trip, all four unrolled loads live; + 4099: blocks 0 .. 3 make a second one
    t = C.traversal(1048576, True)
    assert t['grid'] == 256 and t['trip'].max() == 0 and (t['calls'] >= 0).all()
    t = C.traversal(1048576 + 4099, True)
    assert t['grid'] == 256 and t['trip'].max() == 1
    second = t['trip'] == 1
    assert sorted(set(t['block'][second])) == [0, 1, 2, 3]
    assert (t['calls'][second & (t['unroll'] == 0)] >= 0).all() and (t['calls'][second & (t['unroll'] > 0)] < 0).all()
    assert (t['trip'] == -1).sum() == 1 and (t['calls'][t['trip'] == -1] >= 0).sum() == 3         # the 3-element scalar tail: block 0
    assert C.traversal(1048576 + 4099, False)['trip'].max() == -1


def test_window_and_counting_paths_each_case_exists_for():
    """by the restated traversal of k_sel_top16: 'top' / 'bottom' hold a block whose LDS window is clipped at the end / at the start of
    the key space AND counts elements inside that window; N(0, 1) reaches the leader loop and its more-than-8-digits tail; a constant
    plane takes the one-add-per-wave path only; the unaligned views are visited completely too"""
    for n in C.PCT_KIND_LENGTHS:
        for aligned in (True, False) if n == 257 else (True,):
            a = C.percentile_values('top', n)
            wb = C.window_bases(a, C.traversal(n, aligned))
            assert (wb + C.K_WIN > C.K_FINE).any() and wb[0] + C.K_WIN > C.K_FINE
            p = C.top16_paths(a, aligned)
            assert p['visited'] and p['clipped_hi'] > n // (4 * max(1, wb.size)) and p['clipped_lo'] == 0
            a = C.percentile_values('bottom', n)
            wb = C.window_bases(a, C.traversal(n, aligned))
            assert wb[0] == 0
            p = C.top16_paths(a, aligned)
            assert p['visited'] and p['clipped_lo'] > n // (4 * max(1, wb.size)) and p['clipped_hi'] == 0
    assert (C.window_bases(C.percentile_values('top', 65539), C.traversal(65539, True))[:2] + C.K_WIN > C.K_FINE).all()
    # the other kinds never clip (what the issue found for the earlier inputs): it is these two that add the path
    for kind in ('depth', 'signed', 'ties', 'constant', 'one_prefix'):
        p = C.top16_paths(C.percentile_values(kind, 65539), True)
        assert p['visited'] and p['clipped_lo'] == 0 and p['clipped_hi'] == 0, kind
    p = C.top16_paths(C.percentile_values('signed', 65539), True)
    assert p['leaders'] > 0 and p['overflow'] > 0            # (both signs in every wave: one of them is outside any window)
    p = C.top16_paths(C.percentile_values('depth', 65539), True)
    assert p['mixed'] > 0 and p['leaders'] == 0              # a few neighbouring digits, all inside: per-lane LDS atomics
    p = C.top16_paths(C.percentile_values('constant', 65539), True)
    assert p['uniform'] > 0 and p['mixed'] == 0 and p['leaders'] == 0 and p['idle'] > 0
    p = C.top16_paths(C.percentile_values('wide', 65539), True)
    assert p['leaders'] > 0 and p['overflow'] > 0
    p = C.top16_paths(C.percentile_values('four_prefixes', 65539), False)
    assert p['visited'] and p['overflow'] > 0


# =====================================================================================================================================
# 2. colourise + statistics
# =====================================================================================================================================
def test_bokeh_stats_ref_on_hand_cases():
    assert C.bokeh_stats_ref([7], 100.0) == (7.0, -86.0, 0.0)                                     # one value: mx2 == 0
    assert C.bokeh_stats_ref([0, 255], -1.0) == (255.0, -1.0, 255.0)
    assert C.bokeh_stats_ref([0, 10, 255], 17.25) == (255.0, 17.25, 230.5)                        # t = 237.75, 247.75, 17.25
    assert C.bokeh_stats_ref(np.array([3, 3, 9], np.uint8), 255.0) == (9.0, -243.0, 6.0)


@pytest.mark.parametrize("kind", C.CS_PLANES)
def test_colorize_planes_are_what_they_claim_and_the_oracle_agrees(kind):
    lut = C.lut_gray_r()
    assert np.array_equal(lut, okb.gray_r_lut()) and lut[0] == 255 and lut[255] == 0
    for n in C.CS_PLANE_LENGTHS:
        v, vmin, vmax = C.colorize_plane(kind, n)
        b = C.colorize_bytes(kind, n)
        present = np.unique(b)
        if kind == 'flat':
            assert vmin == vmax and present.tolist() == [255] and C.bokeh_stats_ref(b, 17.25)[2] == 0.0
        elif kind == 'ends':
            assert present.tolist() == [0, 255]
        elif kind == 'noise':
            assert present[0] == 0 and present[-1] == 255 and present.size > 200
        else:
            uni = C.colorize_wave_uniform(b, n)
            assert present.size > 3
            if kind == 'spans':
                assert uni.all() and np.unique(b[:(n // 256) * 256].reshape(-1, 256)[:, 0]).size > 3
            else:
                assert (~uni).any(1).sum() == 1                                                    # exactly one wave trip is mixed
    # the oracle's colorize takes its own percentiles: equal to the reference evaluated at them, on a plane with a spread
    v, _, _ = C.colorize_plane('noise', 1025)
    lo, hi = okb._percentile(v, 2), okb._percentile(v, 85)
    assert lo == C.percentile_ref(v, 2) and hi == C.percentile_ref(v, 85) and lo < hi
    assert np.array_equal(okb.colorize_gray_r(v), C.colorize_ref(v, lo, hi))
    flat = np.full(300, F32(1.5))
    assert np.array_equal(okb.colorize_gray_r(flat), C.colorize_ref(flat, 1.5, 1.5))
    assert C.colorize_grid(262144) == 256 and C.colorize_grid(262140) == 256 and C.colorize_grid(261120) == 255
    assert C.colorize_grid(1) == 1 and C.colorize_grid(1025) == 2


# =====================================================================================================================================
# 3. bokeh depth
# =====================================================================================================================================
class _PassRecorder:
    """stands in for the oracle's C library inside bokeh_blur: keeps the depth plane the passes are given"""

    def __init__(self):
        self.depth = None

    def orc_bokeh_pass(self, src, depth, dst, H, W, ns, dx, dy):
        self.depth = depth.copy()
        dst[...] = src


@pytest.mark.parametrize("focal", C.CS_FOCALS)
def test_oracle_bokeh_depth_equals_the_reference(focal, monkeypatch):
    """the depth plane oracle/kenburns.py bokeh_blur hands to its passes (depth_factor 1, a focal plane) == bokeh_depth_ref fed with
    bokeh_stats_ref, bit for bit -- the statistics taken from the byte values that occur equal numpy's reductions over the plane"""
    rec = _PassRecorder()
    monkeypatch.setattr(okb.oseg, 'lib', lambda: rec)
    monkeypatch.setattr(okb, '_p', lambda a: a)
    for n, single in ((1, False), (17, False), (4097, False), (4097, True)):
        d8 = C.byte_plane(n, single)
        img = C.byte_image(n).reshape(1, n, 3)
        with np.errstate(invalid='ignore', divide='ignore'):
            okb.bokeh_blur(img, d8.reshape(1, n), 32, 10, focal, depth_factor=1)
        want, (dmax, mn, mx2) = C.bokeh_plane_ref(d8, focal)
        assert C.same_bits(rec.depth.reshape(-1), want), (n, single)
        if single or n == 1:
            assert mx2 == 0.0 and np.isnan(want).all()
        else:
            assert mx2 > 0.0 and np.isfinite(want).all() and want.min() == 0.0 and want.max() == F32(0.0005)
    assert set(np.unique(C.byte_plane(4097))) >= {0, 255}


# =====================================================================================================================================
# 4. masked median
# =====================================================================================================================================
@pytest.mark.parametrize("n,n_inst", C.MM_CASES)
def test_masked_cases_hold_every_kind(n, n_inst):
    d8, masks, kinds = C.masked_case(n, n_inst)
    want = C.masked_median_ref(d8, masks)
    assert set(np.unique(masks)) <= {0, 1, 2, 255}
    for k, kind in enumerate(kinds):
        cnt = int((masks[k] != 0).sum())
        if kind == 'empty':
            assert cnt == 0 and np.isnan(want[k])
        elif kind == 'single':
            assert cnt == 1 and want[k] == d8[n - 1]
        elif kind == 'even':
            assert cnt % 2 == 0 and cnt > 0
        elif kind == 'odd':
            assert cnt % 2 == 1 and want[k] == np.sort(d8[masks[k] != 0])[cnt // 2]
        elif kind == 'half':
            assert cnt == 4 and want[k] == 11.5
        elif kind == 'all255':
            assert cnt == 3 and want[k] == 255.0
    assert want[-1] == np.nanmax(want[:-1])
    if n >= 16 and n_inst >= 5:
        assert set(kinds) >= set(C.MM_KINDS[:5]) and set(np.unique(masks)) == {0, 1, 2, 255}
    empty = np.zeros((3, n), np.uint8)
    ref = C.masked_median_ref(d8, empty)
    assert np.isnan(ref[:3]).all() and ref[3] == -1.0


# =====================================================================================================================================
# 5. frames
# =====================================================================================================================================
def test_frames_cover_every_residue_of_the_pixel_count():
    assert sorted((H * W) % 4 for _, _, H, W in C.FRAMES) == [0, 1, 1, 2, 3]
    for name, _, H, W in C.FRAMES:
        c = C.frame_cloud(name)
        assert (c['H'], c['W']) == (H, W) and c['pts'].shape[0] == 3 and c['rgb'].shape == (3, c['pts'].shape[1])
        assert c['depth'].shape == (1, c['pts'].shape[1])
