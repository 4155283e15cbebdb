"""No GPU: the numpy restatement of the tile renderer (tests/warptile_restatement.py) against the C oracle (oracle/warp.py) on every
case of tests/warptile_cases.py, its integer sums against the exact sums, and every case against the property it exists for --
so that the bit-for-bit comparisons of tests/test_gpu_warptile.py cannot be empty."""
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warptile_cases as K  # noqa: E402
import warptile_restatement as R  # noqa: E402
from oracle import warp as orc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = list(K.CASES)


def _rgbd(c):
    return np.concatenate([c['rgb'], c['depth']])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_oracle(name):
    c, rs = K.case(name), K.restated(name)
    H, W, f, b = c['H'], c['W'], c['focal'], c['baseline']
    ps = K.shifted_points(name)
    assert np.array_equal(ps, orc.process_shift(c['pts'][None], c['shift'])[0], equal_nan=True)
    zee = orc.update_zee(ps[None], H, W, f, b)
    assert np.array_equal(rs['zee'], zee[0, 0])
    assert np.array_equal(rs['zd'], orc.degrid(zee, 1)[0, 0])
    ro, eo = orc.render_pointcloud(ps[None], _rgbd(c)[None], W, H, f, b, degrid_mode=1)
    assert np.array_equal(rs['existing'] > 0, eo[0, 0] > 0)
    # the oracle's sequential fp32 sums and the fixed-point sums both approximate the exact quotient (bounds: warptile_cases)
    q = K.exact_quotient(rs)
    assert np.all(np.abs(ro[0].astype(np.float64) - q) <= K.float_bound(rs))
    assert np.all(np.abs(rs['render'].astype(np.float64) - q) <= K.fixed_bound(rs))
    n = rs['n'].astype(np.float64)
    assert np.all(np.abs(eo[0, 0].astype(np.float64) - rs['S'][4]) <= n * 2.0 ** -23 * rs['S'][4])
    assert np.all(np.abs(rs['existing'].astype(np.float64) - rs['S'][4]) <= n * 2.0 ** -40 + 2.0 ** -24 * rs['S'][4])
    # the hole fill: same input, same bits
    filled = orc.fill_disocclusion(rs['render'][None], rs['mdepth'][None, None])[0]
    assert np.array_equal(filled, rs['render_filled'])
    assert np.array_equal(rs['frame'], R.to_u8(filled[:3]).transpose(1, 2, 0))


@pytest.mark.parametrize("name", NAMES)
def test_integer_sums_against_the_exact_sums(name):
    """truncation loses less than one unit per term (a product below one unit becomes one unit: still less than one unit off); the
    float64 running sum S of n exact products is itself within n 2^-53 A of their sum"""
    rs = K.restated(name)
    n = rs['n'].astype(np.float64)
    for c in range(5):
        unit = 1.0 / (rs['scales'][c] if c < 4 else R.SCALE_C)
        acc = rs['acc'][c] if c < 4 else rs['wacc']
        assert np.all(np.abs(acc.astype(np.float64) * unit - rs['S'][c]) <= n * unit + n * 2.0 ** -53 * rs['A'][c]), c


@pytest.mark.parametrize("name", K.CHANNEL_CASES)
def test_channel_restatement_against_the_oracle(name):
    c = K.case(name)
    rs = K.restated_channels(name, 9, False)
    ro, eo = orc.render_pointcloud(K.shifted_points(name)[None], K.channel_data(name, False)[None, :9], c['W'], c['H'], c['focal'],
                                   c['baseline'], degrid_mode=1)
    assert np.array_equal(rs['existing'] > 0, eo[0, 0] > 0)
    q = K.exact_quotient(rs)
    assert np.all(np.abs(ro[0].astype(np.float64) - q) <= K.float_bound(rs))
    assert np.all(np.abs(rs['render'].astype(np.float64) - q) <= K.fixed_bound(rs))
    # the saturating contribution: one term of 2^62 units in channel 0, the other channels and the weight untouched
    sat = K.restated_channels(name, 9, True)
    data = K.channel_data(name, True)
    p = int(np.nonzero(data[0] == np.float32(2.0 ** 33))[0][0])
    k = int(np.nonzero(sat['idx'] == p)[0][0])
    assert sat['passed'][0, k] and float(sat['w'][0, k]) * 2.0 ** 33 >= 2.0 ** 31
    y, x = int(sat['y0'][k]), int(sat['x0'][k])
    assert sat['acc'][0, y, x] - rs['acc'][0, y, x] > 2 ** 61
    assert np.array_equal(sat['acc'][1:], rs['acc'][1:]) and np.array_equal(sat['wacc'], rs['wacc'])


def test_hole_fill_reproduces_the_fixtures():
    g = np.load(os.path.join(GOLDEN, "discfill_48x40.npz"))
    for b in range(g['img'].shape[0]):
        assert np.array_equal(R.fill_disocclusion(g['img'][b], g['depth'][b, 0]), g['out'][b])
    paths = sorted(glob.glob(os.path.join(GOLDEN, "warp_*_c4*.npz")))
    assert len(paths) >= 3
    for p in paths:
        g = np.load(p)
        for b in range(g['render'].shape[0]):
            assert np.array_equal(R.fill_disocclusion(g['render'][b], g['fill_depth'][b, 0]), g['filled'][b]), p


def test_roundf_is_half_away_from_zero():
    f = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, -0.49999997, 8388607.5], np.float32)
    assert R._roundf(f).tolist() == [1, 2, 3, -1, -2, 0, 0, 8388608]


# ---- every case has the property it exists for --------------------------------------------------------------------------------------

def _contributing(rs):
    return rs['passed'].any(0)


def test_seams_footprints_straddle_every_seam():
    for name in ('seams', 'patched_grid', 'two_layers'):
        rs, c = K.restated(name), K.case(name)
        live = _contributing(rs)
        for x in range(31, c['W'] - 1, 32):
            assert (live & (rs['x0'] == x) & (rs['w'][0] > 0) & (rs['w'][1] > 0)).sum() > 0, (name, x)
        for y in range(15, c['H'] - 1, 16):
            assert (live & (rs['y0'] == y) & (rs['w'][0] > 0) & (rs['w'][2] > 0)).sum() > 0, (name, y)
    c = K.case('seams')
    assert (c['H'] % R.TH, c['W'] % R.TW) == (13, 6)
    rs = K.restated('seams')
    assert (rs['zd'] != rs['zee']).sum() > 100 and len(rs['holes']) > 20


def test_tiny_sizes():
    assert [(K.case(n)['H'], K.case(n)['W']) for n in ('tiny_1x1', 'tiny_16x32', 'tiny_17x33', 'tiny_33x17')] == \
        [(1, 1), (16, 32), (17, 33), (33, 17)]
    for n in ('tiny_1x1', 'tiny_16x32', 'tiny_17x33', 'tiny_33x17'):
        rs = K.restated(n)
        assert (rs['existing'] > 0).all() or len(rs['holes']) > 0
        assert (rs['existing'][-1] > 0).any() and (rs['existing'][:, -1] > 0).any()      # the one-row / one-column tiles are hit


def test_patched_clouds():
    H, W = 40, 96
    sizes = {'patched_grid': H * W, 'patched_plus': H * W + 3001, 'patched_minus': H * W - 977}
    for n, N in sizes.items():
        c = K.case(n)
        assert (c['H'], c['W']) == (H, W) and W % 32 == 0 and c['pts'].shape[1] == N
    # whole 16-row bands are visited patch-wise, the rest linearly (make_point_map of csrc/warptile.hip: kPatchH = 16): two bands and
    # eight rows of the full grid, one band and 1327 points of the truncated one
    assert (H * W) // (16 * W) == 2 and H - 32 == 8 and sizes['patched_minus'] // (16 * W) == 1
    assert _contributing(K.restated('patched_plus'))[K.restated('patched_plus')['idx'] >= H * W].sum() > 500


def test_two_layers_blend_strip_and_crowded_tiles():
    c, rs = K.case('two_layers'), K.restated('two_layers')
    P = c['H'] * c['W']
    assert c['pts'].shape[1] == 2 * P
    far = rs['idx'] >= P
    in_strip = (rs['x0'] >= 43) & (rs['x0'] < 54)
    outside = (rs['x0'] < 38) | (rs['x0'] >= 60)
    assert rs['passed'][:, far & in_strip].any(0).all() and (far & in_strip).sum() > 500       # both sheets blend
    assert not rs['passed'][:, far & outside & (rs['x0'] >= 4) & (rs['y0'] >= 4)].any()                            # the far points fail the z-test
    cap = K.tile_cap(c['H'], c['W'], 2 * P)
    assert rs['tile_entries'].max() > K.REG_ENTRIES and rs['tile_entries'].max() <= cap


def test_degrid_changes_the_planted_pixels():
    rs = K.restated('degrid_at_seams')
    for y, x in K.DEGRID_PLANTED:
        assert rs['zee'][y, x] > rs['zd'][y, x] + 30, (y, x)
    for y, x in K.DEGRID_CORNERS:
        assert rs['zee'][y, x] == rs['zd'][y, x] and rs['zee'][y, x] > rs['zee'][1, 1] + 30
    assert (rs['zee'] != rs['zd']).sum() == len(K.DEGRID_PLANTED)
    cols = {x for _, x in K.DEGRID_PLANTED}; rows = {y for y, _ in K.DEGRID_PLANTED}
    assert {31, 32, 63, 64} <= cols and {15, 16, 31, 32} <= rows and {0, 69} <= cols and {0, 44} <= rows


def test_border_footprints_and_the_unit_rule():
    c, rs = K.case('border_footprints'), K.restated('border_footprints')
    H, W = c['H'], c['W']
    fx, fy = rs['fx'], rs['fy']
    for m in ((fx > -1) & (fx < 0), (fx > W - 1) & (fx < W), (fy > -1) & (fy < 0), (fy > H - 1) & (fy < H),
              (fx > -1) & (fx < 0) & (fy > -1) & (fy < 0), (fx > W - 1) & (fy > H - 1) & (fx < W) & (fy < H),
              (fx > -1) & (fx < 0) & (fy > H - 1) & (fy < H), (fx > W - 1) & (fx < W) & (fy > -1) & (fy < 0)):
        assert (m & _contributing(rs)).sum() > 0
    far = (fx < -1) | (fy < -1) | (fx >= W) | (fy >= H)
    assert far.sum() >= 8 and not rs['passed'][:, far].any()
    assert ((fx == np.floor(fx)) & (fy == np.floor(fy))).sum() >= 5 and ((rs['w'] == 0).sum(0) == 3).sum() >= 5
    assert rs['unit_pos'] > 0 and rs['unit_neg'] > 0
    small = K.restated('border_footprints_small')
    assert np.all(small['w'][3] == np.float32(2.0 ** -44)) and small['unit_pos'] > 0 and small['unit_neg'] > 0
    ch = K.restated_channels('border_footprints', 9, False)
    assert ch['unit_pos'] > 0 and ch['unit_neg'] > 0


def test_spill_overflows_four_tiles():
    c, rs = K.case('spill'), K.restated('spill')
    cap = K.tile_cap(c['H'], c['W'], c['pts'].shape[1])
    assert cap == 1984 and np.all(rs['tile_entries'][:2, :2] == 4000) and rs['tile_entries'].sum() == 16000
    assert rs['n'][15:17, 31:33].min() == 4000


@pytest.mark.parametrize("name", ['degenerate_empty', 'degenerate_behind', 'degenerate_outside'])
def test_degenerate_clouds_give_a_zero_frame(name):
    rs = K.restated(name)
    assert not rs['frame'].any() and not rs['render_filled'].any() and (rs['holes'][:, 6] < 0).all()
    assert len(rs['holes']) == rs['frame'].shape[0] * rs['frame'].shape[1]


@pytest.mark.parametrize("name", ['holes_45x70', 'holes_64x70', 'holes_70x45'])
def test_hole_cases(name):
    c, rs = K.case(name), K.restated(name)
    H, W = c['H'], c['W']
    assert np.array_equal(~rs['valid'], c['hole'])
    assert np.array_equal(rs['existing'], np.where(c['hole'], 0, 1).astype(np.float32))     # every point lands exactly on its pixel
    h = rs['holes']; filled = h[:, 6] >= 0
    hf = h[filled]
    # sources across the bitmap word boundaries: columns 31|32 (row bitmap), rows 31|32 (column bitmap)
    assert ((hf[:, 3] // 32) != (hf[:, 5] // 32)).any() and ((hf[:, 1] // 32) != (hf[:, 7] // 32)).any()
    assert ((hf[:, 2] // 32) != (hf[:, 4] // 32)).any() and ((hf[:, 0] // 32) != (hf[:, 6] // 32)).any()
    # holes in the last column, the last row and the corners; the corner holes have no complete direction and stay
    assert (h[:, 1] == W - 1).sum() >= 2 and (h[:, 0] == H - 1).sum() >= 3
    kept = {(int(y), int(x)) for y, x in h[~filled][:, :2]}
    assert kept == {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    # the centre of the cross: the axis rays are long, the winner is oblique and short
    cross = h[(h[:, 0] == 20) & (h[:, 1] == 20)][0]
    assert cross[2] != cross[4] and cross[3] != cross[5] and abs(cross[2] - cross[4]) <= 2 and abs(cross[3] - cross[5]) <= 2
    assert rs['tie'].sum() > 10                                                              # two directions at equal distance
    md = rs['mdepth']
    df, dt = md[hf[:, 2], hf[:, 3]], md[hf[:, 4], hf[:, 5]]
    assert (df == dt).sum() > 10 and (df < dt).sum() > 3 and (df > dt).sum() > 3
    assert K.hole_margin(rs).all()


def test_all_holes_but_one_pixel():
    rs = K.restated('holes_all_but_one')
    assert rs['valid'].sum() == 1 and (rs['holes'][:, 6] < 0).all() and rs['frame'][17, 33].tolist() == [63, 127, 191]


@pytest.mark.parametrize("name", NAMES)
def test_float_path_takes_the_same_hole_decisions(name):
    """the margin that lets tests/test_gpu_warptile.py hold the float-atomic path to the sources chosen here"""
    assert K.hole_margin(K.restated(name)).all()
    if name in ('seams', 'patched_grid'):
        for s in K.MULTI_SHIFTS:
            assert K.hole_margin(K.restated(name, s)).all()
