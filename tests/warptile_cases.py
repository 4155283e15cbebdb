"""Seeded cases for the tiled point-cloud renderer (csrc/warptile.hip) and the bound that holds the float-atomic path (csrc/warp.hip)
to the same exact sums.  numpy only.  Used by tests/test_warptile_restatement.py (no GPU) and tests/test_gpu_warptile.py.

Every case is a function with a docstring saying what it exists for; `CASES[name]()` builds it, `restated(name)` is its frame-mode
restatement (tests/warptile_restatement.py), computed once per process.

The bound for the float-atomic path
-----------------------------------
Per pixel and channel the restatement gives S = the exact sum of the fp32 products t_i = fp32(v_i * w_i), A = sum |t_i| and the
number of terms n; for the weight plane S_w, A_w = S_w.

Accumulator.  Any fp32 summation order of n terms -- sequential atomics in any order, or the in-register merge of two neighbours
followed by atomics -- is a summation tree with at most n - 1 additions on any path, each with relative error u = 2^-24.  The
classical bound is |acc - S| <= ((1 + u)^(n-1) - 1) * A = (n - 1) u A + O(u^2); doubling the first-order term covers the
second order for every n < 2^22:  |acc - S| <= n * 2^-23 * A =: bN.  Terms that are zero add nothing in any order, so with at
most one nonzero term the sum is exact (bN = 0); the restatement counts the terms with a nonzero weight as `nz`.

Denominator.  den = fl(e + c), c = fp32(1e-7), |e - S_w| <= bE.  With D = S_w + c:  |den - D| <= bE + 2^-24 * (D + bE) =: bD
(one rounding of the addition, relative to the exact sum e + c <= D + bE).

Quotient.  r = fl(acc / den).  |acc / den - S / D| = |(acc - S) D - S (den - D)| / (den D) <= (bN + |S / D| bD) / (D - bD) =: t
(needs D > bD, asserted), and the division rounds once:  |r - S / D| <= t + 2^-24 * (|S / D| + t) + 2^-149 =: b.

The same propagation with bN = n * unit + 2^-24 |S| (one unit of truncation per term, one rounding of from_fixed) and
bE = n * 2^-40 + 2^-24 S_w bounds the fixed-point path; the test of the oracle against the restatement allows the sum of the two.

A uint8 level must be one that to_u8 yields over [S/D - b, S/D + b]; to_u8 (a rounded multiplication, a clamp, a truncation) is
monotone, so these are the levels between to_u8 of the interval's ends rounded outward to fp32.
"""
import functools

import numpy as np

import warptile_restatement as R

F = np.float32
FOCAL, BASELINE = 35.0, 40.0
U = 2.0 ** -24


def tile_cap(H, W, N):
    """segment capacity per tile: tile_cap() of csrc/warptile.hip restated (2.5 x the load of a uniform cloud x 1.21 for the shared
    borders, at least 1024, a multiple of 64).  The library sizes it by the N of the call."""
    per_tile = float(N) * (R.TW * R.TH) / (float(H) * W) * 1.21
    c = int(per_tile * 2.5) + 63
    c -= c % 64
    return 1024 if c < 1024 else min(c, 1 << 24)


REG_ENTRIES = 4 * 256                 # kReg * kBlock of k_tile_render: the entries a block keeps in registers


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

def quotient_bound(S, Sw, bN, bE):
    """|fl(acc / fl(e + c)) - S / (Sw + c)| given |acc - S| <= bN and |e - Sw| <= bE (module docstring)"""
    D = Sw + float(F(0.0000001))
    bD = bE + U * (D + bE)
    assert np.all(D > bD)
    q = np.abs(S / D)
    t = (bN + q * bD) / (D - bD)
    return t + U * (q + t) + 2.0 ** -149


def exact_quotient(rs, c=None):
    D = rs['S'][-1] + float(F(0.0000001))
    return (rs['S'][:-1] if c is None else rs['S'][c]) / D


def float_bound(rs):
    """bound [C, H, W] of the float-atomic render against exact_quotient(rs)"""
    n = np.where(rs['nz'] > 1, rs['nz'], 0).astype(np.float64)
    return quotient_bound(rs['S'][:-1], rs['S'][-1], n * 2.0 ** -23 * rs['A'][:-1], n * 2.0 ** -23 * rs['A'][-1])


def fixed_bound(rs):
    """bound [C, H, W] of the fixed-point render against exact_quotient(rs) (no saturated term)"""
    n = rs['n'].astype(np.float64)
    unit = np.array([1.0 / s for s in rs['scales']])[:, None, None]
    return quotient_bound(rs['S'][:-1], rs['S'][-1], n * unit + U * np.abs(rs['S'][:-1]), n * 2.0 ** -40 + U * rs['S'][-1])


def u8_levels(rs):
    """lowest and highest uint8 level [3, H, W] the float path may give at a pixel that is not filled"""
    q, b = exact_quotient(rs)[:3], float_bound(rs)[:3]
    lo = (q - b).astype(F); hi = (q + b).astype(F)
    lo = np.where(lo.astype(np.float64) > q - b, np.nextafter(lo, F(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < q + b, np.nextafter(hi, F(np.inf)), hi)
    return R.to_u8(lo), R.to_u8(hi)


def hole_margin(rs):
    """for every filled hole: the depths at `from` and `to` differ by far more (4 x) than the two float bounds, or both pixels have
    the same exact sums with at most one nonzero term each (the float path then computes the same bits for both, as the fixed-point
    path does) -- either way the float path takes the same `dfrom < dto` decision"""
    h = rs['holes']; h = h[h[:, 6] >= 0]
    q, b = exact_quotient(rs, 3), float_bound(rs)[3]
    f, t = (h[:, 2], h[:, 3]), (h[:, 4], h[:, 5])
    same = (rs['S'][3][f] == rs['S'][3][t]) & (rs['S'][4][f] == rs['S'][4][t]) & (rs['nz'][f] <= 1) & (rs['nz'][t] <= 1)
    return same | (np.abs(q[f] - q[t]) > 4.0 * (b[f] + b[t]))


# ---- clouds ----------------------------------------------------------------------------------------------------------------------

def _unproject(fx, fy, z, H, W):
    """points that project near (fx, fy): x = (fx + 0.5 - W / 2) z / focal"""
    z = np.asarray(z, np.float64)
    return np.stack([(fx + 0.5 - 0.5 * W) * z / FOCAL, (fy + 0.5 - 0.5 * H) * z / FOCAL, z]).astype(F)


def _grid_cloud(H, W, seed, blob=True):
    """the frame's own pixels in row-major order (kenburns_effect.py:928-933): a wavy background with a near ellipse in front"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    z = 40.0 + 6.0 * np.sin(xx / 7.0) + 5.0 * np.cos(yy / 5.0)
    if blob:
        z = np.where(((xx - 0.45 * W) / (0.22 * W + 1)) ** 2 + ((yy - 0.5 * H) / (0.3 * H + 1)) ** 2 < 1.0, 17.0 + 0.02 * xx + 0.013 * yy, z)
    pts = _unproject(xx.ravel(), yy.ravel(), z.ravel(), H, W)
    rgb = g.uniform(0.0, 1.0, (3, H * W)).astype(F)
    return pts, rgb, pts[2:3].copy()


def _exact_points(fx, fy, H, W):
    """points at z = focal: dist = 0, so the projection returns x + W / 2 - 0.5 exactly where that is a float32"""
    fx = np.asarray(fx, np.float64); fy = np.asarray(fy, np.float64)
    p = np.stack([fx + 0.5 - 0.5 * W, fy + 0.5 - 0.5 * H, np.full(fx.shape, FOCAL)])
    assert np.array_equal(p.astype(F).astype(np.float64), p), "coordinates must be exact in float32"
    return p.astype(F)


def _case(name, H, W, pts, rgb, depth, shift=(0.0, 0.0, 0.0), **extra):
    d = dict(name=name, H=H, W=W, pts=np.ascontiguousarray(pts, F), rgb=np.ascontiguousarray(rgb, F),
             depth=np.ascontiguousarray(depth, F), shift=tuple(float(F(v)) for v in shift), focal=FOCAL, baseline=BASELINE)
    d.update(extra)
    return d


def seams():
    """45 x 70: neither side a multiple of the 16 x 32 tile (last tile 13 rows x 6 columns); a moderate shift makes footprints
    straddle every seam column (31|32, 63|64) and seam row (15|16, 31|32) -- a footprint dropped or doubled at a seam, or a
    z-ring pixel missed, changes a sum"""
    return _case('seams', 45, 70, *_grid_cloud(45, 70, 11), shift=(3.3, -2.1, -4.0))


def _tiny(H, W):
    pts, rgb, dep = _grid_cloud(H, W, 100 + H)
    g = np.random.default_rng(H * 100 + W)
    ex = _unproject(g.uniform(-1.5, W + 0.5, 7), g.uniform(-1.5, H + 0.5, 7), g.uniform(20.0, 50.0, 7), H, W)
    return _case('tiny_%dx%d' % (H, W), H, W, np.concatenate([pts, ex], 1), np.concatenate([rgb, g.uniform(0, 1, (3, 7)).astype(F)], 1),
                 np.concatenate([dep, ex[2:3]], 1), shift=(0.4, -0.3, -1.0))


def tiny_1x1():
    """1 x 1: one tile of one pixel; every ring pixel and every stencil pair is outside the image"""
    return _tiny(1, 1)


def tiny_16x32():
    """16 x 32: exactly one whole tile"""
    return _tiny(16, 32)


def tiny_17x33():
    """17 x 33: a second tile row of a single row and a second tile column of a single column"""
    return _tiny(17, 33)


def tiny_33x17():
    """33 x 17: three tile rows, the last of a single row; one narrow tile column"""
    return _tiny(33, 17)


def _patched(kind):
    H, W = 40, 96
    pts, rgb, dep = _grid_cloud(H, W, 21)
    g = np.random.default_rng(22)
    if kind == 'plus':
        n = 3001
        ex = _unproject(g.uniform(-2.0, W + 1.0, n), g.uniform(-2.0, H + 1.0, n), g.uniform(15.0, 60.0, n), H, W)
        pts = np.concatenate([pts, ex], 1); rgb = np.concatenate([rgb, g.uniform(0, 1, (3, n)).astype(F)], 1)
        dep = np.concatenate([dep, ex[2:3]], 1)
    elif kind == 'minus':
        n = H * W - 977
        pts, rgb, dep = pts[:, :n], rgb[:, :n], dep[:, :n]
    return _case('patched_' + kind, H, W, pts, rgb, dep, shift=(-2.7, 1.9, -3.0))


def patched_grid():
    """40 x 96, N == H W: W is a multiple of 32, so point_of visits two whole 16-row bands in 32 x 16 patches and the last eight
    rows linearly -- a point visited twice or never changes a sum"""
    return _patched('grid')


def patched_plus():
    """40 x 96, N == H W + 3001: the appended, scattered points follow the patched grid in linear order"""
    return _patched('plus')


def patched_minus():
    """40 x 96, N == H W - 977: a truncated grid; the last whole band ends before the cloud does"""
    return _patched('minus')


def two_layers():
    """64 x 96, N = 2 H W: a near sheet over a far sheet.  Where the near sheet is at z = 20 the error gap is 35 and the far points
    fail the z-test; in columns 40..55 it is at z = 39.5 (gap 0.44 < 1) and both blend.  Every interior tile gets about 1200
    entries: more than the 1024 held in registers, fewer than its capacity"""
    H, W = 64, 96
    g = np.random.default_rng(31)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    near = np.where((xx >= 40) & (xx < 56), 39.5, 20.0)
    p1 = _unproject(xx.ravel(), yy.ravel(), near.ravel(), H, W)
    p2 = _unproject(xx.ravel(), yy.ravel(), np.full(H * W, 40.0), H, W)
    pts = np.concatenate([p1, p2], 1)
    return _case('two_layers', H, W, pts, g.uniform(0, 1, (3, 2 * H * W)).astype(F), pts[2:3].copy(), shift=(1.3, 0.7, 0.0))


DEGRID_PLANTED = [(15, 10), (16, 20), (31, 40), (32, 50), (7, 31), (22, 32), (38, 63), (12, 64), (15, 31), (16, 32), (31, 63), (32, 64),
                  (0, 25), (44, 45), (25, 0), (20, 69)]
DEGRID_CORNERS = [(0, 0), (0, 69), (44, 0), (44, 69)]


def degrid_at_seams():
    """45 x 70 at rest: isolated far pixels (z = 40) between near neighbours (z = 20) on seam columns and rows -- the degrid stencil of
    a seam pixel reads the neighbour tile's ring -- and on the image border, where pairs that leave the image are skipped (in a
    corner all four are, and the pixel keeps its z)"""
    H, W = 45, 70
    g = np.random.default_rng(41)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    z = np.full((H, W), 20.0)
    for y, x in DEGRID_PLANTED + DEGRID_CORNERS:
        z[y, x] = 40.0
    pts = _unproject(xx.ravel(), yy.ravel(), z.ravel(), H, W)
    depth = (z + 0.05 * xx + 0.07 * yy).reshape(1, -1)      # a slope keeps the two ends of every hole's pair apart
    return _case('degrid_at_seams', H, W, pts, g.uniform(0, 1, (3, H * W)).astype(F), depth)


def border_footprints():
    """45 x 70, hand-placed points at z = focal (exact coordinates): footprints that hang over each border and corner (fx in (-1, 0)
    and (W - 1, W), fy likewise); points with fx or fy in (-4, -1) and beyond the far borders, which are binned nowhere or
    contribute nothing; points exactly on integer coordinates (three zero weights); points one float32 step (2^-18) past an integer
    in both axes with small data, so that the SE product is below one 2^-40 unit and takes the +-1 rule (rgb carries negative
    values here for the -1)"""
    H, W = 45, 70
    g = np.random.default_rng(51)
    fx, fy = [], []
    for x in (-0.5, -0.25, 69.25, 69.75, 31.5, 10.5):
        for y in (-0.5, -0.75, 44.25, 44.5, 15.5, 20.25):
            fx.append(x); fy.append(y)
    for x, y in ((-3.5, 5.5), (-1.5, 7.25), (-2.25, -2.5), (12.5, -3.75), (12.5, -1.25), (70.5, 3.5), (72.75, 44.5), (30.5, 45.5),
                 (30.5, 47.75), (73.5, 48.5), (-3.75, 47.5)):
        fx.append(x); fy.append(y)
    for x, y in ((0.0, 0.0), (69.0, 44.0), (31.0, 15.0), (32.0, 16.0), (64.0, 32.0), (5.0, 20.5), (40.25, 33.0), (-1.0, 3.0), (70.0, 45.0)):
        fx.append(x); fy.append(y)
    n_small = 12
    for i in range(n_small):
        fx.append(33.0 + 2 * (i % 4) + 2.0 ** -18); fy.append(33.0 + 3 * (i // 4) + 2.0 ** -18)
    pts = _exact_points(fx, fy, H, W)
    n = pts.shape[1]
    rgb = g.uniform(-1.0, 1.0, (3, n)).astype(F)
    rgb[:, n - n_small:] = (g.choice([-1.0, 1.0], (3, n_small)) * 2.0 ** -6).astype(F)
    return _case('border_footprints', H, W, pts, rgb, g.uniform(10.0, 50.0, (1, n)).astype(F), n_small=n_small)


def border_footprints_small():
    """7 x 6: points at k + 2^-22 in both axes (representable only below 4): the SE weight is 2^-44, every SE product is below one
    unit; with signed rgb both +1 and -1 occur"""
    H, W = 7, 6
    g = np.random.default_rng(52)
    fx = [k + 2.0 ** -22 for k in (1.0, 2.0, 3.0, 2.0, 1.0, 3.0)]
    fy = [k + 2.0 ** -22 for k in (1.0, 2.0, 3.0, 3.0, 2.0, 1.0)]
    pts = _exact_points(fx, fy, H, W)
    rgb = g.uniform(-1.0, 1.0, (3, 6)).astype(F)
    rgb[:, 0] = (0.5, -0.5, 0.25)
    return _case('border_footprints_small', H, W, pts, rgb, g.uniform(10.0, 50.0, (1, 6)).astype(F))


def spill():
    """45 x 70 with 4000 points inside the 2 x 2 pixels around (31.5, 15.5): the four tiles at that corner receive every point and
    overflow their segment (capacity 1984), so half of the entries travel through the spill list; the depths are within an error
    gap of 0.44, so every point passes the z-test"""
    H, W, n = 45, 70, 4000
    g = np.random.default_rng(61)
    pts = _unproject(g.uniform(31.05, 31.95, n), g.uniform(15.05, 15.95, n), g.uniform(40.0, 40.5, n), H, W)
    return _case('spill', H, W, pts, g.uniform(0, 1, (3, n)).astype(F), pts[2:3].copy())


def degenerate_empty():
    """N = 0: a zero frame, nothing filled"""
    return _case('degenerate_empty', 45, 70, np.zeros((3, 0), F), np.zeros((3, 0), F), np.zeros((1, 0), F))


def degenerate_behind():
    """all points behind the camera (z < 0.001, some negative): a zero frame, nothing filled"""
    g = np.random.default_rng(71)
    pts = np.stack([g.uniform(-30, 30, 300), g.uniform(-20, 20, 300), np.concatenate([g.uniform(-50.0, 0.0009, 299), [0.0]])]).astype(F)
    return _case('degenerate_behind', 45, 70, pts, g.uniform(0, 1, (3, 300)).astype(F), np.ones((1, 300), F))


def degenerate_outside():
    """all points project outside the image (some within the 4-px range of the binning test, some far beyond)"""
    g = np.random.default_rng(72)
    H, W, n = 45, 70, 300
    fx = np.concatenate([g.uniform(-3.9, -1.1, 100), g.uniform(W + 0.1, W + 3.9, 100), g.uniform(-1e4, 1e4, 100)])
    fy = np.concatenate([g.uniform(-10, H + 10, 200), g.uniform(H + 1.0, 1e4, 100)])
    pts = _unproject(fx, fy, g.uniform(20.0, 50.0, n), H, W)
    return _case('degenerate_outside', H, W, pts, g.uniform(0, 1, (3, n)).astype(F), pts[2:3].copy())


def _holes(H, W):
    g = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[:H, :W]
    hole = np.zeros((H, W), bool)
    hole[3:15, 30:34] = True                                # vertical band across columns 31|32: the nearest pair is (y, 29)-(y, 34)
    if W > 67:
        hole[3:15, 62:66] = True                            # ... and 63|64
    hole[30:34, 34:42] = True                               # horizontal band across rows 31|32 (second column-bitmap word)
    hole[20, 12:29] = True; hole[12:29, 20] = True          # a cross: long axis rays at its centre, short oblique ones
    for y, x in ((0, 0), (H - 1, W - 1), (10, W - 1), (H - 1, 25), (H - 1, 0), (0, W - 1), (40, 25), (2, 2), (38, 5)):
        hole[y, x] = True
    pts = _exact_points(xx.ravel().astype(np.float64), yy.ravel().astype(np.float64), H, W)
    pts[2, hole.ravel()] = 0.0                              # rejected by z < 0.001
    depth = np.where(xx < 32, 40.0, np.where(yy < 32, 15.0, 60.0)).astype(F).reshape(1, -1)
    return _case('holes_%dx%d' % (H, W), H, W, pts, g.uniform(0, 1, (3, H * W)).astype(F), depth, hole=hole)


def holes_45x70():
    """45 x 70 (nty = 3, odd: the padded column word): a pixel grid landing exactly on the pixels with points removed.  Hole bands
    across columns 31|32 and 63|64 and rows 31|32, holes in the last column and row and the corners (rays leave the image; the
    corner holes have no complete direction and stay), a cross whose centre has long axis rays and short oblique ones (the early
    give-up), isolated holes (two axis directions at equal distance; dfrom == dto inside a depth layer).  The depth layers
    (40 / 15 / 60) meet at column 32 and row 32, inside the bands, and are far apart"""
    return _holes(45, 70)


def holes_64x70():
    """64 x 70 (nty = 4, even): as holes_45x70; the column bitmap has two whole words"""
    return _holes(64, 70)


def holes_70x45():
    """70 x 45 (nty = 5, odd again; two tile columns, the second 13 wide): as holes_45x70"""
    return _holes(70, 45)


def holes_all_but_one():
    """45 x 70, every pixel a hole but one: no direction ever finds two valid ends, nothing is filled, every ray runs to the border"""
    H, W = 45, 70
    pts = _exact_points([33.0], [17.0], H, W)
    return _case('holes_all_but_one', H, W, pts, np.array([[0.25], [0.5], [0.75]], F), np.array([[20.0]], F))


CASES = {f.__name__: f for f in (seams, tiny_1x1, tiny_16x32, tiny_17x33, tiny_33x17, patched_grid, patched_plus, patched_minus, two_layers,
                                 degrid_at_seams, border_footprints, border_footprints_small, spill, degenerate_empty, degenerate_behind,
                                 degenerate_outside, holes_45x70, holes_64x70, holes_70x45, holes_all_but_one)}
CHANNEL_CASES = ('seams', 'two_layers', 'spill', 'border_footprints')
CHANNEL_COUNTS = (1, 8, 9, 68)
MULTI_SHIFTS = ((3.3, -2.1, -4.0), (-2.7, 1.9, -3.0), (0.0, 0.0, 0.0), (5.5, 0.25, 2.0))


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def restated(name, shift=None):
    """frame-mode restatement of a case (at another shift for the multi-frame call); shared, never written to"""
    c = case(name)
    return R.render(c['pts'], np.concatenate([c['rgb'], c['depth']]), c['H'], c['W'], c['focal'], c['baseline'],
                    shift=c['shift'] if shift is None else shift, mode='frame')


@functools.lru_cache(maxsize=None)
def shifted_points(name):
    c = case(name)
    return np.stack(R.process_shift(c['pts'], c['shift']))


@functools.lru_cache(maxsize=None)
def channel_data(name, saturate):
    """68 signed feature channels, normal(0, 3); with `saturate` one value of channel 0 is raised to 2^33 at a point that passes
    the z-test with a weight above 1/4, so that |v w| >= 2^31: the documented saturation of the tile path (+-2^62 units)"""
    c = case(name)
    n = c['pts'].shape[1]
    data = np.random.default_rng(len(name) * 7 + 5).normal(0.0, 3.0, (68, n)).astype(F)
    if saturate:
        rs = restated(name)
        k = np.nonzero(rs['passed'][0] & (rs['w'][0] > 0.25))[0][0]              # the NW corner passes the z-test
        data[0, rs['idx'][k]] = F(2.0 ** 33)
    return data


@functools.lru_cache(maxsize=None)
def _restated_68(name, saturate):
    c = case(name)
    return R.render(shifted_points(name), channel_data(name, saturate), c['H'], c['W'], c['focal'], c['baseline'], mode='channels')


def restated_channels(name, C, saturate):
    """channel-mode restatement of the first C of the 68 channels: the channels are independent, so it is a view of the 68-channel
    one (the weight plane stays last in S and A)"""
    rs = dict(_restated_68(name, saturate))
    rs.update(render=rs['render'][:C], acc=rs['acc'][:C], scales=rs['scales'][:C],
              S=np.concatenate([rs['S'][:C], rs['S'][-1:]]), A=np.concatenate([rs['A'][:C], rs['A'][-1:]]))
    return rs
