"""Named cases of the autozoom coverage search (csrc/autozoom.hip) -- TEST INFRASTRUCTURE ONLY.  numpy only.
Used by tests/test_autozoom_references.py (no GPU) and tests/test_gpu_autozoom.py.

A case is a dict: H, W, pts (float32 [3, N]), shifts (list of (sx, sy, sz), one sz per case), focal, baseline, and
  band    what csm_autozoom_band_supported(H, W) has to answer (1: the LDS band path really runs under CSM_AUTOZOOM_PATH=bands)
  br      the band height band_geom chooses (0: refused)
  chunks  the chunk sizes of the plane path to run (None: the default)
  literal (hand-placed cases) the counts written down by hand, one per shift
  overflow  True: a band segment overflows, the band path raises its flag and the plane path answers

band_geom (csrc/autozoom.hip), restated below and checked against the kernel's source text by the CPU test: the z-buffer window
(br + 2 rows) and the threshold band (br rows) of a block are fp32 rows of W pixels in LDS, and
  br = 8  iff  (2*8 + 2) * W * 4 <= 40 KiB  iff  W <= 568        br = 4  iff  (2*4 + 2) * W * 4 <= 48 KiB  iff  W <= 1228
  br = 2  iff  (2*2 + 2) * W * 4 <= 72 KiB  iff  W <= 3072       odd W and W > 3072: refused, the plane path answers
(W even: 568, 1228 and 3072 are the last widths of their class; 570, 1230 and 3074 the first of the next).
"""
import functools

import numpy as np

import autozoom_restatement as A
import warptile_restatement as R

F = np.float32
FOCAL, BASELINE = 35.0, 40.0

# ---- band_geom, restated ----------------------------------------------------------------------------------------------------------
BAND_CLASSES = ((8, 40), (4, 48), (2, 72))        # (br, KiB that (2 br + 2) rows of W floats may take)
LDS_KIB = 150                                     # kBandLds: window + threshold band + entry cache
GROUP_MAX, PER_GROUP, MAX_CHUNK = 16, 16, 32      # kGroupMax, kPerGroup, kMaxChunk


def band_rows(W):
    if W % 2:
        return 0
    for br, kib in BAND_CLASSES:
        if (2 * br + 2) * W * 4 <= kib * 1024:
            return br
    return 0


def last_width(br):
    """the last even width of the class of br"""
    kib = dict(BAND_CLASSES)[br]
    w = (kib * 1024) // ((2 * br + 2) * 4)
    return w - w % 2


def band_geom(H, W, N):
    """br, nbands, cap (entries a band segment holds), ncache (entries of a band kept in LDS)"""
    br = band_rows(W)
    if br == 0:
        return dict(br=0, nbands=0, cap=0, ncache=0)
    nbands = (H + br - 1) // br
    cap = int(float(N) * (br + 3) / float(H) * 3.0) + 1023
    cap -= cap % 1024
    cap = min(max(cap, 4096), 1 << 26)
    room = (LDS_KIB * 1024 - (2 * br + 2) * W * 4) // 16
    return dict(br=br, nbands=nbands, cap=cap, ncache=min(room, cap))


def band_entries(c, sy):
    """entries per band of the group with y shift sy (k_band_bin): the points that pass the z tests with fy in (-4, H + 4), once for
    every band whose window rows [b br - 1, b br + br] meet the footprint rows [y0, y0 + 1]"""
    H, W = c['H'], c['W']
    g = band_geom(H, W, c['pts'].shape[1])
    x, y, z = R.process_shift(c['pts'], (0.0, sy, c['shifts'][0][2]))
    ok, _, fy, _ = R.project(x, y, z, H, W, c['focal'], c['baseline'])
    with np.errstate(all='ignore'):
        ok &= (fy > F(-4.0)) & (fy < F(H + 4))
    y0 = np.floor(fy[ok]).astype(np.int64)
    br, nb = g['br'], g['nbands']
    lo = np.maximum(-((br - y0) // br), 0)                       # ceil((y0 - br) / br)
    hi = np.minimum((y0 + 2) // br, nb - 1)
    n = np.zeros(nb, np.int64)
    for b in range(nb):
        n[b] = int(((lo <= b) & (b <= hi)).sum())
    return n


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
def world(fx, fy, z, H, W, focal=FOCAL):
    """points that project() sends to about (fx, fy): ix = x * focal / z"""
    fx, fy, z = (np.asarray(v, np.float64) for v in (fx, fy, z))
    return np.stack([(fx - 0.5 * W + 0.5) * z / focal, (fy - 0.5 * H + 0.5) * z / focal, z + 0 * fx]).astype(F)


def sparse_cloud(seed, H, W, density=0.6, extra=300, n=None):
    """a uniform cloud with holes (about `density` points per pixel, depths 30 .. 80) plus `extra` points scattered over a wider
    area, beyond the frame too"""
    g = np.random.default_rng(seed)
    n = int(density * H * W) if n is None else n
    a = world(g.uniform(-1.5, W + 0.5, n), g.uniform(-1.5, H + 0.5, n), g.uniform(30.0, 80.0, n), H, W)
    b = world(g.uniform(-8.0, W + 8.0, extra), g.uniform(-8.0, H + 8.0, extra), g.uniform(20.0, 90.0, extra), H, W)
    return np.concatenate([a, b], 1)


SHIFTS6 = [(sx, sy, -3.5) for sy in (-1.5, 0.0, 0.7) for sx in (-2.0, 0.5)]


def _case(H, W, pts, shifts, **kw):
    br = band_rows(W)
    c = dict(H=H, W=W, pts=np.ascontiguousarray(pts, F).reshape(3, -1), shifts=[tuple(float(v) for v in s) for s in shifts],
             focal=FOCAL, baseline=BASELINE, br=br, band=int(br > 0 and (H + br - 1) // br <= 4096), chunks=(None,), overflow=False)
    c.update(kw)
    return c


# ---- band_geom's classes -----------------------------------------------------------------------------------------------------------
# name: (H, W, br expected, what it selects)
GEOMETRY = {
    'one_px_rows': (1, 64, 8, "H < br, single band, no vertical lines in the degrid"),
    'short':       (7, 64, 8, "H < br = 8"),
    'exact':       (8, 64, 8, "one full band"),
    'ragged8':     (9, 66, 8, "a second band of 1 row; W % 4 == 2: the scalar plane degrid"),
    'br8_max':     (17, 568, 8, "last width with br = 8"),
    'br4_min':     (9, 570, 4, "first width with br = 4, H % 4 == 1"),
    'br4_max':     (6, 1228, 4, "last width with br = 4"),
    'br2_min':     (5, 1230, 2, "first width with br = 2, H odd"),
    'br2_max':     (3, 3072, 2, "last supported width"),
    'unsupported': (3, 3074, 0, "band path refused, the plane path answers"),
    'odd':         (9, 67, 0, "odd W: band path refused; H * W % 4 != 0: pitch != plane on the plane path"),
    'pitch4':      (6, 1026, 4, "br = 4; W % 4 == 2: the scalar plane degrid"),
}


def _geometry(name):
    H, W, _, _ = GEOMETRY[name]
    return _case(H, W, sparse_cloud(100 + list(GEOMETRY).index(name), H, W), SHIFTS6)


# ---- hand-placed points: 16 x 64, br = 8 (two bands, the seam between rows 7 and 8) ------------------------------------------------
HH, HW = 16, 64
E0 = 999930.0                                     # fltError of a point at depth 20: 1e6 - 35 * 40 / 20; fp32 steps of 1/16 there


def place(fx, fy, err, H=HH, W=HW):
    """a point that project() sends EXACTLY to (fx, fy) with fltError exactly err under the zero shift: searched among the depths
    that give err and the fp32 neighbours of x = (fx - W/2 + 1/2) z / focal, checked with the restated project()"""
    fb = FOCAL * BASELINE
    z0 = F(fb / (1000000.0 - err))
    zs = (z0 + np.arange(-400, 401).astype(F) * np.spacing(z0)).astype(F)
    zs = zs[(1000000.0 - fb / (zs.astype(np.float64) + 0.0000001)).astype(F) == F(err)]
    k = np.arange(-64, 65).astype(F)
    for z in zs:
        got = []
        for t, size in ((fx, W), (fy, H)):                       # fy is fx's expression with H for W
            e = F((t - 0.5 * size + 0.5) * float(z) / FOCAL)
            cand = (e + k * np.spacing(max(abs(e), F(1e-3)))).astype(F)
            zz = np.full(cand.shape, z, F)
            ok, px, _, _ = R.project(*R.process_shift((cand, cand, zz), ZERO), size, size, FOCAL, BASELINE)
            hit = np.nonzero(ok & (px == F(t)))[0]
            if hit.size == 0:
                break
            got.append(cand[hit[0]])
        if len(got) == 2:
            return (got[0], got[1], z)
    raise AssertionError("no fp32 point projects exactly to (%r, %r) with fltError %r" % (fx, fy, err))


def _pts(*p):
    return np.asarray(p, F).T


ZERO = (0.0, 0.0, 0.0)
# a shift of 0.1 world units moves a point at depth 20 by 0.1 * 35 / 20 = 0.175 px
RIGHT, DOWN, UP, LEFT, UPLEFT, DOWNRIGHT = (0.1, 0.0, 0.0), (0.0, 0.1, 0.0), (0.0, -0.1, 0.0), (-0.1, 0.0, 0.0), (-0.1, -0.1, 0.0), (0.1, 0.1, 0.0)


def _hand():
    h = {}
    # one point on (10.5, 7.5): rows 7 | 8 are the last row of band 0 and the first of band 1; both bands hold the point, each
    # marks its own rows -- 4 pixels, not 8; a sub-pixel shift keeps the four corners
    h['hand_seam'] = ([place(10.5, 7.5, E0)], [ZERO, RIGHT, DOWN, UPLEFT], [4, 4, 4, 4])
    # (5.5, 0): fy on row 0, the south weights are zero -> (5,0) (6,0); (20.5, 15): row 15, row 16 is outside -> 2.  DOWN: fy 0.175
    # -> rows 0 and 1 (4), and 15.175 -> row 15 (2).  UP: fy -0.175 -> row 0 only (2), 14.825 -> rows 14, 15 (4)
    h['hand_rows'] = ([place(5.5, 0.0, E0), place(20.5, 15.0, E0)], [ZERO, DOWN, UP], [4, 6, 6])
    # (0, 4.5): column 0 only (the east weights are zero); (63, 10.5): column 63 only.  RIGHT: 0.175 -> columns 0, 1 (4) and 63.175
    # -> column 63 (2).  LEFT: -0.175 -> column 0 (2) and 62.825 -> columns 62, 63 (4)
    h['hand_cols'] = ([place(0.0, 4.5, E0), place(63.0, 10.5, E0)], [ZERO, RIGHT, LEFT], [4, 6, 6])
    # fy = -0.5: only the south corners (row 0) are inside; the point reaches band 0 through its halo row -1
    h['hand_north'] = ([place(12.5, -0.5, E0)], [ZERO, RIGHT, DOWN, UP], [2, 2, 2, 2])
    # fy = 15.5: only the north corners (row 15); fy = 17.5 in (H, H + 4): binned by the band path, contributes nothing
    h['hand_south'] = ([place(12.5, 15.5, E0), place(40.5, 17.5, E0)], [ZERO, DOWN, UP], [2, 2, 2])
    # fx = -2.5 and 66.5 are outside, (8.5, 5.5) gives its four corners
    h['hand_fx_out'] = ([place(-2.5, 5.5, E0), place(66.5, 5.5, E0), place(8.5, 5.5, E0)], [ZERO, RIGHT, LEFT], [4, 4, 4])
    # z shift -0.5: depth 0.5005 becomes 0.0005 < 0.001, rejected (it would land 14 px left of the centre: 4 more pixels); depth
    # 0.502 becomes 0.002, accepted, on (31.5, 7.5): 4; an ordinary point at about (8.3, 5.3): 4.  1e-5 world units are 0.175 px at
    # depth 0.002
    h['hand_z_reject'] = ([(-2e-4, 0.0, 0.5005), (0.0, 0.0, 0.502), tuple(world(8.3, 5.3, 20.0, HH, HW))],
                          [(0.0, 0.0, -0.5), (1e-5, 0.0, -0.5)], [8, 8])
    # exactly on the centre of (20, 6): one weight is 1 and three are 0 -- 1 pixel, not 4; RIGHT / DOWN: 2; DOWNRIGHT: 4
    h['hand_centre'] = ([place(20.0, 6.0, E0)], [ZERO, RIGHT, DOWN, DOWNRIGHT], [1, 2, 2, 4])
    # three points whose arg-max corner is (20, 6): E0 on the centre; E0 + 0.5 at fx 20.25 (passes at (20,6) and marks (21,6));
    # E0 + 5 at fx 19.75: z-rejected at (20,6), but its west corner (19,6) is empty and passes -- 3 pixels.  DOWN: rows 6 and 7: 6
    h['hand_two_on_pixel'] = ([place(20.0, 6.0, E0), place(20.25, 6.0, E0 + 0.5), place(19.75, 6.0, E0 + 5.0)], [ZERO, DOWN], [3, 6])
    # column 30, rows 7 | 8 | 9 (the vertical line crosses the seam): E0, E0 + 5, E0: the degrid pulls (30,8) down to E0 and the far
    # point fails its own z-test: 2 pixels.  Row 3, columns 10, 11, 12: E0, E0 + 1, E0: the degrid fires at equality (c >= a + 1),
    # (11,3) becomes E0 and E0 + 1 <= E0 + 1 passes: 3 pixels.  RIGHT: every point also has an east corner (weight 0.175) on an
    # empty pixel that no line pulls down: column 30 -> (30,7) (31,7) (31,8) (30,9) (31,9), row 3 -> columns 10 .. 13: 9
    h['hand_degrid_line'] = ([place(30.0, 7.0, E0), place(30.0, 8.0, E0 + 5.0), place(30.0, 9.0, E0),
                              place(10.0, 3.0, E0), place(11.0, 3.0, E0 + 1.0), place(12.0, 3.0, E0)], [ZERO, RIGHT], [5, 9])
    # Jacobi order: (51,13) = E0 + 5 is pulled to E0 by its vertical line (51,12) (51,14) = E0.  (52,13) = E0 + 5.5 has the line
    # (53,13) = E0, (51,13): with the value BEFORE the pass, E0 + 5, the test c >= E0 + 6 fails and (52,13) stays covered: 4
    # pixels.  An in-place pass in raster order reads E0 there and un-covers it (3)
    h['hand_degrid_order'] = ([place(51.0, 12.0, E0), place(51.0, 14.0, E0), place(51.0, 13.0, E0 + 5.0), place(52.0, 13.0, E0 + 5.5),
                               place(53.0, 13.0, E0)], [ZERO], [4])
    # lines with one end outside the image are not used: (0,5) = E0 + 5 beside (1,5) = E0, and (20,0) = E0 + 5 above (20,1) = E0,
    # all stay covered: 4
    h['hand_edge_line'] = ([place(0.0, 5.0, E0 + 5.0), place(1.0, 5.0, E0), place(20.0, 0.0, E0 + 5.0), place(20.0, 1.0, E0)], [ZERO], [4])
    # a four-way tie of the weights at (40.5, 11.5) goes to the NW corner (40,11) = E0.  That entry is one end of the line through
    # (39,11) = E0 + 5, whose other end is (38,11) = E0: the far point is pulled down and fails: 4 + 1 = 5 pixels.  (Were the tie
    # given to the SE corner, (40,11) would hold 1e6, no line, 6 pixels.)  UPLEFT: the tie is gone, NW wins; the far point keeps
    # (39,10) only: 4 + 4 + 1 = 9
    h['hand_argmax_tie'] = ([place(40.5, 11.5, E0), place(39.0, 11.0, E0 + 5.0), place(38.0, 11.0, E0)], [ZERO, UPLEFT], [5, 9])
    return h


# ---- candidate grouping: 24 x 96 (br = 8, three bands), one cloud -----------------------------------------------------------------
GH, GW = 24, 96


def _group_shifts(name):
    g = np.random.default_rng(77)
    sx17 = [round(-4.0 + 0.5 * i, 3) for i in range(17)]
    sy17 = [round(-3.2 + 0.4 * i, 3) for i in range(17)]
    lin = [round(-3.0 + 0.4 * i, 3) for i in range(16)]
    if name == 'group_17x1':                                    # one y shift, 17 candidates: the group splits into 16 + 1
        return [(sx, 0.3, -3.5) for sx in sx17]
    if name == 'group_1x17':                                    # 17 y shifts: a second launch batch with one group on re-armed counters
        return [(0.5, sy, -3.5) for sy in sy17]
    if name == 'group_16x16':                                   # one full batch
        return [(sx, sy, -3.5) for sy in lin for sx in lin]
    if name == 'group_257':                                     # the 17th candidate of one y shift makes a 17th group
        return [(sx, sy, -3.5) for sy in lin for sx in lin] + [(3.3, lin[5], -3.5)]
    if name == 'group_shuffled':                                # 17 x 2 in shuffled order with one duplicate (sx, sy): the out[g][c] scatter
        s = [(sx, sy, -3.5) for sy in (-1.1, 0.6) for sx in sx17]
        s = [s[i] for i in g.permutation(len(s))]
        return s[:20] + [s[3]] + s[20:]
    if name == 'k1':
        return [(0.5, -0.7, -3.5)]
    if name == 'k0':
        return []
    if name == 'planes_k33':                                    # plane path: chunks of 32 + 1, 5 x 6 + 3, 33 x 1
        return [(sx, sy, -3.5) for sy in (-1.1, 0.6) for sx in sx17][:33]
    raise KeyError(name)


GROUPING = ('group_17x1', 'group_1x17', 'group_16x16', 'group_257', 'group_shuffled', 'k1', 'k0', 'planes_k33')


def _grouping(name):
    kw = dict(chunks=(None, 32, 5, 1)) if name == 'planes_k33' else {}
    return _case(GH, GW, sparse_cloud(7, GH, GW), _group_shifts(name), **kw)


# ---- load --------------------------------------------------------------------------------------------------------------------------
SHIFTS4 = [(-2.0, -0.5, -3.5), (0.5, -0.5, -3.5), (1.0, 0.4, -3.5), (-0.3, 0.4, -3.5)]


def is_tiny(v):
    """k_band_cover's `tiny`: not zero and below 2^-28, where `a + 1.0` need not be exact in fp64"""
    return (v != 0) & (np.abs(v) < F(2.0 ** -28))


def tiny_baseline(z0):
    """a baseline for which a point at depth z0 has a tiny fltError: focal * baseline a few fp64 steps off 1e6 * (z0 + 1e-7)"""
    b = 1000000.0 * (float(z0) + 0.0000001) / FOCAL
    for k in range(1, 200):
        bb = b * (1.0 + k * 2.0 ** -52)
        if is_tiny(F(1000000.0 - (FOCAL * bb) / (float(z0) + 0.0000001))):
            return bb
    raise AssertionError("no baseline gives a tiny fltError at depth %r" % z0)


def _load(name):
    g = np.random.default_rng(500)
    if name == 'recache':
        # 16 x 64, N = 20000: band_geom keeps ncache = (150 KiB - 18 * 64 * 4) / 16 = 9312 entries of a band in LDS; each of the two
        # bands gets about 20000 * 11 / 19 entries, so the rest is re-read from memory per candidate (total > ncache), and cap =
        # 3 * 20000 * 11 / 16 rounded to 1024 = 41984 is not reached
        return _case(16, 64, sparse_cloud(501, 16, 64, n=19700), SHIFTS4)
    if name == 'pileup':
        # 64 x 64, 6000 points in rows 30 .. 32 of a cloud-less frame: cap = max(4096, 3 * 6000 * 11 / 64) = 4096 < 6000 entries
        # in bands 3 and 4: the segments overflow
        n = 6000
        pts = world(g.uniform(1.0, 62.0, n), g.uniform(30.0, 32.99, n), g.uniform(30.0, 80.0, n), 64, 64)
        return _case(64, 64, pts, [(sx, sy, 0.0) for sy in (0.0, 0.05) for sx in (-0.5, 0.0, 0.4)], overflow=True)
    if name == 'near_zero':
        # the cloud tests/test_gpu_pinned.py calls near-zero, kept as it is there: depths around focal * baseline / 1e6.  The 1e-7 of
        # fltError's denominator is not small beside a depth of 0.0014, so its fltError is 68 .. 75, all positive, in steps of about
        # 0.08; 'tiny_err' below is the cloud whose fltError really lies around 0 with both signs
        n = 30000
        z0 = F(FOCAL * BASELINE / 1e6)
        z = (z0 + g.integers(-40, 41, n).astype(F) * np.spacing(z0)).astype(F)
        xy = g.uniform(-1.0, 1.0, (2, n)).astype(F) * z * np.array([[96 / 70.0], [64 / 70.0]], F)
        return _case(64, 96, np.stack([xy[0], xy[1], z]), [(a * 1e-5, b * 1e-5, 0.0) for b in (-2.0, 0.0, 1.5) for a in (-4.0, -1.0, 0.5, 2.0)])
    if name == 'tiny_err':
        # fltError within 3.3 units of 0 with both signs: the same kind of cloud with the baseline tuned so that the central depth has
        # a fltError that is NOT zero and below 2^-28 (fp64 steps of 2^-33 around 1e6), the other depths up to 40 fp32 steps of 0.08
        # away, so lines fire.  The band path's one-threshold-per-pixel degrid is not exact for such values: they, and every pixel
        # next to one, take its recompute with the reference's fp64 expression
        n = 1200
        z0 = F(FOCAL * BASELINE / 1e6)
        z = (z0 + np.where(g.random(n) < 0.2, 0, g.integers(-40, 41, n)).astype(F) * np.spacing(z0)).astype(F)
        xy = g.uniform(-1.0, 1.0, (2, n)).astype(F) * z * np.array([[48 / 70.0], [32 / 70.0]], F)
        return _case(32, 48, np.stack([xy[0], xy[1], z]), [(a * 1e-5, b * 1e-5, 0.0) for b in (0.0, 1.5) for a in (-4.0, 0.5, 2.0)],
                     baseline=tiny_baseline(z0))
    if name == 'nonfinite':
        # NaN and +-inf coordinates among ordinary points: the counts are those of the finite points
        pts = sparse_cloud(502, 24, 96, extra=100)
        bad = g.choice(pts.shape[1], 60, replace=False)
        vals = np.array([np.nan, np.inf, -np.inf], F)
        for i, p in enumerate(bad):
            pts[i % 3, p] = vals[(i // 3) % 3]
        pts[:, bad[-1]] = np.nan
        return _case(24, 96, pts, SHIFTS6)
    if name == 'empty':
        return _case(64, 64, np.zeros((3, 0), F), SHIFTS6)
    raise KeyError(name)


LOAD = ('recache', 'pileup', 'near_zero', 'tiny_err', 'nonfinite', 'empty')
HAND = ('hand_seam', 'hand_rows', 'hand_cols', 'hand_north', 'hand_south', 'hand_fx_out', 'hand_z_reject', 'hand_centre',
        'hand_two_on_pixel', 'hand_degrid_line', 'hand_degrid_order', 'hand_edge_line', 'hand_argmax_tie')
CASES = tuple(GEOMETRY) + HAND + GROUPING + LOAD


@functools.lru_cache(maxsize=None)
def _hand_cached():
    return _hand()


@functools.lru_cache(maxsize=None)
def case(name):
    if name in GEOMETRY:
        return _geometry(name)
    if name in HAND:
        pts, shifts, literal = _hand_cached()[name]
        return _case(HH, HW, _pts(*pts), shifts, literal=list(literal))
    if name in GROUPING:
        return _grouping(name)
    return _load(name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restated counts of a case, computed once per process: a tuple of Python ints"""
    c = case(name)
    return tuple(A.coverage_counts(c['pts'], c['shifts'], c['H'], c['W'], c['focal'], c['baseline']))


# ---- the search (process_autozoom): a dense cloud that covers the whole frame for the central shifts ------------------------------
def search_case():
    """settings and common of ops.process_autozoom on a 24 x 32 frame.  The cloud (4 points per pixel on the plane z = 50) reaches
    6 px beyond the frame on three sides and starts 3 px inside it on the left: the zoom of the search (z shift -10) stretches it
    by 1.25 about the centre, which puts its left edge on the frame's.  Candidates that move the cloud to the right by more than
    a pixel lose one or two columns, the others cover every pixel and share the best count."""
    H, W = 24, 32
    g = np.random.default_rng(900)
    n = 4 * (H + 12) * (W + 4)
    pts = world(g.uniform(3.0, W + 5.5, n), g.uniform(-6.5, H + 5.5, n), np.full(n, 50.0), H, W)
    common = {'objDepthrange': (50.0, 50.0, (W // 2, H // 2), (0, 0)), 'intWidth': W, 'intHeight': H, 'fltFocal': FOCAL,
              'fltBaseline': BASELINE}
    settings = {'fltShift': 9.0, 'fltZoom': 1.25,
                'objFrom': {'fltCenterU': W / 2.0, 'fltCenterV': H / 2.0, 'intCropWidth': int(np.floor(0.97 * W)), 'intCropHeight': int(np.floor(0.97 * H))}}
    return dict(H=H, W=W, pts=pts, common=common, settings=settings)


def search_candidates(s):
    """the candidates of process_autozoom (anime_3dkenburns/common.py:96-126) that survive the crop filter, and their shifts"""
    st, cm = s['settings'], s['common']
    lin = np.linspace(-st['fltShift'], st['fltShift'], 16)
    oF = st['objFrom']
    cw, ch = oF['intCropWidth'] / st['fltZoom'], oF['intCropHeight'] / st['fltZoom']
    d_from = cm['objDepthrange'][0]
    d_to = cm['objDepthrange'][0] * (cw / oF['intCropWidth'])
    W, H = cm['intWidth'], cm['intHeight']
    cands = []
    for iu in range(16):
        for iv in range(16):
            su, sv = lin[iv].item(), lin[iu].item()
            if oF['fltCenterU'] + su < cw / 2.0 or oF['fltCenterU'] + su > W - cw / 2.0:
                continue
            if oF['fltCenterV'] + sv < ch / 2.0 or oF['fltCenterV'] + sv > H - ch / 2.0:
                continue
            cands.append((su, sv))
    # process_shift's host part (common.py:60-72) in python floats; the crop centre is the frame centre
    cd, f = cm['objDepthrange'][0] + (d_to - d_from), cm['fltFocal']
    fu, fv = cm['objDepthrange'][2]
    shifts = []
    for su, sv in cands:
        fx, fy = ((fu - W / 2.0) * cd) / f, ((fv - H / 2.0) * cd) / f
        tx, ty = ((fu + su - W / 2.0) * cd) / f, ((fv + sv - H / 2.0) * cd) / f
        shifts.append((fx - tx, fy - ty, d_to - d_from))
    return cands, shifts
