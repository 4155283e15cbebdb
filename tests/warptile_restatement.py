"""Exact numpy restatement of the tiled point-cloud renderer (csrc/warptile.hip, csrc/warp_device.h) -- TEST INFRASTRUCTURE ONLY.

numpy only; nothing from the library or from oracle/.  Every output bit of the tile path is predictable: the geometry is fp32
statement for statement (the kernels are built with -ffp-contract=off, so each operation rounds once, which is what numpy's
float32 arithmetic does), every product value * weight is formed in fp32 and converted to a 64-bit integer, the integers are
added (order free) and rounded to fp32 once.

Reference text the kernels cite (anime_3dkenburns/):
  models/utils.py:56-315   render_pointcloud: :59 z-buffer start 1e6, :76-99 projection, :101-147 updateZee (arg-max corner),
                           :152-212 updateDegrid, :215-313 updateOutput (z-test + bilinear splat), :315 normalise
  common.py:60-81          process_shift (:78-81 the per-point part)
  common.py:145-248        fill_disocclusion (:160 validity, :168-175 directions, :186-204 the two marches, :208-217 the choice)
  kenburns_effect.py:1039-1040   depth mask render[3] * (existing > 0), uint8 frame

Units of the integer planes (warptile.hip, to_fixed / to_fixed_sat / from_fixed): frame mode 2^-40 for colour and weight, 2^-20
for depth; channel mode 2^-32 for data, saturating at +-2^62 units, 2^-40 for the weight.  A nonzero product that converts to
zero becomes +-1 unit.
"""
import numpy as np

F = np.float32
D = np.float64
TW, TH = 32, 16                       # destination tile of warptile.hip
SCALE_C, SCALE_D, SCALE_F = 2.0 ** 40, 2.0 ** 20, 2.0 ** 32
DIRX = (-1, 0, 1, 1, -1, 1, 2, 2, -2, -1, 1, 2, 3, 3, 3, 3)       # common.py:168
DIRY = (1, 1, 1, 0, 2, 2, 1, -1, 3, 3, 3, 3, 2, 1, -1, -2)        # common.py:169


def process_shift(pts, shift):
    """load_point<SHIFT> (common.py:78-81): fp32, one rounding per operation"""
    x, y, z = (np.array(pts[i], F) for i in range(3))
    s = [F(v) for v in shift]
    with np.errstate(all='ignore'):
        r = z / (z + F(0.0000001))
        return x * r + s[0], y * r + s[1], z + s[2]


def project(x, y, z, H, W, focal, baseline):
    """project() of warp_device.h (models/utils.py:76-99): fp32 except where the header casts to double"""
    zero, one = F(0.0), F(1.0)
    with np.errstate(all='ignore'):
        ok = ~(z.astype(D) < 0.001)
        lvx, lvy, lvz = zero - x, zero - y, zero - z
        ax, ay, az = zero - x, zero - y, F(focal) - z
        num = (ax * zero + ay * zero) + az * one
        den = (lvx * zero + lvy * zero) + lvz * one
        dist = num / den
        ok &= ~(np.abs(den).astype(D) < 0.001)
        ix = x + dist * lvx
        iy = y + dist * lvy
        fx = ((ix.astype(D) + 0.5 * W) - 0.5).astype(F)
        fy = ((iy.astype(D) + 0.5 * H) - 0.5).astype(F)
        err = (1000000.0 - ((focal * baseline) / (z.astype(D) + 0.0000001))).astype(F)
    return ok, fx, fy, err


def corner_weights(fx, fy):
    """corner_weights(): x0, y0 and the NW, NE, SW, SE weights [4, n] (models/utils.py:101-113)"""
    x0 = np.floor(fx).astype(np.int64); y0 = np.floor(fy).astype(np.int64)
    x1, y1, xf, yf = (x0 + 1).astype(F), (y0 + 1).astype(F), x0.astype(F), y0.astype(F)
    w = np.stack([(x1 - fx) * (y1 - fy), (fx - xf) * (y1 - fy), (x1 - fx) * (fy - yf), (fx - xf) * (fy - yf)])
    assert w.dtype == F
    return x0, y0, w


def argmax_corner(w):
    """argmax_corner(): 0..3 in the reference's if/else order (models/utils.py:115-135), -1 when no branch fires"""
    nw, ne, sw, se = w
    conds = [(nw >= ne) & (nw >= sw) & (nw >= se), (ne >= nw) & (ne >= sw) & (ne >= se),
             (sw >= nw) & (sw >= ne) & (sw >= se), (se >= nw) & (se >= ne) & (se >= sw)]
    return np.select(conds, [0, 1, 2, 3], default=-1)


def degrid(zee):
    """updateDegrid in Jacobi form (models/utils.py:152-212): the four stencil pairs in the kernel's order"""
    H, W = zee.shape
    pad = np.full((H + 2, W + 2), F(0.0)); pad[1:-1, 1:-1] = zee
    inimg = np.zeros((H + 2, W + 2), bool); inimg[1:-1, 1:-1] = True
    c = zee; c64 = c.astype(D)
    cnt = np.zeros((H, W), np.int64); s = np.zeros((H, W), F)
    for ox, oy in ((1, 0), (0, 1), (1, 1), (1, -1)):
        a = pad[1 + oy:H + 1 + oy, 1 + ox:W + 1 + ox]; d = pad[1 - oy:H + 1 - oy, 1 - ox:W + 1 - ox]
        both = inimg[1 + oy:H + 1 + oy, 1 + ox:W + 1 + ox] & inimg[1 - oy:H + 1 - oy, 1 - ox:W + 1 - ox]
        take = both & (c64 >= a.astype(D) + 1.0) & (c64 >= d.astype(D) + 1.0)
        s = np.where(take, (s + a) + d, s)
        cnt = cnt + 2 * take
    assert s.dtype == F
    with np.errstate(all='ignore'):
        m = s / np.maximum(cnt, 1).astype(F)
    return np.where(cnt > 0, np.minimum(c, m), c).astype(F)


def _floor_div(a, b):
    return np.floor_divide(a, b)


def tile_range(v0, T, nt):
    """tile_range(): the tiles whose area expanded by 1 px meets the footprint [v0, v0 + 1]"""
    lo = _floor_div(v0 + T - 1, T) - 1
    hi = _floor_div(v0 + 2, T)
    return np.maximum(lo, 0), np.minimum(hi, nt - 1)


def to_fixed(prod, scale, sat=False):
    """to_fixed / to_fixed_sat: trunc(prod * scale) as int64, +-1 for a nonzero product that converts to zero"""
    with np.errstate(all='ignore'):
        f = prod * F(scale)
    assert f.dtype == F
    if sat:
        f = np.minimum(np.maximum(f, F(-2.0 ** 62)), F(2.0 ** 62))
    q = f.astype(np.int64)                                       # truncation toward zero
    small = (q == 0) & (prod != 0)
    q = np.where(small, np.where(prod > 0, 1, -1), q)
    return q, small


def from_fixed(q, scale):
    return (q.astype(D) * (1.0 / scale)).astype(F)


def to_u8(v):
    """to_u8() of warp_device.h (kenburns_effect.py:1040): v * 255 clamped to [0, 255], truncated"""
    u = np.asarray(v, F) * F(255.0)
    u = np.where(u < F(0.0), F(0.0), np.where(u > F(255.0), F(255.0), u))
    return u.astype(np.uint8)


def _roundf(f):
    """roundf: half away from zero (exact: a float32 plus 0.5 is exact in float64)"""
    f = f.astype(D)
    return np.where(f >= 0, np.floor(f + 0.5), np.ceil(f - 0.5)).astype(np.int64)


def hole_sources(valid, mdepth):
    """fill_disocclusion's choice for every invalid pixel (common.py:160-217).
    Returns int64 [n, 8]: y, x, from_y, from_x, to_y, to_x, src_y, src_x (-1 where no direction is complete), and a bool [n]:
    a second direction reached the winner's distance (a tie)."""
    H, W = valid.shape
    ys, xs = np.nonzero(~valid)
    n = ys.size
    best = np.full(n, F(1000000.0))
    rec = np.full((n, 8), -1, np.int64); rec[:, 0] = ys; rec[:, 1] = xs
    alld = np.full((16, n), np.inf, F)
    for k in range(16):
        dx, dy = F(DIRX[k]), F(DIRY[k])
        nrm = np.sqrt((dx * dx) + (dy * dy)); assert nrm.dtype == F     # common.py:172-175
        dx = dx / nrm; dy = dy / nrm
        end = []
        for sx, sy in ((-dx, -dy), (dx, dy)):                    # from, to
            fx, fy = xs.astype(F), ys.astype(F)
            ix = np.zeros(n, np.int64); iy = np.zeros(n, np.int64)
            found = np.zeros(n, bool); active = np.ones(n, bool)
            while active.any():
                fx = np.where(active, fx + sx, fx); fy = np.where(active, fy + sy, fy)
                jx, jy = _roundf(fx), _roundf(fy)
                ix = np.where(active, jx, ix); iy = np.where(active, jy, iy)
                inb = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
                hit = inb & valid[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)]
                found |= active & hit
                active &= inb & ~hit
            end.append((ix, iy, found))
        (fxi, fyi, fok), (txi, tyi, tok) = end
        ddx, ddy = (txi - fxi).astype(F), (tyi - fyi).astype(F)
        dist = np.sqrt(ddx * ddx + ddy * ddy)                    # common.py:208
        both = fok & tok
        alld[k] = np.where(both, dist, F(np.inf))
        upd = both & (best > dist)                               # strict: the first direction wins ties
        best = np.where(upd, dist, best)
        fyc, fxc = np.clip(fyi, 0, H - 1), np.clip(fxi, 0, W - 1)
        tyc, txc = np.clip(tyi, 0, H - 1), np.clip(txi, 0, W - 1)
        to_wins = mdepth[fyc, fxc] < mdepth[tyc, txc]            # common.py:214-217
        new = np.stack([ys, xs, fyi, fxi, tyi, txi, np.where(to_wins, tyi, fyi), np.where(to_wins, txi, fxi)], 1)
        rec = np.where(upd[:, None], new, rec)
    tie = (rec[:, 6] >= 0) & ((alld == best[None]).sum(0) >= 2)
    return rec, tie


def fill_disocclusion(inp, depth):
    """the stand-alone operator (common.py:145-248): inp [C, H, W], depth [H, W]"""
    rec, _ = hole_sources(depth.astype(D) > 0.0, depth)
    out = inp.copy()
    f = rec[rec[:, 6] >= 0]
    out[:, f[:, 0], f[:, 1]] = inp[:, f[:, 6], f[:, 7]]
    return out


def render(pts, data, H, W, focal, baseline, shift=None, mode='frame'):
    """One call of the tile path.  pts [3, N], data [C, N] (mode 'frame': rgb + depth, C = 4; mode 'channels': any C).
    Returns a dict: zee, zd, acc (int64 [C, H, W]), wacc (int64 [H, W]), existing, render (before the fill) and, in frame mode,
    render_filled, frame, holes (hole_sources), tie; tile_entries [nty, ntx]; the float-path statistics S, A [C + 1, H, W]
    (last plane: the weight), n [H, W] and nz [H, W] (the terms whose weight is not zero); unit_pos / unit_neg: how many products
    took the +-1 rule; the geometry of the points that pass the range test: idx, fx, fy, err, x0, y0, w [4, n], passed [4, n]."""
    pts = np.asarray(pts, F); data = np.asarray(data, F)
    C, N = data.shape
    assert pts.shape == (3, N) and (mode != 'frame' or C == 4)
    x, y, z = process_shift(pts, shift) if shift is not None else (pts[0], pts[1], pts[2])
    ok, fx, fy, err = project(x, y, z, H, W, focal, baseline)
    with np.errstate(all='ignore'):                              # the tile path's range test (bins_of_point)
        ok &= (fx > F(-4.0)) & (fy > F(-4.0)) & (fx < F(W + 4)) & (fy < F(H + 4))
    idx = np.nonzero(ok)[0]
    fx, fy, err = fx[idx], fy[idx], err[idx]
    x0, y0, w = corner_weights(fx, fy)
    ntx, nty = (W + TW - 1) // TW, (H + TH - 1) // TH
    # entries per tile (k_tile_bin)
    txl, txh = tile_range(x0, TW, ntx); tyl, tyh = tile_range(y0, TH, nty)
    binned = (txl <= txh) & (tyl <= tyh)
    tiles = np.zeros((nty, ntx), np.int64)
    for j in range(4):
        ty, tx = tyl + (j >> 1), txl + (j & 1)
        m = binned & (ty <= tyh) & (tx <= txh)
        np.add.at(tiles, (ty[m], tx[m]), 1)
    # updateZee
    zee = np.full(H * W, F(1000000.0))
    sel = argmax_corner(w)
    cx, cy = x0 + (sel & 1), y0 + (sel >> 1)
    m = (sel >= 0) & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    np.minimum.at(zee, cy[m] * W + cx[m], err[m])
    zee = zee.reshape(H, W)
    zd = degrid(zee)
    # updateOutput: z-test + splat
    frame_mode = mode == 'frame'
    acc = np.zeros((C, H * W), np.int64); wacc = np.zeros(H * W, np.int64)
    S = np.zeros((C + 1, H * W), D); A = np.zeros((C + 1, H * W), D); n = np.zeros(H * W, np.int64)
    nz = np.zeros(H * W, np.int64); passed = np.zeros((4, idx.size), bool)
    unit = [0, 0]
    zd64 = zd.astype(D).ravel(); err64 = err.astype(D)
    for k in range(4):
        cx, cy = x0 + (k & 1), y0 + (k >> 1)
        inimg = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        pix = np.where(inimg, cy * W + cx, 0)
        take = inimg & (err64 <= zd64[pix] + 1.0)
        passed[k] = take
        pix, wk, src = pix[take], w[k][take], idx[take]
        np.add.at(n, pix, 1); np.add.at(nz, pix, (wk != 0).astype(np.int64))
        for c in range(C + 1):
            prod = (data[c, src] if c < C else F(1.0)) * wk
            assert prod.dtype == F
            if c == C:
                q, small = to_fixed(prod, SCALE_C)
                np.add.at(wacc, pix, q)
            else:
                if frame_mode:
                    q, small = to_fixed(prod, SCALE_D if c == 3 else SCALE_C)
                else:
                    q, small = to_fixed(prod, SCALE_F, sat=True)
                np.add.at(acc[c], pix, q)
            unit[0] += int((small & (prod > 0)).sum()); unit[1] += int((small & (prod < 0)).sum())
            p64 = prod.astype(D)
            np.add.at(S[c], pix, p64); np.add.at(A[c], pix, np.abs(p64))
    e = from_fixed(wacc, SCALE_C)
    den = e + F(0.0000001)
    scales = [SCALE_C, SCALE_C, SCALE_C, SCALE_D] if frame_mode else [SCALE_F] * C
    rnd = np.stack([from_fixed(acc[c], scales[c]) / den for c in range(C)])
    assert rnd.dtype == F
    out = dict(zee=zee, zd=zd, acc=acc.reshape(C, H, W), wacc=wacc.reshape(H, W), existing=e.reshape(H, W),
               render=rnd.reshape(C, H, W), tile_entries=tiles, S=S.reshape(C + 1, H, W), A=A.reshape(C + 1, H, W),
               n=n.reshape(H, W), nz=nz.reshape(H, W), unit_pos=unit[0], unit_neg=unit[1], scales=scales,
               idx=idx, fx=fx, fy=fy, err=err, x0=x0, y0=y0, w=w, passed=passed)
    if frame_mode:
        mdepth = (rnd[3] * np.where(e > F(0.0), F(1.0), F(0.0))).reshape(H, W)      # kenburns_effect.py:1039
        valid = mdepth.astype(D) > 0.0                                               # common.py:160
        holes, tie = hole_sources(valid, mdepth)
        filled = out['render'].copy()
        f = holes[holes[:, 6] >= 0]
        filled[:, f[:, 0], f[:, 1]] = out['render'][:, f[:, 6], f[:, 7]]
        out.update(mdepth=mdepth, valid=valid, holes=holes, tie=tie, render_filled=filled,
                   frame=np.ascontiguousarray(to_u8(filled[:3]).transpose(1, 2, 0)))
    return out
