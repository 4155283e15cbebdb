"""numpy restatement of the PatchMatch inpainting contract of csrc/patchmatch.hip.

Integer-exact and deterministic: the HIP library must return the same bytes.  Written for clarity, vectorised over the targets of
a level so that the CPU tests run at small sizes in seconds.  Every constant here is the library's.
"""
import numpy as np

M32 = 0xFFFFFFFF
JUMP = 4                       # the longer propagation step
INIT_PASS = 0xFFFF             # the `pass` field of the hash for the initial draws
WEIGHT_ONE = 1 << 16


def em_iters(level):
    return min(2 + 2 * level, 10)


def nnf_passes(level):
    return min(2 + level, 6)


def weight_p(p):
    """P of the vote weight floor(2^16 * P / (P + d)): the SSD of a patch whose every channel is off by 8"""
    return 3 * p * p * 64


def _mix32(x):
    """lowbias32 (C. Wellons): an invertible 32-bit mixer; works on Python ints and uint32 arrays"""
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint32)
        x ^= x >> np.uint32(16); x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15); x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
        return x
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def rng(seed, level, it, pas, pixel, sample):
    """the counter hash of (seed, level, EM iteration, pass, pixel, sample): h = mix(seed ^ 0x9E3779B9), then h = mix(h ^ v) for
    each further field in that order.  pixel: uint32 array of level-local indices y * w + x."""
    h = _mix32((seed & M32) ^ 0x9E3779B9)
    for v in (level, it, pas):
        h = _mix32(h ^ v)
    h = _mix32(np.uint32(h) ^ pixel.astype(np.uint32))
    return _mix32(h ^ np.uint32(sample))


def max_levels(H, W, p):
    """the pyramid the prepare step builds: level l+1 is ceil(h/2) x ceil(w/2), built while both of its sides are > p"""
    n, h, w = 1, H, W
    while (h + 1) // 2 > p and (w + 1) // 2 > p:
        h, w = (h + 1) // 2, (w + 1) // 2
        n += 1
    return n


def _down(col, known, excl):
    h, w = known.shape
    hn, wn = (h + 1) // 2, (w + 1) // 2
    s = np.zeros((hn, wn, 3), np.int64)
    n = np.zeros((hn, wn), np.int64)
    kn = np.zeros((hn, wn), bool)
    ex = np.zeros((hn, wn), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            k = known[dy::2, dx::2]
            c = col[dy::2, dx::2].astype(np.int64)
            e = excl[dy::2, dx::2]
            hh, ww = k.shape
            s[:hh, :ww] += c * k[..., None]
            n[:hh, :ww] += k
            kn[:hh, :ww] |= k
            ex[:hh, :ww] |= e
    out = np.where(n[..., None] > 0, (s + n[..., None] // 2) // np.maximum(n, 1)[..., None], 0)
    return out.astype(np.int32), kn, ex


def _window_any(bad, r):
    """any(bad) over the (2r+1)^2 window of every pixel (False outside the frame)"""
    h, w = bad.shape
    pad = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = bad
    out = np.zeros((h, w), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def _maps(known, excl, r):
    h, w = known.shape
    interior = np.zeros((h, w), bool)
    interior[r:h - r, r:w - r] = True
    valid = interior & ~_window_any(~known | excl, r)
    target = interior & _window_any(~known, r)
    return valid, target


def build_pyramid(img, hole, excl, p):
    """levels [dict(col int32 [h,w,3], known, excl, valid, target)], finest first; all levels the prepare step builds"""
    r = p // 2
    col, known, ex = img.astype(np.int32), ~hole, excl.copy()
    levels = []
    for _ in range(max_levels(img.shape[0], img.shape[1], p)):
        if levels:
            col, known, ex = _down(col, known, ex)
        valid, target = _maps(known, ex, r)
        levels.append(dict(col=col, known=known, excl=ex, valid=valid, target=target))
    return levels


def used_levels(levels):
    """the schedule: level 0 and every following level while it still has a valid source (0 when level 0 has none)"""
    if not levels[0]['valid'].any():
        return 0
    n = 1
    while n < len(levels) and levels[n]['valid'].any():
        n += 1
    return n


def _ssd(col, ty, tx, sy, sx, r):
    d = np.zeros(ty.shape, np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            e = col[ty + dy, tx + dx] - col[sy + dy, sx + dx]
            d += (e.astype(np.int64) ** 2).sum(-1)
    return d


def _nnf_pass(L, lvl, it, pas, seed, r, nnf_y, nnf_x, ty, tx, tidx):
    """one Jacobi pass over the targets: returns the new (sy, sx) of every target and its SSD"""
    col, valid, target = L['col'], L['valid'], L['target']
    h, w = valid.shape
    by, bx = nnf_y[ty, tx].copy(), nnf_x[ty, tx].copy()
    bd = _ssd(col, ty, tx, by, bx, r)

    def consider(cy, cx, ok):
        ok = ok & (cy >= 0) & (cy < h) & (cx >= 0) & (cx < w)
        ok &= valid[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
        if not ok.any():
            return
        i = np.flatnonzero(ok)
        d = _ssd(col, ty[i], tx[i], cy[i], cx[i], r)
        b = d < bd[i]
        j = i[b]
        by[j], bx[j], bd[j] = cy[i][b], cx[i][b], d[b]

    for k in (1, JUMP):
        for dy, dx in ((0, -k), (0, k), (-k, 0), (k, 0)):
            ny, nx = ty + dy, tx + dx
            inb = (ny >= 0) & (ny < h) & (nx >= 0) & (nx < w)
            nyc, nxc = np.clip(ny, 0, h - 1), np.clip(nx, 0, w - 1)
            ok = inb & target[nyc, nxc]
            consider(nnf_y[nyc, nxc] - dy, nnf_x[nyc, nxc] - dx, ok)
    R, j = max(h, w), 0
    while R >= 1:
        m = np.uint32(2 * R + 1)
        oy = (rng(seed, lvl, it, pas, tidx, 2 * j) % m).astype(np.int64) - R
        ox = (rng(seed, lvl, it, pas, tidx, 2 * j + 1) % m).astype(np.int64) - R
        consider(by + oy, bx + ox, np.ones(ty.shape, bool))
        R >>= 1
        j += 1
    return by, bx, bd


def _vote(L, r, nnf_y, nnf_x, wgt):
    col, known = L['col'], L['known']
    h, w = known.shape
    qy, qx = np.nonzero(~known)
    sw = np.zeros(qy.shape, np.int64)
    sc = np.zeros(qy.shape + (3,), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ty, tx = qy - dy, qx - dx
            ok = (ty >= r) & (ty < h - r) & (tx >= r) & (tx < w - r)
            i = np.flatnonzero(ok)
            t_y, t_x = ty[i], tx[i]
            wt = wgt[t_y, t_x]
            c = col[nnf_y[t_y, t_x] + dy, nnf_x[t_y, t_x] + dx].astype(np.int64)
            sw[i] += wt
            sc[i] += wt[:, None] * c
    col[qy, qx] = ((sc + (sw // 2)[:, None]) // sw[:, None]).astype(np.int32)


def _draw(valid_list, seed, lvl, tidx):
    return valid_list[(rng(seed, lvl, 0, INIT_PASS, tidx, 0) % np.uint32(len(valid_list))).astype(np.int64)]


def patchmatch_inpaint(img, mask, global_mask=None, patch_size=15, seed=0):
    """img uint8 [H,W,3]; mask uint8 [H,W] or [H,W,1], nonzero = hole; global_mask likewise, nonzero = never a patch source.
    Returns a new uint8 [H,W,3]."""
    img = np.ascontiguousarray(img)
    p = int(patch_size)
    if p < 3 or p % 2 == 0 or p > 15:
        raise ValueError("patch_size must be odd and in [3, 15] (got %d)" % p)
    H, W = img.shape[:2]
    if H < p or W < p:
        raise ValueError("image %dx%d is smaller than the patch size %d" % (H, W, p))
    hole = mask.reshape(H, W) != 0
    excl = np.zeros((H, W), bool) if global_mask is None else global_mask.reshape(H, W) != 0
    r = p // 2
    levels = build_pyramid(img, hole, excl, p)
    nl = used_levels(levels)
    if nl == 0 or not levels[0]['target'].any():
        return img.copy()
    P = weight_p(p)
    for lvl in range(nl - 1, -1, -1):
        L = levels[lvl]
        col, known, valid, target = L['col'], L['known'], L['valid'], L['target']
        h, w = known.shape
        valid_list = np.flatnonzero(valid)
        ty, tx = np.nonzero(target)
        tidx = (ty * w + tx).astype(np.uint32)
        nnf_y = np.zeros((h, w), np.int64)
        nnf_x = np.zeros((h, w), np.int64)
        if lvl == nl - 1:
            n = known.sum()
            mean = (col[known].astype(np.int64).sum(0) + n // 2) // n
            col[~known] = mean
            s = _draw(valid_list, seed, lvl, tidx)
            nnf_y[ty, tx], nnf_x[ty, tx] = s // w, s % w
        else:
            Pa = levels[lvl + 1]
            hy, hx = np.nonzero(~known)
            col[hy, hx] = Pa['col'][hy // 2, hx // 2]
            py, px = ty // 2, tx // 2
            cy = 2 * pnnf_y[py, px] + (ty & 1)
            cx = 2 * pnnf_x[py, px] + (tx & 1)
            ok = Pa['target'][py, px] & (cy < h) & (cx < w)
            ok &= valid[np.minimum(cy, h - 1), np.minimum(cx, w - 1)]
            s = _draw(valid_list, seed, lvl, tidx)
            nnf_y[ty, tx] = np.where(ok, cy, s // w)
            nnf_x[ty, tx] = np.where(ok, cx, s % w)
        wgt = np.zeros((h, w), np.int64)
        for it in range(em_iters(lvl)):
            for pas in range(nnf_passes(lvl)):
                by, bx, bd = _nnf_pass(L, lvl, it, pas, seed, r, nnf_y, nnf_x, ty, tx, tidx)
                nnf_y, nnf_x = nnf_y.copy(), nnf_x.copy()
                nnf_y[ty, tx], nnf_x[ty, tx] = by, bx
                wgt[ty, tx] = (WEIGHT_ONE * P) // (P + bd)
            _vote(L, r, nnf_y, nnf_x, wgt)
        pnnf_y, pnnf_x = nnf_y, nnf_x
    return levels[0]['col'].astype(np.uint8)
