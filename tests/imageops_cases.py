"""Seeded cases and plain references for the image-glue kernels (csrc/imageops.hip, csrc/zoedepth.hip), shared by
tests/test_imageops_references.py (CPU: the oracle and the property every case exists for) and tests/test_gpu_imageops.py (the HIP
kernels).  The references are numpy float64, or torch CPU float64 for the operations aten defines; nothing here comes from the library
or from the oracle.  Where a tolerance needs a yardstick, the plain float32 evaluation of the same formula stands next to the float64
one and `e32` is its error (the convention of tokens_cases.py): a result may differ from float64 by max(4 * e32, 8 * 2^-23) of the scale."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EPS32 = 2.0 ** -23


def rng_of(*key):
    return np.random.default_rng([0x1A6E] + [int(k) for k in key])


def yardstick(e32):
    """relative bound of the project's convention"""
    return max(4.0 * e32, 8.0 * EPS32)


def ulp32(v):
    return float(np.spacing(F32(abs(v))))


# =====================================================================================================================================
# 1. row resamplers defined by OpenCV
# =====================================================================================================================================
RESIZE_PAIRS = [((64, 64), (1, 1)), ((7, 300), (5, 257)), ((3, 5), (17, 259)), ((1, 9), (4, 9)), ((97, 513), (33, 258)),
                ((31, 257), (62, 514)), ((255, 255), (256, 256)), ((6, 259), (6, 259))]
AREA_PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 257)), ((5, 7), (5, 300)), ((96, 128), (150, 200)), ((32, 255), (33, 257)),
              ((8, 130), (16, 260))]
LANCZOS_PAIRS = RESIZE_PAIRS + [((608, 416), (600, 400)), ((8, 8), (1, 1)), ((40, 520), (33, 513))]
LINEAR_CHANNELS = (1, 3, 4)


def pair_id(p):
    return "%dx%d-%dx%d" % (p[0] + p[1])


def image_u8(shape, *key):
    """uint8 noise: no two neighbours alike, so a wrong tap or fraction moves the result by many levels"""
    return rng_of(*key).integers(0, 256, shape, dtype=np.uint8)


def image_f32(shape, *key):
    return (rng_of(*key).standard_normal(shape) * 3.0).astype(F32)


def leres_image(H, W):
    """BGR frame with three clearly different planes (B in [0, 80), G in [88, 168), R in [176, 256)): a missing swap is off by >= 96"""
    r = rng_of(7, H, W)
    return np.stack([r.integers(0, 80, (H, W)), r.integers(88, 168, (H, W)), r.integers(176, 256, (H, W))], -1).astype(np.uint8)


LERES_MEAN = np.array([0.485, 0.456, 0.406])
LERES_STD = np.array([0.229, 0.224, 0.225])


def cv_taps(in_size, out_size):
    """cv2.resize(INTER_LINEAR): source coordinate at half-pixel centres, ROUNDED TO float32 as resize.cpp defines it
    (`(float)((d + 0.5) * scale - 0.5)`), replicate clamp; everything after the coordinate is float64.  -> (i0, i1, f)"""
    d = np.arange(out_size, dtype=F64)
    fx = ((d + 0.5) * (in_size / out_size) - 0.5).astype(F32).astype(F64)
    sx = np.floor(fx)
    f = fx - sx
    lo, hi = sx < 0, sx >= in_size - 1
    f[lo | hi] = 0.0
    sx = np.clip(sx, 0, in_size - 1).astype(np.int64)
    return sx, np.minimum(sx + 1, in_size - 1), f


def area_taps(in_size, out_size):
    """cv2.resize(INTER_AREA) when enlarging: linear taps with area fractions, sx = floor(d * scale), fx = (d + 1) - (sx + 1) / scale,
    fx <= 0 -> 0 else its fractional part, clamped at both ends; float64"""
    d = np.arange(out_size, dtype=F64)
    scale = in_size / out_size
    sx = np.floor(d * scale)
    fx = (d + 1.0) - (sx + 1.0) / scale
    f = np.where(fx <= 0.0, 0.0, fx - np.floor(fx))
    f[(sx < 0) | (sx >= in_size - 1)] = 0.0
    sx = np.clip(sx, 0, in_size - 1).astype(np.int64)
    return sx, np.minimum(sx + 1, in_size - 1), f


def blend2(src, ty, tx, dtype=F64):
    """two-pass blend of an [H, W, C] image with per-axis taps: rows s0 * (1 - fx) + s1 * fx, then r0 * (1 - fy) + r1 * fy, in `dtype`"""
    s = np.asarray(src, dtype)
    (y0, y1, fy), (x0, x1, fx) = ty, tx
    fx = fx.astype(dtype)[None, :, None]
    fy = fy.astype(dtype)[:, None, None]
    one = dtype(1.0)
    r0 = s[y0][:, x0] * (one - fx) + s[y0][:, x1] * fx
    r1 = s[y1][:, x0] * (one - fx) + s[y1][:, x1] * fx
    return r0 * (one - fy) + r1 * fy


def _hwc(a):
    return a if a.ndim == 3 else a[..., None]


def bilinear_ref(src, h, w, dtype=F64):
    """cv2.resize(src [H, W(, C)], (w, h), INTER_LINEAR) unrounded; identical sizes return the input"""
    s = _hwc(np.asarray(src))
    H, W = s.shape[:2]
    if (H, W) == (h, w):
        return s.astype(dtype)
    return blend2(s, cv_taps(H, h), cv_taps(W, w), dtype)


def area_ref(src, H, W):
    """the enlarging INTER_AREA of an [h, w] plane to [H, W], unrounded"""
    h, w = src.shape
    if (h, w) == (H, W):
        return src.astype(F64)
    return blend2(src[..., None], area_taps(h, H), area_taps(w, W))[..., 0]


def lanczos_weights(in_size, out_size):
    """-> clamped tap indices [out, 8] and weights [out, 8]: sinc(t) sinc(t / 4) at t = fx - (i - 3), normalised per phase"""
    d = np.arange(out_size, dtype=F64)
    fx = ((d + 0.5) * (in_size / out_size) - 0.5).astype(F32).astype(F64)
    sx = np.floor(fx)
    t = (fx - sx)[:, None] - (np.arange(8, dtype=F64) - 3.0)[None, :]
    wgt = np.sinc(t) * np.sinc(t / 4.0)
    wgt /= wgt.sum(1, keepdims=True)
    idx = np.clip(sx.astype(np.int64)[:, None] + np.arange(8)[None, :] - 3, 0, in_size - 1)
    return idx, wgt


def lanczos_ref(src, H, W):
    h, w = src.shape
    iy, wy = lanczos_weights(h, H)
    ix, wx = lanczos_weights(w, W)
    s = src.astype(F64)
    rows = (s[:, ix] * wx[None]).sum(-1)                    # [h, W]
    out = (rows[iy] * wy[:, :, None]).sum(1)                # [H, W]
    return np.clip(out, 0.0, 255.0)


def ramp_u8(H, W, C=1):
    """horizontal ramp 0 .. 255 over the width"""
    r = np.round(np.linspace(0, 255, W)).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(r[None, :, None], (H, W, C)))


# =====================================================================================================================================
# 2. crop + resize (getRectSubPix, then INTER_LINEAR)
# =====================================================================================================================================
CROP_FRAMES = [(1, 1), (3, 63), (4, 64), (5, 65), (9, 257), (150, 200)]
CROP_KINDS = ('same_int', 'same_frac', 'half', 'twice', 'tall', 'outside', 'one')
TILE_X, TILE_Y, WIN_W, WIN_H = 64, 4, 80, 8                 # k_crop_resize_tile's geometry


def crop_case(frame_hw, kind):
    """-> (ph, pw, cx, cy); centres are multiples of 1/4, so the float32 origin of the kernel is exact"""
    H, W = frame_hw
    cx0, cy0 = (W - 1) * 0.5, (H - 1) * 0.5
    return {'same_int': (H, W, cx0, cy0),                                      # origin (0, 0): a = b = 0
            'same_frac': (H, W, cx0 + 0.25, cy0 + 0.75),
            'half': (max(1, H // 2), max(1, W // 2), cx0 + 0.25, cy0 - 0.5),
            'twice': (2 * H, 2 * W, cx0 + 0.5, cy0 + 0.25),
            'tall': (2 * H, W, cx0 - 0.25, cy0 + 0.5),
            'outside': (max(1, H // 2), max(1, W // 2), -1000.0, -1000.0),
            'one': (1, 1, cx0 * 0.5 + 0.25, cy0 * 0.5 + 0.25)}[kind]


def _cv_src_scalar(d, in_size, out_size):
    i0, i1, _ = cv_taps(in_size, out_size)
    return int(i0[d]), int(i1[d])


def crop_fits(frame_hw, ph, pw):
    """the block-uniform `fits` decision of k_crop_resize_tile, evaluated per block -> bool [blocks_y, blocks_x]"""
    H, W = frame_hw
    same = (ph, pw) == (H, W)
    out = np.zeros((-(-H // TILE_Y), -(-W // TILE_X)), bool)
    for j in range(out.shape[0]):
        for i in range(out.shape[1]):
            bx, by = i * TILE_X, j * TILE_Y
            xl, yl = min(bx + TILE_X - 1, W - 1), min(by + TILE_Y - 1, H - 1)
            xmin, xmax, ymin, ymax = bx, xl, by, yl
            if not same:
                xmin, xmax = _cv_src_scalar(bx, pw, W)[0], _cv_src_scalar(xl, pw, W)[1]
                ymin, ymax = _cv_src_scalar(by, ph, H)[0], _cv_src_scalar(yl, ph, H)[1]
            out[j, i] = (xmax - xmin + 2 <= WIN_W) and (ymax - ymin + 2 <= WIN_H)
    return out


def crop_ref(frame, ph, pw, cx, cy):
    """unrounded float64 chain: bilinear sub-pixel patch (replicated border), then the bilinear resize of that patch to the frame size"""
    H, W = frame.shape[:2]
    ox, oy = cx - (pw - 1) * 0.5, cy - (ph - 1) * 0.5
    ix, iy = math.floor(ox), math.floor(oy)
    a, b = ox - ix, oy - iy
    ys, xs = iy + np.arange(ph + 1), ix + np.arange(pw + 1)
    f = frame.astype(F64)[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)]
    patch = (f[:-1, :-1] * (1 - a) * (1 - b) + f[:-1, 1:] * a * (1 - b) + f[1:, :-1] * (1 - a) * b + f[1:, 1:] * a * b)
    return bilinear_ref(patch, H, W)


# =====================================================================================================================================
# 3. reductions
# =====================================================================================================================================
REDUCE_LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 18 + 1027]


def minmax_positions(n):
    """where the extreme is planted: first, last, in the last full float4, in the scalar tail (where the length has one)"""
    pos = {'first': 0, 'last': n - 1}
    n4 = (n // 4) * 4
    if n4 >= 4:
        pos['last_vec'] = n4 - 2
    if n4 < n:
        pos['tail'] = n4
    return pos


def minmax_case(n, where):
    """values in (-1, 1) with the maximum 7 and the minimum -9 at (pos, a distinct pos)"""
    x = rng_of(31, n).uniform(-1.0, 1.0, n).astype(F32)
    p = minmax_positions(n)[where]
    x[p] = 7.0
    q = (p + n // 2) % n
    if q != p:
        x[q] = -9.0
    return x


def minmax_value_cases(n):
    r = rng_of(32, n)
    zeros = np.where(r.integers(0, 2, n) == 1, F32(-0.0), F32(0.0)).astype(F32)
    inf = r.uniform(-1.0, 1.0, n).astype(F32)
    inf[n // 3] = np.inf
    inf[(n // 3 + 1) % n] = -np.inf if n > 1 else np.inf
    return {'all_equal': np.full(n, F32(-2.5)), 'signed_zeros': zeros, 'inf': inf}


FILL_KINDS = ('neg_zero', 'negatives', 'subnormal', 'last_positive', 'no_zero', 'nothing_positive')


def fill_case(n, kind):
    r = rng_of(33, n, FILL_KINDS.index(kind))
    x = r.uniform(0.5, 4.0, n).astype(F32)
    z = r.uniform(0, 1, n) < 0.3
    if kind == 'neg_zero':
        x[z] = 0.0
        x[::2] = np.where(x[::2] == 0, F32(-0.0), x[::2])
        x[0] = F32(-0.0) if n > 1 else x[0]
        if n > 1:
            x[-1] = 1.25
    elif kind == 'negatives':
        x[z] = 0.0
        x[r.uniform(0, 1, n) < 0.3] = -3.0
        if n > 2:
            x[0], x[1], x[2] = 0.0, -1.0, 0.75
    elif kind == 'subnormal':
        x[z] = 0.0
        x[n // 2] = F32(1e-40)
        x[0] = 0.0 if n > 1 else x[0]
    elif kind == 'last_positive':
        x[:] = np.where(z, F32(0.0), F32(-1.0))
        x[0] = 0.0 if n > 1 else x[0]
        x[-1] = 0.625
    elif kind == 'nothing_positive':
        x[:] = np.where(z, F32(0.0), F32(-2.0))
        x[0] = 0.0
    return x


def fill_reference(x):
    d = x.copy()
    pos = d[d > 0]
    if pos.size:
        d[d == 0] = pos.min()
    return d


MEAN_STD_RATIOS = (0.0, 1.0, 100.0, 1e4)


def mean_std_case(n, ratio):
    """sigma 0.5, mean = ratio * sigma"""
    return (rng_of(34, n, int(ratio)).standard_normal(n) * 0.5 + 0.5 * ratio).astype(F32)


def mean_std_bounds(x):
    """(m64, s64, bound on |mean - m64|, bound on |std - s64|): the kernel rounds the mean to float32 (<= 1/2 ulp, allowed 1) and
    centres the second pass on it, which adds delta^2 to the variance with delta <= ulp32(m) / 2: sqrt(s^2 + delta^2) - s <=
    delta^2 / (2 s) = ulp32(m)^2 / (8 s); the float32 rounding of the result is the other ulp"""
    m64, s64 = float(x.astype(F64).mean()), float(x.astype(F64).std())
    bs = ulp32(s64) + (ulp32(m64) ** 2 / (8.0 * s64) if s64 > 0 else 0.0)
    return m64, s64, ulp32(m64), bs


STATS_CASES = ['one', 'whole', 'large', 'ties', 'negative', 'edge']


def stats_case(name):
    """-> (plane [H, W], y0, x0, ch, cw).  'ties': the minimum and the maximum each occur several times, in the index ranges of
    different blocks (block b of 256 reads i = b * 256 + t + k * 65536); the first row-major occurrence is the answer"""
    r = rng_of(35, STATS_CASES.index(name))
    if name == 'one':
        H, W, y0, x0, ch, cw = 5, 7, 3, 4, 1, 1
    elif name == 'whole':
        H, W, y0, x0, ch, cw = 19, 23, 0, 0, 19, 23
    elif name == 'large':
        H, W, y0, x0, ch, cw = 262, 300, 1, 2, 260, 257                      # 66820 > 65536: the grid-stride loop turns
    elif name == 'ties':
        H, W, y0, x0, ch, cw = 70, 90, 2, 3, 64, 80                          # 5120 elements = 20 blocks' ranges
    elif name == 'negative':
        H, W, y0, x0, ch, cw = 33, 40, 4, 5, 20, 30
    else:
        H, W, y0, x0, ch, cw = 40, 50, 25, 33, 15, 17                        # touches the last row and the last column
    d = r.uniform(1.0, 2.0, (H, W)).astype(F32)
    if name == 'negative':
        d = r.uniform(-5.0, -1.0, (H, W)).astype(F32)
        d[y0 + 3, x0 + 4] = -0.5
    if name == 'ties':
        c = d[y0:y0 + ch, x0:x0 + cw]
        for i in (300, 1500, 4000):                                          # blocks 1, 5, 15
            c[i // cw, i % cw] = 0.25
        for i in (700, 2600, 5000):                                          # blocks 2, 10, 19
            c[i // cw, i % cw] = 9.0
    d[0, 0], d[-1, 0] = -100.0, 100.0                                        # outside every crop but 'whole'
    if name == 'whole':
        d[0, 0], d[-1, 0] = 1.5, 1.5
    if name == 'edge':
        d[H - 1, W - 1] = 0.125
        d[H - 1, x0] = 3.0
    return d, y0, x0, ch, cw


def stats_reference(d, y0, x0, ch, cw, mm_raw, scale):
    c = d[y0:y0 + ch, x0:x0 + cw]
    mn, mx = F32(mm_raw[0]), F32(mm_raw[1])
    return [float(F32(F32(mn / mx) * F32(scale))), float(F32(F32(mx / mx) * F32(scale))), float(c.min()), float(c.max()),
            float(np.argmin(c)), float(np.argmax(c))]


ADJUST_CASES = ['w1', 'w255', 'w256', 'w257', 'h1', 'h255', 'h257', 'one_row', 'half_even', 'half_odd', 'empty']


def adjust_case(name):
    """-> (disparity [H, W] >= 0, mask uint8 [H, W], (top, bottom) of the instance or None).  'half_even' / 'half_odd':
    top + 0.97 * (bottom - top) is exactly k + 0.5 in float64 (bottom - top = 50: 48.5) with k even / odd"""
    H, W = {'w1': (9, 1), 'w255': (6, 255), 'w256': (6, 256), 'w257': (6, 257), 'h1': (1, 40), 'h255': (255, 5), 'h257': (257, 5),
            'one_row': (12, 33), 'half_even': (70, 9), 'half_odd': (70, 9), 'empty': (8, 19)}[name]
    r = rng_of(36, ADJUST_CASES.index(name))
    disp = (r.uniform(0.5, 1.0, (H, W)) + 0.75 * (H - np.arange(H))[:, None]).astype(F32)    # row maxima fall with the row index
    mask = np.zeros((H, W), np.uint8)
    if name == 'one_row':
        top, bot = 7, 7
    elif name == 'half_even':
        top, bot = 0, 50                                                      # 48.5 -> 48
    elif name == 'half_odd':
        top, bot = 1, 51                                                      # 49.5 -> 50
    elif name == 'empty':
        top, bot = 2, 5
    else:
        top, bot = (0, H - 1) if H <= 9 else (3, H - 2)
    mask[top:bot + 1] = (r.uniform(0, 1, (bot + 1 - top, W)) < 0.6)
    mask[top:bot + 1, W // 2] = 1
    if name == 'empty':
        disp[mask != 0] = 0.0
        return disp, mask, None
    return disp, mask, (top, bot)


def adjust_reference(disp, mask):
    """kenburns_effect.py:68-78 for one mask (use_medium False), numpy"""
    adj = disp[None, None].copy()
    m = mask.astype(F32)[None, None]
    plane = adj * m
    if float(plane.sum()) == 0:
        return adj[0, 0]
    rows = np.nonzero((plane.sum(axis=3, keepdims=True) > 0.0).reshape(-1))[0]
    top, bottom = int(rows[0]), int(rows[-1])
    r0 = int(round(top + (0.97 * (bottom - top))))
    return (((F32(1.0) - m) * adj) + (m * plane[:, :, r0:, :].max()))[0, 0].astype(F32)


# =====================================================================================================================================
# 4. operations defined by aten
# =====================================================================================================================================
PLANES_PAIRS = [((1, 1), (5, 7)), ((5, 7), (1, 1)), ((2, 2), (255, 257)), ((23, 23), (45, 45)), ((301, 17), (77, 259)), ((9, 31), (9, 31))]


def planes_input(planes, hw, kind):
    H, W = hw
    if kind == 'noise':
        return rng_of(41, planes, H, W).standard_normal((planes, H, W)).astype(F32)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    p = np.arange(planes, dtype=F64)[:, None, None]
    return (np.sin(0.11 * y + 0.3 * p) * np.cos(0.07 * x - 0.2 * p) + 0.5 * p + 1.0).astype(F32)


def interp_bilinear(x, size, align, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None]
    return torch.nn.functional.interpolate(t, size=size, mode='bilinear', align_corners=bool(align))[0].numpy()


AREA_MASK_PAIRS = [((250, 310), (125, 155)), ((250, 310), (83, 31)), ((250, 310), (400, 512)), ((250, 310), (250, 310)),
                   ((250, 310), (1, 1)), ((7, 5), (3, 257)),
                   ((20, 15), (10, 3)), ((20, 15), (5, 3)), ((40, 9), (2, 3))]         # windows of 2x5, 4x5, 20x3: the planted 30 % ties
AREA_THR = 0.3


def _area_window(o, I, O):
    return (o * I) // O, -((-(o + 1) * I) // O)


def area_mask_case(n, hw, ohw):
    """random 0 / 1 masks (different densities per instance); where a window of 2x5, 4x5 or 20x3 input pixels exists in the geometry,
    one of each is planted with exactly 30 % of its pixels set.  -> (masks [n, H, W], list of planted (kh, kw, oy, ox))"""
    (H, W), (h, w) = hw, ohw
    r = rng_of(42, n, H, W, h, w)
    m = np.stack([(r.uniform(0, 1, (H, W)) < (0.3 if k == 0 else 0.7)).astype(np.uint8) for k in range(n)])
    wins = {}
    for oy in range(h):
        ys, ye = _area_window(oy, H, h)
        for ox in range(w):
            xs, xe = _area_window(ox, W, w)
            wins.setdefault((ye - ys, xe - xs), []).append((oy, ox, ys, xs))
    planted = []
    for k, (kh, kw) in enumerate(((2, 5), (4, 5), (20, 3))):
        if (kh, kw) in wins:
            lst = wins[(kh, kw)]
            oy, ox, ys, xs = lst[(len(lst) * (k + 1)) // 4]
            cnt = 3 * kh * kw // 10
            blk = np.zeros(kh * kw, np.uint8)
            blk[r.permutation(kh * kw)[:cnt]] = 1 + 254 * (k == 1)            # any non-zero byte counts as set
            m[0, ys:ys + kh, xs:xs + kw] = blk.reshape(kh, kw)
            planted.append((kh, kw, oy, ox))
    return m, planted


def area_mask_reference(m, ohw):
    """integer arithmetic: window [floor(o I / O), ceil((o + 1) I / O)), set iff 10 * count > 3 * kh * kw; at equality (exactly 30 %)
    the bit of the float32 sequence count / kh / kw > 0.3f.  -> (out [n, h, w], ties [n, h, w] bool)"""
    n, H, W = m.shape
    h, w = ohw
    S = np.zeros((n, H + 1, W + 1), np.int64)
    S[:, 1:, 1:] = np.cumsum(np.cumsum(m != 0, axis=1), axis=2)
    ys, ye = np.array([_area_window(o, H, h) for o in range(h)]).T
    xs, xe = np.array([_area_window(o, W, w) for o in range(w)]).T
    cnt = (S[:, ye][:, :, xe] - S[:, ys][:, :, xe] - S[:, ye][:, :, xs] + S[:, ys][:, :, xs])
    kh, kw = (ye - ys)[None, :, None], (xe - xs)[None, None, :]
    out = (10 * cnt > 3 * kh * kw)
    ties = (10 * cnt == 3 * kh * kw) & (cnt > 0)
    f = (cnt.astype(F32) / kh.astype(F32) / kw.astype(F32)) > F32(AREA_THR)
    return np.where(ties, f, out).astype(np.uint8), ties


# (B, H, W, pad_h, pad_w, nh, nw)
def _zoe_pad(n):
    return int(math.sqrt(n / 2) * 3)


ZOE_PREP_CASES = {
    'b2': (2, 33, 47, _zoe_pad(33), _zoe_pad(47), 32, 64),
    'pad0_same': (1, 12, 17, 0, 0, 12, 17),
    'pad0': (1, 12, 17, 0, 0, 32, 32),
    'pad_max': (1, 7, 9, 6, 8, 32, 32),
    'tiny': (1, 2, 2, 1, 1, 32, 32),
    'pipeline': (1, 96, 130, _zoe_pad(96), _zoe_pad(130), 128, 160),
    'nh1': (1, 33, 47, 3, 4, 1, 64),
    'padded_same': (1, 10, 12, 3, 2, 16, 16),
}


def zoe_image(B, H, W):
    return rng_of(43, B, H, W).uniform(0.0, 1.0, (B, 3, H, W)).astype(F32)


def zoe_prep_ref(img, pad_h, pad_w, flip, nh, nw, dtype):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(img)).to(dtype)
    if flip:
        x = x.flip(-1)
    x = torch.nn.functional.pad(x, (pad_w, pad_w, pad_h, pad_h), mode='reflect')
    x = torch.nn.functional.interpolate(x, size=(nh, nw), mode='bilinear', align_corners=True)
    return ((x - 0.5) / 0.5).numpy()


# (B, h, w, pad_h, pad_w, H, W)
ZOE_CROP_CASES = {
    'copy': (1, 14, 19, 2, 3, 10, 13),
    'up3_clamped': (1, 4, 5, 1, 1, 10, 13),
    'reduce': (1, 48, 64, 6, 7, 20, 25),
    'b2': (2, 16, 24, 5, 6, 33, 46),
    'pad0': (1, 8, 8, 0, 0, 21, 30),
}


def zoe_depth(B, h, w):
    y, x = np.mgrid[0:h, 0:w].astype(F64)
    b = np.arange(B, dtype=F64)[:, None, None]
    smooth = 3.0 + np.sin(0.4 * y + b) + np.cos(0.3 * x - b)
    return (smooth + 0.3 * rng_of(44, B, h, w).standard_normal((B, h, w)))[:, None].astype(F32)


def zoe_crop_ref(d, pad_h, pad_w, H, W, unflip, dtype):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(d)).to(dtype)
    x = torch.nn.functional.interpolate(x, size=(H + 2 * pad_h, W + 2 * pad_w), mode='bicubic', align_corners=False)
    x = x[:, :, pad_h:pad_h + H, pad_w:pad_w + W]
    if unflip:
        x = x.flip(-1)
    return np.ascontiguousarray(x.numpy())


# =====================================================================================================================================
# 5. single-rounding chains
# =====================================================================================================================================
CHAIN_LENGTHS = [1, 255, 256, 257]


def chain_input(n, *key):
    return rng_of(51, n, *key).uniform(0.05, 4.0, n).astype(F32)


def normalise_disparity_ref(x, mx, scale):
    return ((x / F32(mx)) * F32(scale)).astype(F32), F32(F32(mx) / F32(mx)) * F32(scale)


def normalise_ms_ref(x, mean, std):
    return ((x - F32(mean)) / (F32(std) + F32(0.0000001))).astype(F32)


def denormalise_input(n):
    """values that land exactly on 0 and on 1 with (mean, std) = (0.5, 0.25 - 1e-7 rounded) are hard to arrange for every std; the
    chain is evaluated with std + 1e-7 == 0.25 exactly (std = fl(0.25 - 1e-7)) and mean 0.5: x = -2 -> 0, x = 2 -> 1, x = -2 +- ulp,
    and mean -0.0 with x = -0.0 -> -0.0 for the clip and the threshold"""
    x = rng_of(52, n).uniform(-4.0, 4.0, n).astype(F32)
    special = np.array([-2.0, 2.0, np.nextafter(F32(-2.0), F32(0)), np.nextafter(F32(-2.0), F32(-3)), F32(2.000001), -0.0, 0.0],
                       F32)
    k = min(n, len(special))
    x[:k] = special[:k]
    return x


def denormalise_ms_ref(x, mean, std, mode):
    v = (x * (F32(std) + F32(0.0000001)) + F32(mean)).astype(F32)
    if mode == 1:
        v = np.minimum(np.maximum(v, F32(0.0)), F32(1.0))
    elif mode == 2:
        v = np.where(v > F32(0.0), v, F32(0.0)).astype(F32)
    return v


def bytes_image(hw):
    """[H * W, 3] image holding all 256 byte values in every channel (cyclic, a different phase per channel)"""
    i = np.arange(hw)
    return np.stack([(i * 1) % 256, (i * 3 + 85) % 256, (255 - i) % 256], -1).astype(np.uint8)


def u8_to_chw_ref(img):
    return (img.astype(F32) * F32(1.0 / 255.0)).astype(F32).transpose(2, 0, 1)


def bokeh_depth_ref(d8, dmax, focal, mn, mx2):
    v = F32(dmax) - np.abs(d8.astype(F32) - F32(focal))
    v = v - F32(mn)
    v = v / F32(mx2)
    v = F32(1.0) - v
    return (v * F32(0.0005)).astype(F32)


ZOE_DISP_SPECIAL = np.array([-1e-5, np.nan, np.inf, 0.0, 1e-40, -np.inf, 1e-5, 1e38, 3.4e38, -2e-5], F32)


def zoe_disp_input(n):
    x = rng_of(53, n).uniform(0.2, 30.0, n).astype(F32)
    k = min(n, len(ZOE_DISP_SPECIAL))
    x[:k] = ZOE_DISP_SPECIAL[:k]
    return x


def zoe_disp_ref(d, fb):
    with np.errstate(all='ignore'):
        v = ((F32(1.0) / (d + F32(0.00001))) * F32(fb)).astype(F32)
    return np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0).astype(F32)


COLORIZE_CASES = {'range': (0.5, 3.25), 'flat': (1.5, 1.5)}              # name -> (vmin, vmax)


def colorize_input(n, vmin, vmax):
    """values across [vmin, vmax] and 30 % of the span beyond it on both sides.  The first elements are, in this order: vmax itself
    (x * 256 == 256, which matplotlib maps to 255), vmin, the float32 neighbours of vmax below and above, a value so little below vmin
    that x * 256 lies in (-1, 0) and int() truncates it to 0, one far below vmin (clipped to -1: under), one far above vmax (clipped to
    256: over)"""
    vmin, vmax = F32(vmin), F32(vmax)
    span = max(float(vmax) - float(vmin), 1.0)
    x = rng_of(54, n, float(vmin), float(vmax)).uniform(float(vmin) - 0.3 * span, float(vmax) + 0.3 * span, n).astype(F32)
    special = np.array([vmax, vmin, np.nextafter(vmax, F32(-np.inf)), np.nextafter(vmax, F32(np.inf)), vmin - F32(span / 1024),
                        vmin - F32(100 * span), vmax + F32(100 * span)], F32)
    k = min(n, len(special))
    x[:k] = special[:k]
    return x


def colorize_ref(v, vmin, vmax):
    """colorize(value, cmap='gray_r')[..., 0] (zoedepth/utils/misc.py:97-135 + matplotlib Colormap.__call__) in numpy float32, in the
    written order: (v - vmin) / (vmax - vmin), or 0 where vmin == vmax; * 256; 256 -> 255; clip to [-1, 256]; int(); under -> 0,
    over -> 255; the gray_r table as bytes, uint8((1 - linspace(0, 1, 256)) * 255): truncated, so not 255 - k everywhere"""
    vmin, vmax = F32(vmin), F32(vmax)
    x = ((v - vmin) / (vmax - vmin)).astype(F32) if vmin != vmax else np.zeros(v.shape, F32)
    xa = (x * F32(256.0)).astype(F32)
    xa[xa == F32(256.0)] = F32(255.0)
    k = np.clip(xa, F32(-1.0), F32(256.0)).astype(np.int64)                # astype truncates toward zero, as int() does
    return ((1.0 - np.linspace(0.0, 1.0, 256)) * 255).astype(np.uint8)[np.clip(k, 0, 255)]


QUANT_CASES = ['noise', 'constant', 'two_valued', 'tiny_range', 'ramp']


def quant_case(name):
    """-> (d float32 [n], mn, mx)"""
    r = rng_of(54, QUANT_CASES.index(name))
    n = 257 * 9
    if name == 'noise':
        d = r.normal(0, 3, n).astype(F32)
    elif name == 'constant':
        d = np.full(n, F32(1.75))
    elif name == 'two_valued':
        d = np.where(r.uniform(0, 1, n) < 0.5, F32(-1.0), F32(2.5)).astype(F32)
    elif name == 'tiny_range':                                                # mx - mn = 1e-16 <= DBL_EPSILON: o = 0 everywhere
        d = np.where(r.uniform(0, 1, n) < 0.5, F32(0.0), F32(1e-16)).astype(F32)
    else:
        d = np.linspace(0.0, 11.0, n).astype(F32)
    return d, F32(d.min()), F32(d.max())


def _quant_tail(o):
    """the steps after `o`: uint16 truncation, * 255 / 65535, round half even, saturate, invert; float64"""
    u16 = np.floor(np.clip(o, 0.0, 65535.0))
    v = np.minimum(np.rint(np.abs(u16 * (255.0 / 65535.0))), 255.0)
    return (255.0 - v).astype(np.int64)


def quant_bracket(d, mn, mx):
    """-> (lo, hi): the output lies between the float64 evaluations of the tail at o64 (1 -+ 2^-20) (the map is decreasing)"""
    rngv = float(mx) - float(mn)
    if not rngv > 2.220446049250313e-16:
        o = np.zeros(d.shape, F64)
    else:
        o = 65535.0 * (d.astype(F64) - float(mn)) / rngv
    a, b = _quant_tail(o * (1.0 - 2.0 ** -20)), _quant_tail(o * (1.0 + 2.0 ** -20))
    return np.minimum(a, b), np.maximum(a, b)


POW_LIGHTNESS = (10.0, 2.5)


def pow_share(got_u8, ref_u8):
    d = np.abs(got_u8.astype(np.int64) - ref_u8.astype(np.int64))
    return float((d == 0).mean()), int(d.max())


def highlight_refs(img_u8, lf):
    """-> (ref64, e32): (img / 255) ^ lf; e32 = numpy's float32 power against float64, relative to max|ref|"""
    x32 = img_u8.astype(F32) / F32(255.0)
    ref = np.power(x32.astype(F64), float(F32(lf)))
    f32 = np.power(x32, F32(lf)).astype(F32)
    return ref, float(np.abs(f32 - ref).max() / np.abs(ref).max())


def finish_refs(a, b, lf):
    """-> (u8 of float64, u8 of numpy float32): uint8(((a + b) / 2) ^ (1 / lf) * 255); the sum and the halving are the float32 ones
    (single roundings of the written chain), the power is the step in question"""
    inv = F32(1.0 / float(lf))
    s = ((a + b) / F32(2.0)).astype(F32)
    u64 = np.floor(np.power(s.astype(F64), float(inv)) * 255.0).astype(np.uint8)
    u32 = (np.power(s, inv).astype(F32) * F32(255.0)).astype(np.uint8)
    return u64, u32


def bokeh_general_input(n, is_u8):
    r = rng_of(55, n, int(is_u8))
    return r.integers(0, 256, n, dtype=np.uint8) if is_u8 else r.uniform(0.5, 200.0, n).astype(F32)


def bokeh_general_refs(depth, focal, factor):
    """utils/effects.py:146-153, :162-163 -> (ref64, f32 numpy, e32 relative to 0.0005).  The float64 reference takes the float32
    d' (before the power) as its input: the steps before it are exact or single roundings shared by every evaluation"""
    d = depth.astype(F32)
    if focal is not None:
        d = (d.max() - np.abs(d - F32(focal))).astype(F32)
    f32 = d
    if factor == 2:
        f32 = d * d
    elif factor != 1:
        f32 = np.power(d, F32(factor)).astype(F32)
    t = f32 - f32.min()
    f32 = ((F32(1.0) - t / t.max()) * F32(0.0005)).astype(F32)
    p = np.power(d.astype(F64), float(factor)) if factor != 1 else d.astype(F64)
    p = p - p.min()
    ref = (1.0 - p / p.max()) * 0.0005
    return ref, f32, float(np.abs(f32 - ref).max() / 0.0005)


# =====================================================================================================================================
# 6. bokeh pass
# =====================================================================================================================================
BOKEH_TX, BOKEH_TY = 32, 8
# (name, H, W, nsamples, depth scale, zero region)
BOKEH_CASES = [('5x7', 5, 7, 32, 0.0005, False), ('8x32', 8, 32, 32, 0.0005, False), ('9x33', 9, 33, 32, 0.0005, False),
               ('50x70', 50, 70, 32, 0.0005, False), ('r9', 96, 128, 32, 0.0005, False), ('r16', 96, 128, 512, 0.0005, False),
               ('r20', 96, 128, 700, 0.0005, False), ('far_interior', 96, 128, 32, 0.01, False), ('far_border', 70, 70, 32, 0.01, False),
               ('zero_region', 96, 128, 32, 0.0005, True)]
BOKEH_DIRS = [(0.0, 1.0), (math.cos(-math.pi / 6), math.sin(-math.pi / 6)), (math.cos(-math.pi * 5 / 6), math.sin(-math.pi * 5 / 6))]


def bokeh_dirs(name):
    """the three directions of bokeh_blur; the 512- and 700-sample cases take the diagonal only (both axes move), to stay quick"""
    return BOKEH_DIRS[1:2] if name in ('r16', 'r20') else BOKEH_DIRS


def bokeh_template(H, W, nsamples):
    """the launch rule of bokeh_pass_launch -> R of the template"""
    reach = int(0.0005 * float((nsamples + 1) // 2) * float(min(H, W)) + 0.5) + 1
    return 9 if reach <= 9 else (16 if reach <= 16 else 20)


def bokeh_interior_blocks(H, W, R):
    """bool [blocks_y, blocks_x]: the staged window (tile + R halo) lies inside the image"""
    by = np.arange(-(-H // BOKEH_TY)) * BOKEH_TY
    bx = np.arange(-(-W // BOKEH_TX)) * BOKEH_TX
    return ((by - R >= 0) & (by + BOKEH_TY + R <= H))[:, None] & ((bx - R >= 0) & (bx + BOKEH_TX + R <= W))[None, :]


def bokeh_case(name):
    _, H, W, ns, scale, zero = [c for c in BOKEH_CASES if c[0] == name][0]
    r = rng_of(61, H, W, ns)
    img = r.uniform(0.0, 1.0, (H, W, 3)).astype(F32)
    depth = (r.uniform(0.05, 1.0, (H, W)) * scale).astype(F32)
    if zero:
        depth[10:60, 20:100] = 0.0
    return img, depth, ns


def bokeh_offsets(depth, ns, dx, dy):
    """sample offsets as the reference text defines them: float32 products, roundf (half away from zero) -> (ox, oy) int [H, W, ns]"""
    H, W = depth.shape
    sp = ((np.arange(ns) - ns // 2) * min(H, W)).astype(F32)

    def roundf(v):
        return (np.sign(v) * np.floor(np.abs(v).astype(F64) + 0.5)).astype(np.int64)
    ddx, ddy = (F32(dx) * depth).astype(F32), (F32(dy) * depth).astype(F32)
    return roundf((ddx[..., None] * sp).astype(F32)), roundf((ddy[..., None] * sp).astype(F32))


def bokeh_pass_ref(img, depth, ns, dx, dy, dtype=F64):
    """kernel_bokeh with the float32 sample positions and the accumulation in `dtype` (sequential over the samples)"""
    H, W = depth.shape
    ox, oy = bokeh_offsets(depth, ns, dx, dy)
    yy, xx = np.mgrid[0:H, 0:W]
    weight = np.zeros((H, W), dtype)
    color = np.zeros((H, W, 3), dtype)
    im, dp = img.astype(dtype), depth.astype(dtype)
    for s in range(ns):
        x_, y_ = xx + ox[..., s], yy + oy[..., s]
        ok = (x_ < W) & (y_ < H) & (x_ >= 0) & (y_ >= 0)
        xc, yc = np.clip(x_, 0, W - 1), np.clip(y_, 0, H - 1)
        w_ = np.where(ok, dp[yc, xc], dtype(0))
        weight = weight + w_
        color = color + im[yc, xc] * w_[..., None]
    nz = weight != 0
    out = np.where(nz[..., None], color / np.where(nz, weight, dtype(1))[..., None], im)
    return out.astype(dtype)


def bokeh_leaves_window(depth, ns, dx, dy, R):
    """number of in-image samples whose offset exceeds the halo R in either axis"""
    H, W = depth.shape
    ox, oy = bokeh_offsets(depth, ns, dx, dy)
    yy, xx = np.mgrid[0:H, 0:W]
    x_, y_ = xx[..., None] + ox, yy[..., None] + oy
    ok = (x_ < W) & (y_ < H) & (x_ >= 0) & (y_ >= 0)
    return int((ok & ((np.abs(ox) > R) | (np.abs(oy) > R))).sum())
