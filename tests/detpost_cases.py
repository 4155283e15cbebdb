"""Case generators and plain references for the detector post-processing kernels (csrc/maskhead.hip, csrc/detdecode.hip):
csm_nms, csm_mask_resize_threshold, csm_maskhead_logits, csm_det_preprocess, csm_pack_mask_bits and the decode -> NMS -> gather chain.

The references are float64 numpy / CPU torch and use nothing from the library or the oracle.  tests/test_detpost_references.py holds the
oracle (oracle/segment.py) against them on a machine without a GPU and asserts that every case has the property it exists for;
tests/test_gpu_detpost.py holds the HIP kernels against the same references and against the oracle.  All generators are seeded.
"""
import numpy as np

# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
# Exact inputs: integer coordinates in [0, 1024), widths / heights in [0, 64], integer class offsets label * (max + 1) <= 2 * 1024 and
# thr in {1/2, 5/8}.  Then coordinates + offsets < 2^12, areas and intersections <= 2^12, sa + sb - inter < 2^13, and thr times that has
# at most 13 + 3 significant bits: every sum and product is exact in fp32 as in float64, so both take the same decision on every pair.
NMS_SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 1000, 2400, 4096)
NMS_THRS = (0.5, 0.625)
NMS_CLASSES = 3
BAND_Y = 900          # clusters live in y < 880, the planted boxes in y >= BAND_Y: a plant meets nothing but its own partners


def nms_max_keeps(n):
    return (1, 7, 100, n + 5)


def nms_reference(boxes, offsets, thr, max_keep, dtype=np.float64):
    """greedy NMS in score order (= index order): j > i is suppressed by a kept i iff inter > thr * (sa + sb - inter), box width
    x2 - x1; stops after max_keep keeps.  dtype=np.float32 evaluates the same expression, operation by operation, in fp32."""
    b = np.asarray(boxes, dtype).reshape(-1, 4)
    if offsets is not None:
        b = b + np.asarray(offsets, dtype)[:, None]
    thr = dtype(thr)
    n = len(b)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(n, bool)
    keep = []
    zero = dtype(0)
    for i in range(n):
        if len(keep) >= max_keep:
            break
        if dead[i]:
            continue
        keep.append(i)
        r = b[i + 1:]
        iw = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]), zero)
        ih = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]), zero)
        inter = iw * ih
        dead[i + 1:] |= inter > thr * (area[i] + area[i + 1:] - inter)
    return np.asarray(keep, np.int32)


def nms_pair_matrix(boxes, offsets, thr):
    """float64 [n, n] bool: entry (i, j) iff j > i and box i would suppress box j -- the bitmap k_nms_mask hands to the scan"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    if offsets is not None:
        b = b + np.asarray(offsets, np.float64)[:, None]
    n = len(b)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    out = np.zeros((n, n), bool)
    for i0 in range(0, n, 512):
        a = b[i0:i0 + 512, None, :]
        iw = np.maximum(np.minimum(a[..., 2], b[None, :, 2]) - np.maximum(a[..., 0], b[None, :, 0]), 0.0)
        ih = np.maximum(np.minimum(a[..., 3], b[None, :, 3]) - np.maximum(a[..., 1], b[None, :, 1]), 0.0)
        inter = iw * ih
        out[i0:i0 + 512] = inter > thr * (area[i0:i0 + 512, None] + area[None, :] - inter)
    return np.triu(out, 1)


def nms_suppresses(a, b, thr):
    """the pair test alone, in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    return inter > thr * ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _band(x, w, h, y=BAND_Y):
    return [x, y, x + w, y + h]


def nms_case(n, with_classes, seed=0):
    """one box list of n boxes in score order.  Returns dict(boxes f32 [n,4], labels i32 [n], offsets f32 [n] or None, plants=...):

    (a) clusters   5..40 boxes jittered by +-1 px around a random 40..62 px box, members spread over the whole list by a permutation
    (b) chain      A, B, C (same label) with A > B, B > C, A !> C at both thresholds, at indices in three different 64-bit words
    (c) exact      a pair whose IoU is exactly thr (kept: the test is a strict >) and a pair that is over it by the smallest amount the
                   integer grid allows, for each thr; the 0.5 pair sits on boxes 63 / 64 where the list has them
    (d) twins      two identical boxes with labels 0 and 2
    (e) tail       from n >= 1000 the last third are zero boxes with label 0 (what csm_det_decode writes into slots without a candidate)
    plants maps a name to the indices it occupies; a plant is present iff the list is long enough for its indices."""
    rng = np.random.default_rng(1000 * n + 17 * seed + (1 if with_classes else 0))
    boxes = np.zeros((n, 4), np.int64)
    labels = rng.integers(0, NMS_CLASSES, n).astype(np.int32)
    live = n - n // 3 if n >= 1000 else n
    plants = {}
    if n == 2:                                                       # the exact-threshold pair on its own
        wanted = [('exact_0.5', (0, 1), [_band(100, 2, 2), _band(100, 2, 1)], (1, 1))]
    else:
        c = min(200, live - 1)
        wanted = [
            ('chain', (3, 70, c), [_band(0, 40, 40), _band(8, 40, 40), _band(16, 40, 40)], (1, 1, 1)),
            ('exact_0.5', (63, 64) if live > 64 else (live - 2, live - 1), [_band(100, 2, 2, 950), _band(100, 2, 1, 950)], (1, 1)),
            ('above_0.5', (5, 66), [_band(200, 63, 1, 950), _band(200, 32, 1, 950)], (2, 2)),
            ('exact_0.625', (10, 127), [_band(300, 8, 1, 950), _band(300, 5, 1, 950)], (0, 0)),
            ('above_0.625', (11, 128), [_band(400, 3, 1, 950), _band(400, 2, 1, 950)], (0, 0)),
            ('twins', (20, 90), [_band(500, 40, 40), _band(500, 40, 40)], (0, 2)),
        ]
    taken = set()
    for name, idx, bx, lab in wanted:
        if min(idx) < 0 or max(idx) >= live or len(set(idx)) < len(idx) or taken & set(idx):
            continue
        if name == 'chain' and len({i // 64 for i in idx}) < 3:
            continue
        for i, b, l in zip(idx, bx, lab):
            boxes[i], labels[i] = b, l
        taken |= set(idx)
        plants[name] = tuple(idx)
    free = np.array([i for i in range(live) if i not in taken], np.int64)
    free = free[rng.permutation(len(free))]
    k = 0
    while k < len(free):
        size = min(int(rng.integers(5, 41)), len(free) - k)
        w, h = rng.integers(40, 63, 2)
        x, y = int(rng.integers(1, 1022 - 64)), int(rng.integers(1, 880 - 66))
        j = rng.integers(-1, 2, (size, 4))
        boxes[free[k:k + size]] = np.array([x, y, x + w, y + h]) + j
        k += size
    if live < n:
        labels[live:] = 0
        plants['tail'] = (live, n)
    if n:
        assert boxes.min() >= 0 and boxes.max() < 1024
        assert (boxes[:, 2:] - boxes[:, :2]).min() >= 0 and (boxes[:, 2:] - boxes[:, :2]).max() <= 64
    bf = boxes.astype(np.float32)
    offsets = None
    if with_classes:
        offsets = (labels.astype(np.float32) * (np.float32(bf.max() if n else 0) + np.float32(1))).astype(np.float32)
    return dict(n=n, boxes=bf, labels=labels, offsets=offsets, plants=plants, live=live)


# ---- mask resize + threshold -----------------------------------------------------------------------------------------------------
MASK_UP = 8
MASK_EPS = 1e-4                 # a pixel is compared iff its float64 probability is further than this from thr
MASK_EXCLUDED_CAP = 0.005       # a condition the inputs meet (measured share: DESIGN.md §6.1), not a tolerance
# (h, w, rh, rw, oh, ow, thr, n)
MASK_CASES = (
    (5, 7, 37, 61, 37, 61, 0.5, 3),
    (8, 8, 64, 64, 64, 64, 0.5, 3),              # the second resize is the identity
    (9, 6, 100, 33, 98, 33, 0.5, 3),
    (4, 4, 131, 77, 130, 75, 0.5, 3),
    (16, 12, 129, 257, 128, 256, 0.5, 3),
    (3, 5, 24, 40, 24, 40, 0.5, 3),
    (1, 1, 9, 5, 9, 5, 0.5, 3),
    (6, 10, 47, 81, 47, 79, 0.5, 3),
    (2, 33, 9, 1030, 9, 1026, 0.5, 3),           # ow > 1024: a second block along x; ow % 4 == 2
    (7, 5, 50, 50, 50, 38, 0.5, 3),              # the box-prompt call form: rh = rw = max(H, W), (oh, ow) = (H, W) = (50, 38)
    (4, 4, 131, 77, 130, 75, 0.3, 3),            # thr 0.3 on two of the shapes
    (6, 10, 47, 81, 47, 79, 0.3, 3),
    (5, 7, 37, 61, 37, 61, 0.5, 0),              # n = 0
)


def mask_logits(case, seed=0):
    h, w, n = case[0], case[1], case[7]
    return np.random.default_rng(7919 * (seed + 1) + 31 * h + w).normal(0.0, 2.0, (n, h, w)).astype(np.float32)


def mask_reference_prob(logits, up, rh, rw, oh, ow):
    """float64 probabilities [n, oh, ow] by torch's own two bilinear resamplings (mmdet _bbox_mask_post_process)"""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.asarray(logits, np.float64))[None]
    x = F.interpolate(x, scale_factor=up, mode='bilinear')
    x = F.interpolate(x, size=(rh, rw), mode='bilinear')
    return x[0, :, :oh, :ow].sigmoid().numpy()


# ---- dynamic-conv mask head --------------------------------------------------------------------------------------------------------
MASKHEAD_LDS = (8, 24, 40)
MASKHEAD_HW = ((1, 1), (15, 17), (16, 16), (1, 257), (20, 33))      # h*w = 1, 255, 256, 257, 660
MASKHEAD_NS = (0, 1, 5)
MASKHEAD_FEAT_STRIDE = 8


def maskhead_case(ld, hw, n, seed=0):
    """wide [h, w, ld] random buffer whose channels c0 .. c0+7 are the prototypes, kernels [n, 169], priors [n, 4] with strides 8/16/32"""
    h, w = hw
    rng = np.random.default_rng(100003 * (seed + 1) + 1000 * ld + 10 * h * w + n)
    wide = rng.normal(0.0, 1.0, (h, w, ld)).astype(np.float32)
    c0 = (ld - 8) // 2
    kernels = rng.normal(0.0, 0.4, (n, 169)).astype(np.float32)
    st = np.array([8, 16, 32, 8, 32, 16, 8][:n], np.float32)
    priors = np.zeros((n, 4), np.float32)
    if n:
        priors[:, 0] = rng.integers(0, 12, n) * st
        priors[:, 1] = rng.integers(0, 12, n) * st
        priors[:, 2] = priors[:, 3] = st
    return dict(wide=wide, c0=c0, kernels=kernels, priors=priors, h=h, w=w, ld=ld, n=n)


def maskhead_reference(feat, kernels, priors, feat_stride):
    """float64 statement of RTMDetInsHead's dynamic conv (rtmdet_inshead_custom.py:253-303, parse_dynamic_params 80/64/8 | 8/8/1):
    x = [rel_x, rel_y, feat(8)] -> 10->8 relu -> 8->8 relu -> 8->1.  feat [h, w, 8]"""
    feat, kernels, priors = (np.asarray(a, np.float64) for a in (feat, kernels, priors))
    h, w, _ = feat.shape
    out = np.zeros((len(priors), h, w))
    ys, xs = np.meshgrid(np.arange(h) * float(feat_stride), np.arange(w) * float(feat_stride), indexing='ij')
    for i, (k, p) in enumerate(zip(kernels, priors)):
        w0, w1, w2 = k[:80].reshape(8, 10), k[80:144].reshape(8, 8), k[144:152].reshape(1, 8)
        b0, b1, b2 = k[152:160], k[160:168], k[168:169]
        x = np.concatenate([((p[0] - xs) / (p[2] * 8.0))[..., None], ((p[1] - ys) / (p[2] * 8.0))[..., None], feat], -1)
        x = np.maximum(x @ w0.T + b0, 0.0)
        x = np.maximum(x @ w1.T + b1, 0.0)
        out[i] = (x @ w2.T + b2)[..., 0]
    return out


def maskhead_rel_err(got, ref):
    """largest absolute error over the largest |reference logit| of the case (element-wise ratios are meaningless at a logit near 0)"""
    if ref.size == 0:
        return 0.0
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ---- detector preprocess -----------------------------------------------------------------------------------------------------------
class DetNorm:
    mean = (103.53, 116.28, 123.675)
    std = (57.375, 57.12, 58.395)
    pad_value = 114.0


def _checker(H, W, cell):
    yy, xx = np.mgrid[:H, :W]
    return np.repeat((((yy // cell + xx // cell) & 1) * 255).astype(np.uint8)[..., None], 3, 2)


def preprocess_cases():
    """(name, img u8 [H,W,3], rh, rw, S_h, S_w)"""
    rng = np.random.default_rng(4242)
    rnd = lambda H, W: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)                                                   # noqa: E731
    return [
        ('down_rh_short', rnd(100, 150), 43, 64, 64, 64),               # rh < S_h, rw == S_w
        ('down_rw_short', rnd(150, 100), 64, 43, 64, 64),               # rw < S_w, rh == S_h
        ('up_257', rnd(20, 30), 171, 257, 200, 257),                    # up-scaling, S_h != S_w, a second block along x
        ('copy', rnd(64, 64), 64, 64, 64, 64),                          # rh == H, rw == W: the copy branch, no padding
        ('copy_pad', rnd(40, 50), 40, 50, 64, 64),                      # the copy branch with padding on both sides
        ('wide_1024', rnd(30, 500), 61, 1024, 64, 1024),
        ('down_1024', rnd(700, 1300), 551, 1024, 600, 1024),
        ('one_pixel', rnd(1, 1), 1, 1, 64, 64),
        ('one_pixel_up', rnd(1, 1), 5, 7, 8, 64),
        ('checker_down', _checker(33, 47, 1), 21, 30, 32, 64),
        ('checker_up', _checker(33, 47, 1), 90, 128, 96, 257),
        ('checker2_down', _checker(64, 64, 2), 37, 37, 64, 64),
    ]


def preprocess_reference(img, rh, rw, S_h, S_w, norm=DetNorm):
    """float64: bilinear at cv2's half-pixel centres with clamped edges, rounded to a grey level, (v - mean) / std, pad outside
    (rh, rw).  [1, 3, S_h, S_w]"""
    H, W = img.shape[:2]
    f = img.astype(np.float64)

    def taps(n_out, n_in):
        s = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        i0 = np.floor(s)
        fr = s - i0
        fr[(i0 < 0) | (i0 >= n_in - 1)] = 0.0
        i0 = np.clip(i0, 0, n_in - 1).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_in - 1), fr
    if (rh, rw) == (H, W):
        g = f
    else:
        y0, y1, fy = taps(rh, H)
        x0, x1, fx = taps(rw, W)
        fy, fx = fy[:, None, None], fx[None, :, None]
        top = f[y0][:, x0] * (1 - fx) + f[y0][:, x1] * fx
        bot = f[y1][:, x0] * (1 - fx) + f[y1][:, x1] * fx
        g = np.rint(top * (1 - fy) + bot * fy)
    out = np.full((S_h, S_w, 3), float(norm.pad_value))
    out[:rh, :rw] = g
    out = (out - np.asarray(norm.mean, np.float64)) / np.asarray(norm.std, np.float64)
    return np.ascontiguousarray(out.transpose(2, 0, 1))[None]


def preprocess_bound(norm=DetNorm):
    """one grey level after normalisation, per channel [3,1,1]; plus 1e-6 for the fp32 rounding of (v - mean) / std (|value| < 2.7, so
    an fp32 ulp is 2.4e-7 and the subtraction and the division round once each)"""
    return (1.0 / np.asarray(norm.std, np.float64) + 1e-6)[:, None, None]


# ---- bit packing -------------------------------------------------------------------------------------------------------------------
PACK_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 100003)
PACK_VALUES = np.array([0, 1, 2, 128, 255], np.uint8)


def pack_case(n, seed=0):
    return PACK_VALUES[np.random.default_rng(13 * n + seed).integers(0, len(PACK_VALUES), n)]


def pack_reference(m):
    return np.packbits(m != 0, bitorder='little')


# ---- decode -> NMS -> gather ---------------------------------------------------------------------------------------------------------
def decode_reference(cls, reg, hw, strides, nc, nms_pre, thr, clamp_w, clamp_h, sx, sy, min_box):
    """numpy statement of mmdet's filter_scores_and_topk -> distance2bbox -> rescale -> min_bbox_size filter -> score sort [EXT] for
    one image.  cls[l] [h, w, nc], reg[l] [h, w, 4] per level.  Returns scores, boxes, global prior index, label of the candidates in
    NMS order (stable: score descending, then prior * nc + class ascending, then level)."""
    sx, sy = np.float32(sx), np.float32(sy)
    sc_l, box_l, src_l, lab_l = [], [], [], []
    prior0 = 0
    for l, ((h, w), s) in enumerate(zip(hw, strides)):
        flat = cls[l].reshape(-1)
        idx = np.nonzero(flat > np.float32(thr))[0]
        order = np.argsort(-flat[idx], kind='stable')[:nms_pre]
        idx = idx[order]
        p, lab = idx // nc, idx % nc
        px, py = ((p % w) * s).astype(np.float32), ((p // w) * s).astype(np.float32)
        dist = reg[l].reshape(-1, 4)[p] * np.float32(s)
        x1 = np.clip(px - dist[:, 0], 0, np.float32(clamp_w)) * sx; y1 = np.clip(py - dist[:, 1], 0, np.float32(clamp_h)) * sy
        x2 = np.clip(px + dist[:, 2], 0, np.float32(clamp_w)) * sx; y2 = np.clip(py + dist[:, 3], 0, np.float32(clamp_h)) * sy
        sc_l.append(flat[idx]); box_l.append(np.stack([x1, y1, x2, y2], 1).astype(np.float32)); src_l.append(prior0 + p); lab_l.append(lab)
        prior0 += h * w
    sc, bx, sr, lb = np.concatenate(sc_l), np.concatenate(box_l), np.concatenate(src_l), np.concatenate(lab_l)
    ok = ((bx[:, 2] - bx[:, 0]) > np.float32(min_box)) & ((bx[:, 3] - bx[:, 1]) > np.float32(min_box))
    n_before = len(sc)
    sc, bx, sr, lb = sc[ok], bx[ok], sr[ok], lb[ok]
    order = np.argsort(-sc, kind='stable')
    return sc[order], bx[order], sr[order], lb[order], n_before


CHAIN_HW = ((80, 80), (40, 40), (20, 20))
CHAIN_STRIDES = (8, 16, 32)
CHAIN = dict(nms_pre=1000, score_thr=0.3, iou=0.6, max_keep=100, det=640.0, scale=1.6, min_box=0.0, G=169)


def chain_case(nc, seed=0):
    """random head maps of the shipped detector (det 640: 80x80, 40x40, 20x20).  A dozen objects; a prior inside an object regresses
    that object's box +-3 px and scores above the threshold, a prior outside every object scores below it: the candidates are
    heavily overlapping clusters, level 2 has fewer candidates than slots (trailing score -1 slots with zero boxes), level 0 more than
    nms_pre."""
    rng = np.random.default_rng(555 + 10 * nc + seed)
    n_obj, det = 12, CHAIN['det']
    ow, oh = rng.uniform(100, 200, n_obj), rng.uniform(100, 200, n_obj)
    ox, oy = rng.uniform(0, det - ow), rng.uniform(0, det - oh)
    cls, reg, kern = [], [], []
    for (h, w), s in zip(CHAIN_HW, CHAIN_STRIDES):
        ys, xs = np.meshgrid(np.arange(h) * float(s), np.arange(w) * float(s), indexing='ij')
        inside = (xs[..., None] > ox + 4) & (xs[..., None] < ox + ow - 4) & (ys[..., None] > oy + 4) & (ys[..., None] < oy + oh - 4)   # [h,w,n_obj]
        pick = np.argmax(inside * rng.uniform(0.1, 1.0, inside.shape), -1)                                   # a random containing object
        has = inside.any(-1)
        jit = rng.uniform(-3.0, 3.0, (h, w, 4))
        d = np.stack([xs - ox[pick], ys - oy[pick], ox[pick] + ow[pick] - xs, oy[pick] + oh[pick] - ys], -1) + jit
        d = np.where(has[..., None], d, rng.uniform(0.0, 2.0 * s, (h, w, 4)))
        reg.append((np.maximum(d, 0.0) / s).astype(np.float32))
        sc = np.where(has[..., None], rng.uniform(0.35, 0.99, (h, w, nc)), rng.uniform(0.01, 0.25, (h, w, nc)))
        cls.append(sc.astype(np.float32))
        kern.append(rng.normal(0, 1, (h, w, CHAIN['G'])).astype(np.float32))
    return dict(cls=cls, reg=reg, kern=kern, nc=nc)
