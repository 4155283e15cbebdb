"""The files of the lossless WebP decoder's tests, generated at test time and cached per process.

    NAMES / ACCEPTED       the files the decoder takes: most written by Pillow (libwebp's encoder) at several methods and qualities,
                           a few by the hand writer below for what libwebp does not emit
    case_file(name)        the bytes of one
    reference(name)        imread's pixels of one: uint8 B, G, R [H,W,3]
    reference_bgra(name)   PIL's RGBA of one as B, G, R, A
    REFUSED                {name: (build, a word of the reason)} of files webpread.probe refuses
    write_vp8l(..)         the hand writer

Every side stays at or below 320; PREDICT_BAND_ROWS names what the inverse-predictor kernel bands by."""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import webpdec_restatement as R  # noqa: E402
import webpll_restatement as L  # noqa: E402

PREDICT_BAND_ROWS = 256          # csrc/webpdec.hip kBandRows: k_wd_predict takes the rows of a file in bands of this many
GROUP_CAP = 2600


# ---- pictures -----------------------------------------------------------------------------------------------------------------
def cartoon(H, W, seed, channels=3):
    """a gradient, six flat discs and one noisy quadrant: uint8 [H,W,channels] (R, G, B (, A))"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 255) // max(1, W - 1), (y * 255) // max(1, H - 1), ((x + y) * 255) // max(1, H + W - 2)], axis=2).astype(np.uint8)
    for _ in range(6):
        cy, cx, rad = rng.integers(0, H), rng.integers(0, W), rng.integers(2, max(3, min(H, W) // 3 + 3))
        img[(y - cy) ** 2 + (x - cx) ** 2 < rad * rad] = rng.integers(0, 256, 3)
    img[:H // 2, W // 2:] = rng.integers(0, 256, (H // 2, W - W // 2, 3))
    if channels == 4:
        a = np.clip(255 - ((y - H / 2) ** 2 + (x - W / 2) ** 2) * 600 // max(1, H * W), 0, 255).astype(np.uint8)
        img = np.concatenate([img, a[:, :, None]], axis=2)
    return img


def indexed(H, W, colours, seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (colours, 3)).astype(np.uint8)
    return pal[rng.integers(0, colours, (H, W))]


def photo(H, W, seed):
    rng = np.random.default_rng(seed)
    walk = np.cumsum(np.cumsum(rng.integers(-3, 4, (H, W, 3)), axis=0), axis=1) // 8
    return (walk % 256).astype(np.uint8)


def pil_webp(img, method, quality, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, 'WEBP', lossless=True, method=method, quality=quality, exact=True, **kw)
    return b.getvalue()


# ---- the hand writer ------------------------------------------------------------------------------------------------------------
def _write_code(w, hist):
    """webpll_restatement.write_code, with a second used symbol where a simple code cannot name the only one"""
    hist = list(hist)
    used = [s for s, c in enumerate(hist) if c]
    if len(used) == 1 and used[0] > 255:
        hist[0] = 1
    return L.write_code(w, hist)


def _write_image(w, px, xs, ys, cache_bits=0, meta=None, meta_bits=0, main=False):
    """one entropy-coded image of literals and colour-cache hits; meta: the group of every block (a list, row by row)"""
    w.number(1 if cache_bits else 0, 1)
    if cache_bits:
        w.number(cache_bits, 4)
    ngroups = 1
    if main:
        w.number(1 if meta is not None else 0, 1)
        if meta is not None:
            w.number(meta_bits - 2, 3)
            _write_image(w, [0xff000000 | g << 8 for g in meta], R.subsample(xs, meta_bits), R.subsample(ys, meta_bits))
            ngroups = max(meta) + 1
    mw = R.subsample(xs, meta_bits) if meta is not None else 0
    cache = [0] * (1 << cache_bits) if cache_bits else None
    tokens = []
    hists = [[[0] * n for n in (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)] for _ in range(ngroups)]
    for i, v in enumerate(px):
        g = meta[((i // xs) >> meta_bits) * mw + ((i % xs) >> meta_bits)] if meta is not None else 0
        key = (0x1e35a7bd * v & 0xffffffff) >> (32 - cache_bits) if cache_bits else 0
        if cache is not None and cache[key] == v and i > 0:
            tokens.append((g, 280 + key, None))
            hists[g][0][280 + key] += 1
        else:
            tokens.append((g, None, v))
            for a, s in enumerate((v >> 8 & 255, v >> 16 & 255, v & 255, v >> 24)):
                hists[g][a][s] += 1
        if cache is not None:
            cache[key] = v
    codes = [[_write_code(w, h) for h in hg] for hg in hists]
    for g, hit, v in tokens:
        c = codes[g]
        if hit is not None:
            w.huffman(c[0][1][hit], c[0][0][hit])
        else:
            for a, s in enumerate((v >> 8 & 255, v >> 16 & 255, v & 255, v >> 24)):
                w.huffman(c[a][1][s], c[a][0][s])


def write_vp8l(argb, transforms=(), cache_bits=0, meta_bits=0, groups=1, has_alpha=True):
    """A .webp file of the uint32 ARGB image `argb` [H,W].  transforms: a sequence of (0, bits) predictor with mode (bx + 3 by) % 14
    in block (bx, by), (1, bits) cross-colour with multipliers that vary by block, (2,) subtract-green, (3,) colour indexing
    (at most 256 colours).  meta_bits: 0 = one group; otherwise block (bx, by) of 1 << meta_bits pixels takes group
    (bx + by * blocks per row) % groups."""
    H, W = argb.shape
    w = L.BitWriter()
    w.number(0x2f, 8); w.number(W - 1, 14); w.number(H - 1, 14); w.number(int(has_alpha), 1); w.number(0, 3)
    px = [int(v) for v in argb.reshape(-1)]
    xs = W
    for tr in transforms:
        t = tr[0]
        w.number(1, 1); w.number(t, 2)
        if t == 2:
            px = [(v & 0xff00ff00) | ((v & 0x00ff00ff) - ((v >> 8 & 255) * 0x00010001) + 0x01000100) & 0x00ff00ff for v in px]
        elif t == 0:
            bits = tr[1]
            bw, bh = R.subsample(xs, bits), R.subsample(H, bits)
            modes = [(bx + 3 * by) % 14 for by in range(bh) for bx in range(bw)]
            c = [R.ch(v) for v in px]
            res = []
            for y in range(H):
                for x in range(xs):
                    if y == 0:
                        p = [255, 0, 0, 0] if x == 0 else c[x - 1]
                    elif x == 0:
                        p = c[(y - 1) * xs]
                    else:
                        TR = c[(y - 1) * xs + x + 1] if x + 1 < xs else c[y * xs]
                        p = R.predict(modes[(y >> bits) * bw + (x >> bits)], c[y * xs + x - 1], c[(y - 1) * xs + x], c[(y - 1) * xs + x - 1], TR)
                    res.append(R.unch([(a - b) & 255 for a, b in zip(c[y * xs + x], p)]))
            px = res
            w.number(bits - 2, 3)
            _write_image(w, [0xff000000 | m << 8 for m in modes], bw, bh)
        elif t == 1:
            bits = tr[1]
            bw, bh = R.subsample(xs, bits), R.subsample(H, bits)
            data = [0xff000000 | ((7 * bx + 200) & 255) << 16 | ((11 * by + 3) & 255) << 8 | ((5 * (bx + by) + 250) & 255) for by in range(bh) for bx in range(bw)]
            out = []
            for i, v in enumerate(px):
                m = data[((i // xs) >> bits) * bw + ((i % xs) >> bits)]
                a, r, g, b = R.ch(v)
                nr = (r - ((R.s8(m & 255) * R.s8(g)) >> 5)) & 255
                nb = (b - ((R.s8(m >> 8 & 255) * R.s8(g)) >> 5) - ((R.s8(m >> 16 & 255) * R.s8(r)) >> 5)) & 255
                out.append(R.unch([a, nr, g, nb]))
            px = out
            w.number(bits - 2, 3)
            _write_image(w, data, bw, bh)
        else:
            colours = sorted(set(px))
            n = len(colours)
            assert n <= 256
            bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            w.number(n - 1, 8)
            pal = [R.ch(v) for v in colours]
            _write_image(w, [R.unch([(a - b) & 255 for a, b in zip(pal[i], pal[i - 1] if i else [0, 0, 0, 0])]) for i in range(n)], n, 1)
            index = {v: i for i, v in enumerate(colours)}
            per, pw, packed = 8 >> bits, R.subsample(xs, bits), []
            for y in range(H):
                for bx in range(pw):
                    v = 0
                    for k in range(1 << bits):
                        x = (bx << bits) + k
                        if x < xs:
                            v |= index[px[y * xs + x]] << (k * per)
                    packed.append(0xff000000 | v << 8)
            px, xs = packed, pw
    w.number(0, 1)
    meta = None
    if meta_bits:
        mw, mh = R.subsample(xs, meta_bits), R.subsample(H, meta_bits)
        meta = [(bx + by * mw) % groups for by in range(mh) for bx in range(mw)]
    _write_image(w, px, xs, H, cache_bits, meta, meta_bits, main=True)
    return L.container(w.tobytes())


def argb_of(img):
    """uint32 ARGB [H,W] of uint8 [H,W,3 or 4] R, G, B (, A)"""
    a = img[..., 3].astype(np.uint32) if img.shape[2] == 4 else np.full(img.shape[:2], 255, np.uint32)
    return a << 24 | img[..., 0].astype(np.uint32) << 16 | img[..., 1].astype(np.uint32) << 8 | img[..., 2]


# ---- the set --------------------------------------------------------------------------------------------------------------------
def _pil(picture, method, quality):
    return lambda: pil_webp(picture(), method, quality)


PICTURES = {
    'c1': lambda: cartoon(1, 1, 1), 'c37': lambda: cartoon(53, 37, 2), 'c96': lambda: cartoon(128, 96, 3), 'c200': lambda: cartoon(300, 200, 4),
    'i2': lambda: indexed(64, 83, 2, 5), 'i4': lambda: indexed(64, 85, 4, 6), 'i16': lambda: indexed(64, 97, 16, 7), 'i200': lambda: indexed(64, 281, 200, 8),
    'photo': lambda: photo(128, 160, 9), 'cut': lambda: cartoon(128, 96, 10, 4),
}
# picture, method, quality: the subset of the grid (methods 0 2 4 6, qualities 20 75 100) that holds the features the CPU test asserts
PIL_CASES = [
    ('c1', 0, 75), ('c1', 6, 100),
    ('c37', 0, 20), ('c37', 2, 75), ('c37', 4, 75), ('c37', 6, 100),
    ('c96', 0, 75), ('c96', 2, 100), ('c96', 4, 20), ('c96', 6, 75),
    ('c200', 0, 20), ('c200', 2, 75), ('c200', 4, 75), ('c200', 6, 100),
    ('i2', 0, 75), ('i2', 4, 75), ('i4', 2, 75), ('i4', 6, 100), ('i16', 0, 20), ('i16', 4, 75), ('i16', 6, 100), ('i200', 0, 75), ('i200', 6, 75),
    ('photo', 0, 75), ('photo', 2, 75), ('photo', 4, 75), ('photo', 6, 100),
    ('cut', 0, 75), ('cut', 4, 75), ('cut', 6, 100),
]


def _one_colour():
    return pil_webp(np.full((9, 13, 3), 77, np.uint8), 4, 75)


def _hand(name):
    if name == 'hand_cache11':
        return write_vp8l(argb_of(indexed(40, 40, 500, 20)), cache_bits=11, has_alpha=False)
    if name.startswith('hand_cache'):                               # 16 colours, no transform: at 6 bits almost every pixel is a cache hit
        k = int(name[10:])
        return write_vp8l(argb_of(indexed(40 if k == 6 else 12 + k, 40 if k == 6 else 17, 16, 40 + k)), cache_bits=k, has_alpha=False)
    if name == 'hand_groups4':
        return write_vp8l(argb_of(cartoon(70, 66, 35)), meta_bits=6, groups=4, has_alpha=False)
    if name == 'hand_palette_predictor':
        return write_vp8l(argb_of(indexed(21, 19, 5, 21)), transforms=((3,), (0, 2)), has_alpha=False)
    if name == 'hand_green_predictor_cross':
        return write_vp8l(argb_of(cartoon(30, 41, 22, 4)), transforms=((2,), (0, 3), (1, 2)), cache_bits=3)
    if name == 'hand_groups64':
        return write_vp8l(argb_of(cartoon(48, 40, 23)), meta_bits=2, groups=70, has_alpha=False)
    if name == 'hand_small_block':
        return write_vp8l(argb_of(cartoon(3, 5, 24, 4)), transforms=((0, 4), (1, 5)), meta_bits=5, groups=1)
    if name == 'hand_w1':
        return write_vp8l(argb_of(cartoon(37, 1, 25)), transforms=((0, 7),), has_alpha=False)
    if name == 'hand_h1':
        return write_vp8l(argb_of(cartoon(1, 37, 26, 4)), transforms=((2,), (0, 8)), cache_bits=1)
    if name == 'hand_tall':                                         # taller than one band of the inverse predictor
        return write_vp8l(argb_of(cartoon(PREDICT_BAND_ROWS + 7, 5, 27)), transforms=((0, 3),), has_alpha=False)
    if name == 'hand_wide':                                         # wider than one band is tall: more steps than lanes
        return write_vp8l(argb_of(cartoon(6, PREDICT_BAND_ROWS + 45, 28)), transforms=((0, 2),), has_alpha=False)
    if name == 'hand_alpha_residue':                                # the header says "no alpha", the stream holds other values
        return write_vp8l(argb_of(cartoon(8, 9, 29, 4)), has_alpha=False)
    raise KeyError(name)


HAND = ['hand_cache1', 'hand_cache2', 'hand_cache3', 'hand_cache4', 'hand_cache5', 'hand_cache6', 'hand_groups4', 'hand_cache11', 'hand_palette_predictor', 'hand_green_predictor_cross', 'hand_groups64', 'hand_small_block', 'hand_w1', 'hand_h1',
        'hand_tall', 'hand_wide', 'hand_alpha_residue']
NAMES = ['%s_m%d_q%d' % c for c in PIL_CASES] + ['one_colour', 'vp8x_meta'] + HAND
ACCEPTED = set(NAMES)
_files = {}


def chunk(kind, body):
    return kind + struct.pack('<I', len(body)) + body + (b'\x00' if len(body) & 1 else b'')


def riff(body):
    return b'RIFF' + struct.pack('<I', 4 + len(body)) + b'WEBP' + body


def exif(orientation):
    return b'II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x03\x00\x01\x00\x00\x00' + struct.pack('<H', orientation) + b'\x00\x00\x00\x00\x00\x00'


def extended(payload, W, H, alpha, before=b'', after=b'', flags=None):
    f = (0x10 if alpha else 0) if flags is None else flags
    size = struct.pack('<I', W - 1)[:3] + struct.pack('<I', H - 1)[:3]
    return riff(chunk(b'VP8X', bytes([f, 0, 0, 0]) + size) + before + chunk(b'VP8L', payload) + after)


def _vp8x_meta():
    """VP8X + ICCP + VP8L + EXIF (orientation 1) + XMP: what libwebp's muxer writes around a lossless image"""
    img = cartoon(20, 24, 30, 4)
    payload = R.vp8l_chunk(pil_webp(img, 4, 75))
    return extended(payload, 24, 20, True, before=chunk(b'ICCP', b'not a real profile'), after=chunk(b'EXIF', exif(1)) + chunk(b'XMP ', b'<x:xmpmeta/>'),
                    flags=0x10 | 0x20 | 0x08 | 0x04)


def case_file(name):
    if name not in _files:
        if name in HAND:
            _files[name] = _hand(name)
        elif name == 'one_colour':
            _files[name] = _one_colour()
        elif name == 'vp8x_meta':
            _files[name] = _vp8x_meta()
        else:
            pic, m, q = name.rsplit('_', 2)
            _files[name] = pil_webp(PICTURES[pic](), int(m[1:]), int(q[1:]))
    return _files[name]


_refs = {}


def reference_bgra(name):
    if name not in _refs:
        with Image.open(io.BytesIO(case_file(name))) as im:
            _refs[name] = np.ascontiguousarray(np.asarray(im.convert('RGBA'))[..., [2, 1, 0, 3]])
    return _refs[name]


def reference(name):
    """imread's pixels (the test of the routing reads the same through utils.io_utils.imread from a path)"""
    from PIL import ImageOps
    with Image.open(io.BytesIO(case_file(name))) as im:
        return np.ascontiguousarray(np.asarray(ImageOps.exif_transpose(im).convert('RGB'))[:, :, ::-1])


# ---- refused files --------------------------------------------------------------------------------------------------------------
def _small_payload():
    return R.vp8l_chunk(pil_webp(cartoon(5, 8, 31), 0, 75))


def _lossy():
    b = io.BytesIO()
    Image.fromarray(cartoon(16, 16, 32)).save(b, 'WEBP', quality=80)
    return b.getvalue()


def _lossy_alpha():
    b = io.BytesIO()
    Image.fromarray(cartoon(16, 16, 33, 4)).save(b, 'WEBP', quality=80)
    return b.getvalue()


def _animated():
    b = io.BytesIO()
    frames = [Image.fromarray(cartoon(16, 16, 34 + k)) for k in range(2)]
    frames[0].save(b, 'WEBP', save_all=True, append_images=frames[1:], lossless=True, duration=40)
    return b.getvalue()


def _version():
    p = bytearray(_small_payload())
    p[4] |= 0x20
    return riff(chunk(b'VP8L', bytes(p)))


def _riff_overrun():
    d = bytearray(riff(chunk(b'VP8L', _small_payload())))
    d[4:8] = struct.pack('<I', len(d) + 2)
    return bytes(d)


def _chunk_overrun():
    d = bytearray(riff(chunk(b'VP8L', _small_payload())))
    d[16:20] = struct.pack('<I', len(d))
    return bytes(d)


REFUSED = {
    'lossy': (_lossy, 'lossy'),
    'lossy_alpha': (_lossy_alpha, 'lossy'),
    'animated': (_animated, 'animated'),
    'version': (_version, 'version'),
    'riff_overrun': (_riff_overrun, 'RIFF length'),
    'chunk_overrun': (_chunk_overrun, 'runs past'),
    'exif6': (lambda: extended(_small_payload(), 8, 5, False, after=chunk(b'EXIF', exif(6)), flags=0x08), 'orientation 6'),
    'xmp_orientation': (lambda: extended(_small_payload(), 8, 5, False, after=chunk(b'XMP ', b'<x tiff:Orientation="6"/>'), flags=0x04), 'XMP'),
    'not_webp': (lambda: b'RIFF\x04\x00\x00\x00WAVE', 'not a WebP'),
}
