"""An independent Python / numpy restatement of the lossless WebP decoder's contract, written from the format
(the WebP lossless bitstream specification) and sharing no code with cartoonsegmentation_amd (csrc/csm_vp8l.h, csrc/webpdec.hip,
webpread.py).  Pillow (libwebp) judges it: tests/test_webpdec.py holds it to PIL's pixels on every file of tests/webpdec_cases.py.

    decode(data)           (argb uint32 [H,W], features) of a .webp file (a bare VP8L chunk, or VP8X + VP8L)
    decode_payload(b)      the same of a VP8L chunk's payload
    bgr(argb), bgra(argb, has_alpha)     the two outputs of ops.webp_decode as uint8 arrays

features: 'transforms' (types in stream order: 0 predictor, 1 cross-colour, 2 subtract-green, 3 colour indexing), 'modes' (the
predictor modes of blocks that hold a pixel outside row 0 and column 0), 'block_bits' ({transform type: bits}), 'cache_bits' (one
entry per entropy-coded image, sub-images included, 0 = none; the main image is the last), 'cache_hits', 'groups', 'meta_bits',
'forms' (the kinds of code headers: 'simple1', 'simple2', 'normal', 'normal_max'), 'refs' ({'map', 'beyond', 'overlap'} counts of
backward references by kind, over all entropy-coded images), 'palette' (colours, 0 = none), 'alpha' (the header's flag), 'bits'
(consumed) and 'size' (W, H)."""
import struct

import numpy as np

ORDER = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
DISTANCE_MAP = [
    (0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3),
    (-1, 3), (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3),
    (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5),
    (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1),
    (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7),
    (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7),
    (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6),
    (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]
assert len(DISTANCE_MAP) == 120


class Corrupt(ValueError):
    pass


class Reader:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder='little').tolist()
        self.n = len(self.bits)
        self.bits += [0] * 64
        self.pos = 0

    def read(self, n):
        if self.pos + n > self.n:
            raise Corrupt("the stream ends early")
        v = 0
        for k in range(n):
            v |= self.bits[self.pos + k] << k
        self.pos += n
        return v


def subsample(v, bits):
    return (v + (1 << bits) - 1) >> bits


def make_code(lengths):
    """{(length, code): symbol} of a complete canonical code, or {'single': symbol} for a code of one symbol"""
    used = [s for s, l in enumerate(lengths) if l]
    if not used:
        raise Corrupt("a code without symbols")
    if len(used) == 1:
        return {'single': used[0]}
    if sum(1 << (15 - l) for l in lengths if l) != 1 << 15:
        raise Corrupt("an incomplete or over-subscribed code")
    table, code = {}, 0
    for l in range(1, 16):
        for s in used:
            if lengths[s] == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def symbol(r, table):
    if 'single' in table:
        return table['single']
    code = 0
    for l in range(1, 16):
        code = code << 1 | r.read(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise Corrupt("an unassigned code")


def read_code(r, n, feat):
    lengths = [0] * n
    if r.read(1):
        two = r.read(1)
        syms = [r.read(8 if r.read(1) else 1)]
        if two:
            syms.append(r.read(8))
        feat['forms'].add('simple2' if two else 'simple1')
        for s in syms:
            if s < n:
                lengths[s] = 1
    else:
        ncl = 4 + r.read(4)
        if ncl > 19:
            raise Corrupt("too many code length codes")
        cl = [0] * 19
        for k in range(ncl):
            cl[ORDER[k]] = r.read(3)
        table = make_code(cl)
        limit = n
        if r.read(1):
            bits = 2 + 2 * r.read(3)
            limit = 2 + r.read(bits)
            if limit > n:
                raise Corrupt("max_symbol above the alphabet")
            feat['forms'].add('normal_max')
        else:
            feat['forms'].add('normal')
        s, prev = 0, 8
        while s < n and limit > 0:
            limit -= 1
            l = symbol(r, table)
            if l < 16:
                lengths[s] = l
                s += 1
                prev = l or prev
            else:
                rep = r.read((2, 3, 7)[l - 16]) + (3, 3, 11)[l - 16]
                if s + rep > n:
                    raise Corrupt("a run of code lengths past the alphabet")
                if l == 16:
                    lengths[s:s + rep] = [prev] * rep
                s += rep
    return make_code(lengths)


def prefix_value(r, s):
    if s < 4:
        return s + 1
    extra = (s - 2) >> 1
    return ((2 + (s & 1)) << extra) + r.read(extra) + 1


def read_image(r, xs, ys, main, feat, group_cap=None):
    """one entropy-coded image: a list of xs * ys ARGB values"""
    cache_bits = 0
    if r.read(1):
        cache_bits = r.read(4)
        if not 1 <= cache_bits <= 11:
            raise Corrupt("colour cache bits %d" % cache_bits)
    meta, meta_bits, meta_w, ngroups = None, 0, 0, 1
    if main and r.read(1):
        meta_bits = r.read(3) + 2
        meta_w = subsample(xs, meta_bits)
        meta = [(v >> 8) & 0xffff for v in read_image(r, meta_w, subsample(ys, meta_bits), False, feat)]
        ngroups = max(meta) + 1
    feat['cache_bits'].append(cache_bits)
    if main:
        feat['groups'], feat['meta_bits'] = ngroups, meta_bits
        if group_cap is not None and ngroups > group_cap:
            raise OverCap(ngroups)
    sizes = (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    groups = [[read_code(r, n, feat) for n in sizes] for _ in range(ngroups)]
    cache = [0] * (1 << cache_bits) if cache_bits else None
    shift = 32 - cache_bits
    out = [0] * (xs * ys)
    pos, total = 0, xs * ys
    while pos < total:
        x, y = pos % xs, pos // xs
        g = groups[meta[(y >> meta_bits) * meta_w + (x >> meta_bits)]] if meta else groups[0]
        s = symbol(r, g[0])
        if s < 256:
            red = symbol(r, g[1]); blue = symbol(r, g[2]); a = symbol(r, g[3])
            px = a << 24 | red << 16 | s << 8 | blue
            out[pos] = px
            pos += 1
            if cache is not None:
                cache[(0x1e35a7bd * px & 0xffffffff) >> shift] = px
        elif s < 280:
            length = prefix_value(r, s - 256)
            code = prefix_value(r, symbol(r, g[4]))
            if code > 120:
                dist = code - 120
                feat['refs']['beyond'] += 1
            else:
                dx, dy = DISTANCE_MAP[code - 1]
                dist = max(1, dx + dy * xs)
                feat['refs']['map'] += 1
            if dist < length:
                feat['refs']['overlap'] += 1
            if dist > pos or pos + length > total:
                raise Corrupt("a reference outside the image")
            for k in range(length):
                px = out[pos - dist]
                out[pos] = px
                pos += 1
                if cache is not None:
                    cache[(0x1e35a7bd * px & 0xffffffff) >> shift] = px
        else:
            if cache is None or s - 280 >= len(cache):
                raise Corrupt("a cache index beyond the cache")
            out[pos] = cache[s - 280]
            pos += 1
            feat['cache_hits'] += 1
    return out


class OverCap(ValueError):
    pass


# ---- the inverse transforms -----------------------------------------------------------------------------------------------------
def ch(v):
    return [(v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255]


def unch(c):
    return c[0] << 24 | c[1] << 16 | c[2] << 8 | c[3]


def avg(a, b):
    return [(p + q) >> 1 for p, q in zip(a, b)]


def clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def predict(mode, L, T, TL, TR):
    if mode == 1: return L
    if mode == 2: return T
    if mode == 3: return TR
    if mode == 4: return TL
    if mode == 5: return avg(avg(L, TR), T)
    if mode == 6: return avg(L, TL)
    if mode == 7: return avg(L, T)
    if mode == 8: return avg(TL, T)
    if mode == 9: return avg(T, TR)
    if mode == 10: return avg(avg(L, TL), avg(T, TR))
    if mode == 11:
        p_l = sum(abs(t - tl) for t, tl in zip(T, TL))
        p_t = sum(abs(l - tl) for l, tl in zip(L, TL))
        return L if p_l < p_t else T
    if mode == 12: return [clip(l + t - tl) for l, t, tl in zip(L, T, TL)]
    if mode == 13: return [clip(a + int((a - tl) / 2)) for a, tl in zip(avg(L, T), TL)]
    return [255, 0, 0, 0]


def inverse_predictor(px, xs, ys, modes, bits, feat):
    bw = subsample(xs, bits)
    out = [None] * (xs * ys)
    for y in range(ys):
        for x in range(xs):
            if y == 0:
                p = [255, 0, 0, 0] if x == 0 else out[x - 1]
            elif x == 0:
                p = out[(y - 1) * xs]
            else:
                mode = (modes[(y >> bits) * bw + (x >> bits)] >> 8) & 15
                feat['modes'].add(mode)
                TR = out[(y - 1) * xs + x + 1] if x + 1 < xs else out[y * xs]
                p = predict(mode, out[y * xs + x - 1], out[(y - 1) * xs + x], out[(y - 1) * xs + x - 1], TR)
            out[y * xs + x] = [(a + b) & 255 for a, b in zip(ch(px[y * xs + x]), p)]
    return [unch(c) for c in out]


def s8(v):
    return v - 256 if v > 127 else v


def inverse_cross_colour(px, xs, ys, data, bits):
    bw = subsample(xs, bits)
    out = []
    for i, v in enumerate(px):
        m = data[((i // xs) >> bits) * bw + ((i % xs) >> bits)]
        g2r, g2b, r2b = m & 255, (m >> 8) & 255, (m >> 16) & 255
        a, r, g, b = ch(v)
        r = (r + ((s8(g2r) * s8(g)) >> 5)) & 255
        b = (b + ((s8(g2b) * s8(g)) >> 5) + ((s8(r2b) * s8(r)) >> 5)) & 255
        out.append(unch([a, r, g, b]))
    return out


def decode_payload(data, group_cap=None):
    r = Reader(data)
    feat = {'transforms': [], 'modes': set(), 'block_bits': {}, 'cache_bits': [], 'cache_hits': 0, 'groups': 0, 'meta_bits': 0,
            'forms': set(), 'refs': {'map': 0, 'beyond': 0, 'overlap': 0}, 'palette': 0}
    if r.read(8) != 0x2f:
        raise Corrupt("no signature")
    W, H = r.read(14) + 1, r.read(14) + 1
    feat['alpha'] = bool(r.read(1))
    if r.read(3) != 0:
        raise Corrupt("version")
    feat['size'] = (W, H)
    xs, trans = W, []
    while r.read(1):
        t = r.read(2)
        if t in feat['transforms']:
            raise Corrupt("a second transform of type %d" % t)
        feat['transforms'].append(t)
        if t in (0, 1):
            bits = r.read(3) + 2
            feat['block_bits'][t] = bits
            trans.append((t, xs, bits, read_image(r, subsample(xs, bits), subsample(H, bits), False, feat)))
        elif t == 3:
            n = r.read(8) + 1
            bits = 0 if n > 16 else 1 if n > 4 else 2 if n > 2 else 3
            pal = [ch(v) for v in read_image(r, n, 1, False, feat)]
            for i in range(1, n):
                pal[i] = [(a + b) & 255 for a, b in zip(pal[i], pal[i - 1])]
            feat['palette'] = n
            trans.append((t, xs, bits, [unch(c) for c in pal]))
            xs = subsample(xs, bits)
        else:
            trans.append((t, xs, 0, None))
    px = read_image(r, xs, H, True, feat, group_cap)
    feat['bits'] = r.pos
    for t, w, bits, data in reversed(trans):
        if t == 0:
            px = inverse_predictor(px, w, H, data, bits, feat)
        elif t == 1:
            px = inverse_cross_colour(px, w, H, data, bits)
        elif t == 2:
            px = [(v & 0xff00ff00) | ((v & 0x00ff00ff) + ((v >> 8 & 255) * 0x00010001) & 0x00ff00ff) for v in px]
        else:
            per, pw, out = 8 >> bits, subsample(w, bits), []
            for y in range(H):
                for x in range(w):
                    idx = ((px[y * pw + (x >> bits)] >> 8) & 255) >> ((x & ((1 << bits) - 1)) * per) & ((1 << per) - 1)
                    out.append(data[idx] if idx < len(data) else 0)
            px = out
    return np.array(px, np.uint32).reshape(H, W), feat


def vp8l_chunk(data):
    """the VP8L chunk's payload of a .webp file (a plain walk over the RIFF chunks)"""
    assert data[:4] == b'RIFF' and data[8:12] == b'WEBP'
    p, end = 12, 8 + struct.unpack('<I', data[4:8])[0]
    while p + 8 <= end:
        kind, n = data[p:p + 4], struct.unpack('<I', data[p + 4:p + 8])[0]
        if kind == b'VP8L':
            return data[p + 8:p + 8 + n]
        p += 8 + n + (n & 1)
    raise Corrupt("no VP8L chunk")


def decode(data, group_cap=None):
    return decode_payload(vp8l_chunk(bytes(data)), group_cap)


def bgr(argb):
    return np.stack([argb & 255, argb >> 8 & 255, argb >> 16 & 255], axis=2).astype(np.uint8)


def bgra(argb, has_alpha):
    a = argb >> 24 if has_alpha else np.full_like(argb, 255)
    return np.stack([argb & 255, argb >> 8 & 255, argb >> 16 & 255, a], axis=2).astype(np.uint8)
