"""Deterministic PNG files for the decoder tests: built with PIL, zlib.compressobj and a small PNG writer that
forces the filter type of every row.  ACCEPTED maps a name to a builder of a file the device decoder takes; REFUSED maps a name to
(builder, a word of the reason pngread.probe must give).  tests/test_pngdec.py asserts with the restatement's walker that the set
has the deflate properties it is there for (block types, match lengths and distances, doubling rounds)."""
import functools
import io
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


# ---- content ----------------------------------------------------------------------------------------------------------------
def cartoon(H, W, ch, seed):
    """flat regions with hard edges and a few thin lines: long matches, distance-1 runs"""
    rng = np.random.default_rng(seed)
    img = np.empty((H, W, ch), np.uint8)
    img[:] = rng.integers(0, 256, ch)
    for _ in range(6):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        y1, x1 = y0 + int(rng.integers(1, max(2, H // 2))), x0 + int(rng.integers(1, max(2, W // 2)))
        img[y0:y1, x0:x1] = rng.integers(0, 256, ch)
    for _ in range(3):
        img[int(rng.integers(0, H)), :] = rng.integers(0, 256, ch)
        img[:, int(rng.integers(0, W))] = rng.integers(0, 256, ch)
    return img


def gradient(H, W, ch, seed):
    """a smooth picture plus light noise: short matches, many distinct literals"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(3 * x + 2 * y * (c + 1) + 40 * c) for c in range(ch)], axis=2) + rng.integers(0, 4, (H, W, ch))
    return (img & 255).astype(np.uint8)


def mixed(H, W, ch, seed):
    """a cartoon picture with two textured patches: short blocks of it take the dynamic code here and the fixed code there"""
    img, g = cartoon(H, W, ch, seed), gradient(H, W, ch, seed)
    img[H // 8:3 * H // 8, W // 12:W - 4] = g[H // 8:3 * H // 8, W // 12:W - 4]
    img[5 * H // 8:7 * H // 8, W // 3:] = (g[5 * H // 8:7 * H // 8, W // 3:] >> 4) << 4
    return img


def noise(H, W, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, ch)).astype(np.uint8)


# ---- the writer -------------------------------------------------------------------------------------------------------------
def chunk(kind, body=b''):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def ihdr(W, H, ct, depth=8, interlace=0):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, ct, 0, 0, interlace))


def filtered(img, types):
    """the raw scanlines (filter byte + filtered bytes) of img uint8 [H, W, ch] with row y filtered by types[y % len(types)]"""
    H, W, ch = img.shape
    rows = img.reshape(H, W * ch).astype(np.int64)
    out = np.empty((H, 1 + W * ch), np.uint8)
    for y in range(H):
        t = types[y % len(types)]
        x = rows[y]
        a = np.concatenate([np.zeros(ch, np.int64), x[:-ch]]) if W * ch > ch else np.zeros(W * ch, np.int64)
        b = rows[y - 1] if y else np.zeros(W * ch, np.int64)
        c = (np.concatenate([np.zeros(ch, np.int64), b[:-ch]]) if W * ch > ch else np.zeros(W * ch, np.int64)) if y else np.zeros(W * ch, np.int64)
        if t == 0:
            pred = 0
        elif t == 1:
            pred = a
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[y, 0] = t
        out[y, 1:] = (x - pred) & 255
    return out.tobytes()


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    if not flush_every:
        return c.compress(raw) + c.flush()
    out = b''
    for k, o in enumerate(range(0, len(raw), flush_every)):
        out += c.compress(raw[o:o + flush_every]) + c.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH)
    return out + c.flush()


def split(stream, sizes):
    """IDAT chunks of the given sizes in turn (0 = an empty chunk)"""
    out, o, k = b'', 0, 0
    while o < len(stream):
        n = sizes[k % len(sizes)]
        out += chunk(b'IDAT', stream[o:o + n])
        o += n
        k += 1
    return out


def png(img, ct, types=(0, 1, 2, 3, 4), stream=None, idat=None, before=b'', after=b'', palette=None, **kw):
    """a PNG file of img uint8 [H, W, channels of ct]; `stream` replaces the zlib stream, `idat` the IDAT chunk sizes, `before` /
    `after` are chunks in front of / behind the IDATs, kw goes to deflate()"""
    H, W, ch = img.shape
    assert ch == CHANNELS[ct]
    if stream is None:
        stream = deflate(filtered(img, types), **kw)
    body = split(stream, idat) if idat else chunk(b'IDAT', stream)
    plte = chunk(b'PLTE', np.asarray(palette, np.uint8).tobytes()) if palette is not None else b''
    return SIGNATURE + ihdr(W, H, ct) + plte + before + body + after + chunk(b'IEND')


def pil_png(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img if img.shape[2] > 1 else img[:, :, 0]).save(buf, 'PNG', **kw)
    return buf.getvalue()


# ---- one hand-assembled fixed-Huffman stream ----------------------------------------------------------------------------------
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):                    # LSB first
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, n):                    # a Huffman code: MSB first
        self.bits(int(format(value, '0%db' % n)[::-1], 2), n)

    def symbol(self, s):                         # the fixed literal/length code (RFC 1951 3.2.6)
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length, dist):
        k = max(i for i in range(29) if LENGTH_BASE[i] <= length and (i == 28 or length < 258))
        self.symbol(257 + k)
        self.bits(length - LENGTH_BASE[k], LENGTH_EXTRA[k])
        d = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.code(d, 5)
        self.bits(dist - DIST_BASE[d], DIST_EXTRA[d])

    def done(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def hand_assembled():
    """a 127 x 261 grey picture whose stream is one fixed-Huffman block written by hand: a length-3 match at distance 1, runs of
    length-258 matches at distance 1, one length-258 match at distance 32 768 (it repeats the first, distinct row 256 rows further
    down) and a length-258 match at distance 1 behind it.  Returns (file, raw bytes, tokens)."""
    W, H = 127, 261
    raw = np.zeros((H, 1 + W), np.uint8)
    raw[0, 1:] = np.arange(1, 128)
    raw[256] = raw[0]
    raw = raw.tobytes()
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    tokens = []
    for v in raw[:129]:
        w.symbol(v)
    pos = 129

    def match(n, d):
        nonlocal pos
        w.match(n, d)
        tokens.append((pos, n, d))
        pos += n
    match(3, 1)
    while pos < 32768:
        match(min(258, 32768 - pos) if 32768 - pos >= 3 else 3, 1)
    assert pos == 32768
    match(258, 32768)
    match(258, 1)
    match(len(raw) - pos, 1)
    w.symbol(256)
    stream = b'\x78\x01' + w.done() + struct.pack('>I', zlib.adler32(raw))
    assert zlib.decompress(stream) == raw
    img = np.frombuffer(raw, np.uint8).reshape(H, 1 + W)[:, 1:, None]
    return png(img, 0, stream=stream), raw, tokens


# ---- the accepted files -------------------------------------------------------------------------------------------------------
def _far():
    """200 x 200 grey: the lower half repeats the noisy upper half 20 100 bytes further down"""
    top = noise(100, 200, 1, 8)
    return png(np.concatenate([top, top]), 0, types=(0,), level=9)


def _palette(n, trns=False, seed=3):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    idx = (cartoon(19, 23, 1, seed).astype(np.int64) % n).astype(np.uint8)
    idx[0, :min(n, 23), 0] = np.arange(min(n, 23))
    if n == 256:
        idx = np.concatenate([idx, np.arange(23 * 12, dtype=np.int64).reshape(12, 23, 1) % 256]).astype(np.uint8)
    before = chunk(b'tRNS', bytes(rng.integers(0, 256, n // 2).astype(np.uint8))) if trns else b''
    return png(idx, 3, palette=pal, before=before)


def _ancillary():
    tiff = b'II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x03\x00\x01\x00\x00\x00\x01\x00\x00\x00\x00\x00\x00\x00'      # orientation 1
    before = chunk(b'gAMA', struct.pack('>I', 45455)) + chunk(b'sRGB', b'\x00') + chunk(b'pHYs', struct.pack('>IIB', 2835, 2835, 1)) + \
        chunk(b'tEXt', b'Comment\x00a comment') + chunk(b'eXIf', tiff) + chunk(b'prVt', b'a private chunk')
    return png(gradient(9, 14, 3, 6), 2, before=before, after=chunk(b'tIME', struct.pack('>HBBBBB', 2024, 1, 2, 3, 4, 5)))


ACCEPTED = {
    'stored': lambda: png(cartoon(16, 16, 3, 1), 2, level=0),
    'fixed': lambda: png(cartoon(20, 24, 3, 2), 2, strategy=zlib.Z_FIXED),
    'cartoon': lambda: png(cartoon(80, 64, 1, 3), 0, types=(0,)),
    'cartoon_rgb': lambda: png(cartoon(80, 64, 3, 3), 2, types=(0,)),
    'blocks': lambda: png(mixed(80, 64, 3, 3), 2, level=9, mem_level=1),
    'flushes': lambda: png(cartoon(40, 33, 3, 4), 2, flush_every=300),
    'huffman_only': lambda: png(gradient(24, 31, 3, 5), 2, strategy=zlib.Z_HUFFMAN_ONLY),
    'rle': lambda: png(cartoon(30, 40, 4, 6), 6, strategy=zlib.Z_RLE),
    'far': _far,
    'hand': lambda: hand_assembled()[0],
    'deep': lambda: png(np.full((3, 1500, 1), 77, np.uint8), 0, types=(0,), strategy=zlib.Z_RLE),
    'flat_paeth': lambda: png(np.full((64, 64, 4), 200, np.uint8), 6, types=(4,)),
    'natural': lambda: pil_png(np.dstack([gradient(300, 200, 3, 9), cartoon(300, 200, 1, 9)])),
    'pil_grey': lambda: pil_png(gradient(33, 47, 1, 10), optimize=True),
    'palette256': lambda: _palette(256),
    'palette7': lambda: _palette(7),
    'palette_trns': lambda: _palette(16, trns=True),
    'ancillary': _ancillary,
    'rgb_trns': lambda: png(gradient(6, 9, 3, 12), 2, before=chunk(b'tRNS', struct.pack('>HHH', 1, 2, 3))),
    'rgb_plte': lambda: png(gradient(6, 9, 3, 13), 2, palette=noise(1, 5, 3, 13)[0]),
    'idat_1': lambda: png(cartoon(12, 17, 3, 14), 2, idat=(1,)),
    'idat_prime': lambda: png(gradient(21, 30, 4, 15), 6, idat=(7,)),
    'idat_empty': lambda: png(cartoon(12, 17, 2, 16), 4, idat=(0, 5, 0, 0, 64)),
    'trailing': lambda: png(cartoon(14, 19, 3, 21), 2, stream=deflate(filtered(cartoon(14, 19, 3, 21), (0, 4, 2))) + b'bytes behind the trailer',
                            idat=(50,)),
    '1x1': lambda: png(noise(1, 1, 3, 17), 2),
    '1x37': lambda: png(gradient(37, 1, 3, 18), 2),
    '37x1': lambda: png(gradient(1, 37, 4, 19), 6, types=(4,)),
    '3x1030': lambda: png(gradient(1030, 3, 3, 20), 2),
}
for _t in range(5):                                   # one filter type on every row: the first row and the later ones
    ACCEPTED['filter%d' % _t] = functools.partial(lambda t: png(gradient(9, 11, 3, 30 + t), 2, types=(t,)), _t)
    ACCEPTED['filter%d_first' % _t] = functools.partial(lambda t: png(cartoon(7, 10, 4, 40 + t), 6, types=(t, (t + 2) % 5, (t + 4) % 5)), _t)
for _ct in (0, 4, 2, 6):                              # all five types cycling at 1, 2, 3 and 4 bytes per pixel
    ACCEPTED['cycle_ct%d' % _ct] = functools.partial(lambda ct: png(gradient(11, 13, CHANNELS[ct], 50 + ct), ct), _ct)
    ACCEPTED['cycle_noise_ct%d' % _ct] = functools.partial(lambda ct: png(noise(10, 6, CHANNELS[ct], 60 + ct), ct, types=(4, 3, 1, 2, 0)), _ct)
for _w in (1, 2, 3, 5):
    ACCEPTED['width%d' % _w] = functools.partial(lambda w: png(noise(7, w, 3, 70 + w), 2), _w)
    ACCEPTED['width%d_ga' % _w] = functools.partial(lambda w: png(noise(6, w, 2, 80 + w), 4, types=(3, 4, 1)), _w)

NAMES = sorted(ACCEPTED)


@functools.lru_cache(maxsize=None)
def case_file(name):
    return ACCEPTED[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """imread's pixels of the file: uint8 [H, W, 3], B, G, R"""
    import warnings
    from PIL import Image, ImageOps
    with warnings.catch_warnings(), Image.open(io.BytesIO(case_file(name))) as im:
        warnings.simplefilter('ignore')          # PIL's advice on palette files with tRNS
        return np.ascontiguousarray(np.asarray(ImageOps.exif_transpose(im).convert('RGB'))[:, :, ::-1])


# ---- the refused files ------------------------------------------------------------------------------------------------------
def _good():
    return png(gradient(8, 8, 3, 1), 2)


def _with_ihdr(**kw):
    g = _good()
    W, H, depth, ct, _, _, lace = struct.unpack('>IIBBBBB', g[16:29])
    v = dict(W=W, H=H, ct=ct, depth=depth, interlace=lace)
    v.update(kw)
    return g[:8] + ihdr(v['W'], v['H'], v['ct'], v['depth'], v['interlace']) + g[33:]


def _pil(mode, **kw):
    from PIL import Image
    buf = io.BytesIO()
    img = gradient(8, 8, 1, 2)[:, :, 0]
    {'1': Image.fromarray(img > 128), 'I;16': Image.fromarray(img.astype(np.uint16) * 257)}.get(mode, Image.fromarray(img)).save(buf, 'PNG', **kw)
    return buf.getvalue()


def _exif(orientation):
    tiff = b'MM\x00*\x00\x00\x00\x08\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01' + struct.pack('>H', orientation) + b'\x00\x00\x00\x00\x00\x00'
    return png(gradient(8, 5, 3, 1), 2, before=chunk(b'eXIf', tiff))


def _bad_crc(kind):
    g = bytearray(png(gradient(8, 8, 1, 1), 3, palette=noise(1, 256, 3, 1)[0]))
    at = g.index(kind) + 4
    g[at] ^= 1
    return bytes(g)


def _zlib_header(cmf, flg):
    s = bytearray(deflate(filtered(gradient(8, 8, 3, 1), (0,))))
    s[0], s[1] = cmf, flg
    return png(gradient(8, 8, 3, 1), 2, stream=bytes(s))


REFUSED = {
    'depth1': (lambda: _pil('1'), 'bit depth 1'),
    'depth2': (lambda: _with_ihdr(ct=0, depth=2), 'bit depth 2'),
    'depth4': (lambda: _with_ihdr(ct=3, depth=4), 'bit depth 4'),
    'depth16': (lambda: _pil('I;16'), 'bit depth 16'),
    'interlaced': (lambda: _with_ihdr(interlace=1), 'interlaced'),
    'colour_type5': (lambda: _with_ihdr(ct=5), 'colour type'),
    'apng': (lambda: png(gradient(8, 8, 3, 1), 2, before=chunk(b'acTL', struct.pack('>II', 1, 0))), 'animated'),
    'exif6': (lambda: _exif(6), 'orientation 6'),
    'exif_magic': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'eXIf', b'II+\x00\x08\x00\x00\x00\x00\x00')), 'orientation unreadable'),
    'exif_offset': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'eXIf', b'II*\x00\x40\x00\x00\x00\x00\x00')), 'orientation unreadable'),
    'exif_entries': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'eXIf', b'II*\x00\x08\x00\x00\x00\x05\x00')), 'orientation unreadable'),
    'exif_type': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(
        b'eXIf', b'II*\x00\x08\x00\x00\x00\x01\x00\x12\x01\x04\x00\x01\x00\x00\x00\x06\x00\x00\x00\x00\x00\x00\x00')), 'orientation unreadable'),
    'raw_profile': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'tEXt', b'Raw profile type exif\x00\nexif\n 0\n')), 'text chunk'),
    'itxt_compressed': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'iTXt', b'Comment\x00\x01\x00\x00\x00' + zlib.compress(b'text'))),
                        'compressed text'),
    'exif_broken': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'eXIf', b'not a TIFF block')), 'orientation unreadable'),
    'xmp': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'iTXt', b'XML:com.adobe.xmp\x00\x00\x00\x00\x00<x tiff:Orientation="6"/>')),
            'text chunk'),
    'ztxt': (lambda: png(gradient(8, 5, 3, 1), 2, before=chunk(b'zTXt', b'Comment\x00\x00' + zlib.compress(b'text'))), 'compressed text'),
    'crc_ihdr': (lambda: _bad_crc(b'IHDR'), 'bad CRC'),
    'crc_plte': (lambda: _bad_crc(b'PLTE'), 'bad CRC'),
    'crc_idat': (lambda: _bad_crc(b'IDAT'), 'bad CRC'),
    'fctl': (lambda: png(gradient(8, 8, 3, 1), 2, before=chunk(b'fcTL', bytes(26))), 'animated PNG (fcTL)'),
    'fdat': (lambda: png(gradient(8, 8, 3, 1), 2, after=chunk(b'fdAT', bytes(8))), 'animated PNG (fdAT)'),
    'ihdr_size': (lambda: SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBBB', 8, 8, 8, 2, 0, 0, 0, 0)) + _good()[33:], 'IHDR of 14 bytes'),
    'compression': (lambda: _good()[:8] + chunk(b'IHDR', struct.pack('>IIBBBBB', 8, 8, 8, 2, 1, 0, 0)) + _good()[33:], 'compression or filter'),
    'filter_method': (lambda: _good()[:8] + chunk(b'IHDR', struct.pack('>IIBBBBB', 8, 8, 8, 2, 0, 1, 0)) + _good()[33:], 'compression or filter'),
    'signature_only': (lambda: SIGNATURE, 'no IHDR'),
    'cut_header': (lambda: _good()[:37], 'chunk header runs past'),
    'plte_length': (lambda: png(gradient(8, 8, 1, 1), 3, before=chunk(b'PLTE', bytes(10))), 'PLTE'),
    'plte_empty': (lambda: png(gradient(8, 8, 1, 1), 3, before=chunk(b'PLTE', b'')), 'PLTE'),
    'plte_long': (lambda: png(gradient(8, 8, 1, 1), 3, before=chunk(b'PLTE', bytes(771))), 'PLTE'),
    'plte_twice': (lambda: png(gradient(8, 8, 1, 1), 3, palette=noise(1, 256, 3, 1)[0], before=chunk(b'PLTE', bytes(9))), 'PLTE'),
    'huge_width': (lambda: _with_ihdr(W=2 ** 31), 'invalid width'),
    'no_iend': (lambda: _good()[:-12], 'no IEND'),
    'no_idat': (lambda: SIGNATURE + ihdr(8, 8, 2) + chunk(b'IEND'), 'no IDAT'),
    'cut_chunk': (lambda: _good()[:60], 'past the end'),
    'zero_width': (lambda: _with_ihdr(W=0), 'zero'),
    'too_large': (lambda: _with_ihdr(W=40000, H=40000), '32-bit'),
    'many_pixels': (lambda: _with_ihdr(W=10000, H=10000, ct=0), 'more pixels'),
    'not_png': (lambda: b'\xff\xd8\xff\xe0' + _good(), 'not a PNG'),
    'no_plte': (lambda: png(gradient(8, 8, 1, 1), 3), 'without PLTE'),
    'plte_late': (lambda: png(gradient(8, 8, 3, 1), 2, after=chunk(b'PLTE', bytes(9))), 'PLTE'),
    'idat_apart': (lambda: png(gradient(8, 8, 3, 1), 2, after=chunk(b'tEXt', b'k\x00v') + chunk(b'IDAT', b'')), 'not consecutive'),
    'two_ihdr': (lambda: png(gradient(8, 8, 3, 1), 2, before=ihdr(8, 8, 2)), 'IHDR'),
    'critical': (lambda: png(gradient(8, 8, 3, 1), 2, before=chunk(b'ABCD', b'x')), 'critical'),
    'zlib_cm': (lambda: _zlib_header(0x77, 0x09), 'zlib header'),
    'zlib_fdict': (lambda: _zlib_header(0x78, 0x20 + 31 - (0x7820 % 31)), 'zlib header'),
    'zlib_fcheck': (lambda: _zlib_header(0x78, 0x9D), 'zlib header'),
    'short_stream': (lambda: png(gradient(8, 8, 3, 1), 2, stream=b'\x78\x9c\x03'), 'zlib stream'),
}


def wrong_adler():
    """a file whose only defect is the Adler-32 trailer: the CRCs are right, the deflate data valid"""
    img = cartoon(20, 24, 3, 2)
    s = bytearray(deflate(filtered(img, (0, 1, 2, 3, 4))))
    s[-1] ^= 0x55
    return png(img, 2, stream=bytes(s))
