"""An independent numpy / Python restatement of the PNG contract: filter choice, run parse, histogram, the
length-limited code, the dynamic block header, the bit writer, the Adler-32 and the PNG / APNG containers.  It shares no code with
cartoonsegmentation_amd (csrc/png.hip, pngcode.py, video.py); the tests hold the product to it byte for byte.

    encode(img)            a complete PNG file of one image
    stream(img)            its zlib stream alone (what IDAT holds)
    filtered(img)          the filtered scanlines uint8 [H, 1 + W * C]
    build(hist)            the code of one image from its 286 counts
    apng(streams, ...)     an animated PNG from zlib streams

img: uint8 [H,W] (grey), uint8 [H,W,3] (B, G, R in memory unless bgr=False) or bool [H,W] (a mask, written 0 / 255).
"""
import binascii
import itertools
import struct
import zlib

import numpy as np

# RFC 1951 §3.2.5: (symbol, extra bits, first length)
LENGTH_TABLE = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10),
                (265, 1, 11), (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31),
                (273, 3, 35), (274, 3, 43), (275, 3, 51), (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115),
                (281, 5, 131), (282, 5, 163), (283, 5, 195), (284, 5, 227), (285, 0, 258)]
ORDER_OF_CODE_LENGTHS = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _length_lookup():
    sym, eb, ev = np.zeros(259, np.int64), np.zeros(259, np.int64), np.zeros(259, np.int64)
    for (s, e, first), nxt in zip(LENGTH_TABLE, LENGTH_TABLE[1:] + [(0, 0, 259)]):
        last = 257 if s == 284 else nxt[2] - 1                  # symbol 284 stops at 257: 258 has its own symbol
        for ln in range(first, last + 1):
            sym[ln], eb[ln], ev[ln] = s, e, ln - first
    return sym, eb, ev


LEN_SYM, LEN_EB, LEN_EV = _length_lookup()


# ---- filter -----------------------------------------------------------------------------------------------------------------
def file_order(img, bgr=True):
    """the image as the file holds it: int64 [H, W, C] in R, G, B (or grey) order"""
    a = np.asarray(img)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8) * 255
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    if a.ndim == 2:
        a = a[:, :, None]
    elif bgr:
        a = a[:, :, ::-1]
    return a.astype(np.int64)


def filtered(img, bgr=True):
    px = file_order(img, bgr)
    H, W, C = px.shape
    left = np.zeros_like(px); left[:, 1:] = px[:, :-1]
    up = np.zeros_like(px); up[1:] = px[:-1]
    upleft = np.zeros_like(px); upleft[1:, 1:] = px[:-1, :-1]
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    cands = np.stack([px, px - left, px - up, px - (left + up) // 2, px - pred]).reshape(5, H, W * C) % 256
    score = np.minimum(cands, 256 - cands).sum(axis=2)          # [5, H]
    kind = np.argmin(score, axis=0)                             # the first minimum: ties go to the lowest type
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = kind
    out[:, 1:] = cands[kind, np.arange(H)]
    return out


# ---- parse ------------------------------------------------------------------------------------------------------------------
def tokens(filt):
    """(symbol, extra bits, extra value, is a match) of every token of the image, scanline by scanline, without the end-of-block"""
    H, L = filt.shape
    start = np.ones((H, L), bool)
    start[:, 1:] = filt[:, 1:] != filt[:, :-1]                  # column 0 always starts a run: runs never cross scanlines
    pos = np.flatnonzero(start.reshape(-1))
    value = filt.reshape(-1)[pos].astype(np.int64)
    length = np.diff(np.append(pos, H * L))
    rest = length - 1
    full, rem = rest // 258, rest % 258
    per_run = 1 + full + np.where(rem >= 3, 1, rem)
    run = np.repeat(np.arange(len(pos)), per_run)
    k = np.arange(per_run.sum()) - np.repeat(np.cumsum(per_run) - per_run, per_run)
    is_full = (k >= 1) & (k <= full[run])
    is_rem = (k > full[run]) & (rem[run] >= 3)
    match_len = np.where(is_full, 258, np.where(is_rem, rem[run], 0))
    match = match_len > 0
    sym = np.where(match, LEN_SYM[match_len], value[run])
    return sym, np.where(match, LEN_EB[match_len], 0), np.where(match, LEN_EV[match_len], 0), match


def histogram(filt):
    h = np.bincount(tokens(filt)[0], minlength=286)
    h[256] += 1
    return h


# ---- codes ------------------------------------------------------------------------------------------------------------------
def code_lengths(hist, limit):
    """package-merge with explicit items.  Leaves in the order (count ascending, symbol descending); every level merges the leaves
    with the pairs of the level before, a leaf first where the weights are equal; the first 2n - 2 items of the last level count."""
    used = [s for s in range(len(hist)) if hist[s] > 0]
    used.sort(key=lambda s: (int(hist[s]), -s))
    n = len(used)
    assert 2 <= n <= 2 ** limit
    unit = np.eye(n, dtype=np.int64)
    leaves = [(int(hist[s]), unit[i]) for i, s in enumerate(used)]
    level = list(leaves)
    for _ in range(limit - 1):
        pairs = [(level[j][0] + level[j + 1][0], level[j][1] + level[j + 1][1]) for j in range(0, len(level) - 1, 2)]
        merged, a, b = [], 0, 0
        while a < n or b < len(pairs):
            if b == len(pairs) or (a < n and leaves[a][0] <= pairs[b][0]):
                merged.append(leaves[a]); a += 1
            else:
                merged.append(pairs[b]); b += 1
        level = merged
    depth = sum(item[1] for item in level[:2 * n - 2])
    out = [0] * len(hist)
    for i, s in enumerate(used):
        out[s] = int(depth[i])
    return out


def assign_codes(lengths):
    """canonical codes (shorter first, then by symbol), as MSB-first integers"""
    codes, code, prev = [0] * len(lengths), 0, 0
    for ln, s in sorted((ln, s) for s, ln in enumerate(lengths) if ln):
        code <<= ln - prev
        codes[s] = code
        code += 1
        prev = ln
    return codes


def mirrored(code, n):
    r = 0
    for _ in range(n):
        r = r << 1 | code & 1
        code >>= 1
    return r


class BitWriter:
    """deflate's bit order: the first bit written is the lowest bit of the first byte"""
    def __init__(self):
        self.bits = []

    def number(self, v, n):                                     # plain value, lowest bit first
        self.bits += [(v >> k) & 1 for k in range(n)]

    def huffman(self, code, n):                                 # Huffman code, highest bit first
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]


def length_symbols(seq):
    """run coding of a code-length sequence -> [(symbol, extra bits, extra value)]"""
    out = []
    for v, grp in itertools.groupby(seq):
        c = len(list(grp))
        if v == 0:
            while c >= 11:
                k = min(c, 138); out.append((18, 7, k - 11)); c -= k
            if c >= 3:
                out.append((17, 3, c - 3)); c = 0
            out += [(0, 0, 0)] * c
        else:
            out.append((v, 0, 0)); c -= 1
            while c >= 3:
                k = min(c, 6); out.append((16, 2, k - 3)); c -= k
            out += [(v, 0, 0)] * c
    return out


FIXED = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8              # 288 symbols


def build(hist):
    """{'btype', 'lengths' [286], 'codes' [286] MSB-first, 'dist_bits', 'header' (list of bits after the zlib bytes), 'bits' (of
    the block: header + symbols + end-of-block), 'bytes' of the zlib stream, 'fixed_bits' / 'dynamic_bits': 'bits' under either code}"""
    hist = [int(v) for v in hist]
    assert len(hist) == 286 and hist[256] == 1
    extra = [0] * 257 + [e for _, e, _ in LENGTH_TABLE]
    matches = sum(hist[257:])

    def payload(lengths, dist_bits):
        return sum(hist[s] * (lengths[s] + extra[s]) for s in range(286)) + matches * dist_bits

    lengths = code_lengths(hist, 15)
    hlit = max(257, max(s for s in range(286) if lengths[s]) + 1)
    syms = length_symbols(lengths[:hlit] + [1])                 # one distance code: symbol 0, length 1
    cl_hist = [0] * 19
    for s, _, _ in syms:
        cl_hist[s] += 1
    cl_len = code_lengths(cl_hist, 7)
    cl_code = assign_codes(cl_len)
    hclen = max(4, max(k for k in range(19) if cl_len[ORDER_OF_CODE_LENGTHS[k]]) + 1)
    w = BitWriter()
    w.number(1, 1); w.number(2, 2); w.number(hlit - 257, 5); w.number(0, 5); w.number(hclen - 4, 4)
    for k in range(hclen):
        w.number(cl_len[ORDER_OF_CODE_LENGTHS[k]], 3)
    for s, eb, ev in syms:
        w.huffman(cl_code[s], cl_len[s])
        w.number(ev, eb)
    dyn = len(w.bits) + payload(lengths, 1)
    fix = 3 + payload(FIXED, 5)
    if dyn < fix:
        return {'btype': 2, 'lengths': lengths, 'codes': assign_codes(lengths), 'dist_bits': 1, 'header': w.bits, 'bits': dyn,
                'bytes': 2 + (dyn + 7) // 8 + 4, 'fixed_bits': fix, 'dynamic_bits': dyn}
    return {'btype': 1, 'lengths': FIXED[:286], 'codes': assign_codes(FIXED)[:286], 'dist_bits': 5, 'header': [1, 1, 0], 'bits': fix,
            'bytes': 2 + (fix + 7) // 8 + 4, 'fixed_bits': fix, 'dynamic_bits': dyn}


# ---- stream -----------------------------------------------------------------------------------------------------------------
def stream_of_filtered(filt):
    sym, eb, ev, match = tokens(filt)
    hist = np.bincount(sym, minlength=286)
    hist[256] += 1
    code = build(hist)
    lengths = np.array(code['lengths'], np.int64)
    mirror = np.array([mirrored(c, n) for c, n in zip(code['codes'], code['lengths'])], np.int64)
    # a token as one LSB-first number: mirrored code, extra bits of the length, the distance code (zeros)
    value = mirror[sym] | ev << lengths[sym]
    nbits = lengths[sym] + eb + np.where(match, code['dist_bits'], 0)
    head = np.array(code['header'], np.uint8)
    at = len(head) + np.cumsum(nbits) - nbits
    total = len(head) + int(nbits.sum()) + code['lengths'][256]
    assert total == code['bits']
    bits = np.zeros(total, np.uint8)
    bits[:len(head)] = head
    for k in range(int(nbits.max())):
        m = nbits > k
        bits[at[m] + k] = (value[m] >> k) & 1
    eob = mirrored(code['codes'][256], code['lengths'][256])
    for k in range(code['lengths'][256]):
        bits[total - code['lengths'][256] + k] = (eob >> k) & 1
    body = np.packbits(bits, bitorder='little').tobytes()
    out = b'\x78\x01' + body + struct.pack('>I', zlib.adler32(filt.tobytes()) & 0xFFFFFFFF)
    assert len(out) == code['bytes']
    return out


def stream(img, bgr=True):
    return stream_of_filtered(filtered(img, bgr))


# ---- containers -------------------------------------------------------------------------------------------------------------
def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', binascii.crc32(data, binascii.crc32(kind)) & 0xFFFFFFFF)


def _ihdr(W, H, colour_type):
    return _chunk(b'IHDR', struct.pack('>II', W, H) + bytes([8, colour_type, 0, 0, 0]))


def encode(img, bgr=True):
    a = np.asarray(img)
    return b'\x89PNG\r\n\x1a\n' + _ihdr(a.shape[1], a.shape[0], 2 if a.ndim == 3 else 0) + _chunk(b'IDAT', stream(a, bgr)) + _chunk(b'IEND', b'')


def apng(streams, W, H, colour_type, fps=25, order=None):
    order = list(range(len(streams))) if order is None else list(order)
    out = [b'\x89PNG\r\n\x1a\n', _ihdr(W, H, colour_type), _chunk(b'acTL', struct.pack('>II', len(order), 0))]
    seq = 0
    for k, i in enumerate(order):
        out.append(_chunk(b'fcTL', struct.pack('>I', seq) + struct.pack('>IIII', W, H, 0, 0) + struct.pack('>HH', 1, fps) + b'\x00\x00'))
        seq += 1
        if k == 0:
            out.append(_chunk(b'IDAT', streams[i]))
        else:
            out.append(_chunk(b'fdAT', struct.pack('>I', seq) + streams[i]))
            seq += 1
    out.append(_chunk(b'IEND', b''))
    return b''.join(out)
