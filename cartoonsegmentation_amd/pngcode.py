"""Host side of the PNG writer (contract DESIGN.md §4.7; pure Python / numpy, no device): the deflate code of one image from the
histogram that csrc/png.hip measured, the table the write call reads, and the PNG container.

    build_code(hist)  286 counts (the end-of-block symbol included) -> the cheaper of the fixed code and a dynamic code:
                      code lengths, bit-reversed codes, the header bits and the exact size of the stream
    table_row(...)    the uint32 [384] row of csm_png_write for one image
    png_file(...)     signature + IHDR + one IDAT + IEND around a zlib stream
"""
import struct
import zlib

import numpy as np

LIT_SYMS = 286
EOB = 256
MAX_BITS = 15                # deflate's limit of a literal / length code
CL_MAX_BITS = 7              # and of a code-length code
TABLE_WORDS = 384
HEADER_WORDS_MAX = TABLE_WORDS - 292
# extra bits of the length symbols 257..285 (RFC 1951 §3.2.5)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LENGTHS = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 6        # symbols 0..285 of the fixed code
PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def limited_lengths(hist, limit):
    """Code lengths <= limit of the symbols with a non-zero count, by package-merge: optimal under the limit (so the plain
    Huffman cost whenever that tree is no deeper), complete (Kraft sum exactly 1), and deterministic.  The symbols are ordered by
    (count ascending, symbol descending); lengths never increase along that order, so a higher count never gets a longer code
    and of two equal counts the lower symbol never gets the longer one.  Each of the `limit` lists is the sorted leaves merged
    with the pairs of the list before it, a leaf before a package of the same weight; the first 2n - 2 items of the last list
    are taken, and a symbol's length is the number of lists in which its leaf is taken.  Returns a list as long as hist (0 = no
    code).  At least two symbols must be used."""
    hist = [int(v) for v in hist]
    order = sorted((s for s, c in enumerate(hist) if c > 0), key=lambda s: (hist[s], -s))
    n = len(order)
    if n < 2:
        raise ValueError("limited_lengths: at least two symbols must have a count (got %d)" % n)
    if n > 1 << limit:
        raise ValueError("limited_lengths: %d symbols do not fit codes of %d bits" % (n, limit))
    leaves = np.array([hist[s] for s in order], dtype=np.int64)
    leaf_flag = np.zeros(n, dtype=np.int64)
    flags, weights = [leaf_flag], leaves
    for _ in range(limit - 1):
        m = len(weights) // 2
        packages = weights[0:2 * m:2] + weights[1:2 * m:2]
        both = np.concatenate([leaves, packages])
        idx = np.argsort(both, kind='stable')                  # stable: leaves stay ahead of packages of the same weight
        weights = both[idx]
        flags.append(np.concatenate([leaf_flag, np.ones(m, dtype=np.int64)])[idx])
    depth = np.zeros(n, dtype=np.int64)
    take = 2 * n - 2
    for is_package in reversed(flags):
        p = int(is_package[:take].sum())
        depth[:take - p] += 1                                  # the leaves taken in a list are the first ones
        take = 2 * p
    out = [0] * len(hist)
    for s, d in zip(order, depth.tolist()):
        out[s] = d
    return out


def canonical_codes(lengths):
    """RFC 1951 §3.2.2 codes of `lengths`, each reversed bit by bit: deflate packs LSB-first and reads a Huffman code from its
    first bit on."""
    count = [0] * (max(lengths) + 2)
    for v in lengths:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * len(count), 0
    for b in range(1, len(count)):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for v in lengths:
        if v == 0:
            out.append(0)
            continue
        c = nxt[v]
        nxt[v] += 1
        out.append(int(format(c, '0%db' % v)[::-1], 2))
    return out


def run_code(lengths):
    """The code-length symbols of a sequence of code lengths as [(symbol, extra bits, extra value)].  A run of zeros gives 18s of
    up to 138 while 11 or more are left, then one 17 if 3 or more are left, else plain zeros; a run of another value gives the
    value once, then 16s of up to 6 while 3 or more are left, then the value plainly."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        c = j - i
        i = j
        if v == 0:
            while c >= 11:
                k = min(c, 138)
                out.append((18, 7, k - 11))
                c -= k
            if c >= 3:
                out.append((17, 3, c - 3))
                c = 0
        else:
            out.append((v, 0, 0))
            c -= 1
            while c >= 3:
                k = min(c, 6)
                out.append((16, 2, k - 3))
                c -= k
        out += [(v, 0, 0)] * c
    return out


class _Bits:
    """LSB-first bit string"""
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v, k):
        self.value |= int(v) << self.n
        self.n += k


def _payload_bits(hist, lengths, dist_bits):
    bits = sum(hist[s] * lengths[s] for s in range(LIT_SYMS))
    bits += sum(hist[257 + k] * (LEN_EXTRA[k] + dist_bits) for k in range(29))
    return bits


def dynamic_header(lengths):
    """the bits of a BTYPE 2 block header (BFINAL = 1) for the literal / length code `lengths` and the one-symbol distance code
    (symbol 0, length 1), behind the two zlib bytes 78 01"""
    hlit = max(257, max(s for s in range(LIT_SYMS) if lengths[s]) + 1)
    symbols = run_code(list(lengths[:hlit]) + [1])
    cl_hist = [0] * 19
    for s, _, _ in symbols:
        cl_hist[s] += 1
    cl_len = limited_lengths(cl_hist, CL_MAX_BITS)
    cl_code = canonical_codes(cl_len)
    hclen = max(4, max(k for k in range(19) if cl_len[CL_ORDER[k]]) + 1)
    b = _Bits()
    b.put(0x0178, 16)
    b.put(1, 1); b.put(2, 2); b.put(hlit - 257, 5); b.put(0, 5); b.put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cl_len[CL_ORDER[k]], 3)
    for s, eb, ev in symbols:
        b.put(cl_code[s], cl_len[s])
        b.put(ev, eb)
    return b


def build_code(hist):
    """The code of one image from its 286 counts (end-of-block included).  Returns a dict: 'btype' (1 fixed, 2 dynamic),
    'lengths' and 'codes' (bit-reversed) of the 286 symbols, 'dist_bits' (bits of a match's distance code: all zero),
    'header' / 'header_bits' (LSB-first integer: the zlib bytes 78 01 and the block header), 'bits' (header + symbols, the
    end-of-block symbol included), 'bytes' of the whole zlib stream (header, block, Adler-32), and 'fixed_bits' / 'dynamic_bits'
    (what 'bits' is under either code).  The dynamic code is taken only where it is smaller in bits."""
    hist = [int(v) for v in hist]
    if len(hist) != LIT_SYMS or hist[EOB] != 1 or min(hist) < 0:
        raise ValueError("build_code: 286 counts with the end-of-block symbol counted once are expected")
    dyn_len = limited_lengths(hist, MAX_BITS)
    dyn_hdr = dynamic_header(dyn_len)
    dyn_bits = dyn_hdr.n + _payload_bits(hist, dyn_len, 1)
    fix_bits = 16 + 3 + _payload_bits(hist, FIXED_LENGTHS, 5)
    if dyn_bits < fix_bits:
        btype, lengths, dist_bits, hdr, bits = 2, dyn_len, 1, dyn_hdr, dyn_bits
    else:
        hdr = _Bits()
        hdr.put(0x0178, 16)
        hdr.put(1, 1); hdr.put(1, 2)
        btype, lengths, dist_bits, bits = 1, list(FIXED_LENGTHS), 5, fix_bits
    if hdr.n > 32 * HEADER_WORDS_MAX:
        raise ValueError("build_code: a block header of %d bits does not fit the table" % hdr.n)
    codes = canonical_codes(lengths) if btype == 2 else list(FIXED_CODES)
    return {'btype': btype, 'lengths': lengths, 'codes': codes, 'dist_bits': dist_bits, 'header': hdr.value, 'header_bits': hdr.n,
            'bits': bits, 'bytes': (bits + 7) // 8 + 4, 'fixed_bits': fix_bits, 'dynamic_bits': dyn_bits}


# the fixed code is canonical over its 288 symbols (286 and 287 take part in the construction and never occur)
FIXED_CODES = tuple(canonical_codes(list(FIXED_LENGTHS) + [8, 8])[:LIT_SYMS])


def table_row(code, adler, offset):
    """the uint32 [384] row of csm_png_write (include/csm355.h) for one image: `code` from build_code, the measured Adler-32 and
    the stream's byte offset in the blob (a multiple of 4)"""
    row = np.zeros(TABLE_WORDS, dtype=np.uint32)
    row[:LIT_SYMS] = [c | (l << 16) for c, l in zip(code['codes'], code['lengths'])]
    row[286] = code['header_bits']
    row[287] = int(adler)
    row[288], row[289] = offset & 0xFFFFFFFF, offset >> 32
    row[290] = code['dist_bits']
    row[291] = code['bytes']
    h = code['header']
    for k in range((code['header_bits'] + 31) // 32):
        row[292 + k] = (h >> (32 * k)) & 0xFFFFFFFF
    return row


def chunk(kind, data):
    """one PNG chunk: length, type, data, CRC-32 of type + data"""
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def ihdr(width, height, colour_type):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, colour_type, 0, 0, 0))


def png_file(stream, width, height, colour_type):
    """a complete PNG (8 bit, colour type 0 grey or 2 RGB, no interlace) around the zlib stream of its filtered scanlines"""
    return PNG_SIGNATURE + ihdr(width, height, colour_type) + chunk(b'IDAT', stream) + chunk(b'IEND', b'')
