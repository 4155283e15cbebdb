"""The contract of the PNG decoder restated in numpy / pure Python, stage by stage as csrc/pngdec.hip runs it: the
walk of the deflate stream to literals plus match records, the source map, pointer doubling, the gather, the unfiltering and the
colour conversion.  Written from RFC 1950, RFC 1951 and the PNG specification (second edition, clauses 9 and 11), not from the HIP.
The chunk walk is a few lines of its own here, so that cartoonsegmentation_amd.pngread is checked against it rather than trusted.
"""
import struct
import zlib

import numpy as np

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


class Corrupt(ValueError):
    pass


def huffman_table(lengths, may_be_empty=False):
    """(table, bits): table[next `bits` bits of the stream] = length << 9 | symbol, or 0 where no code matches (RFC 1951 3.2.2)"""
    maxlen = max(lengths) if len(lengths) else 0
    if maxlen == 0:
        if may_be_empty:
            return [0, 0], 1
        raise Corrupt("a code without symbols")
    count = [0] * (maxlen + 1)
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    left = 1
    for ln in range(1, maxlen + 1):
        left = 2 * left - count[ln]
        if left < 0:
            raise Corrupt("over-subscribed code")
    if left > 0 and not (maxlen == 1 and count[1] == 1):
        raise Corrupt("incomplete code")
    code, next_code = 0, [0] * (maxlen + 2)
    for ln in range(1, maxlen + 1):
        code = (code + count[ln - 1]) << 1
        next_code[ln] = code
    table = [0] * (1 << maxlen)
    for sym, ln in enumerate(lengths):
        if ln:
            c = next_code[ln]
            next_code[ln] += 1
            r = int(format(c, '0%db' % ln)[::-1], 2)
            n = 1 << (maxlen - ln)
            table[r::1 << ln] = [ln << 9 | sym] * n
    return table, maxlen


FIXED_LIT = huffman_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = huffman_table([5] * 32)


def walk(stream):
    """The walk over one zlib stream.  Returns (lit, matches, stats): lit uint8 [raw bytes] with the literal (and stored) bytes at
    their own positions and 0 elsewhere, matches int64 [m, 3] of (position, length, distance) in stream order, stats: 'blocks' (the
    list of block types: 0 stored, 1 fixed, 2 dynamic), 'empty_stored', 'literal_only_dynamic' (dynamic blocks without a match),
    'adler' (the trailer: the four bytes behind the deflate data), 'trailing' (bytes behind the trailer, which are ignored)."""
    stream = bytes(stream)
    if len(stream) < 6:
        raise Corrupt("short stream")
    cmf, flg = stream[0], stream[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or (flg & 0x20) or (cmf * 256 + flg) % 31:
        raise Corrupt("zlib header")
    data = stream[2:]
    nbytes = len(data) - 4                       # the deflate data end in front of the four trailer bytes at the latest
    pos, bitbuf, nbits = 0, 0, 0
    lit = bytearray()
    matches = []
    stats = {'blocks': [], 'empty_stored': 0, 'literal_only_dynamic': 0}

    def need(n):
        nonlocal pos, bitbuf, nbits
        while nbits < n:
            if pos >= nbytes:
                raise Corrupt("out of input")
            bitbuf |= data[pos] << nbits
            pos += 1
            nbits += 8

    def get(n):
        nonlocal bitbuf, nbits
        need(n)
        v = bitbuf & ((1 << n) - 1)
        bitbuf >>= n
        nbits -= n
        return v

    def symbol(table, bits):
        nonlocal pos, bitbuf, nbits
        while nbits < bits and pos < nbytes:
            bitbuf |= data[pos] << nbits
            pos += 1
            nbits += 8
        e = table[bitbuf & ((1 << bits) - 1)]
        ln = e >> 9
        if e == 0:
            raise Corrupt("invalid code")
        if ln > nbits:
            raise Corrupt("out of input")
        bitbuf >>= ln
        nbits -= ln
        return e & 511

    while True:
        last, kind = get(1), get(2)
        stats['blocks'].append(kind)
        if kind == 3:
            raise Corrupt("block type 3")
        if kind == 0:
            bitbuf >>= nbits & 7
            nbits -= nbits & 7
            n, inv = get(16), get(16)
            if n ^ inv != 0xFFFF:
                raise Corrupt("stored length")
            assert nbits % 8 == 0
            pos -= nbits // 8
            bitbuf, nbits = 0, 0
            if pos + n > nbytes:
                raise Corrupt("out of input")
            lit += data[pos:pos + n]
            pos += n
            stats['empty_stored'] += n == 0
        else:
            if kind == 1:
                (lt, lb), (dt, db) = FIXED_LIT, FIXED_DIST
            else:
                nlit, ndist, ncl = get(5) + 257, get(5) + 1, get(4) + 4
                if nlit > 286 or ndist > 30:
                    raise Corrupt("too many symbols")
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = get(3)
                ct, cb = huffman_table(cl)
                if sum(1 for v in cl if v) == 1:
                    raise Corrupt("incomplete code-length code")
                lens = []
                while len(lens) < nlit + ndist:
                    s = symbol(ct, cb)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise Corrupt("repeat without a length")
                        lens += [lens[-1]] * (3 + get(2))
                    elif s == 17:
                        lens += [0] * (3 + get(3))
                    else:
                        lens += [0] * (11 + get(7))
                if len(lens) > nlit + ndist:
                    raise Corrupt("a run of lengths past the end")
                if lens[256] == 0:
                    raise Corrupt("no end-of-block code")
                lt, lb = huffman_table(lens[:nlit])
                dt, db = huffman_table(lens[nlit:], may_be_empty=True)
            before = len(matches)
            while True:
                s = symbol(lt, lb)
                if s < 256:
                    lit.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise Corrupt("length symbol %d" % s)
                    ln = LENGTH_BASE[s - 257] + get(LENGTH_EXTRA[s - 257])
                    d = symbol(dt, db)
                    if d > 29:
                        raise Corrupt("distance symbol %d" % d)
                    dist = DIST_BASE[d] + get(DIST_EXTRA[d])
                    if dist > len(lit):
                        raise Corrupt("distance before byte 0")
                    matches.append((len(lit), ln, dist))
                    lit += bytes(ln)
            if kind == 2 and len(matches) == before:
                stats['literal_only_dynamic'] += 1
        if last:
            break
    end = pos - nbits // 8                       # whole unread bytes go back; the trailer stands behind the last started byte
    stats['adler'] = int.from_bytes(data[end:end + 4], 'big')
    stats['trailing'] = len(data) - end - 4
    return np.frombuffer(bytes(lit), np.uint8).copy(), np.asarray(matches, np.int64).reshape(-1, 3), stats


def source_map(n, matches):
    """src[p] for every raw byte: its own position for a literal, p - distance for a byte of a match"""
    src = np.arange(n, dtype=np.int64)
    if len(matches):
        pos, ln, dist = matches[:, 0], matches[:, 1], matches[:, 2]
        first = np.repeat(pos, ln)
        k = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        src[first + k] = first + k - np.repeat(dist, ln)
    return src


def pointer_doubling(src):
    """src[p] = src[src[p]] until nothing changes: (the resolved map, the rounds that changed something)"""
    rounds = 0
    while True:
        nxt = src[src]
        if np.array_equal(nxt, src):
            return src, rounds
        src = nxt
        rounds += 1


def inflate(stream):
    """(raw bytes as uint8, stats) of one zlib stream, through the stages above; stats gains 'rounds', 'matches', 'adler_ok'"""
    lit, matches, stats = walk(stream)
    src, rounds = pointer_doubling(source_map(len(lit), matches))
    raw = lit[src]
    stats.update(rounds=rounds, matches=matches, adler_ok=zlib.adler32(raw.tobytes()) == stats['adler'])
    return raw, stats


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, H, W, bpp):
    """the reconstructed bytes uint8 [H, W * bpp] of the raw scanlines (PNG specification 9.2): the row above the first row and the
    pixel left of the first pixel are zero; everything per byte, mod 256, at a distance of bpp bytes"""
    stride = 1 + W * bpp
    if raw.size != H * stride:
        raise Corrupt("raw size %d for %dx%d at %d bytes per pixel" % (raw.size, W, H, bpp))
    rows = raw.reshape(H, stride)
    out = np.zeros((H, W * bpp), np.uint8)
    prev = np.zeros(W * bpp, np.int64)
    for y in range(H):
        ft, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if ft == 0:
            cur = x
        elif ft == 1:
            cur = np.cumsum(x.reshape(W, bpp), axis=0).reshape(-1) & 255
        elif ft == 2:
            cur = (x + prev) & 255
        elif ft == 3:
            cur = np.zeros(W * bpp, np.int64)
            for i in range(W * bpp):
                a = cur[i - bpp] if i >= bpp else 0
                cur[i] = (x[i] + ((a + prev[i]) >> 1)) & 255
        elif ft == 4:
            cur = np.zeros(W * bpp, np.int64)
            for i in range(W * bpp):
                a, c = (int(cur[i - bpp]), int(prev[i - bpp])) if i >= bpp else (0, 0)
                cur[i] = (x[i] + paeth(a, int(prev[i]), c)) & 255
        else:
            raise Corrupt("filter type %d" % ft)
        out[y] = cur
        prev = cur
    return out


def colour(px, H, W, ct, palette):
    """B, G, R uint8 [H, W, 3]: grey replicated, alpha dropped, R and B swapped, palette entries looked up (zero beyond its end)"""
    p = px.reshape(H, W, CHANNELS[ct])
    if ct in (0, 4):
        return np.repeat(p[:, :, :1], 3, axis=2)
    if ct in (2, 6):
        return np.ascontiguousarray(p[:, :, 2::-1])
    pal = np.zeros((256, 3), np.uint8)
    pal[:len(palette)] = palette
    return np.ascontiguousarray(pal[p[:, :, 0]][:, :, ::-1])


def chunks(data):
    """[(type, payload)] of a PNG file, lengths and CRCs checked"""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    p, out = 8, []
    while p < len(data):
        n, = struct.unpack('>I', data[p:p + 4])
        kind, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        assert len(body) == n and zlib.crc32(kind + body) == struct.unpack('>I', data[p + 8 + n:p + 12 + n])[0]
        out.append((kind, body))
        p += 12 + n
        if kind == b'IEND':
            break
    return out


def decode(data):
    """(raw, pixels, stats, header) of a PNG file of 8 bits per sample: the zlib stream's raw bytes, the B, G, R image, the walk's
    statistics and (W, H, colour type)"""
    ch = chunks(data)
    W, H, depth, ct, _, _, lace = struct.unpack('>IIBBBBB', ch[0][1])
    assert ch[0][0] == b'IHDR' and depth == 8 and lace == 0
    stream = b''.join(body for kind, body in ch if kind == b'IDAT')
    palette = next((np.frombuffer(body, np.uint8).reshape(-1, 3) for kind, body in ch if kind == b'PLTE'), np.zeros((0, 3), np.uint8))
    raw, stats = inflate(stream)
    if not stats['adler_ok']:
        raise Corrupt("Adler-32")
    px = unfilter(raw, H, W, CHANNELS[ct])
    return raw, colour(px, H, W, ct, palette), stats, (W, H, ct)
