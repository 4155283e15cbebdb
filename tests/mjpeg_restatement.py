"""numpy restatement of the baseline-JPEG contract of csrc/mjpeg.hip.

Integer-exact: the HIP library must return the same bytes.  Every constant here is the library's: the Annex K tables of ITU T.81,
the IJG quality rule, the JFIF colour conversion in 16 fractional bits and the 13-bit integer matrix DCT.  Written for clarity and
vectorised over the blocks of a frame (about a second for 1024 x 1024).
"""
import numpy as np

# ---- Annex K tables ---------------------------------------------------------------------------------------------------------
QUANT_LUM = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHR = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], np.int64)
# ZIGZAG[i] = natural (row-major) index of the i-th coefficient of the scan
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
# (table class << 4 | table id, BITS, HUFFVAL) in the order the DHT segments are written
HUFF_SPECS = ((0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS),
              (0x01, DC_CHR_BITS, DC_VALS), (0x11, AC_CHR_BITS, AC_CHR_VALS))


def huff_lut(bits, vals):
    """T.81 Annex C: (code[256], length[256]) indexed by symbol; length 0 = the symbol has no code"""
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    assert k == len(vals)
    return code, length


# ---- forward DCT ------------------------------------------------------------------------------------------------------------
def dct_matrix():
    """C[k][n] = round(8192 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2"""
    k = np.arange(8)[:, None]
    n = np.arange(8)[None, :]
    ck = np.where(k == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(8192.0 * ck * np.cos((2 * n + 1) * k * np.pi / 16.0)).astype(np.int64)


DCT = dct_matrix()
_I32 = 2 ** 31


def fdct(blocks):
    """blocks int64 [..., 8(y), 8(x)] of samples - 128 -> coefficients [..., 8(v), 8(u)] (v vertical frequency)"""
    t = np.einsum('kn,...yn->...yk', DCT, blocks)
    assert np.abs(t).max(initial=0) + 512 < _I32
    t = (t + 512) >> 10
    u = np.einsum('kn,...nx->...kx', DCT, t)
    assert np.abs(u).max(initial=0) + 32768 < _I32
    return (u + 32768) >> 16


# ---- quantisation -----------------------------------------------------------------------------------------------------------
def quant_table(base, quality):
    """IJG jpeg_quality_scaling + jpeg_add_quant_table (force_baseline): natural order"""
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def quantise(coef, table):
    """sign(c) * ((|c| + Q/2) / Q); coef [..., 64] natural order"""
    a = (np.abs(coef) + (table >> 1)) // table
    return np.where(coef < 0, -a, a)


# ---- colour, padding, subsampling -------------------------------------------------------------------------------------------
def ycbcr_planes(frame):
    """uint8 BGR [H,W,3] -> Y, Cb, Cr int64 [H,W] (JFIF, 16 fractional bits)"""
    f = frame.astype(np.int64)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def _check(frame, quality, subsampling):
    if not (isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3):
        raise ValueError("uint8 [H,W,3] frame expected")
    H, W = frame.shape[:2]
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("H and W must be in [1, 65535]")
    if subsampling not in ('420', '444'):
        raise ValueError("subsampling must be '420' or '444'")
    if not (isinstance(quality, (int, np.integer)) and 1 <= quality <= 100):
        raise ValueError("quality must be an integer in [1, 100]")


def _blocks(plane):
    """[Hp, Wp] -> [Hp/8, Wp/8, 8, 8]"""
    Hp, Wp = plane.shape
    return plane.reshape(Hp // 8, 8, Wp // 8, 8).transpose(0, 2, 1, 3)


def quantised_blocks(frame, quality=90, subsampling='420'):
    """int64 [mcu_rows, blocks_per_row, 64]: the quantised coefficients in zigzag order, blocks in scan order (per MCU: the Y
    blocks row-major, then Cb, then Cr), and comp [blocks_per_row] (0 = Y, 1 = Cb, 2 = Cr)"""
    _check(frame, quality, subsampling)
    H, W = frame.shape[:2]
    m = 16 if subsampling == '420' else 8
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    planes = [np.pad(p, ((0, Hp - H), (0, Wp - W)), mode='edge') for p in ycbcr_planes(frame)]
    if subsampling == '420':
        for i in (1, 2):
            p = planes[i]
            planes[i] = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    tables = (quant_table(QUANT_LUM, quality), quant_table(QUANT_CHR, quality))
    q = []
    for i, p in enumerate(planes):
        c = fdct(_blocks(p) - 128).reshape(p.shape[0] // 8, p.shape[1] // 8, 64)
        q.append(quantise(c, tables[min(i, 1)])[..., ZIGZAG])
    my, mx = Hp // m, Wp // m
    if subsampling == '420':
        y = q[0].reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        out = np.concatenate([y, q[1][:, :, None], q[2][:, :, None]], axis=2)
        comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), mx)
    else:
        out = np.stack(q, axis=2)
        comp = np.tile(np.array([0, 1, 2]), mx)
    return out.reshape(my, -1, 64), comp


# ---- entropy coding ---------------------------------------------------------------------------------------------------------
def _bit_size(a):
    """number of bits of the magnitudes a >= 0 (0 for 0)"""
    s = np.zeros(a.shape, np.int64)
    v = a.copy()
    while v.any():
        s += v > 0
        v >>= 1
    return s


def _value_bits(v, size):
    """the `size` low bits that follow a Huffman code: v for v >= 0, v - 1 for v < 0 (T.81 F.1.2.1)"""
    return np.where(v < 0, v - 1, v) & ((1 << size) - 1)


def _row_symbols(q, comp):
    """q [nb, 64] of one MCU row -> (bits, lengths) int64 [nb, 65]: slot 0 the DC difference, slot k the AC coefficient k with the
    ZRLs before it, slot 64 the EOB; each slot's bits are right-aligned in `lengths` bits (at most 59)"""
    nb = q.shape[0]
    bits = np.zeros((nb, 65), np.int64)
    lens = np.zeros((nb, 65), np.int64)
    luts = [huff_lut(b, v) for _, b, v in HUFF_SPECS]                    # DC lum, AC lum, DC chroma, AC chroma
    chroma = comp > 0
    # DC: the difference to the previous block of the same component, 0 before the first of the row
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        dc = q[idx, 0]
        diff = dc - np.concatenate([[0], dc[:-1]])
        size = _bit_size(np.abs(diff))
        assert size.max(initial=0) <= 11
        code, ln = luts[0 if c == 0 else 2]
        bits[idx, 0] = (code[size] << size) | _value_bits(diff, size)
        lens[idx, 0] = ln[size] + size
    # AC
    ac = q[:, 1:]
    nz = ac != 0
    pos = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)          # position of the last non-zero at or before k
    prev = np.concatenate([np.zeros((nb, 1), np.int64), last[:, :-1]], axis=1)
    run = pos - prev - 1
    size = _bit_size(np.abs(ac))
    assert size.max(initial=0) <= 10
    for is_chroma in (False, True):
        code, ln = luts[3 if is_chroma else 1]
        sel = nz & (chroma == is_chroma)[:, None]
        r, s, v = run[sel], size[sel], ac[sel]
        zrl = r >> 4
        sym = ((r & 15) << 4) | s
        assert ln[sym].all() and ln[0xf0] and ln[0x00]
        b = np.zeros(r.shape, np.int64)
        n = np.zeros(r.shape, np.int64)
        for i in range(3):                                               # up to three ZRL (run of 16 zeros) codes
            m = zrl > i
            b = np.where(m, (b << ln[0xf0]) | code[0xf0], b)
            n = n + np.where(m, ln[0xf0], 0)
        b = (((b << ln[sym]) | code[sym]) << s) | _value_bits(v, s)
        n = n + ln[sym] + s
        bits[:, 1:64][sel] = b
        lens[:, 1:64][sel] = n
        eob = (last[:, -1] != 63) & (chroma == is_chroma)
        bits[eob, 64] = code[0x00]
        lens[eob, 64] = ln[0x00]
    return bits, lens


def _pack_row(bits, lens):
    """concatenate the slots' bits MSB first, pad the last byte with 1-bits, stuff FF -> FF 00"""
    b, n = bits.ravel(), lens.ravel()
    keep = n > 0
    b, n = b[keep], n[keep]
    start = np.cumsum(n) - n
    total = int(n.sum())
    slot = np.repeat(np.arange(n.size), n)
    j = np.arange(total) - start[slot]
    stream = ((b[slot] >> (n[slot] - 1 - j)) & 1).astype(np.uint8)
    stream = np.concatenate([stream, np.ones((-total) % 8, np.uint8)])
    by = np.packbits(stream)
    ff = np.nonzero(by == 0xFF)[0]
    return np.insert(by, ff + 1, 0).tobytes()


def entropy_segments(frame, quality=90, subsampling='420'):
    """the stuffed bytes of each MCU row (restart interval), without the RST markers"""
    q, comp = quantised_blocks(frame, quality, subsampling)
    return [_pack_row(*_row_symbols(q[r], comp)) for r in range(q.shape[0])]


# ---- headers ----------------------------------------------------------------------------------------------------------------
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def header(H, W, quality=90, subsampling='420'):
    """SOI, APP0 (JFIF 1.01, no density, no thumbnail), two DQT, SOF0, four DHT, DRI, SOS"""
    m = 16 if subsampling == '420' else 8
    out = b'\xff\xd8' + _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for i, base in enumerate((QUANT_LUM, QUANT_CHR)):
        out += _seg(0xDB, bytes([i]) + bytes(quant_table(base, quality)[ZIGZAG].tolist()))
    ysamp = 0x22 if subsampling == '420' else 0x11
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') +
                bytes([3, 1, ysamp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFF_SPECS:
        out += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _seg(0xDD, (-(-W // m)).to_bytes(2, 'big'))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(frame, quality=90, subsampling='420'):
    """one complete baseline JPEG of the uint8 BGR frame [H,W,3]"""
    _check(frame, quality, subsampling)
    H, W = frame.shape[:2]
    segs = entropy_segments(frame, quality, subsampling)
    out = [header(H, W, quality, subsampling)]
    for r, s in enumerate(segs):
        out.append(s)
        if r + 1 < len(segs):
            out.append(bytes([0xFF, 0xD0 + (r % 8)]))
    out.append(b'\xff\xd9')
    return b''.join(out)
