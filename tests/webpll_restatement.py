"""An independent numpy / Python restatement of the lossless WebP contract: subtract-green, the predictor
transform with one mode per 16 x 16 block, the row-wise run parse, the five histograms, the length-limited prefix codes and their
headers, the bit writer and the RIFF container.  It shares no code with cartoonsegmentation_amd (csrc/webpll.hip, webpcode.py);
the tests hold the product to it byte for byte, and Pillow (libwebp) judges that its files decode to the input.

    encode(img)            a complete .webp file of one image
    payload(img)           the VP8L chunk's payload alone
    planes(img)            (mode image, residual image) as uint32 ARGB [h,w]
    histograms(plane)      the five count vectors of a plane
    worst_case_bytes(W,H)  the contract's cap on a file

img: uint8 [H,W] (grey), [H,W,3] (B, G, R in memory), [H,W,4] (B, G, R, A in memory) or bool [H,W] (a mask, written 0 / 255).
"""
import struct

import numpy as np

from png_restatement import assign_codes, code_lengths, length_symbols, mirrored

BLOCK_BITS = 4                                                  # one predictor mode per 16 x 16 pixels
BLOCK = 1 << BLOCK_BITS
MODES = 13                                                      # the candidates are the modes 0..12
MAX_REF = 4096                                                  # the longest backward reference
ALPHABETS = (256 + 24, 256, 256, 256, 40)                       # green + length prefixes, red, blue, alpha, distance prefixes
ORDER_OF_CODE_LENGTHS = [17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
DIST_LEFT = 2                                                   # the plane code of "the pixel to the left"


# ---- pixels -----------------------------------------------------------------------------------------------------------------
def channels(img):
    """(int64 [H,W,4] in A, R, G, B order, has_alpha)"""
    a = np.asarray(img)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8) * 255
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    H, W = a.shape[:2]
    out = np.full((H, W, 4), 255, np.int64)
    if a.ndim == 2:
        out[..., 1] = out[..., 2] = out[..., 3] = a
    else:
        assert a.shape[2] in (3, 4)
        out[..., 3], out[..., 2], out[..., 1] = a[..., 0], a[..., 1], a[..., 2]
        if a.shape[2] == 4:
            out[..., 0] = a[..., 3]
    return out, a.ndim == 3 and a.shape[2] == 4


def pack(px):
    px = px.astype(np.uint32)
    return px[..., 0] << 24 | px[..., 1] << 16 | px[..., 2] << 8 | px[..., 3]


def subtract_green(px):
    out = px.copy()
    out[..., 1] = (px[..., 1] - px[..., 2]) % 256
    out[..., 3] = (px[..., 3] - px[..., 2]) % 256
    return out


def candidates(px):
    """the 13 predictions of every pixel from its neighbours in px (int64 [H,W,4]); meaningful where y >= 1 and x >= 1"""
    H, W, _ = px.shape
    L = np.zeros_like(px); L[:, 1:] = px[:, :-1]
    T = np.zeros_like(px); T[1:] = px[:-1]
    TL = np.zeros_like(px); TL[1:, 1:] = px[:-1, :-1]
    TR = np.zeros_like(px); TR[1:, :-1] = px[:-1, 1:]
    TR[1:, W - 1] = px[1:, 0]                                   # behind the last column: the first pixel of the current row

    def avg(a, b):
        return (a + b) // 2
    black = np.zeros_like(px); black[..., 0] = 255
    select = np.where((np.abs(T - TL).sum(axis=2) < np.abs(L - TL).sum(axis=2))[..., None], L, T)
    return np.stack([black, L, T, TR, TL, avg(avg(L, TR), T), avg(L, TL), avg(L, T), avg(TL, T), avg(T, TR),
                     avg(avg(L, TL), avg(T, TR)), select, np.clip(L + T - TL, 0, 255)])


def planes(img):
    """(modes uint32 [hb,wb], residuals uint32 [H,W], has_alpha)"""
    px, has_alpha = channels(img)
    px = subtract_green(px)
    H, W, _ = px.shape
    cand = candidates(px)
    res = (px[None] - cand) % 256                               # [13,H,W,4]
    cost = np.minimum(res, 256 - res).sum(axis=3)
    cost[:, 0, :] = 0                                           # the border pixels do not depend on the mode
    cost[:, :, 0] = 0
    hb, wb = -(-H // BLOCK), -(-W // BLOCK)
    padded = np.zeros((MODES, hb * BLOCK, wb * BLOCK), np.int64)
    padded[:, :H, :W] = cost
    score = padded.reshape(MODES, hb, BLOCK, wb, BLOCK).sum(axis=(2, 4))
    mode = np.argmin(score, axis=0)                             # the first minimum: ties go to the lowest mode
    per_pixel = np.repeat(np.repeat(mode, BLOCK, axis=0), BLOCK, axis=1)[:H, :W]
    pred = np.take_along_axis(cand, per_pixel[None, :, :, None], axis=0)[0]
    pred[0, 1:] = px[0, :-1]                                    # row 0: L
    pred[1:, 0] = px[:-1, 0]                                    # column 0: T
    pred[0, 0] = (255, 0, 0, 0)
    return (np.uint32(0xff000000) | mode.astype(np.uint32) << 8), pack((px - pred) % 256), has_alpha


# ---- parse ------------------------------------------------------------------------------------------------------------------
def prefix(v):
    """(prefix symbol, extra bits, extra value) of a length or distance value v >= 1"""
    d = v - 1
    if d < 4:
        return d, 0, 0
    hb = d.bit_length() - 1
    return 2 * hb + ((d >> (hb - 1)) & 1), hb - 1, d & ((1 << (hb - 1)) - 1)


def tokens(plane):
    """the tokens of a plane, row by row: ('lit', pixel) or ('ref', length); a run of n equal pixels of a row is its first pixel
    as a literal, (n - 1) // 4096 references of 4096, then one reference of the remainder if there is one"""
    H, W = plane.shape
    start = np.ones((H, W), bool)
    start[:, 1:] = plane[:, 1:] != plane[:, :-1]
    pos = np.flatnonzero(start.reshape(-1))
    value = plane.reshape(-1)[pos]
    length = np.diff(np.append(pos, H * W))
    out = []
    for v, n in zip(value.tolist(), length.tolist()):
        out.append(('lit', v))
        rest = n - 1
        out += [('ref', MAX_REF)] * (rest // MAX_REF)
        if rest % MAX_REF:
            out.append(('ref', rest % MAX_REF))
    return out


def histograms(plane):
    h = [np.zeros(n, np.int64) for n in ALPHABETS]
    for kind, v in tokens(plane):
        if kind == 'lit':
            h[0][v >> 8 & 255] += 1; h[1][v >> 16 & 255] += 1; h[2][v & 255] += 1; h[3][v >> 24] += 1
        else:
            h[0][256 + prefix(v)[0]] += 1
            h[4][prefix(DIST_LEFT)[0]] += 1
    return h


# ---- codes ------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """the first bit written is the lowest bit of the first byte"""
    def __init__(self):
        self.bits = []

    def number(self, v, n):                                     # plain value, lowest bit first
        self.bits += [(v >> k) & 1 for k in range(n)]

    def huffman(self, code, n):                                 # prefix code, highest bit first
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]

    def tobytes(self):
        return np.packbits(np.array(self.bits, np.uint8), bitorder='little').tobytes()


def write_code(w, hist):
    """one prefix code into w; returns (lengths, codes MSB-first).  No or one used symbol: a simple code of one symbol (symbol 0
    if none is used), whose occurrences cost no bits; otherwise a normal code, limit 15, every length of the alphabet written"""
    used = [s for s in range(len(hist)) if hist[s] > 0]
    if len(used) < 2:
        s = used[0] if used else 0
        assert s < 256
        w.number(1, 1); w.number(0, 1)
        if s < 2:
            w.number(0, 1); w.number(s, 1)
        else:
            w.number(1, 1); w.number(s, 8)
        return [0] * len(hist), [0] * len(hist)
    lengths = code_lengths(hist, 15)
    syms = length_symbols(lengths)
    cl_hist = [0] * 19
    for s, _, _ in syms:
        cl_hist[s] += 1
    cl_len = code_lengths(cl_hist, 7)
    cl_code = assign_codes(cl_len)
    count = max(4, max(k for k in range(19) if cl_len[ORDER_OF_CODE_LENGTHS[k]]) + 1)
    w.number(0, 1); w.number(count - 4, 4)
    for k in range(count):
        w.number(cl_len[ORDER_OF_CODE_LENGTHS[k]], 3)
    w.number(0, 1)                                              # every length of the alphabet follows
    for s, eb, ev in syms:
        w.huffman(cl_code[s], cl_len[s])
        w.number(ev, eb)
    return lengths, assign_codes(lengths)


def write_plane(w, plane):
    """the five codes of a plane, then its pixels"""
    codes = [write_code(w, h) for h in histograms(plane)]
    dist_sym = prefix(DIST_LEFT)[0]
    for kind, v in tokens(plane):
        if kind == 'lit':
            for a, s in ((0, v >> 8 & 255), (1, v >> 16 & 255), (2, v & 255), (3, v >> 24)):
                w.huffman(codes[a][1][s], codes[a][0][s])
        else:
            p, eb, ev = prefix(v)
            w.huffman(codes[0][1][256 + p], codes[0][0][256 + p])
            w.number(ev, eb)
            w.huffman(codes[4][1][dist_sym], codes[4][0][dist_sym])


def plane_bits(plane):
    """(bits of the five code headers, bits of the pixels) of a plane"""
    head = BitWriter()
    for h in histograms(plane):
        write_code(head, h)
    whole = BitWriter()
    write_plane(whole, plane)
    return len(head.bits), len(whole.bits) - len(head.bits)


def payload(img):
    mode, res, has_alpha = planes(img)
    H, W = res.shape
    w = BitWriter()
    w.number(0x2f, 8); w.number(W - 1, 14); w.number(H - 1, 14); w.number(int(has_alpha), 1); w.number(0, 3)
    w.number(1, 1); w.number(2, 2)                              # subtract-green
    w.number(1, 1); w.number(0, 2); w.number(BLOCK_BITS - 2, 3)  # predictor, then its sub-image
    w.number(0, 1)                                              # no colour cache
    write_plane(w, mode)
    w.number(0, 1)                                              # no further transform
    w.number(0, 1); w.number(0, 1)                              # no colour cache, no meta prefix codes
    write_plane(w, res)
    return w.tobytes()


def container(data):
    body = b'WEBP' + b'VP8L' + struct.pack('<I', len(data)) + data + (b'\x00' if len(data) & 1 else b'')
    return b'RIFF' + struct.pack('<I', len(body)) + body


def encode(img):
    return container(payload(img))


def worst_case_bytes(W, H):
    """the contract's cap on a file: every pixel of both planes four literals of 15 bits, ten code headers of
    the longest form, the image header and transform bits, the container"""
    wb, hb = -(-W // BLOCK), -(-H // BLOCK)
    header = sum(1 + 4 + 19 * 3 + 1 + 7 * n for n in ALPHABETS)
    bits = 40 + 3 + 6 + 1 + 3 + 2 * header + 60 * (W * H + wb * hb)
    return 20 + ((bits + 7) // 8 + 1) // 2 * 2
